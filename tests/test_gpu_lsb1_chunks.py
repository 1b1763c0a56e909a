"""The +-1 LSB LC kernels (modes 4 and 6) across chunk geometries.  A chunk is one wave's share of a
run; the waves of a workgroup exchange their remaining frame counts through LDS every frame (issue
priority) while the previous frame's PCM stores are still in flight, and a chunk that does not
start its run re-decodes a prefix frame whose stores are dropped.  None of that may reach the PCM:
every batch here is decoded with short chunks (JAAD_CHUNK_FRAMES, read at context creation) and
with the default chunking, the two must agree byte for byte, and each is within 1 LSB of the C
restatement of the reference (float32 output: within one int16 unit).

Geometries: 5 streams x 23 frames in 7-frame chunks (20 chunks: one full 12-wave workgroup and a
partly filled one, chunks of 7 and 2 frames, prefix frames in 15 chunks) and 13 streams x 4 frames
in 3-frame chunks (short chunks behind a prefix frame)."""
import numpy as np
import pytest

from jaadec_amd import native as N
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GEOMETRIES = [(5, 23, 7), (13, 4, 3)]  # streams, frames per stream, JAAD_CHUNK_FRAMES
KINDS = {
    # name: (synth config, channel_config, sf_index, synth overrides)
    "stereo": (2, 2, 3, {}),
    "mono": (1, 1, 4, dict(window_switching=1, pns_percent=5)),
    "mixed_windows": (3, 2, 3, {}),  # C3: all four window sequences -> the mixed-window kernel (mode 6)
}
FORMATS = [N.PCM_BIG_ENDIAN, N.PCM_LITTLE_ENDIAN, N.PCM_FLOAT32]

_cache = {}


def _case(kind, n_streams, fps):
    """The batch and the restatement's PCM in every format, computed once per (kind, geometry)."""
    key = (kind, n_streams, fps)
    if key not in _cache:
        cfg_id, cc, sf_index, over = KINDS[kind]
        p = N.synth_params(cfg_id, n_streams=n_streams, frames_per_stream=fps, sf_index=sf_index, **over)
        b = N.synth_batch(p)
        want = {fl: O.decode_batch(N.make_cfg(sf_index=sf_index, channel_config=cc), b, O.Streams(n_streams), fl)
                for fl in FORMATS}
        for w in want.values():
            w.setflags(write=False)
        _cache[key] = (b, cc, sf_index, want)
    return _cache[key]


def _assert_within_one_lsb(got, want, flags):
    if flags & N.PCM_FLOAT32:
        d = np.abs(got.view(np.float32).astype(np.float64) - want.view(np.float32).astype(np.float64))
    else:
        dt = "<i2" if flags & N.PCM_LITTLE_ENDIAN else ">i2"
        d = np.abs(got.view(dt).astype(np.int32) - want.view(dt).astype(np.int32))
    print(f"flags {flags:#x}: max |delta| {d.max()}")
    assert d.max() <= 1, d.max()


def _decode(cfg, n_slots, batches, flags):
    with N.Context(cfg, n_slots) as ctx:
        return [ctx.decode(b, flags) for b in batches]


@pytest.mark.parametrize("n_streams,fps,chunk", GEOMETRIES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_short_chunks_equal_default_chunking(kind, n_streams, fps, chunk, monkeypatch):
    b, cc, sf_index, want = _case(kind, n_streams, fps)
    if kind == "mixed_windows" and fps > 8:
        assert (b.ics["window_sequence"] == 2).any()  # EIGHT_SHORT frames: the host entry picks mode 6
    cfg = N.make_cfg(sf_index=sf_index, channel_config=cc, precision=N.PRECISION_LSB1)
    for flags in FORMATS:
        monkeypatch.delenv("JAAD_CHUNK_FRAMES", raising=False)
        (plain,) = _decode(cfg, n_streams, [b], flags)
        monkeypatch.setenv("JAAD_CHUNK_FRAMES", str(chunk))
        (short,) = _decode(cfg, n_streams, [b], flags)
        _assert_within_one_lsb(plain, want[flags], flags)
        _assert_within_one_lsb(short, want[flags], flags)
        assert (short == plain).all(), (flags, int((short != plain).sum()))


@pytest.mark.parametrize("kind", ["stereo", "mixed_windows"])
def test_continuation_call_with_short_chunks(kind, monkeypatch):
    """The same context decodes a second batch continuing every stream: the first call's chunk tails
    store the overlap state behind their last PCM stores, and the second call's chunks load it."""
    n_streams, fps, chunk = GEOMETRIES[0]
    cut = 9
    b, cc, sf_index, want = _case(kind, n_streams, fps)
    first, second = b.split_frames(cut)
    cfg = N.make_cfg(sf_index=sf_index, channel_config=cc, precision=N.PRECISION_LSB1)
    fb = b.frame_begin
    for flags in (N.PCM_BIG_ENDIAN, N.PCM_FLOAT32):
        monkeypatch.delenv("JAAD_CHUNK_FRAMES", raising=False)
        plain = _decode(cfg, n_streams, [first, second], flags)
        monkeypatch.setenv("JAAD_CHUNK_FRAMES", str(chunk))
        short = _decode(cfg, n_streams, [first, second], flags)
        ref1 = np.concatenate([want[flags][fb[r]:fb[r] + cut] for r in range(n_streams)])
        ref2 = np.concatenate([want[flags][fb[r] + cut:fb[r + 1]] for r in range(n_streams)])
        for got in (plain, short):
            _assert_within_one_lsb(got[0], ref1, flags)
            _assert_within_one_lsb(got[1], ref2, flags)
        assert (short[0] == plain[0]).all() and (short[1] == plain[1]).all()
