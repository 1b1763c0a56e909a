"""The frame loop of the +-1 LSB LC kernels (modes 4 and 6) outside the transforms.  The loop runs
unrolled by two: the two bodies take turns in which register set holds the overlap, an odd iteration
count leaves after the first body, and the overlap a chunk stores as stream state comes from
whichever body ran last.  Each lane takes its two ms_used bits from the word its 16-lane row holds
(the skip entry of a batch with dropped frames sits in other lanes than in the exact modes), and the
M/S patterns below are the ones a per-quad uniform test or a branch-free form would treat apart.
None of that may reach the PCM: every batch here is decoded
with several chunk lengths (JAAD_CHUNK_FRAMES, read at context creation), all of which must agree
byte for byte and be within 1 LSB of the C restatement of the reference (float32: one int16 unit).

A chunk of n frames that does not start its run runs n + 1 iterations (a prefix frame first), so
chunk lengths 1, 2, 3 and the default give 1 to 4 and 7 iterations, with and without a prefix."""
import numpy as np
import pytest

from jaadec_amd import native as N
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FORMATS = [N.PCM_BIG_ENDIAN, N.PCM_LITTLE_ENDIAN, N.PCM_FLOAT32]
KINDS = {
    # name: (synth config, channel_config, sf_index, synth overrides)
    "stereo": (2, 2, 3, {}),
    "mono": (1, 1, 4, dict(window_switching=1, pns_percent=5)),
    "mixed_windows": (3, 2, 3, {}),  # all four window sequences -> the mixed-window kernel (mode 6)
    "intensity": (2, 2, 3, dict(is_percent=30)),  # intensity bands next to M/S bands
}

_cache = {}


def _synth(kind, n_streams, fps):
    cfg_id, cc, sf_index, over = KINDS[kind]
    p = N.synth_params(cfg_id, n_streams=n_streams, frames_per_stream=fps, sf_index=sf_index, **over)
    return N.synth_batch(p), cc, sf_index


def _oracle(b, cc, sf_index, formats):
    want = {fl: O.decode_batch(N.make_cfg(sf_index=sf_index, channel_config=cc), b, O.Streams(len(b.stream_slot)), fl)
            for fl in formats}
    for w in want.values():
        w.setflags(write=False)
    return want


def _case(key, make, formats=FORMATS):
    """A batch and the restatement's PCM in every format, computed once per key."""
    if key not in _cache:
        b, cc, sf_index = make()
        _cache[key] = (b, cc, sf_index, _oracle(b, cc, sf_index, formats))
    return _cache[key]


def _sub(b, per_run):
    """Sub-batch with the given (possibly empty) frame index arrays, one per run, slots kept."""
    frames = np.concatenate(per_run).astype(np.int64)
    cfr = (frames[:, None] * b.nch + np.arange(b.nch)[None, :]).reshape(-1)
    begin = np.zeros(len(per_run) + 1, np.uint32)
    begin[1:] = np.cumsum([len(x) for x in per_run])
    return N.Batch(np.ascontiguousarray(b.q[cfr]), np.ascontiguousarray(b.sf[cfr]), np.ascontiguousarray(b.cb[cfr]),
                   np.ascontiguousarray(b.ics[cfr]), None if b.ms_used is None else np.ascontiguousarray(b.ms_used[frames]),
                   None if b.tns is None else np.ascontiguousarray(b.tns[cfr]), b.stream_slot.copy(), begin, b.nch,
                   frame_status=None if b.frame_status is None else np.ascontiguousarray(b.frame_status[frames])), frames


def _max_delta(got, want, flags):
    if flags & N.PCM_FLOAT32:
        d = np.abs(got.view(np.float32).astype(np.float64) - want.view(np.float32).astype(np.float64))
    else:
        dt = "<i2" if flags & N.PCM_LITTLE_ENDIAN else ">i2"
        d = np.abs(got.view(dt).astype(np.int32) - want.view(dt).astype(np.int32))
    return d.max() if d.size else 0


def _decode_calls(cfg, n_slots, calls, flags, chunk, monkeypatch):
    if chunk is None:
        monkeypatch.delenv("JAAD_CHUNK_FRAMES", raising=False)
    else:
        monkeypatch.setenv("JAAD_CHUNK_FRAMES", str(chunk))
    with N.Context(cfg, n_slots) as ctx:
        return [ctx.decode(c, flags) for c in calls]


def _check_chunkings(b, cc, sf_index, want, calls, chunks, formats, monkeypatch):
    """calls: [(sub-batch, its frames in b)]; every chunking within 1 LSB of the restatement and byte
    for byte equal to the first chunking."""
    cfg = N.make_cfg(sf_index=sf_index, channel_config=cc, precision=N.PRECISION_LSB1)
    for flags in formats:
        first = None
        for chunk in chunks:
            got = _decode_calls(cfg, len(b.stream_slot), [c for c, _ in calls], flags, chunk, monkeypatch)
            for g, (_, frames) in zip(got, calls):
                d = _max_delta(g, want[flags][frames], flags)
                print(f"flags {flags:#x} chunk {chunk}: max |delta| {d}")
                assert d <= 1, (flags, chunk, d)
            if first is None:
                first = got
            for g, f in zip(got, first):
                assert (g == f).all(), (flags, chunk, int((g != f).sum()))


# runs of 1, 2, 3, 4 and 7 frames (and 5, 6) in the first call; run 2 is empty in the second call and
# goes on in the third from the state its 3 frames left; the first call's run lengths are odd and even,
# so the state a chunk stores comes from either body of the unrolled loop
CALL_LENS = [[1, 2, 3, 4, 7, 5, 6], [3, 3, 0, 2, 1, 4, 2], [2, 1, 4, 1, 3, 2, 1]]


@pytest.mark.parametrize("kind", ["stereo", "mono"])
def test_iteration_count_parity(kind, monkeypatch):
    n_streams, fps = 7, 14
    b, cc, sf_index, want = _case((kind, n_streams, fps), lambda: _synth(kind, n_streams, fps))
    fb, done, calls = b.frame_begin, np.zeros(n_streams, np.int64), []
    for lens in CALL_LENS:
        calls.append(_sub(b, [np.arange(fb[r] + done[r], fb[r] + done[r] + lens[r]) for r in range(n_streams)]))
        done += lens
    assert (done <= fps).all()
    _check_chunkings(b, cc, sf_index, want, calls, [1, 2, 3, None], FORMATS, monkeypatch)


def _with_drops(kind, n_streams, fps):
    b, cc, sf_index = _synth(kind, n_streams, fps)
    st = np.zeros((n_streams, fps), np.uint8)
    for r in range(6):
        st[r, r + 1] = N.FRAME_EOS   # one dropped frame after 1 .. 6 decoded ones: after odd and even iterations
    st[6, 2:4] = N.FRAME_EOS         # a dropped run at the end of a 4-frame chunk
    st[7, 6:8] = N.FRAME_EOS         # ... of its second 4-frame chunk
    st[7, fps - 2:] = N.FRAME_EOS    # and at the end of the run: the last chunk's end in every chunking
    b.frame_status = st.reshape(-1)
    return b, cc, sf_index


@pytest.mark.parametrize("kind", ["stereo", "mixed_windows"])  # kernel modes 4 and 6
def test_dropped_frames_across_the_unroll_boundary(kind, monkeypatch):
    n_streams, fps = 8, 12
    formats = [N.PCM_BIG_ENDIAN, N.PCM_FLOAT32]
    b, cc, sf_index, want = _case((kind, "drops"), lambda: _with_drops(kind, n_streams, fps), formats)
    if kind == "mixed_windows":
        assert (b.ics["window_sequence"] == 2).any()  # EIGHT_SHORT frames: the host entry picks mode 6
    _check_chunkings(b, cc, sf_index, want, [(b, np.arange(b.n_frames))], [3, 4, None], formats, monkeypatch)


def _ms_patterns():
    n_streams, fps = 7, 5
    b, cc, sf_index = _synth("stereo", n_streams, fps)
    assert (b.ics["window_sequence"] == 0).all() and (b.ics["flags"][0::2] & N.ICS_MS_PRESENT).all()
    ms = b.ms_used.reshape(n_streams, fps, 2)
    ones, alt = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0xAAAAAAAAAAAAAAAA)
    ms[0] = ones                                   # every band
    ms[1] = 0                                      # ms_present with no band
    ms[2] = alt                                    # alternating bands: a lane's bands, and its quads, differ
    last = int(b.ics["max_sfb"][0]) - 1
    ms[3] = 0
    ms[3, :, last >> 6] = np.uint64(1) << np.uint64(last & 63)  # only the last band
    # stream 4: the generator's random mask (the two quads of a lane differ in many lanes)
    ms[5] = ones                                   # M/S on all-zero spectra: both channels, then the right one only
    ms[6] = alt
    for s in (5, 6):
        for f in range(fps):
            fr = s * fps + f
            for cf in ([2 * fr, 2 * fr + 1] if f % 2 else [2 * fr + 1]):
                b.q[cf] = 0
                b.sf[cf] = 0
                b.cb[cf] = 0  # ZERO_HCB
    return b, cc, sf_index


def test_ms_patterns(monkeypatch):
    formats = [N.PCM_BIG_ENDIAN, N.PCM_FLOAT32]
    b, cc, sf_index, want = _case("ms_patterns", _ms_patterns, formats)
    _check_chunkings(b, cc, sf_index, want, [(b, np.arange(b.n_frames))], [1, 2, None], formats, monkeypatch)


def test_intensity_next_to_ms(monkeypatch):
    formats = [N.PCM_BIG_ENDIAN, N.PCM_FLOAT32]
    b, cc, sf_index, want = _case("intensity", lambda: _synth("intensity", 3, 5), formats)
    assert (b.ics["flags"] & N.ICS_HAS_IS).any() and (b.ics["flags"] & N.ICS_MS_PRESENT).any()
    _check_chunkings(b, cc, sf_index, want, [(b, np.arange(b.n_frames))], [1, 2, None], formats, monkeypatch)


def test_mixed_windows_on_both_bodies(monkeypatch):
    n_streams, fps = 5, 23
    b, cc, sf_index, want = _case(("mixed_windows", n_streams, fps), lambda: _synth("mixed_windows", n_streams, fps))
    seqs = set(b.ics["window_sequence"].tolist())
    assert seqs == {0, 1, 2, 3}, seqs  # ONLY_LONG, START, EIGHT_SHORT, STOP
    _check_chunkings(b, cc, sf_index, want, [(b, np.arange(b.n_frames))], [1, 2, 3, None], FORMATS, monkeypatch)
