"""The AAC-LC kernels on records the synthetic generator never emits (tests/lc_records.py; what the
batches contain is asserted without a GPU by tests/test_lc_records.py): a CPE whose channels have
their own window sequences, grouping and max_sfb (the right channel's band records looked up by its
own layout; one channel's long transform next to the other's eight short ones inside the stereo
kernels), max_sfb below the band count with junk above it, every scalefactor value, output at and far
past int16 full scale, and the spec-TNS filter walk.

Every batch goes through the host entry with JAAD_CHUNK_FRAMES = 3 and with the default chunk length
(read at context creation): the two must agree byte for byte, and the result is held against the C
restatement of the reference -- bit for bit in PRECISION_EXACT, within 1 LSB (float32: within
tests/test_gpu_precision.py's FLOAT_TOL_*) in PRECISION_LSB1."""
import sys
from pathlib import Path

import numpy as np
import pytest

from jaadec_amd import native as N

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lc_records as R  # noqa: E402
from test_gpu_precision import FLOAT_TOL_PEAK, FLOAT_TOL_RMS  # noqa: E402

pytestmark = pytest.mark.gpu

BE, LE, F32 = N.PCM_BIG_ENDIAN, N.PCM_LITTLE_ENDIAN, N.PCM_FLOAT32
EXACT, LSB1 = N.PRECISION_EXACT, N.PRECISION_LSB1


def _host_entry(name, flags, precision, monkeypatch, tns_mode=None):
    """The batch through N.Context.decode with chunks of 3 frames and of the default length: equal
    byte for byte; returns the PCM."""
    rec = R.records(name)
    got = []
    for chunk in (3, None):
        if chunk is None:
            monkeypatch.delenv("JAAD_CHUNK_FRAMES", raising=False)
        else:
            monkeypatch.setenv("JAAD_CHUNK_FRAMES", str(chunk))
        with N.Context(rec.cfg(precision, tns_mode), rec.n_slots) as ctx:
            got.append(ctx.decode(rec.batch, flags))
    assert (got[0] == got[1]).all(), (name, flags, int((got[0] != got[1]).sum()))
    return got[1]


def _device_entry(name, flags, precision, hint, tns_mode=None):
    """The batch through jaad_decode_batch_device, with or without JAAD_HINT_SHORT_WINDOWS."""
    import torch
    rec = R.records(name)
    b = rec.batch
    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d = {k: up(getattr(b, k)) for k in ("q", "sf", "cb", "ics", "ms_used", "tns")}
    ptr = {k: (v.data_ptr() if v is not None else None) for k, v in d.items()}
    nb = N.pcm_frame_bytes(flags)
    pcm = torch.empty(b.n_frames * nb, dtype=torch.uint8, device=dev)
    with N.Context(rec.cfg(precision, tns_mode), rec.n_slots) as ctx:
        ctx.decode_device(ptr, b, pcm.data_ptr(), pcm.numel(), flags | (N.HINT_SHORT_WINDOWS if hint else 0))
        ctx.wait()
    return pcm.cpu().numpy().reshape(b.n_frames, nb)


def _assert_identical(got, name, flags, tns_mode=None):
    want = R.oracle_pcm(name, flags, tns_mode)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{name} flags {flags:#x}: {len(bad)} bytes differ, first at frame/byte {bad[0].tolist()}"


def _int16_delta(got, name, flags):
    dt = "<i2" if flags & LE else ">i2"
    d = np.abs(got.view(dt).astype(np.int32) - R.oracle_pcm(name, flags).view(dt).astype(np.int32))
    return int(d.max())


def _float_report(got, name):
    """max |delta| / frame peak and max rel-RMS per frame, as test_float32_within_the_float_tolerance."""
    w = R.oracle_pcm(name, F32).view(np.float32).astype(np.float64)
    g = got.view(np.float32).astype(np.float64)
    d = np.abs(g - w)
    peak = np.abs(w).max(axis=1)
    rms = np.sqrt((w ** 2).mean(axis=1))
    rel_peak = (d.max(axis=1) / np.maximum(peak, 1e-30)).max()
    rel_rms = (np.sqrt((d ** 2).mean(axis=1)) / np.maximum(rms, 1e-30)).max()
    print(f"{name} LSB1 float32: max |delta| {d.max():.4g} (int16 units), max |delta| / frame peak {rel_peak:.3g}, "
          f"max rel-RMS {rel_rms:.3g}")
    return rel_peak, rel_rms


# ---------------------------------------------------------------------------------------------
# independent layouts, partial max_sfb
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.INDEPENDENT)
def test_independent_layouts_exact(name, monkeypatch):
    for flags in (BE, LE, F32):
        _assert_identical(_host_entry(name, flags, EXACT, monkeypatch), name, flags)


@pytest.mark.parametrize("name", R.INDEPENDENT)
def test_independent_layouts_lsb1(name, monkeypatch):
    """The single-channel long and short transforms inside the stereo +-1 LSB kernel (mode 6)."""
    for flags in (BE, LE):
        d = _int16_delta(_host_entry(name, flags, LSB1, monkeypatch), name, flags)
        print(f"{name} LSB1 flags {flags:#x}: max |delta| {d} LSB")
        assert d <= 1, (flags, d)
    got = _host_entry(name, F32, LSB1, monkeypatch)
    rel_peak, rel_rms = _float_report(got, name)
    assert rel_peak <= FLOAT_TOL_PEAK, rel_peak
    assert rel_rms <= FLOAT_TOL_RMS, rel_rms
    assert (got != R.oracle_pcm(name, F32)).any()  # the fused kernel ran, not the exact one


@pytest.mark.parametrize("precision", [EXACT, LSB1])
def test_independent_layouts_through_the_device_entry(precision):
    """Without the hint the long-window instantiations (modes 0 / 4) meet the frames with one short
    channel, with it the mixed-window ones (modes 5 / 6)."""
    name = "independent_pns"
    outs = [_device_entry(name, BE, precision, hint) for hint in (False, True)]
    for got in outs:
        if precision == EXACT:
            _assert_identical(got, name, BE)
        else:
            assert _int16_delta(got, name, BE) <= 1
    if precision == EXACT:
        assert (outs[0] == outs[1]).all()


@pytest.mark.parametrize("name", R.PARTIAL)
def test_partial_max_sfb_exact(name, monkeypatch):
    """int16 bit-identical with the junk; float32 bit-identical without it, and with it equal sample
    for sample except the sign of a zero.

    Left out: float32 bit for bit WITH the junk.  The kernel gives a band that is not spectral the
    gain -0.0 (iq_channel: q is 0 there and -0.0 * -0.0 = +0.0, jaad_gpu.h requires q = 0 at and above
    swb_offset[max_sfb]), so a junk q > 0 there comes out as -0.0 where the reference, which never
    reads it, has +0.0.  Measured on MI355X: 19 (stereo 48 kHz), 10 (stereo 8 kHz) and 4 (mono) sign
    bytes of zero samples differ in the 120-frame batches; nothing else does.  A rare-path fix (uncoded bins read as +0.0 in the exact modes when max_sfb is
    below the band count) made all three batches bit-identical; it is not part of this change (see
    profiles/lc_records/README.md)."""
    _assert_identical(_host_entry(name, BE, EXACT, monkeypatch), name, BE)
    got = _host_entry(name, F32, EXACT, monkeypatch).view(np.float32)
    want = R.oracle_pcm(name, F32).view(np.float32)
    assert np.array_equal(got, want)  # (as numbers: -0.0 == +0.0)
    signs = got.view(np.uint32) != want.view(np.uint32)
    print(f"{name}: {int(signs.sum())} zero samples differ in sign from the restatement's")
    assert not want[signs].any()
    clean = name + "_clean"
    _assert_identical(_host_entry(clean, F32, EXACT, monkeypatch), clean, F32)


@pytest.mark.parametrize("name", R.PARTIAL)
def test_partial_max_sfb_lsb1(name, monkeypatch):
    d = _int16_delta(_host_entry(name, BE, LSB1, monkeypatch), name, BE)
    print(f"{name} LSB1: max |delta| {d} LSB")
    assert d <= 1, d
    rel_peak, rel_rms = _float_report(_host_entry(name, F32, LSB1, monkeypatch), name)
    assert rel_peak <= FLOAT_TOL_PEAK, rel_peak
    assert rel_rms <= FLOAT_TOL_RMS, rel_rms


# ---------------------------------------------------------------------------------------------
# gain range, full scale
# ---------------------------------------------------------------------------------------------
def test_every_scalefactor_value_exact(monkeypatch):
    """All 256 entries of the kernel's LDS gain table against JAAD_SCALEFACTOR_TABLE[sf + 100]."""
    _assert_identical(_host_entry("gain_walk", F32, EXACT, monkeypatch), "gain_walk", F32)


def test_full_scale_saturates_as_the_reference(monkeypatch):
    """Math.round and the short clamp (SampleBuffer.java:193-206): -32768 and +32767 come out where
    the restatement has them; the +-1 LSB kernel's conversion stays within its bar (it saturates at
    -32767)."""
    for flags in (BE, LE):
        got = _host_entry("full_scale", flags, EXACT, monkeypatch)
        _assert_identical(got, "full_scale", flags)
        v = got.view("<i2" if flags & LE else ">i2")
        assert (v == 32767).any() and (v == -32768).any()
    d = _int16_delta(_host_entry("full_scale", BE, LSB1, monkeypatch), "full_scale", BE)
    print(f"full_scale LSB1: max |delta| {d} LSB")
    assert d <= 1, d


def test_samples_far_past_int32_exact(monkeypatch):
    """Gains up to sf = 255 on |q| up to 8190: float32 bit-identical; int16 saturated as
    Math.round's int and then the short clamp saturate."""
    for flags in (F32, BE):
        _assert_identical(_host_entry("huge", flags, EXACT, monkeypatch), "huge", flags)


# ---------------------------------------------------------------------------------------------
# spec TNS
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [EXACT, LSB1])
def test_tns_shapes_spec(precision, monkeypatch):
    """Kernel mode 1 in either precision (spec TNS has no fused instantiation): stacked filters,
    orders 0 to 20, the tns_max / max_sfb / band-0 clamps, short frames with bare windows and with
    two filters on one, a long TNS channel next to a short one (synth_channel's TNS)."""
    _assert_identical(_host_entry("tns_shapes", F32, precision, monkeypatch), "tns_shapes", F32)


def test_tns_shapes_compat_through_the_device_entry():
    """The same records under the reference's TNS (a no-op): modes 0 and 5 per hint."""
    for hint in (False, True):
        _assert_identical(_device_entry("tns_shapes", F32, EXACT, hint, N.TNS_COMPAT), "tns_shapes", F32, N.TNS_COMPAT)


# ---------------------------------------------------------------------------------------------
# device parser
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.INDEPENDENT + R.PARTIAL)
def test_device_parser_records_equal_the_host_parser(name):
    from test_gparse_gpu import _assert_run_equal, _device, _host
    cfg, runs = R.written_runs(name)
    with N.DeviceParser(cfg) as gp:
        rec, got = _device(gp, [r[0] for r in runs], [r[1] for r in runs])
    assert (rec.frame_result == 0).all()
    g0 = 0
    for r, (frames, pns0, _) in enumerate(runs):
        want, pns = _host(cfg, frames, pns0)
        _assert_run_equal(got, g0, want)
        assert int(rec.state["pns_state"][r]) == pns
        g0 += len(frames)
