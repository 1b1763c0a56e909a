"""Device bitstream front end on the GPU (include/jaad_gparse.h): the records jaad_gparse_batch
leaves in device memory equal the host parser's (jaad_parse_frame) byte for byte, per-frame status
included; wave and chunk edges of the two kernels; continuation across calls; frames whose
bitstream ends early; refused frames; bitstream bytes to the golden PCM."""
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from jaadec_amd import native as N
from oracle import oracle as O

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_parse import CASES  # noqa: E402  (the host parser's round-trip cases)


@lru_cache(maxsize=None)
def _streams(cfgid, extras, over):
    """(cfg, per run: frames, pns0) of a synthetic batch written as raw_data_blocks."""
    p = N.synth_params(cfgid, **dict(over))
    b = N.synth_batch(p)
    runs = []
    for r in range(len(b.stream_slot)):
        one = b.select_runs([r])
        runs.append((tuple(O.write_frames(one, p.sf_index, extras=extras)), int(one.ics["pns_state"][0])))
    return N.cfg_for(p), tuple(runs)


def _host(cfg, frames, pns0, **kw):
    P = N.Parser(cfg)
    P.pns_state = pns0
    b = P.parse(list(frames), **kw)
    pns = P.pns_state
    P.close()
    return b, pns


def _nbands(ic):
    ng = 8 - bin(int(ic["grouping"]) & 0x7F).count("1") if ic["window_sequence"] == N.EIGHT_SHORT_SEQUENCE else 1
    return ng * int(ic["max_sfb"])


def _assert_run_equal(got, g0, want, skip=()):
    """Frames [g0, g0 + want.n_frames) of the device batch `got` against the host batch `want`."""
    nch, nf = want.nch, want.n_frames
    keep = np.array([f not in skip for f in range(nf)])
    ck = np.repeat(keep, nch)
    c0 = g0 * nch
    for name in ("q", "sf", "cb"):
        a, b = getattr(got, name)[c0:c0 + nf * nch][ck], getattr(want, name)[ck]
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{name} differs at {bad[:4].tolist()}"
    a, b = got.ics[c0:c0 + nf * nch][ck], want.ics[ck]
    assert a.tobytes() == b.tobytes(), f"ics differs at {np.flatnonzero(a != b)[:4].tolist()}"
    if want.ms_used is not None:  # bits beyond the frame's bands carry no meaning
        for f in np.flatnonzero(keep):
            n = _nbands(want.ics[2 * f])
            for i in range(2):
                m = (1 << min(max(n - 64 * i, 0), 64)) - 1
                assert int(got.ms_used[g0 + f, i]) & m == int(want.ms_used[f, i]) & m, f"ms_used frame {f}"
    gt = got.tns[c0:c0 + nf * nch][ck]
    wt = want.tns[ck] if want.tns is not None else np.zeros(int(ck.sum()), N.TNS_DTYPE)
    assert gt.tobytes() == wt.tobytes(), "tns differs"


def _device(gp, runs, pns0s, state=None):
    st = N.gparse_state(len(runs), pns0s) if state is None else state
    rec = gp.parse_frames([list(r) for r in runs], st)
    return rec, gp.records_to_host(rec)


@pytest.mark.parametrize("extras", [0, 3], ids=["plain", "dse_fil_pulse"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_records_equal_the_host_parser(case, extras):
    cfgid, over = CASES[case]
    cfg, runs = _streams(cfgid, extras, tuple(sorted(over.items())))
    with N.DeviceParser(cfg) as gp:
        rec, got = _device(gp, [r[0] for r in runs], [r[1] for r in runs])
    assert (rec.frame_result == 0).all()
    g0 = 0
    for r, (frames, pns0) in enumerate(runs):
        want, pns = _host(cfg, frames, pns0)
        _assert_run_equal(got, g0, want)
        assert int(rec.state["pns_state"][r]) == pns
        g0 += len(frames)


@lru_cache(maxsize=None)
def _stereo65():
    cfg, runs = _streams(3, 0, (("frames_per_stream", 65), ("n_streams", 1), ("pns_percent", 8)))
    frames, pns0 = runs[0]
    return cfg, frames, pns0, _host(cfg, frames, pns0)[0]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_frame_counts_around_a_wave(n):
    cfg, frames, pns0, want = _stereo65()
    with N.DeviceParser(cfg) as gp:
        rec, got = _device(gp, [frames[:n]], [pns0])
    first, _ = want.split_frames(n)
    _assert_run_equal(got, 0, first)


def test_runs_straddle_a_wave_of_the_frame_kernel():
    cfg, runs = _streams(3, 0, (("frames_per_stream", 43), ("n_streams", 3), ("pns_percent", 8)))
    with N.DeviceParser(cfg) as gp:
        rec, got = _device(gp, [r[0] for r in runs], [r[1] for r in runs])
    for r, (frames, pns0) in enumerate(runs):
        want, pns = _host(cfg, frames, pns0)
        _assert_run_equal(got, 43 * r, want)
        assert int(rec.state["pns_state"][r]) == pns


def test_link_scan_crosses_two_chunks_of_a_mono_run():
    cfg, runs = _streams(1, 0, (("frames_per_stream", 150), ("n_streams", 1), ("pns_percent", 8), ("window_switching", 1)))
    frames, pns0 = runs[0]
    want, pns = _host(cfg, frames, pns0)
    assert (want.ics["flags"] & N.ICS_HAS_PNS).sum() > 20  # the LCG does move along the run
    with N.DeviceParser(cfg) as gp:
        rec, got = _device(gp, [frames], [pns0])
    _assert_run_equal(got, 0, want)
    assert int(rec.state["pns_state"][0]) == pns


def test_continuation_across_two_calls():
    cfg, runs = _streams(3, 0, (("frames_per_stream", 30), ("n_streams", 1), ("pns_percent", 8), ("window_switching", 1)))
    frames, pns0 = runs[0]
    want, pns = _host(cfg, frames, pns0)
    with N.DeviceParser(cfg) as gp:
        _, whole = _device(gp, [frames], [pns0])
        st = N.gparse_state(1, pns0)
        _, a = _device(gp, [frames[:11]], None, st)
        _, b = _device(gp, [frames[11:]], None, st)
    _assert_run_equal(whole, 0, want)
    wa, wb = want.split_frames(11)
    _assert_run_equal(a, 0, wa)
    _assert_run_equal(b, 0, wb)
    assert int(st["pns_state"][0]) == pns


def test_frames_that_end_early_are_dropped_and_move_the_state():
    """Three truncated frames of a 12-frame stereo PNS run without a common window: 5 bytes end
    inside the left channel's section data, half the frame inside spectral data, 4 bytes right
    after the left ics_info (id 3 + tag 4 + common_window 1 + global_gain 8 + ics_info 11 or 15
    bits: the left shape is read, the right one is not)."""
    import torch
    cfg, runs = _streams(3, 0, (("common_window", 0), ("frames_per_stream", 13), ("ms_mode", 0), ("n_streams", 1),
                                ("pns_percent", 8), ("window_switching", 1)))
    frames, pns0 = runs[0]
    frames = list(frames)
    frames[2] = frames[2][:5]
    frames[6] = frames[6][:len(frames[6]) // 2]
    frames[9] = frames[9][:4]
    last = frames.pop()  # parsed afterwards: it shows the window shapes the run left
    P = N.Parser(cfg)
    P.pns_state = pns0
    want = P.parse(frames, drop_eos=True)
    pns = P.pns_state
    want_last = P.parse([last])
    P.close()
    assert want.frame_status.tolist() == [int(i in (2, 6, 9)) for i in range(12)]
    with N.DeviceParser(cfg) as gp:
        rec, got = _device(gp, [frames], [pns0])
        assert rec.status == N.OK
        assert rec.frame_result.tolist() == [N.ERR_EOS if i in (2, 6, 9) else 0 for i in range(12)]
        assert rec.batch.frame_status.tolist() == want.frame_status.tolist()
        _assert_run_equal(got, 0, want, skip=(2, 6, 9))
        assert int(rec.state["pns_state"][0]) == pns
        _, got_last = _device(gp, [[last]], None, rec.state)
        _assert_run_equal(got_last, 0, want_last)
        # decoded with that frame_status: the PCM of the host-parser path
        nb = N.pcm_frame_bytes(N.PCM_BIG_ENDIAN)
        pcm = torch.zeros((12, nb), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with N.Context(cfg, 1) as ctx:
            ctx.decode_device(rec.dev, rec.batch, pcm.data_ptr(), 12 * nb, N.PCM_BIG_ENDIAN | N.HINT_SHORT_WINDOWS)
            ctx.wait()
        with N.Context(cfg, 1) as ctx:
            ref = ctx.decode(want, N.PCM_BIG_ENDIAN)
    assert pcm.cpu().numpy().tobytes() == ref.tobytes()


def _host_statuses(cfg, frames, pns0):
    P = N.Parser(cfg)
    P.pns_state = pns0
    out = []
    for f in frames:
        try:
            P.parse([f])
            out.append(0)
        except N.JaadError as e:
            out.append(e.status)
    P.close()
    return out


@pytest.mark.parametrize("which", ["codebook_12", "cpe_in_mono"])
def test_refused_frames_report_the_host_status_and_leave_the_state(which):
    cfg, runs = _streams(1, 0, (("frames_per_stream", 8), ("n_streams", 1), ("pns_percent", 8), ("sf_index", 4)))
    frames, pns0 = runs[0]
    frames = list(frames)
    if which == "codebook_12":  # tests/test_parse.py test_reserved_codebook_and_unsupported_elements
        bits = "000" + "0000" + "10000010" + "0" + "00" + "0" + "110001" + "0" + "1100" + "00001"
        want = N.ERR_BITSTREAM
    else:
        bits = "001" + "0000"
        want = N.ERR_UNSUPPORTED
    frames[5] = int(bits.ljust(64, "0"), 2).to_bytes(8, "big")
    host = _host_statuses(cfg, frames, pns0)
    assert host == [0, 0, 0, 0, 0, want, 0, 0]
    st = N.gparse_state(1, pns0)
    st["window_shape"][0] = (1, 0)
    before = st.copy()
    with N.DeviceParser(cfg) as gp:
        rec = gp.parse_frames([frames], st, check=False)
    assert rec.frame_result.tolist() == host
    assert rec.status == want
    assert st.tobytes() == before.tobytes()


def test_frames_reaching_past_the_buffer_are_cut_off_there():
    """jaad_gparse.h: a frame whose length reaches past data_bytes is parsed as cut off at the
    buffer's end (here: its own end, so it parses), one that starts past it as an empty frame
    (JAAD_ERR_EOS, as jaad_parse_frame answers zero bytes)."""
    cfg, runs = _streams(2, 0, (("frames_per_stream", 6), ("n_streams", 2)))
    frames, pns0 = runs[0]
    want, _ = _host(cfg, frames, pns0)
    blob = np.frombuffer(b"".join(frames), np.uint8).copy()
    lens = np.array([len(f) for f in frames], np.uint32)
    offs = np.zeros(6, np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    lens[5] += 1000
    offs = np.append(offs, np.uint64(blob.nbytes + 5))
    lens = np.append(lens, np.uint32(100))
    with N.DeviceParser(cfg) as gp:
        rec = gp.parse_blob(blob, offs, lens, np.array([0, 7], np.uint32), N.gparse_state(1, pns0))
        got = gp.records_to_host(rec)
    assert rec.status == N.OK
    assert rec.frame_result.tolist() == [0] * 6 + [N.ERR_EOS]
    _assert_run_equal(got, 0, want)


def test_invalid_sizes_are_refused_before_any_launch():
    cfg, runs = _streams(2, 0, (("frames_per_stream", 6), ("n_streams", 2)))
    import torch
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    out = dict(q=p, sf=p, cb=p, ics=p, ms_used=p)
    with N.DeviceParser(cfg) as gp:
        st = N.gparse_state(2)
        assert gp.parse(np.array([0, 3, 2], np.uint32), p, 64, p, p, st, out)[0] == N.ERR_INVALID_ARG  # not monotone
        assert gp.parse(np.array([0, 0, 0], np.uint32), p, 64, p, p, st, out)[0] == N.ERR_INVALID_ARG  # zero frames
        assert gp.parse(np.array([0, 1, 2], np.uint32), p, 64, p, p, st, dict(out, ms_used=None))[0] == N.ERR_INVALID_ARG
        assert gp.parse(np.array([0, 1, 2], np.uint32), p, 0, p, p, st, out)[0] == N.ERR_INVALID_ARG
    assert st.tobytes() == N.gparse_state(2).tobytes()


def test_adts_bytes_to_the_golden_pcm():
    from jaadec_amd.batch import decode_adts_streams
    z = np.load(GOLD / "c3_adts_stream.npz", allow_pickle=False)
    sf_index, chc, pns0, nframes = (int(v) for v in z["meta"])
    (pcm,) = decode_adts_streams([z["data"].tobytes()], N.PCM_BIG_ENDIAN, pns_state=pns0)
    assert pcm.shape[0] == nframes
    assert pcm.tobytes() == z["pcm"].tobytes()


def test_raw_frame_to_the_golden_pcm():
    import torch
    z = np.load(GOLD / "c1_raw_frame.npz", allow_pickle=False)
    sf_index, chc, pns0, nframes = (int(v) for v in z["meta"])
    cfg = N.make_cfg(sf_index=sf_index, channel_config=chc)
    nb = N.pcm_frame_bytes(N.PCM_BIG_ENDIAN)
    with N.DeviceParser(cfg) as gp, N.Context(cfg, 1) as ctx:
        rec = gp.parse_frames([[z["data"].tobytes()]], N.gparse_state(1, pns0))
        pcm = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.decode_device(rec.dev, rec.batch, pcm.data_ptr(), nb, N.PCM_BIG_ENDIAN | N.HINT_SHORT_WINDOWS)
        ctx.wait()
    assert pcm.cpu().numpy().tobytes() == z["pcm"].tobytes()
