"""Device bitstream front end for HE-AAC on the GPU (include/jaad_gparse.h, jaad_gparse_batch_sbr):
core records in device memory, SBR records, per-frame statuses and parser state equal the host
parser's (jaad_parse_frame); edges of the scan and the gather kernel; continuation across calls and
across host / device parsing; frames cut short; refused frames; bitstream bytes to PCM."""
import ctypes as C
import faulthandler
import importlib.util
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from jaadec_amd import native as N
from oracle import oracle as O

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from gparse_sbr_streams import streams  # noqa: E402
from test_gparse_gpu import _assert_run_equal  # noqa: E402


@pytest.fixture(autouse=True)
def _time_limit():
    """A test here takes a few seconds; one that has not ended after a minute ends the process, so
    that nothing more is started on a GPU that may be hung."""
    faulthandler.dump_traceback_later(60, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _parsers(cfg, pns0s):
    out = []
    for s in pns0s:
        p = N.Parser(cfg)
        p.pns_state = s
        out.append(p)
    return out


def _host(cfg, frames, pns0, parser=None, **kw):
    """The host parser over one run: (Batch, the parser afterwards)."""
    P = parser or _parsers(cfg, [pns0])[0]
    return P.parse(list(frames), **kw), P


def _host_results(parser, frames):
    """jaad_parse_frame's status per frame (the state moves with 0 and EOS, as the parser moves it)."""
    out = []
    for f in frames:
        try:
            b = parser.parse([f], drop_eos=True)
            out.append(N.ERR_EOS if b.frame_status is not None else 0)
        except N.JaadError as e:
            out.append(e.status)
    return out


def _assert_same_state(a, b, probe):
    """Two parsers are in the same state: the LCG, and the records of the frames `probe` parsed
    next on copies (window shapes through window_shape_prev, the SBR / PS history through the
    time-delta coded envelopes)."""
    assert a.pns_state == b.pns_state
    sa, sb = a.snapshot(), b.snapshot()
    for f in probe:  # (a frame may be refused from this state: then by both)
        got = []
        for s in (sa, sb):
            try:
                x = s.parse([f], drop_eos=True)
                got.append((0, x.frame_status is not None, x.ics.tobytes(), x.sbr.tobytes()))
            except N.JaadError as e:
                got.append((e.status,))
        assert got[0] == got[1]
    sa.close()
    sb.close()


def _assert_equal(gp, rec, cfg, runs, parsers):
    """Device records of `runs` ((frames, pns0) each) against the host parser run by run."""
    got = gp.records_to_host(rec)
    g0 = 0
    for r, (frames, pns0) in enumerate(runs):
        want, P = _host(cfg, frames, pns0, drop_eos=True)
        skip = set(np.flatnonzero(want.frame_status).tolist()) if want.frame_status is not None else set()
        _assert_run_equal(got, g0, want, skip=skip)
        nf = len(frames)
        assert got.sbr[g0:g0 + nf].tobytes() == want.sbr.tobytes(), f"sbr records of run {r}"
        assert rec.frame_result[g0:g0 + nf].tolist() == [N.ERR_EOS if f in skip else 0 for f in range(nf)]
        _assert_same_state(parsers[r], P, frames[:6])
        g0 += nf


@pytest.mark.parametrize("extras", [0, 3], ids=["plain", "dse_fil_pulse"])
@pytest.mark.parametrize("cfgid", [4, 5])
def test_records_equal_the_host_parser(cfgid, extras):
    cfg, runs, b = streams(cfgid, extras)
    assert (b.sbr["status"] == N.SBR_UPSAMPLE).any()  # frames without a payload among them
    parsers = _parsers(cfg, [r[1] for r in runs])
    with N.SbrDeviceParser(cfg) as gp:
        rec = gp.parse_frames([list(r[0]) for r in runs], parsers)
        assert rec.status == N.OK and (rec.frame_result == 0).all()
        _assert_equal(gp, rec, cfg, runs, parsers)
        assert len(gp.last_ms()) == 6


@lru_cache(maxsize=None)
def _stereo65():
    cfg, runs, _ = streams(4, 0, frames=65, n_streams=1)
    return cfg, runs[0]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_frame_counts_around_a_wave(n):
    cfg, (frames, pns0) = _stereo65()
    parsers = _parsers(cfg, [pns0])
    with N.SbrDeviceParser(cfg) as gp:
        rec = gp.parse_frames([list(frames[:n])], parsers)
        _assert_equal(gp, rec, cfg, [(frames[:n], pns0)], parsers)


def test_runs_straddle_a_wave():
    cfg, runs, _ = streams(5, 0, frames=43, n_streams=3)
    parsers = _parsers(cfg, [r[1] for r in runs])
    with N.SbrDeviceParser(cfg) as gp:
        rec = gp.parse_frames([list(r[0]) for r in runs], parsers)
        _assert_equal(gp, rec, cfg, runs, parsers)


def test_scan_crosses_its_chunk_of_1024_frames():
    """The scan kernel takes 1024 frames a step: 87 runs of 12 frames carry the pool offsets over
    the step's edge, and every lane of the gather kernel finds its frame among 1044."""
    cfg, runs, _ = streams(4, 0)
    many = [runs[i % 2] for i in range(87)]
    parsers = _parsers(cfg, [r[1] for r in many])
    with N.SbrDeviceParser(cfg) as gp:
        rec = gp.parse_frames([list(r[0]) for r in many], parsers)
        got = gp.records_to_host(rec)
    assert rec.status == N.OK and (rec.frame_result == 0).all()
    want = [_host(cfg, *r)[0] for r in runs]
    for i in range(87):
        assert got.sbr[12 * i:12 * i + 12].tobytes() == want[i % 2].sbr.tobytes(), f"run {i}"
    _assert_run_equal(got, 12 * 85, want[1])
    _assert_run_equal(got, 12 * 86, want[0])


@pytest.mark.parametrize("every", [2, 1], ids=["every_second_frame", "no_frame"])
def test_frames_without_a_tail(every):
    """Zeros in the scan (every second frame carries no payload) and an empty pool (no frame does)."""
    cfg, runs, b = streams(4, 0, frames=10, n_streams=1, upsample_percent=0)
    pns0 = runs[0][1]
    one = b.select_runs([0])
    lc = O.write_frames(one, cfg.sf_index)  # the same core frames without any SBR payload
    w = O.SbrWriter(cfg.ext_sf_index, 3)
    frames = [lc[f] if f % every == every - 1 else O.write_frames(one, cfg.sf_index, frames=[f], sbr_writer=w)[0]
              for f in range(10)]
    parsers = _parsers(cfg, [pns0])
    with N.SbrDeviceParser(cfg) as gp:
        rec = gp.parse_frames([frames], parsers)
        _assert_equal(gp, rec, cfg, [(tuple(frames), pns0)], parsers)
    up = rec.batch.sbr["status"] == N.SBR_UPSAMPLE
    assert up[every - 1::every].all() and (every == 1 or not up[0::2].any())


def _shifted(frame, k):
    """The frame behind k empty fill elements (id_syn_ele 6, count 0: 7 bits each): every later
    element, the tail included, moves by 7k bits."""
    bits = 7 * k + 8 * len(frame)
    v = (int("1100000" * k, 2) if k else 0) << (8 * len(frame)) | int.from_bytes(frame, "big")
    pad = -bits % 8
    return (v << pad).to_bytes((bits + pad) // 8, "big")


@pytest.mark.parametrize("end_mod4", [1, 2, 3, 0])
@pytest.mark.parametrize("cfgid", [4, 5])
def test_gather_at_every_bit_and_byte_phase(cfgid, end_mod4):
    """Four runs of the same eight frames: frame i sits behind i empty fill elements, so the tails
    start at all 8 bit phases, and run r lies r bytes further (mod 4) than run 0, so each of them
    starts at all 4 byte phases of a dword.  The last frame ends exactly at data_bytes."""
    cfg, runs, _ = streams(cfgid, 0, frames=8, n_streams=1, upsample_percent=0)  # every frame has a tail
    frames, pns0 = runs[0]
    frames = [_shifted(f, i) for i, f in enumerate(frames)]
    want, P = _host(cfg, frames, pns0)
    blob, offs, lens = bytearray(), [], []
    for r in range(4):
        while len(blob) % 4 != r:
            blob.append(0xFF)
        for f in frames:
            offs.append(len(blob))
            lens.append(len(f))
            blob += f
    lead = (end_mod4 - len(blob)) % 4  # bytes in front: all offsets move alike
    blob = bytes([0xFF] * lead) + bytes(blob)
    assert len(blob) % 4 == end_mod4 and offs[-1] + lead + lens[-1] == len(blob)
    parsers = _parsers(cfg, [pns0] * 4)
    with N.SbrDeviceParser(cfg) as gp:
        rec = gp.parse_blob(np.frombuffer(blob, np.uint8), np.array(offs, np.uint64) + np.uint64(lead),
                            np.array(lens, np.uint32), np.arange(5, dtype=np.uint32) * 8, parsers)
        got = gp.records_to_host(rec)
    assert rec.status == N.OK and (rec.frame_result == 0).all()
    for r in range(4):
        _assert_run_equal(got, 8 * r, want)
        assert got.sbr[8 * r:8 * r + 8].tobytes() == want.sbr.tobytes(), f"run {r}"
        _assert_same_state(parsers[r], P, frames[:6])


@pytest.mark.parametrize("cfgid", [4, 5])
def test_continuation_across_calls_and_from_the_host_parser(cfgid):
    cfg, runs, _ = streams(cfgid, 0, frames=30, n_streams=1)
    frames, pns0 = runs[0]
    want, P = _host(cfg, frames, pns0)
    wa, wb = want.split_frames(11)
    with N.SbrDeviceParser(cfg) as gp:
        whole = _parsers(cfg, [pns0])
        rec = gp.parse_frames([list(frames)], whole)
        _assert_equal(gp, rec, cfg, [(frames, pns0)], whole)
        # 11 + 19 frames on the same parser: time-delta coded envelopes and the PS history cross the seam
        two = _parsers(cfg, [pns0])
        a = gp.records_to_host(gp.parse_frames([list(frames[:11])], two))
        b = gp.records_to_host(gp.parse_frames([list(frames[11:])], two))
        for got, w in ((a, wa), (b, wb)):
            _assert_run_equal(got, 0, w)
            assert got.sbr.tobytes() == w.sbr.tobytes()
        _assert_same_state(two[0], P, frames[:6])
        # a host-parsed segment, then a device-parsed one
        mixed = _parsers(cfg, [pns0])
        ha = mixed[0].parse(list(frames[:11]))
        assert ha.sbr.tobytes() == wa.sbr.tobytes()
        b = gp.records_to_host(gp.parse_frames([list(frames[11:])], mixed))
        _assert_run_equal(b, 0, wb)
        assert b.sbr.tobytes() == wb.sbr.tobytes()
        _assert_same_state(mixed[0], P, frames[:6])


def _upload(batch):
    """A host Batch as device tensors for Context.decode_device."""
    import torch
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k)).view(np.uint8).reshape(-1)).cuda()
         for k in ("q", "sf", "cb", "ics", "ms_used", "tns") if getattr(batch, k) is not None}
    return t, {k: v.data_ptr() for k, v in t.items()}


def _decode_device(cfg, dev, batch, flags, n_slots=1):
    import torch
    nf = batch.n_frames
    nb = N.lib().jaad_frame_pcm_bytes(C.byref(cfg), flags)
    pcm = torch.zeros((nf, nb), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with N.Context(cfg, n_slots) as ctx:
        ctx.decode_device(dev, batch, pcm.data_ptr(), nf * nb, flags | N.HINT_SHORT_WINDOWS)
        ctx.wait()
    return pcm.cpu().numpy()


def _pcm_host_path(cfg, batch, flags, n_slots=1):
    keep, dev = _upload(batch)
    return _decode_device(cfg, dev, batch, flags, n_slots)


def _cut_after_the_payload(cfg, frames, pns0, at):
    """frames[at] behind as many empty fill elements as make its SBR fill element end on a byte, and
    without its last byte: the payload is whole, the END element is gone."""
    for k in range(8):
        f = _shifted(frames[at], k)[:-1]
        P = _parsers(cfg, [pns0])[0]
        P.parse(list(frames[:at]), drop_eos=True)
        b = P.parse([f], drop_eos=True)
        if b.frame_status is not None and b.sbr[0]["status"] == N.SBR_OK and b.sbr.tobytes() != bytes(b.sbr.nbytes):
            return f
    raise AssertionError("no shift puts the END element alone into the last byte")


@pytest.mark.parametrize("cfgid", [4, 5])
def test_frames_cut_short_are_dropped_as_the_host_parser_drops_them(cfgid):
    """Frame 6 ends after its whole SBR payload (EOS with the payload's record, header kept); frame
    9 ends inside the core (EOS, zero record; the last one: the frame after a dropped one finds its
    time-delta coded envelopes without their base).  The decode with that frame_status gives the
    PCM of the host-parser path."""
    cfg, runs, _ = streams(cfgid, 0, frames=10, n_streams=1, upsample_percent=0)
    frames, pns0 = runs[0]
    frames = list(frames)
    frames[9] = frames[9][:6]
    frames[6] = _cut_after_the_payload(cfg, frames, pns0, 6)
    want, P = _host(cfg, frames, pns0, drop_eos=True)
    assert want.frame_status.tolist() == [int(f in (6, 9)) for f in range(10)]
    assert want.sbr[9].tobytes() == bytes(N.SBR_FRAME_DTYPE.itemsize) and want.sbr[6]["status"] == N.SBR_OK
    parsers = _parsers(cfg, [pns0])
    with N.SbrDeviceParser(cfg) as gp:
        rec = gp.parse_frames([frames], parsers)
        assert rec.status == N.OK and rec.batch.frame_status.tolist() == want.frame_status.tolist()
        _assert_equal(gp, rec, cfg, [(tuple(frames), pns0)], parsers)
        got = _decode_device(cfg, rec.dev, rec.batch, N.PCM_BIG_ENDIAN)
    assert got.tobytes() == _pcm_host_path(cfg, want, N.PCM_BIG_ENDIAN).tobytes()


def _payload_that_ends_inside_its_fill_element(cfg, frames, pns0, at):
    """frames[at] with one bit of its last 40 bytes flipped so that the host parser meets the end of
    the SBR payload's bytes inside the payload (JAAD_ERR_UNSUPPORTED)."""
    f = frames[at]
    P = _parsers(cfg, [pns0])[0]
    P.parse(list(frames[:at]))
    for bit in range(8 * len(f) - 1, 8 * (len(f) - 40), -1):
        m = bytearray(f)
        m[bit >> 3] ^= 0x80 >> (bit & 7)
        if _host_results(P.snapshot(), [bytes(m)]) == [N.ERR_UNSUPPORTED]:
            return bytes(m)
    raise AssertionError("no single bit flip ends the payload early")


def _refused(cfgid, which):
    cfg, runs, _ = streams(cfgid, 0, frames=8, n_streams=1, upsample_percent=0)
    frames, pns0 = runs[0]
    frames = list(frames)
    if which == "cut_in_payload":  # the fill element's own length check fails: the host says EOS or refuses
        frames[5] = frames[5][:-3]
    elif which == "payload_ends_early":
        frames[5] = _payload_that_ends_inside_its_fill_element(cfg, frames, pns0, 5)
    elif which == "cpe_after_payload":  # a second channel element where END was: id 1
        f = bytearray(_cut_after_the_payload(cfg, frames, pns0, 5))
        frames[5] = bytes(f) + bytes([0b00100000, 0, 0, 0])
    else:  # codebook 12 in the core (tests/test_parse.py)
        bits = "000" + "0000" + "10000010" + "0" + "00" + "0" + "110001" + "0" + "1100" + "00001"
        frames[5] = int(bits.ljust(64, "0"), 2).to_bytes(8, "big")
    return cfg, frames, pns0


@pytest.mark.parametrize("which", ["cut_in_payload", "payload_ends_early", "cpe_after_payload", "codebook_12"])
def test_refused_frames_report_the_host_status_and_leave_the_parsers(which):
    cfgid = 5  # mono: a CPE is a wrong element
    cfg, frames, pns0 = _refused(cfgid, which)
    host = _host_results(_parsers(cfg, [pns0])[0], frames)
    want = {"payload_ends_early": N.ERR_UNSUPPORTED, "cpe_after_payload": N.ERR_UNSUPPORTED,
            "codebook_12": N.ERR_BITSTREAM}.get(which, host[5])
    assert host[5] == want and [h for i, h in enumerate(host) if i != 5] == [0] * 7
    parsers = _parsers(cfg, [pns0])
    parsers[0].parse(frames[:1])  # not a fresh parser: there is SBR history to keep
    before = parsers[0].snapshot()
    host = _host_results(before.snapshot(), frames[1:])
    with N.SbrDeviceParser(cfg) as gp:
        rec = gp.parse_frames([frames[1:]], parsers, check=False)
    assert rec.frame_result.tolist() == host
    failed = [h for h in host if h not in (0, N.ERR_EOS)]
    assert rec.status == (failed[0] if failed else N.OK)
    if failed:
        _assert_same_state(parsers[0], before, frames[1:7])


def _golden(name):
    spec = importlib.util.spec_from_file_location("make_golden", HERE / "golden" / "make_golden.py")
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg.load(HERE / "golden" / f"{name}.npz")


@pytest.mark.parametrize("name", ["c4_sbr_stereo_f32", "c5_sbr_ps_be"])
def test_bytes_to_the_golden_pcm(name):
    """The golden batch written as raw_data_blocks, parsed on the device and by the host tail
    stage, decoded by decode_device: the golden PCM, and the PCM of host parse + decode_device."""
    b, cfg, flags, pcm = _golden(name)
    n_runs = len(b.stream_slot)
    runs, hosts = [], []
    for r in range(n_runs):
        one = b.select_runs([r])
        frames = O.write_frames(one, cfg.sf_index, sbr_writer=O.SbrWriter(cfg.ext_sf_index, 1))
        runs.append((frames, int(one.ics["pns_state"][0])))
    parsers = _parsers(cfg, [r[1] for r in runs])
    with N.SbrDeviceParser(cfg) as gp:
        rec = gp.parse_frames([r[0] for r in runs], parsers, slots=b.stream_slot)
        got = _decode_device(cfg, rec.dev, rec.batch, flags, int(b.stream_slot.max()) + 1)
        host = gp.records_to_host(rec)
    assert got.tobytes() == pcm.tobytes()
    assert got.tobytes() == _pcm_host_path(cfg, host, flags, int(b.stream_slot.max()) + 1).tobytes()
    g0 = 0
    for frames, pns0 in runs:  # and those records are the host parser's
        want, _ = _host(cfg, frames, pns0)
        _assert_run_equal(host, g0, want)
        assert host.sbr[g0:g0 + len(frames)].tobytes() == want.sbr.tobytes()
        g0 += len(frames)


@pytest.mark.parametrize("cfgid,flags", [(4, N.PCM_BIG_ENDIAN), (4, N.PCM_FLOAT32), (5, N.PCM_BIG_ENDIAN)],
                         ids=["c4_int16", "c4_float32", "c5_int16"])
def test_bytes_to_pcm_equal_host_parse_and_decode_device(cfgid, flags):
    cfg, runs, _ = streams(cfgid, 3)
    parsers = _parsers(cfg, [r[1] for r in runs])
    with N.SbrDeviceParser(cfg) as gp:
        rec = gp.parse_frames([list(r[0]) for r in runs], parsers)
        got = _decode_device(cfg, rec.dev, rec.batch, flags, len(runs))
    want = None
    for r, (frames, pns0) in enumerate(runs):
        hb, _ = _host(cfg, frames, pns0)
        hb.stream_slot[:] = r
        one = _pcm_host_path(cfg, hb, flags, len(runs))
        want = one if want is None else np.concatenate([want, one])
    assert np.abs(got.view(np.int8)).max() > 0
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("cfgid", [4, 5])
def test_adts_streams_with_implicit_sbr_equal_the_decoder_facade(cfgid):
    from jaadec_amd.batch import decode_adts_streams
    from jaadec_amd.decoder import ADTSDemultiplexer, Decoder, SampleBuffer
    cfg, runs, _ = streams(cfgid, 0, upsample_percent=0)
    data = [O.adts_wrap(list(frames), cfg.sf_index, cfg.channel_config) for frames, _ in runs]
    got = decode_adts_streams(data, N.PCM_BIG_ENDIAN, implicit_sbr=True)
    for stream, pcm in zip(data, got):
        demux = ADTSDemultiplexer(stream)
        dec = Decoder.create(demux.getDecoderInfo())
        payloads = []
        while True:
            try:
                payloads.append(demux.readNextFrame())
            except EOFError:
                break
        bufs = [SampleBuffer() for _ in payloads]
        dec.decodeFrames(payloads, bufs)  # no PNS bands in C4 / C5: the parser's LCG start is moot
        dec.close()
        assert pcm.shape == (len(payloads), 2048 * 2 * 2)
        assert pcm.tobytes() == b"".join(x.data for x in bufs)
    with pytest.raises(N.JaadError) as e:  # the default is the parent's behaviour: an SBR payload is refused
        decode_adts_streams(data, N.PCM_BIG_ENDIAN)
    assert e.value.status == N.ERR_UNSUPPORTED


def test_a_parser_object_of_the_other_create_is_refused_before_any_launch():
    import torch
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    out = dict(q=p, sf=p, cb=p, ics=p, ms_used=p)
    fb = np.array([0, 1], np.uint32)
    sbr_cfg, lc_cfg = N.make_cfg(6, 2, sbr=True), N.make_cfg(6, 2)
    with N.SbrDeviceParser(sbr_cfg) as gs, N.DeviceParser(lc_cfg) as gl:
        st = N.gparse_state(1)
        assert N.DeviceParser.parse(gs, fb, p, 64, p, p, st, out)[0] == N.ERR_INVALID_ARG
        assert st.tobytes() == N.gparse_state(1).tobytes()
        P = N.Parser(sbr_cfg)
        assert N.SbrDeviceParser.parse(gl, fb, p, 64, p, p, [P], out)[0] == N.ERR_INVALID_ARG
        assert N.SbrDeviceParser.parse(gs, fb, p, 64, p, p, [N.Parser(N.make_cfg(6, 2))], out)[0] == N.ERR_INVALID_ARG
        assert P.pns_state == N.PNS_STATE0
    assert not d.any().item()
