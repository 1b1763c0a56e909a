"""The record builders of tests/lc_records.py, checked without a GPU: each batch contains the cases
it is meant to (asserted on the records and on the C restatement's output), the restatement ignores
the junk the partial_max_sfb batches carry, and every batch is one a bitstream can hold: written as
raw_data_blocks by the test writer, the host parser -- and the parse core it shares with the device
parser, under ASan + UBSan -- gives the records back."""
import re
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from jaadec_amd import native as N
from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lc_records as R  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
LONG, START, SHORT, STOP = R.LONG, R.START, R.SHORT, R.STOP

BATCHES = R.CASES
batch = R.records


def oracle_f32(name, tns_mode=None) -> np.ndarray:
    return R.oracle_pcm(name, N.PCM_FLOAT32, tns_mode).view(np.float32).reshape(batch(name).batch.n_frames, -1)


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_every_batch_decodes_and_is_deterministic(name):
    rec = batch(name)
    assert np.isfinite(oracle_f32(name)).all()  # (O.decode_batch raises on a status other than OK)
    again = BATCHES[name]().batch
    for k in ("q", "sf", "cb", "ics", "ms_used", "tns"):
        a, b = getattr(again, k), getattr(rec.batch, k)
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), k
    b = rec.batch
    assert 4 <= len(b.stream_slot) <= 6 and all(16 <= int(n) <= 24 for n in np.diff(b.frame_begin))


@pytest.mark.parametrize("name", R.INDEPENDENT)
def test_independent_layouts_cover_the_channel_pairings(name):
    rec = batch(name)
    ics = rec.batch.ics.reshape(-1, 2)
    L, Rt = ics[:, 0], ics[:, 1]
    assert not (rec.batch.ics["flags"] & (N.ICS_COMMON_WINDOW | N.ICS_MS_PRESENT)).any()
    assert not rec.batch.ms_used.any()
    sl, sr = L["window_sequence"] == SHORT, Rt["window_sequence"] == SHORT
    assert (sl & ~sr).any() and (~sl & sr).any()  # exactly one channel short: synth_channel per channel
    assert (~sl & ~sr & (L["max_sfb"] != Rt["max_sfb"])).any()
    assert (sl & sr & (L["grouping"] != Rt["grouping"])).any()
    same = sl & sr & (L["grouping"] == Rt["grouping"]) & (L["max_sfb"] == Rt["max_sfb"])
    assert same.any()  # the lockstep short path next to the others
    for c in (L, Rt):
        assert set(c["window_sequence"].tolist()) == {LONG, START, SHORT, STOP}
    # each channel's own shape chain
    b = rec.batch
    for r in range(len(b.stream_slot)):
        run = ics[int(b.frame_begin[r]):int(b.frame_begin[r + 1])]
        for c in range(2):
            assert run["window_shape_prev"][0, c] == 0
            assert (run["window_shape_prev"][1:, c] == run["window_shape"][:-1, c]).all()
    assert (L["window_shape"] != Rt["window_shape"]).any()
    if name == "independent_is":
        off_idx = [(f, i) for f in range(len(Rt)) for i in range(R.n_bands(Rt[f]))
                   if b.cb[2 * f + 1, i] in (N.INTENSITY_HCB, N.INTENSITY_HCB2)]
        assert len(off_idx) > 50 and (Rt["flags"] & N.ICS_HAS_IS).any() and not (L["flags"] & N.ICS_HAS_IS).any()
        # I/S bands in frames where the two layouts differ: the right channel's index is not the left one's
        assert any(sl[f] != sr[f] or L["max_sfb"][f] != Rt["max_sfb"][f] for f, _ in off_idx)
    if name == "independent_pns":
        assert (L["flags"] & N.ICS_HAS_PNS).any() and (Rt["flags"] & N.ICS_HAS_PNS).any()
        assert len(set(b.ics["pns_state"].tolist())) > 20  # the LCG moves: left, then right, frame by frame


@pytest.mark.parametrize("name", R.PARTIAL)
def test_partial_max_sfb_covers_the_band_counts_and_groupings(name):
    rec = batch(name)
    b = rec.batch
    offs = R.band_tables(rec.sf_index)
    ics = b.ics[::b.nch]
    for short in (False, True):
        nswb = len(offs[int(short)]) - 1
        got = set(ics["max_sfb"][(ics["window_sequence"] == SHORT) == short].tolist())
        assert {0, 1, nswb - 1, nswb} <= got, (short, got)
        assert any(v % 2 for v in got - {1, nswb - 1, nswb}) and any(v % 2 == 0 for v in got - {0, nswb - 1, nswb})
    groups = {len(R.group_lengths(ic)) for ic in ics if ic["window_sequence"] == SHORT}
    assert groups == set(range(1, 9)), groups
    if b.nch == 2:
        assert (b.ics["flags"][0::2] & N.ICS_MS_PRESENT).all() and (b.ics["flags"] & N.ICS_COMMON_WINDOW).all()
        assert (b.ics["flags"][1::2] & N.ICS_HAS_IS).any()
    else:
        assert (b.ics["flags"] & N.ICS_HAS_PNS).any()


@pytest.mark.parametrize("name", R.PARTIAL)
def test_the_restatement_ignores_the_junk(name):
    """q above offsets[max_sfb] and ms_used bits from groups*max_sfb up: the restatement's output is
    the same with them random and with them zero -- and they are there."""
    rec, clean = batch(name), batch(name + "_clean")
    b, c = rec.batch, clean.batch
    assert (b.q != c.q).sum() > 1000
    if b.nch == 2:
        assert (b.ms_used != c.ms_used).any()
        for f in range(b.n_frames):
            nb = R.n_bands(b.ics[2 * f])
            assert np.array_equal(R.mask_ms(b.ms_used[f], nb), c.ms_used[f])
    for k in ("sf", "cb", "ics"):
        assert getattr(b, k).tobytes() == getattr(c, k).tobytes()
    assert np.array_equal(oracle_f32(name).view(np.uint32), oracle_f32(name + "_clean").view(np.uint32))


def _spectral_sf(rec):
    b = rec.batch
    vals = []
    for cf in range(len(b.ics)):
        nb = R.n_bands(b.ics[cf])
        cb = b.cb[cf, :nb]
        vals.append(b.sf[cf, :nb][(cb > 0) & (cb < N.NOISE_HCB)])
    return np.concatenate(vals)


def test_gain_walk_uses_every_scalefactor_value():
    rec = batch("gain_walk")
    assert set(_spectral_sf(rec).tolist()) == set(range(256))
    assert np.isfinite(oracle_f32("gain_walk")).all()


def test_full_scale_peaks_sit_just_past_int16():
    rec = batch("full_scale")
    f32 = oracle_f32("full_scale")
    peaks = R.frame_peaks(rec, f32)
    print(f"full_scale frame peaks: {peaks.min():.1f} .. {peaks.max():.1f}")
    assert (peaks <= 40000).all() and (peaks > 32768).all()
    b = rec.batch
    for r in range(len(b.stream_slot)):
        run = f32[int(b.frame_begin[r]):int(b.frame_begin[r + 1])]
        # Math.round then the short clamp: >= 32767.5 and < -32768.5 are clipped
        assert (run >= 32767.5).sum() >= 1 and (run < -32768.5).sum() >= 1, r
    i16 = O.decode_batch(rec.cfg(), b, O.Streams(rec.n_slots), N.PCM_BIG_ENDIAN).view(">i2")
    assert (i16 == 32767).any() and (i16 == -32768).any()


def test_huge_is_finite_and_past_int32():
    rec = batch("huge")
    f32 = oracle_f32("huge")
    assert np.isfinite(f32).all()
    assert (np.abs(f32) > 2.0 ** 31).any()
    sf = _spectral_sf(rec)
    assert sf.max() == 255 and sf.min() >= 200
    assert np.abs(rec.batch.q).max() > 4096
    i16 = O.decode_batch(rec.cfg(), rec.batch, O.Streams(rec.n_slots), N.PCM_BIG_ENDIAN).view(">i2")
    assert (i16 == 32767).any() and (i16 == -32768).any()


def test_tns_shapes_cover_the_filter_cases():
    rec = batch("tns_shapes")
    b = rec.batch
    tmax = R.TNS_MAX_SFB[rec.sf_index]
    assert rec.tns_mode == N.TNS_SPEC
    orders, stacks, flagsets = set(), set(), set()
    cut_tns_max = cut_max_sfb = into_band0 = bare_window = two_on_short = 0
    mixed_pair = 0
    for cf in np.flatnonzero(b.ics["flags"] & N.ICS_TNS):
        ic, t = b.ics[cf], b.tns[cf]
        short = ic["window_sequence"] == SHORT
        ranges = R.tns_spec_ranges(ic, t, rec.sf_index)
        assert 1 <= len(ranges) <= 8
        per_window = np.bincount([w for _, w, *_ in ranges], minlength=8)
        if short:
            bare_window += int((per_window == 0).any())
            two_on_short += int((per_window == 2).any())
            assert per_window.max() <= 2
        else:
            stacks.add(len(ranges))
            assert (per_window[1:] == 0).all()
        for k, w, order, top, bottom, s, e in ranges:
            F = t["filt"][k]
            res, comp = int(F["flags"]) >> 1 & 1, int(F["flags"]) >> 2 & 1
            assert (F["coef"][:order] < (1 << (res + 3 - comp))).all() and not F["coef"][order:].any()
            assert order <= (7 if short else 20) and F["length"] <= (15 if short else 63)
            if not short:
                orders.add(order)
            if order:
                flagsets.add(int(F["flags"]) & 7)
                if e > s:  # the filter acts, and on a range some clamp has cut
                    cut_tns_max += int(top > tmax[int(short)] and e == tmax[int(short)])
                    cut_max_sfb += int(min(top, tmax[int(short)]) > ic["max_sfb"] and e == ic["max_sfb"])
                    into_band0 += int(top - int(F["length"]) < 0 and s == 0)
        other = b.ics[cf ^ 1]
        if not (ic["flags"] & N.ICS_COMMON_WINDOW) and (other["flags"] & N.ICS_TNS):
            mixed_pair += int(short != (other["window_sequence"] == SHORT))
    assert orders == {0, 1, 7, 12, 20}, orders
    assert stacks == {1, 2, 3}, stacks
    assert flagsets == set(range(8)), flagsets  # both directions, resolutions and compress values
    assert cut_tns_max and cut_max_sfb and into_band0, (cut_tns_max, cut_max_sfb, into_band0)
    assert bare_window and two_on_short
    assert mixed_pair  # one long channel with TNS next to one short channel with TNS
    # every coefficient index the four (res, compress) widths allow occurs
    for res in (0, 1):
        for comp in (0, 1):
            seen = set()
            for cf in np.flatnonzero(b.ics["flags"] & N.ICS_TNS):
                for k in range(int(b.tns["n_filters"][cf])):
                    F = b.tns["filt"][cf, k]
                    if F["order"] and (int(F["flags"]) >> 1 & 3) == (res | comp << 1):
                        seen |= set(F["coef"][:F["order"]].tolist())
            assert seen == set(range(1 << (res + 3 - comp))), (res, comp, seen)
    # the batch that can be written: at most one filter per short window, nothing else changed
    syn = rec.syntax_batch
    assert (syn.tns["n_filters"] <= b.tns["n_filters"]).all()
    assert (syn.tns["n_filters"] < b.tns["n_filters"]).sum() == two_on_short


def test_tns_shapes_filters_act_and_stay_finite():
    rec = batch("tns_shapes")
    spec, compat = oracle_f32("tns_shapes"), oracle_f32("tns_shapes", N.TNS_COMPAT)
    assert np.isfinite(spec).all()
    print(f"tns_shapes: spec-TNS peak {np.abs(spec).max():.4g}, compat peak {np.abs(compat).max():.4g}")
    tns_frames = (rec.batch.ics["flags"].reshape(-1, 2) & N.ICS_TNS).any(axis=1)
    differs = (spec.view(np.uint32) != compat.view(np.uint32)).any(axis=1)
    assert not differs[~tns_frames & ~np.roll(tns_frames, 1)].any()
    share = differs[tns_frames].mean()
    print(f"tns_shapes: {tns_frames.sum()} TNS frames, {100 * share:.1f} % differ from the compat output")
    assert share >= 0.8


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_write_parse_round_trip(name):
    """Every batch written by the test writer parses back to its records (q where the reference
    reads it, ms_used below groups*max_sfb): the records are ones a bitstream can carry.  The one
    exception is stated by the builder: a short window's n_filt is one bit (TNS.java:20,40), so
    tns_shapes is written without its second filters on a short window (Records.syntax_batch); the
    GPU tests decode the batch with them."""
    rec = batch(name)
    cfg, runs = R.written_runs(name)
    for frames, pns0, want in runs:
        P = N.Parser(cfg)
        P.pns_state = pns0
        got = P.parse(list(frames), slot=int(want.stream_slot[0]))
        P.close()
        R.assert_records_equal(got, want, rec.sf_index)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_shared_core_equals_the_host_parser_on_these_frames_under_sanitizers(tmp_path):
    """tools/gparse_diff (tests/test_gparse_core.py) with the independent_layouts and partial_max_sfb
    frames as seeds: the parse core the device parser runs against the host parser, stand-alone with
    ASan + UBSan, the frames as they are and 2000 mutants of them."""
    seeds = tmp_path / "seeds.bin"
    n_seeds = 0
    with open(seeds, "wb") as out:
        for name in sorted(BATCHES):
            if not name.startswith(("independent", "partial")):
                continue
            cfg, runs = R.written_runs(name)
            for frames, _, _ in runs:
                for f in frames:
                    out.write(struct.pack("<BBBI", cfg.sf_index, cfg.channel_config, cfg.tns_mode, len(f)) + f)
                    n_seeds += 1
    exe = tmp_path / "gparse_diff"
    csrc = ROOT / "jaadec_amd" / "csrc"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{csrc}",
                    str(ROOT / "tools" / "gparse_diff.cpp"), str(csrc / "jaad_parse.cpp"), str(csrc / "jaad_parse_sbr.cpp"),
                    str(csrc / "jaad_sbr_host.cpp"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe), str(seeds), "2000"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert n_seeds > 500
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "mismatches: 0" in r.stdout
    assert "lcg jump: ok" in r.stdout
    counts = {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"status (-?\d+): (\d+)", r.stdout)}
    for st in (N.OK, N.ERR_EOS, N.ERR_BITSTREAM, N.ERR_UNSUPPORTED):
        assert counts.get(st, 0) > 0, (st, counts)
    assert sum(counts.values()) == 2000
