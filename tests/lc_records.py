"""Record builders for the AAC-LC kernels: side info the synthetic generator never emits.

The generator (jaadec_amd/csrc/jaad_synth.cpp) draws window sequence, grouping and max_sfb once per
frame, always codes every band (max_sfb = the band count), keeps the scalefactors within 6 of the
global gain, and writes one shape of TNS record.  The builders here start from a small generator
batch (its run table and array shapes) and rewrite the records in numpy:

* independent_layouts  a CPE without a common window: each channel has its own window-sequence
                       machine, window shapes, grouping and max_sfb (optionally I/S and PNS bands)
* partial_max_sfb      common-window M/S stereo, or mono: max_sfb from 0 to the band count, every
                       group count, junk where the decoder must not look
* gain_range           every one of the 256 scalefactor values on a spectral band; the variants
                       full_scale (frame peaks just past int16 full scale) and huge (past int32)
* tns_shapes           spec-TNS records: stacked filters, every order class, both directions,
                       resolutions and compress values, filters cut by tns_max / max_sfb / band 0

Every builder is deterministic in its seed.  tests/test_lc_records.py checks what the batches
contain with the C restatement and the host parser; tests/test_gpu_lc_records.py decodes them on the
GPU.  This is a helper module, not a conftest."""
from __future__ import annotations

import re
from dataclasses import dataclass
from functools import lru_cache
from pathlib import Path

import numpy as np

from jaadec_amd import native as N

ROOT = Path(__file__).resolve().parents[1]
_INC = ROOT / "jaadec_amd" / "csrc" / "tables" / "jaad_tables.inc"

LONG, START, SHORT, STOP = (N.ONLY_LONG_SEQUENCE, N.LONG_START_SEQUENCE, N.EIGHT_SHORT_SEQUENCE,
                            N.LONG_STOP_SEQUENCE)
# TNS_MAX_BANDS of the 1024-sample AAC-LC frame per sampling-frequency index: (long, short)
# (ISO/IEC 14496-3 table 4.139; the value orc_tns_spec and the kernel clamp `top` / `bottom` with)
TNS_MAX_SFB = [(31, 9), (31, 9), (34, 10), (40, 14), (42, 14), (51, 14), (46, 14), (46, 14), (42, 14), (42, 14),
               (42, 14), (39, 14)]


@lru_cache(maxsize=None)
def band_tables(sf_index: int):
    """(long, short) scalefactor-band offsets of a sampling-frequency index (band count = len - 1)."""
    src = _INC.read_text()

    def names(tag):
        m = re.search(r"JAAD_SWB_OFFSET_" + tag + r"_WINDOW\[12\] = \{([^}]*)\}", src)
        return [s.strip() for s in m.group(1).split(",")]

    def arr(name):
        m = re.search(r"static const short " + name + r"\[\d+\] = \{([^}]*)\}", src)
        return np.array([int(x) for x in m.group(1).split(",")])

    return arr(names("LONG")[sf_index]), arr(names("SHORT")[sf_index])


@dataclass
class Records:
    """A batch with the configuration it decodes under."""

    batch: N.Batch
    sf_index: int
    channel_config: int
    tns_mode: int = N.TNS_COMPAT
    # the same batch without the records the raw_data_block syntax cannot carry (tns_shapes: a second
    # filter on a short window); None: the whole batch can be written
    syntax_batch: N.Batch | None = None

    def cfg(self, precision: int = N.PRECISION_EXACT, tns_mode: int | None = None) -> N.StreamCfg:
        return N.make_cfg(sf_index=self.sf_index, channel_config=self.channel_config,
                          tns_mode=self.tns_mode if tns_mode is None else tns_mode, precision=precision)

    @property
    def n_slots(self) -> int:
        return len(self.batch.stream_slot)


# ---------------------------------------------------------------------------------------------
# layout helpers
# ---------------------------------------------------------------------------------------------
def group_lengths(ic) -> list:
    """Window-group lengths of a channel's ics record (ICSInfo.java:93-107)."""
    if ic["window_sequence"] != SHORT:
        return [1]
    glen = [1]
    for i in range(7):
        if int(ic["grouping"]) >> i & 1:
            glen[-1] += 1
        else:
            glen.append(1)
    return glen


def n_bands(ic) -> int:
    return len(group_lengths(ic)) * int(ic["max_sfb"])


def bands(ic, off):
    """(idx, group, sfb, first window, windows, lo, hi) of every coded band, idx = g*max_sfb + sfb."""
    idx, w0 = 0, 0
    for g, gl in enumerate(group_lengths(ic)):
        for sfb in range(int(ic["max_sfb"])):
            yield idx, g, sfb, w0, gl, int(off[sfb]), int(off[sfb + 1])
            idx += 1
        w0 += gl


def window_rows(b: N.Batch, cf: int) -> np.ndarray:
    """The channel's q row as [windows, bins] (a view)."""
    return b.q[cf].reshape(8, 128) if b.ics["window_sequence"][cf] == SHORT else b.q[cf].reshape(1, 1024)


def coded_mask(b: N.Batch, cf: int, off) -> np.ndarray:
    """bool [1024]: the bins whose q the reference reads (spectral codebooks below max_sfb)."""
    rows = np.zeros((8, 128) if b.ics["window_sequence"][cf] == SHORT else (1, 1024), bool)
    for idx, _, _, w0, gl, lo, hi in bands(b.ics[cf], off):
        if 0 < b.cb[cf, idx] < N.NOISE_HCB:
            rows[w0:w0 + gl, lo:hi] = True
    return rows.reshape(-1)


def grouping_with(rng, n_groups: int) -> int:
    """A scale_factor_grouping byte with the given number of window groups (bit set: same group)."""
    joined = rng.choice(7, 8 - n_groups, replace=False)
    return int(sum(1 << int(i) for i in joined))


def sequences(rng, n: int, script=(), p_start: float = 0.3) -> list:
    """A legal window-sequence chain (ONLY_LONG -> LONG_START -> EIGHT_SHORT x k -> LONG_STOP): the
    scripted frames first, then random ones."""
    out = list(script)[:n]
    prev = out[-1] if out else LONG
    while len(out) < n:
        if prev in (LONG, STOP):
            seq = START if rng.random() < p_start else LONG
        elif prev == START:
            seq = SHORT
        else:
            seq = SHORT if rng.random() < 0.5 else STOP
        out.append(seq)
        prev = seq
    for a, c in zip([LONG] + out, out):  # every step is one the block-switching rules allow
        assert (c in (LONG, START)) == (a in (LONG, STOP)), out
    return out


def _codebook_for(maxabs: int, rng) -> int:
    if maxabs == 0:
        return N.ZERO_HCB
    base = 1 if maxabs <= 1 else 3 if maxabs <= 2 else 5 if maxabs <= 4 else 7 if maxabs <= 7 else 9 if maxabs <= 12 else 11
    return 11 if base == 11 else base + int(rng.integers(0, 2))


def _shell(seed: int, sf_index: int, cc: int, n_streams: int, fps: int, with_tns: bool = False) -> N.Batch:
    """A generator batch of the wanted size: run table, slots and arrays, every record rewritten later."""
    p = N.synth_params(3 if cc == 2 else 1, n_streams=n_streams, frames_per_stream=fps, sf_index=sf_index,
                       channel_config=cc, window_switching=1, tns_percent=50 if with_tns else 0)
    p.seed = (p.seed + seed) & 0xFFFFFFFFFFFFFFFF
    b = N.synth_batch(p, with_tns=with_tns)
    b.ics[:] = np.zeros((), N.ICS_DTYPE)
    if b.ms_used is not None:
        b.ms_used[:] = 0
    if b.tns is not None:
        b.tns[:] = np.zeros((), N.TNS_DTYPE)
    return b


def _set_layout(b, cf, seq, shape, max_sfb, grouping=0):
    ic = b.ics[cf:cf + 1]
    ic["window_sequence"], ic["window_shape"], ic["max_sfb"] = seq, shape, max_sfb
    ic["grouping"] = grouping if seq == SHORT else 0


def fill_channel(b, cf, off, rng, walk, gg=130, pns_percent=0, is_percent=0, esc_permille=1) -> int:
    """Spectrum, scalefactors and codebooks of one channel for the layout its ics record holds, in
    the generator's manner (level falling with frequency, scalefactor walk around gg, short windows
    12 lower); q is zero outside the spectral bands.  Returns the HAS_PNS / HAS_IS flags."""
    short = b.ics["window_sequence"][cf] == SHORT
    rows = window_rows(b, cf)
    pos = np.arange(rows.shape[1]) * (8 if short else 1)
    v = np.floor(-(12.0 - 11.0 * pos / 1023.0) * np.log1p(-rng.random(rows.shape)) + 0.5).astype(np.int64)
    esc = rng.random(rows.shape) < esc_permille / 1000.0
    v = np.minimum(np.where(esc, 16 + rng.integers(0, 1008, rows.shape), v), 8190)
    rows[...] = v * rng.choice(np.array([-1, 1]), rows.shape)
    rows[:, int(off[int(b.ics["max_sfb"][cf])]):] = 0
    b.sf[cf] = 0
    b.cb[cf] = 0
    flags = 0
    for idx, _, _, w0, gl, lo, hi in bands(b.ics[cf], off):
        walk[0] = int(np.clip(walk[0] + rng.integers(-1, 2), gg - 6, gg + 6))
        r = int(rng.integers(0, 100))
        blk = rows[w0:w0 + gl, lo:hi]
        if r < pns_percent:
            b.cb[cf, idx], b.sf[cf, idx] = N.NOISE_HCB, 120 + int(rng.integers(0, 30))
            blk[...] = 0
            flags |= N.ICS_HAS_PNS
        elif r < pns_percent + is_percent:
            b.cb[cf, idx] = N.INTENSITY_HCB if rng.integers(0, 2) else N.INTENSITY_HCB2
            b.sf[cf, idx] = 100 - (int(rng.integers(0, 25)) - 4)
            blk[...] = 0
            flags |= N.ICS_HAS_IS
        else:
            c = _codebook_for(int(np.abs(blk).max()), rng)
            b.cb[cf, idx] = c
            b.sf[cf, idx] = walk[0] + (-12 if short else 0) if c else 0
    return flags


def _lcg_jump(state: int, n: int) -> int:
    """n steps of the static PNS LCG (ICStream.java:26,247) by squaring the affine map."""
    a, c = 1664525, 1013904223
    ra, rc = 1, 0
    while n:
        if n & 1:
            ra, rc = (a * ra) & 0xFFFFFFFF, (a * rc + c) & 0xFFFFFFFF
        a, c = (a * a) & 0xFFFFFFFF, (a * c + c) & 0xFFFFFFFF
        n >>= 1
    return (ra * state + rc) & 0xFFFFFFFF


def chain_state(b: N.Batch, sf_index: int) -> None:
    """window_shape_prev per channel along each run, and pns_state in parse order (a frame's left
    channel, then its right one) through the whole batch, as the generator chains them."""
    offs = band_tables(sf_index)
    rs = N.PNS_STATE0
    for r in range(len(b.stream_slot)):
        prev = [0] * b.nch
        for f in range(int(b.frame_begin[r]), int(b.frame_begin[r + 1])):
            for c in range(b.nch):
                cf = f * b.nch + c
                b.ics["window_shape_prev"][cf] = prev[c]
                prev[c] = int(b.ics["window_shape"][cf])
                b.ics["pns_state"][cf] = rs
                if b.ics["flags"][cf] & N.ICS_HAS_PNS:
                    off = offs[1] if b.ics["window_sequence"][cf] == SHORT else offs[0]
                    steps = sum(gl * (hi - lo) for idx, _, _, _, gl, lo, hi in bands(b.ics[cf], off)
                                if b.cb[cf, idx] == N.NOISE_HCB)
                    rs = _lcg_jump(rs, steps)


def _random_bits(rng) -> np.ndarray:
    return rng.integers(0, 1 << 63, 2, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 2, dtype=np.uint64)


def mask_ms(ms_row: np.ndarray, nb: int) -> np.ndarray:
    """An ms_used pair with the bits at indices >= nb cleared."""
    out = ms_row.copy()
    for i in range(2):
        out[i] &= np.uint64((1 << min(max(nb - 64 * i, 0), 64)) - 1)
    return out


# ---------------------------------------------------------------------------------------------
# independent_layouts
# ---------------------------------------------------------------------------------------------
# scripted openings, (left, right) per stream: lockstep short frames; L short while R long and the
# reverse; the random continuation follows
_OPENINGS = [
    ([LONG, START, SHORT, SHORT, SHORT, SHORT, STOP], [LONG, START, SHORT, SHORT, SHORT, SHORT, STOP]),
    ([START, SHORT, STOP, LONG, LONG, LONG], [LONG, LONG, START, SHORT, SHORT, STOP]),
    ([LONG, LONG, LONG, START, SHORT, STOP], [START, SHORT, SHORT, STOP, LONG, START]),
]


def independent_layouts(seed: int, sf_index: int = 3, n_streams: int = 6, fps: int = 20, is_percent: int = 0,
                        pns_percent: int = 0) -> Records:
    """Stereo without a common window: per channel its own window sequences, shapes, grouping and
    max_sfb; ms_used all zero (ms_mask_present needs a common window).  The right channel's I/S
    bands are indexed by the right channel's layout."""
    rng = np.random.default_rng([seed, sf_index, 1])
    offs = band_tables(sf_index)
    b = _shell(seed, sf_index, 2, n_streams, fps)
    for r in range(n_streams):
        script = _OPENINGS[r] if r < len(_OPENINGS) else ((), ())
        seqs = [sequences(rng, fps, script[c]) for c in range(2)]
        walk = [[130], [130]]
        for i in range(fps):
            f = int(b.frame_begin[r]) + i
            for c in range(2):
                seq = seqs[c][i]
                nswb = len(offs[1 if seq == SHORT else 0]) - 1
                max_sfb = int(rng.choice([nswb, nswb, nswb - 1, nswb - 3, (nswb + 1) // 2, 3, 1, 0]))
                _set_layout(b, 2 * f + c, seq, int(rng.integers(0, 2)), max_sfb, int(rng.integers(0, 128)))
            if seqs[0][i] == SHORT and seqs[1][i] == SHORT and i % 2 == 0:
                # the same layout in both channels, still without a common window: the lockstep path
                b.ics["max_sfb"][2 * f + 1] = b.ics["max_sfb"][2 * f]
                b.ics["grouping"][2 * f + 1] = b.ics["grouping"][2 * f]
            for c in range(2):
                cf = 2 * f + c
                off = offs[1 if seqs[c][i] == SHORT else 0]
                b.ics["flags"][cf] = fill_channel(b, cf, off, rng, walk[c], pns_percent=pns_percent,
                                                  is_percent=is_percent if c == 1 else 0)
    chain_state(b, sf_index)
    return Records(b, sf_index, 2)


# ---------------------------------------------------------------------------------------------
# partial_max_sfb
# ---------------------------------------------------------------------------------------------
def partial_max_sfb(seed: int, sf_index: int = 3, channel_config: int = 2, n_streams: int = 6, fps: int = 20,
                    junk: bool = True) -> Records:
    """Common-window M/S stereo (some I/S bands on the right) or mono (some PNS bands): max_sfb walks
    through 0, 1, odd, even, count-1 and count for long and for short frames, short frames through
    every group count.  With junk, q above offsets[max_sfb] and the ms_used bits from groups*max_sfb
    up are random: the reference reads neither.  junk=False gives the same batch with both zeroed."""
    rng = np.random.default_rng([seed, sf_index, channel_config, 2])
    jrng = np.random.default_rng([seed, sf_index, channel_config, 3])  # (the junk: its own stream)
    offs = band_tables(sf_index)
    nch = 2 if channel_config == 2 else 1
    b = _shell(seed, sf_index, channel_config, n_streams, fps)
    count = [0, 0]  # long / short frames so far
    for r in range(n_streams):
        seqs = sequences(rng, fps, [LONG, START, SHORT] if r % 2 else (), p_start=0.45)
        walk = [[130], [130]]
        for i in range(fps):
            f = int(b.frame_begin[r]) + i
            short = seqs[i] == SHORT
            off = offs[1 if short else 0]
            nswb = len(off) - 1
            choices = [nswb, 0, nswb - 1, 1, 7, nswb // 2 & ~1, 3, nswb - 2]
            max_sfb = choices[count[short] % len(choices)]
            grouping = grouping_with(rng, 1 + (count[1] * 3) % 8) if short else 0  # 3 is coprime to 8
            count[short] += 1
            shape = int(rng.integers(0, 2))
            for c in range(nch):
                cf = nch * f + c
                _set_layout(b, cf, seqs[i], shape, max_sfb, grouping)
                fl = fill_channel(b, cf, off, rng, walk[c], pns_percent=5 if nch == 1 else 0,
                                  is_percent=8 if c == 1 else 0)
                if nch == 2:
                    fl |= N.ICS_COMMON_WINDOW | (N.ICS_MS_PRESENT if c == 0 else 0)
                b.ics["flags"][cf] = fl
                jq = jrng.integers(-8190, 8191, 1024).astype(np.int16).reshape(window_rows(b, cf).shape)
                if junk:
                    window_rows(b, cf)[:, int(off[max_sfb]):] = jq[:, int(off[max_sfb]):]
            if nch == 2:
                bits, jbits = _random_bits(rng), _random_bits(jrng)
                nb = n_bands(b.ics[2 * f])
                b.ms_used[f] = mask_ms(bits, nb)
                if junk:
                    b.ms_used[f] |= jbits & ~mask_ms(np.full(2, ~np.uint64(0)), nb)
    chain_state(b, sf_index)
    return Records(b, sf_index, channel_config)


# ---------------------------------------------------------------------------------------------
# gain_range
# ---------------------------------------------------------------------------------------------
def _gain(sf: int) -> float:
    return 2.0 ** ((sf - 100) / 4.0)


def _regain(b, cf, off, rng, next_sf, amplitude, density=0.5) -> None:
    """Give every coded band of the channel a spectral codebook, the scalefactor next_sf() yields and
    quantised values whose dequantised magnitude is about amplitude() (as far as |q| in 1..8190
    reaches): some bins of the band, at least one."""
    rows = window_rows(b, cf)
    for idx, _, _, w0, gl, lo, hi in bands(b.ics[cf], off):
        sf = next_sf()
        blk = rows[w0:w0 + gl, lo:hi]
        qmag = (amplitude() / _gain(sf)) ** 0.75
        mag = np.clip(np.rint(qmag * rng.uniform(0.25, 1.0, blk.shape)), 1, 8190).astype(np.int64)
        keep = rng.random(blk.shape) < density
        keep.flat[int(rng.integers(0, keep.size))] = True
        blk[...] = np.where(keep, mag, 0) * rng.choice(np.array([-1, 1]), blk.shape)
        b.cb[cf, idx] = _codebook_for(int(np.abs(blk).max()), rng)
        b.sf[cf, idx] = sf


def _triangle(start: int):
    """0 .. 255 .. 0 in steps of one, from `start`."""
    state = [start, 1]

    def nxt():
        v = state[0]
        if not 0 <= v + state[1] <= 255:
            state[1] = -state[1]
        state[0] = v + state[1]
        return v
    return nxt


def _bounce(rng, lo: int, hi: int, start: int, step_lo: int, step_hi: int):
    """A walk between lo and hi in steps of step_lo..step_hi (at most 60: one scalefactor codeword)."""
    state = [start, 1]

    def nxt():
        v = state[0]
        step = int(rng.integers(step_lo, step_hi + 1))
        if not lo <= v + state[1] * step <= hi:
            state[1] = -state[1]
        state[0] = int(np.clip(v + state[1] * step, lo, hi))
        return v
    return nxt


def _long_short_layout(b, rng, offs, r, fps, p_start=0.3):
    """Common-window stereo frames of run r with full max_sfb, no M/S; returns the sequences."""
    seqs = sequences(rng, fps, (), p_start)
    for i in range(fps):
        f = int(b.frame_begin[r]) + i
        nswb = len(offs[1 if seqs[i] == SHORT else 0]) - 1
        shape, grouping = int(rng.integers(0, 2)), int(rng.integers(0, 128))
        for c in range(2):
            _set_layout(b, 2 * f + c, seqs[i], shape, nswb, grouping)
            b.ics["flags"][2 * f + c] = N.ICS_COMMON_WINDOW
    return seqs


def gain_range(seed: int, variant: str = "walk", sf_index: int = 3, n_streams: int = 4, fps: int = 16) -> Records:
    """Common-window stereo, no M/S.
    walk        the left channel's bands step through 0..255..0 one by one, the right channel's
                bounce across the whole range in steps of 20..60; |q| chosen for a moderate level
                where 1..8190 allows one.  Every scalefactor value occurs on a spectral band.
    full_scale  generator-like content, long windows, levelled frame by frame until every frame's
                peak in the restatement's float32 output lies just past int16 full scale: in
                (32768, 40000].
    huge        scalefactors 215..255 on |q| up to 8190 (the IQ table's last entry): samples past
                int32, all finite."""
    assert variant in ("walk", "full_scale", "huge")
    rng = np.random.default_rng([seed, sf_index, 4, ("walk", "full_scale", "huge").index(variant)])
    offs = band_tables(sf_index)
    b = _shell(seed, sf_index, 2, n_streams, fps)
    for r in range(n_streams):
        # (full_scale: long windows only -- after a LONG_START frame's flat second half the
        # levelling below has no solution often enough)
        seqs = _long_short_layout(b, rng, offs, r, fps, 0.0 if variant == "full_scale" else 0.3)
        if variant == "walk":
            nxt = [_triangle((67 * r) % 256), _bounce(rng, 0, 255, (91 * r) % 256, 20, 60)]
        elif variant == "huge":
            nxt = [_bounce(rng, 215, 255, 255 - r, 1, 9), _bounce(rng, 215, 255, 230 + r, 1, 9)]
        walk = [[130], [130]]
        for i in range(fps):
            f = int(b.frame_begin[r]) + i
            off = offs[1 if seqs[i] == SHORT else 0]
            for c in range(2):
                cf = 2 * f + c
                if variant == "full_scale":
                    fill_channel(b, cf, off, rng, walk[c], esc_permille=0)
                    continue
                b.sf[cf] = 0
                b.cb[cf] = 0
                b.q[cf] = 0
                if variant == "walk":
                    _regain(b, cf, off, rng, nxt[c], lambda: float(rng.uniform(200.0, 3000.0)))
                else:  # large |q| under the huge gains on a quarter of the bins
                    _regain(b, cf, off, rng, nxt[c], lambda: 1e30, density=0.25)
    chain_state(b, sf_index)
    rec = Records(b, sf_index, 2)
    if variant == "full_scale":
        _level_to_full_scale(rec, rng)
    return rec


def frame_peaks(rec: Records, pcm_f32: np.ndarray) -> np.ndarray:
    return np.abs(pcm_f32.view(np.float32).reshape(rec.batch.n_frames, -1)).max(axis=1)


def _level_to_full_scale(rec: Records, rng, lo=32768.0, hi=40000.0, aim=36200.0) -> None:
    """Raise or lower each frame's spectral scalefactors (both channels; quarter steps: a step on
    the first k quarters of the frame's bands) until the frame's peak in the restatement's float32
    output is in (lo, hi].  A frame's samples also carry its predecessor's overlap, so the levels
    are found by iteration over the whole batch."""
    from oracle import oracle as O
    b = rec.batch
    base = b.sf.copy()
    spectral = (b.cb > 0) & (b.cb < N.NOISE_HCB)
    level = np.zeros(b.n_frames, np.int64)

    def apply(f):
        for cf in (2 * f, 2 * f + 1):
            idx = np.flatnonzero(spectral[cf])
            up = (np.arange(len(idx)) * 4 < (level[f] % 4) * len(idx)).astype(np.int64)
            b.sf[cf, idx] = np.clip(base[cf, idx].astype(np.int64) + level[f] // 4 + up, 0, 255)

    fps = int(b.frame_begin[1])
    assert (np.diff(b.frame_begin) == fps).all()
    t, decodes, conflicts = 0, 0, np.zeros(b.n_frames, np.int64)
    while t < fps:  # the frames at position t of every run, their predecessors settled
        frames = [int(x) + t for x in b.frame_begin[:-1]]
        lowered = {}
        for trial in range(16):
            pcm = O.decode_batch(rec.cfg(), b, O.Streams(rec.n_slots), N.PCM_FLOAT32)
            decodes += 1
            assert decodes < 3000, "full_scale: the levels did not settle"
            peak = frame_peaks(rec, pcm)
            out = [f for f in frames if not lo < peak[f] <= hi]
            # too loud, and lowering the frame did not help: its predecessor's second half alone is
            stuck = [f for f in out if peak[f] > hi and f in lowered and peak[f] > 0.999 * lowered[f]]
            if not out or stuck:
                break
            for f in out:
                # one sf step is 2^(1/4): 16 quarter steps per octave; single steps once close
                step = int(np.rint(16.0 * np.log2(aim / max(float(peak[f]), 1e-3))))
                if trial >= 6 or not step:
                    step = 1 if peak[f] <= lo else -1
                if step < 0:
                    lowered[f] = float(peak[f])
                level[f] += step
                apply(f)
        if out:
            # lower the predecessor a quarter step; where that only swings back and forth (its own
            # frame then falls below full scale), give its spectrum new signs: another ratio between
            # the peaks of its two halves.  Then settle it, and this frame, again.
            assert t > 0, out
            for f in stuck or out:
                conflicts[f] += 1
                if conflicts[f] % 3:
                    level[f - 1] -= 1
                    apply(f - 1)
                else:
                    for cf in (2 * f - 2, 2 * f - 1):
                        b.q[cf] *= rng.choice(np.array([-1, 1], np.int16), 1024)
                level[f] = level[f - 1]
                apply(f)
            t -= 1
            continue
        t += 1


# ---------------------------------------------------------------------------------------------
# tns_shapes
# ---------------------------------------------------------------------------------------------
def _tns_filter(rng, window, length, order, direction, res, compress, wild=0.2):
    """One jaad_tns_filter.  Coefficient indices use the res + 3 - compress bits the syntax gives:
    most of them small reflection coefficients (the generator's), a share `wild` of them anywhere
    in the index range."""
    F = np.zeros((), N.TNS_FILTER_DTYPE)
    F["window"], F["length"], F["order"] = window, length, order
    if not order:  # direction / compress are not transmitted for an empty filter
        F["flags"] = res << 1
        return F
    F["flags"] = direction | res << 1 | compress << 2
    n = 1 << (res + 3 - compress)
    for i in range(order):
        if rng.random() < wild:
            F["coef"][i] = int(rng.integers(0, n))
        else:
            mag = int(rng.integers(0, 3))
            F["coef"][i] = (mag if rng.integers(0, 2) else n - 1 - mag) & (n - 1)
    return F


def _long_tns_patterns(nswb, tns_max):
    """(max_sfb, [(length, order)]) per pattern; top starts at nswb > tns_max, so a first filter of
    a full-band frame is cut by tns_max."""
    low = tns_max - 10  # a reduced max_sfb below tns_max
    return [
        (nswb, [(20, 12)]),                                  # cut by tns_max
        (nswb, [(15, 7), (20, 1)]),                          # two stacked
        (nswb, [(10, 20), (12, 0), (63, 12)]),               # three; an empty one; the last runs into band 0
        (low, [(nswb - tns_max + 3, 7), (15, 7)]),           # the first wholly above max_sfb, the second cut by it
        (low, [(nswb - tns_max + 3, 1), (10, 12), (63, 7)]),  # reduced max_sfb and the stack into band 0
        (nswb, [(25, 1)]),
        (nswb - 1, [(nswb - 6, 20)]),
    ]


def tns_spec_ranges(ic, tns_rec, sf_index):
    """(filter index, window, order, top, bottom, s, e) per filter, as orc_tns_spec walks them."""
    short = ic["window_sequence"] == SHORT
    nswb = len(band_tables(sf_index)[1 if short else 0]) - 1
    tns_max = TNS_MAX_SFB[sf_index][1 if short else 0]
    bottom_w = [nswb] * 8
    out = []
    for k in range(int(tns_rec["n_filters"])):
        F = tns_rec["filt"][k]
        w = int(F["window"])
        top = bottom_w[w]
        bottom = max(top - int(F["length"]), 0)
        bottom_w[w] = bottom
        s = min(bottom, tns_max, int(ic["max_sfb"]))
        e = min(top, tns_max, int(ic["max_sfb"]))
        out.append((k, w, int(F["order"]), top, bottom, s, e))
    return out


def tns_shapes(seed: int, sf_index: int = 3, n_streams: int = 6, fps: int = 20) -> Records:
    """Stereo for spec TNS.  Even runs: common window with M/S; odd runs: independent layouts (one
    channel long with TNS while the other is short with TNS occurs there).  About three channels in
    four carry TNS.  Long windows: the patterns of _long_tns_patterns in turn.  Short frames: one
    filter (order 0, 1, 3 or 7) on some of the windows only -- and, in every third short TNS channel,
    a second filter on one of them, which jaad_tns can hold but the 1-bit n_filt of a short window
    cannot: Records.syntax_batch is the batch without those second filters."""
    rng = np.random.default_rng([seed, sf_index, 5])
    offs = band_tables(sf_index)
    tmax = TNS_MAX_SFB[sf_index]
    b = _shell(seed, sf_index, 2, n_streams, fps, with_tns=True)
    patterns = _long_tns_patterns(len(offs[0]) - 1, tmax[0])
    n_long = n_short = n_filt = 0
    second = []  # (cf, filter index) of the filters beyond the syntax
    for r in range(n_streams):
        common = r % 2 == 0
        script = _OPENINGS[1 + (r // 2) % 2] if not common else ([LONG, START, SHORT, SHORT, STOP],) * 2
        seqs = [sequences(rng, fps, script[0], 0.35)]
        seqs.append(seqs[0] if common else sequences(rng, fps, script[1], 0.35))
        walk = [[130], [130]]
        for i in range(fps):
            f = int(b.frame_begin[r]) + i
            shape, grouping = int(rng.integers(0, 2)), int(rng.integers(0, 128))
            for c in range(2):
                cf = 2 * f + c
                seq = seqs[c][i]
                short = seq == SHORT
                nswb = len(offs[1 if short else 0]) - 1
                has_tns = rng.random() < 0.75
                max_sfb = nswb
                filters = []
                if common and c == 1:  # the common window: the left channel's layout
                    max_sfb = int(b.ics["max_sfb"][cf - 1])
                if has_tns and not short:
                    pat_sfb, stack = patterns[n_long % len(patterns)]
                    n_long += 1
                    if not (common and c == 1):
                        max_sfb = pat_sfb
                    res = n_long // len(patterns) % 2
                    for length, order in stack:
                        filters.append(_tns_filter(rng, 0, length, order, n_filt % 2, res, n_filt // 2 % 2))
                        n_filt += 1
                elif has_tns:
                    if not (common and c == 1):
                        max_sfb = [nswb, nswb - 2, tmax[1] - 4][n_short % 3]
                    windows = sorted(rng.choice(8, int(rng.integers(1, 7)), replace=False).tolist())
                    twice = windows[int(rng.integers(0, len(windows)))] if n_short % 3 == 2 else -1
                    n_short += 1
                    for w in windows:
                        res = int(rng.integers(0, 2))
                        for k in range(2 if w == twice else 1):
                            order = [7, 1, 0, 3][n_filt % 4] if k == 0 else 7
                            length = int(rng.integers(1, nswb + 1)) if k == 0 else 5
                            if k == 1:
                                second.append((cf, len(filters)))
                            filters.append(_tns_filter(rng, w, length, order, n_filt // 4 % 2, res, n_filt // 8 % 2))
                            n_filt += 1
                if common:
                    _set_layout(b, cf, seq, shape, max_sfb, grouping)
                else:
                    _set_layout(b, cf, seq, int(rng.integers(0, 2)), max_sfb, int(rng.integers(0, 128)))
                fl = fill_channel(b, cf, offs[1 if short else 0], rng, walk[c])
                if common:
                    fl |= N.ICS_COMMON_WINDOW | (N.ICS_MS_PRESENT if c == 0 else 0)
                if filters:
                    fl |= N.ICS_TNS
                    assert len(filters) <= 8
                    b.tns["n_filters"][cf] = len(filters)
                    for k, F in enumerate(filters):
                        b.tns["filt"][cf, k] = F
                b.ics["flags"][cf] = fl
            if common:
                b.ms_used[f] = mask_ms(_random_bits(rng), n_bands(b.ics[2 * f]))
    chain_state(b, sf_index)
    syn = N.Batch(b.q, b.sf, b.cb, b.ics, b.ms_used, b.tns.copy(), b.stream_slot, b.frame_begin, 2)
    for cf in sorted({cf for cf, _ in second}):
        drop = [k for c2, k in second if c2 == cf]
        keep = [k for k in range(int(b.tns["n_filters"][cf])) if k not in drop]
        filt = syn.tns["filt"][cf].copy()
        syn.tns["filt"][cf] = np.zeros((), N.TNS_FILTER_DTYPE)
        syn.tns["filt"][cf, :len(keep)] = filt[keep]
        syn.tns["n_filters"][cf] = len(keep)
    return Records(b, sf_index, 2, tns_mode=N.TNS_SPEC, syntax_batch=syn)


# ---------------------------------------------------------------------------------------------
# comparing records with what a bitstream carries
# ---------------------------------------------------------------------------------------------
def assert_records_equal(got: N.Batch, want: N.Batch, sf_index: int) -> None:
    """The parser's records of frames written from `want` (tests/test_parse.py's comparison): sf, cb,
    ics and tns equal, ms_used equal below groups*max_sfb, q equal where the reference reads it (a
    spectral codebook below max_sfb); elsewhere the parser leaves zeros."""
    offs = band_tables(sf_index)
    for name in ("sf", "cb", "ics"):
        a, w = getattr(got, name), getattr(want, name)
        bad = np.argwhere(a != w)
        assert bad.size == 0, f"{name} differs at {bad[:4].tolist()}"
    for cf in range(len(want.ics)):
        m = coded_mask(want, cf, offs[1 if want.ics["window_sequence"][cf] == SHORT else 0])
        assert np.array_equal(got.q[cf][m], want.q[cf][m]), f"q differs in channel-frame {cf}"
        assert not got.q[cf][~m].any(), f"q set outside the coded bands in channel-frame {cf}"
    if want.ms_used is not None:
        for f in range(want.n_frames):
            nb = n_bands(want.ics[2 * f])
            assert np.array_equal(mask_ms(got.ms_used[f], nb), mask_ms(want.ms_used[f], nb)), f"ms_used frame {f}"
    if want.tns is not None and want.tns["n_filters"].any():
        assert got.tns is not None and np.array_equal(got.tns, want.tns), "tns differs"


# ---------------------------------------------------------------------------------------------
# the batches both test files use, built (and decoded by the restatement) once per process
# ---------------------------------------------------------------------------------------------
CASES = {
    "independent_48k": lambda: independent_layouts(1, 3),
    "independent_16k": lambda: independent_layouts(2, 8),
    "independent_is": lambda: independent_layouts(3, 3, is_percent=25),
    "independent_pns": lambda: independent_layouts(4, 3, pns_percent=8, is_percent=10),
    "partial_stereo_48k": lambda: partial_max_sfb(5, 3, 2),
    "partial_stereo_8k": lambda: partial_max_sfb(6, 11, 2),
    "partial_mono_48k": lambda: partial_max_sfb(7, 3, 1),
    "partial_stereo_48k_clean": lambda: partial_max_sfb(5, 3, 2, junk=False),
    "partial_stereo_8k_clean": lambda: partial_max_sfb(6, 11, 2, junk=False),
    "partial_mono_48k_clean": lambda: partial_max_sfb(7, 3, 1, junk=False),
    "gain_walk": lambda: gain_range(8, "walk"),
    "full_scale": lambda: gain_range(9, "full_scale"),
    "huge": lambda: gain_range(10, "huge"),
    "tns_shapes": lambda: tns_shapes(11, 3),
}
INDEPENDENT = ["independent_48k", "independent_16k", "independent_is", "independent_pns"]
PARTIAL = ["partial_stereo_48k", "partial_stereo_8k", "partial_mono_48k"]  # (name + "_clean": the same without junk)


@lru_cache(maxsize=None)
def records(name: str) -> Records:
    return CASES[name]()


@lru_cache(maxsize=None)
def oracle_pcm(name: str, flags: int, tns_mode: int | None = None) -> np.ndarray:
    """The restatement's PCM of a batch (uint8 [n_frames, bytes], read-only), exact configuration."""
    from oracle import oracle as O
    rec = records(name)
    out = O.decode_batch(rec.cfg(tns_mode=tns_mode), rec.batch, O.Streams(rec.n_slots), flags)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def written_runs(name: str):
    """(cfg, per run: (raw_data_blocks, pns state at the run's start, the run's records)) of a batch
    written by the test writer (Records.syntax_batch where the batch itself cannot be)."""
    from oracle import oracle as O
    rec = records(name)
    b = rec.syntax_batch if rec.syntax_batch is not None else rec.batch
    runs = []
    for r in range(len(b.stream_slot)):
        one = b.select_runs([r])
        runs.append((tuple(O.write_frames(one, rec.sf_index)), int(one.ics["pns_state"][0]), one))
    return rec.cfg(), tuple(runs)
