#!/usr/bin/env python3
"""Device bitstream front end (include/jaad_gparse.h): frames/s of jaad_gparse_batch and
jaad_gparse_batch_sbr.

The host front-end corpora (tests/golden/parse_c2.bin .. parse_c5.bin) are tiled to 16 384 and
65 536 frames.  After a settle phase the stages are timed with what the library records around them
(jaad_gparse_last_ms: HIP events; for the HE-AAC corpora C4 / C5 jaad_gparse_last_ms_sbr: five
device stages by HIP events and the host tail stage by the wall clock), and, separately, the wall
time of a whole call from host bytes: upload, zeroing, the kernels, read-back -- for C4 / C5 up to
the SBR records and statuses on the host.  tools/bench_parse gives the host parser's rate on the
same corpus at 1 and 16 threads: the yardstick.  Prints one JSON line; --out writes it to a file too.

    python tools/bench_gparse.py --configs 2 3 --out profiles/gparse/mi355x.json
    python tools/bench_gparse.py --configs 4 5 --out profiles/gparse/mi355x_sbr.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import struct
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from jaadec_amd import native as N  # noqa: E402


def load_corpus(path: Path):
    data = path.read_bytes()
    n = struct.unpack_from("<I", data, 4)[0]
    cfg = N.StreamCfg.from_buffer_copy(data[8:8 + n])
    at = 8 + n
    streams, fps = struct.unpack_from("<II", data, at)
    at += 8
    runs = []
    for _ in range(streams):
        pns = struct.unpack_from("<I", data, at)[0]
        at += 4
        frames = []
        for _ in range(fps):
            ln = struct.unpack_from("<I", data, at)[0]
            frames.append(data[at + 4:at + 4 + ln])
            at += 4 + ln
        runs.append((pns, frames))
    return cfg, runs


def tile(runs, n_frames):
    """Whole corpus streams repeated until n_frames frames: (blob, offsets, lengths, frame_begin, pns)."""
    parts, lens, fb, pns = [], [], [0], []
    k = 0
    while fb[-1] < n_frames:
        p, frames = runs[k % len(runs)]
        frames = frames[:n_frames - fb[-1]]
        parts += frames
        lens += [len(f) for f in frames]
        fb.append(fb[-1] + len(frames))
        pns.append(p)
        k += 1
    lens = np.array(lens, np.uint32)
    offs = np.zeros(len(lens), np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), offs, lens, np.array(fb, np.uint32), np.array(pns, np.uint32)


def host_rate(corpus: Path, threads: int, secs: float) -> float | None:
    tool = ROOT / "tools" / "bench_parse"
    if not tool.exists():
        return None
    r = subprocess.run([str(tool), str(corpus), str(threads), str(secs)], capture_output=True, text=True, timeout=120)
    return float(json.loads(r.stdout)["frames_per_s"]) if r.returncode == 0 else None


def measure(gp, blob, offs, lens, fb, pns, settle_s: float, timed_s: float) -> dict:
    nf, n_runs = len(lens), len(fb) - 1
    rec = gp.parse_blob(blob, offs, lens, fb, N.gparse_state(n_runs, pns))  # uploads; the tensors stay
    assert rec.status == 0 and (rec.frame_result == 0).all(), "the corpus must parse"
    t = rec.tensors
    args = (fb, t["data"].data_ptr(), blob.nbytes, t["frame_off"].data_ptr(), t["frame_len"].data_ptr())
    zero, frames, link = [], [], []
    for phase, secs in (("settle", settle_s), ("timed", timed_s)):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < secs:
            rc, _ = gp.parse(*args, N.gparse_state(n_runs, pns), rec.dev)
            assert rc == 0
            if phase == "timed":
                z, f, l = gp.last_ms()
                zero.append(z)
                frames.append(f)
                link.append(l)
    wall = []
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < timed_s or len(wall) < 3:
        w0 = time.perf_counter()
        r2 = gp.parse_blob(blob, offs, lens, fb, N.gparse_state(n_runs, pns))
        wall.append(time.perf_counter() - w0)
        assert r2.status == 0
    med = statistics.median
    kern_ms = med(frames) + med(link)
    return {"frames": nf, "runs": n_runs, "calls_timed": len(frames), "zero_ms": round(med(zero), 4),
            "frames_kernel_ms": round(med(frames), 4), "frames_kernel_ms_min_max": [round(min(frames), 4), round(max(frames), 4)],
            "link_kernel_ms": round(med(link), 4), "kernels_frames_per_s": round(nf / (kern_ms * 1e-3)),
            "with_zeroing_frames_per_s": round(nf / ((kern_ms + med(zero)) * 1e-3)),
            "wall_ms_upload_to_status": round(med(wall) * 1e3, 3), "wall_frames_per_s": round(nf / med(wall))}


SBR_STAGES = ("zero_ms", "frames_kernel_ms", "link_kernel_ms", "scan_gather_ms", "pool_copy_ms", "host_tail_ms")


def measure_sbr(gp, cfg, blob, offs, lens, fb, pns, settle_s: float, timed_s: float) -> dict:
    """The HE-AAC split parse: every call starts from the same parser states (restored outside the
    timed region: a run's time-delta coded envelopes need the history they were written against)."""
    nf, n_runs = len(lens), len(fb) - 1
    parsers = []
    for s in pns:
        p = N.Parser(cfg)
        p.pns_state = int(s)
        parsers.append(p)
    snaps = [p.snapshot() for p in parsers]

    def rewind():
        for p, s in zip(parsers, snaps):
            p.restore(s)

    rec = gp.parse_blob(blob, offs, lens, fb, parsers)  # uploads; the tensors stay
    assert rec.status == 0 and (rec.frame_result == 0).all(), "the corpus must parse"
    t = rec.tensors
    args = (fb, t["data"].data_ptr(), blob.nbytes, t["frame_off"].data_ptr(), t["frame_len"].data_ptr())
    stages = [[] for _ in SBR_STAGES]
    for phase, secs in (("settle", settle_s), ("timed", timed_s)):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < secs:
            rewind()
            rc, _, _ = gp.parse(*args, parsers, rec.dev)
            assert rc == 0
            if phase == "timed":
                for lst, v in zip(stages, gp.last_ms()):
                    lst.append(v)
    wall = []
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < timed_s or len(wall) < 3:
        rewind()
        w0 = time.perf_counter()
        r2 = gp.parse_blob(blob, offs, lens, fb, parsers)
        wall.append(time.perf_counter() - w0)
        assert r2.status == 0
    med = statistics.median
    m = {"frames": nf, "runs": n_runs, "calls_timed": len(stages[0])}
    for name, lst in zip(SBR_STAGES, stages):
        m[name] = round(med(lst), 4)
    fk = stages[1]
    m["frames_kernel_ms_min_max"] = [round(min(fk), 4), round(max(fk), 4)]
    total = sum(med(lst) for lst in stages)
    m["stages_frames_per_s"] = round(nf / (total * 1e-3))
    m["bounding_stage"] = max(SBR_STAGES, key=lambda k: m[k])
    m["wall_ms_upload_to_sbr_records"] = round(med(wall) * 1e3, 3)
    m["wall_frames_per_s"] = round(nf / med(wall))
    for p in parsers + snaps:
        p.close()
    return m


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16384, 65536])
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 3, 4, 5])
    ap.add_argument("--settle", type=float, default=1.0)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--host-seconds", type=float, default=1.0)
    ap.add_argument("--out", type=Path)
    a = ap.parse_args()
    import torch
    result = {"tool": "bench_gparse", "device": torch.cuda.get_device_name(0), "corpora": {}}
    for c in a.configs:
        corpus = ROOT / "tests" / "golden" / f"parse_c{c}.bin"
        cfg, runs = load_corpus(corpus)
        entry = {"host_frames_per_s_1_thread": host_rate(corpus, 1, a.host_seconds),
                 "host_frames_per_s_16_threads": host_rate(corpus, 16, a.host_seconds), "device": []}
        with (N.SbrDeviceParser if cfg.sbr else N.DeviceParser)(cfg) as gp:
            for n in a.sizes:
                blob, offs, lens, fb, pns = tile(runs, n)
                if cfg.sbr:
                    m = measure_sbr(gp, cfg, blob, offs, lens, fb, pns, a.settle, a.seconds)
                    h16 = entry["host_frames_per_s_16_threads"]
                    m["wall_speedup_over_host_16_threads"] = round(m["wall_frames_per_s"] / h16, 2) if h16 else None
                else:
                    m = measure(gp, blob, offs, lens, fb, pns, a.settle, a.seconds)
                m["bitstream_bytes_per_frame"] = round(blob.nbytes / n, 1)
                entry["device"].append(m)
        result["corpora"][f"c{c}"] = entry
    line = json.dumps(result)
    print(line)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
