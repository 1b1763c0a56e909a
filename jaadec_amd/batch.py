"""Bitstream bytes to PCM without the host Huffman decode: the device front end
(include/jaad_gparse.h) feeding the device-resident decode (jaad_decode_batch_device)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native as N


def adts_index(data: bytes):
    """The ADTS header walk alone (jaad_adts_find): the first header, and each raw_data_block's
    byte offset and length in `data`.  No payload is copied or read."""
    L = N.lib()
    data = bytes(data)
    base = C.cast(C.c_char_p(data), C.c_void_p).value
    h, off = N.AdtsHeader(), C.c_size_t()
    first, offs, lens, pos = None, [], [], 0
    while pos < len(data):
        rc = L.jaad_adts_find(C.c_void_p(base + pos), len(data) - pos, C.byref(off), C.byref(h))
        if rc == N.ERR_EOS:
            break
        if rc:
            raise N.JaadError(rc, "jaad_adts_find")
        start, end = pos + off.value + h.header_bytes, pos + off.value + h.frame_length
        if h.frame_length < h.header_bytes or end > len(data):
            break  # truncated last frame
        if first is None:
            first = N.AdtsHeader.from_buffer_copy(h)
        offs.append(start)
        lens.append(end - start)
        pos = end
    return first, np.array(offs, np.uint64), np.array(lens, np.uint32)


def decode_adts_streams(streams: list, flags: int = N.PCM_BIG_ENDIAN, pns_state=N.PNS_STATE0, device: int = 0,
                        implicit_sbr: bool = False) -> list:
    """ADTS byte streams of one AAC-LC mono / stereo configuration -> PCM, one uint8 array
    [n_frames, frame_bytes] per stream.  The host only walks the ADTS headers; the bytes go up once,
    are parsed and decoded on the device, and the PCM comes back.  Frames whose bitstream ends early
    are dropped as the reference drops them (their PCM rows stay zero).  pns_state: the PNS LCG each
    stream's parser starts from (one value or one per stream).
    implicit_sbr: each stream's first frame is probed for an SBR payload (native.probe_sbr), and a
    stream that has one is opened as the facade opens it (native.implicit_sbr_cfg: output rate
    doubled, PS on a mono core): the device parses the core, the host the SBR / PS payloads
    (native.SbrDeviceParser), and the PCM rows are 2048 samples per channel."""
    import torch
    if not streams:
        return []
    cfg, offs, lens, fb, at = None, [], [], [0], 0
    for s in streams:
        h, o, n = adts_index(s)
        if h is None:
            raise N.JaadError(N.ERR_EOS, "no ADTS frame found")
        c = N.adts_cfg(h)
        if implicit_sbr and N.probe_sbr(c, bytes(s)[int(o[0]):int(o[0]) + int(n[0])]):
            c = N.implicit_sbr_cfg(c)
        if cfg is None:
            cfg = c
        elif bytes(c) != bytes(cfg):
            raise ValueError("decode_adts_streams: the streams differ in configuration")
        offs.append(o + np.uint64(at))
        lens.append(n)
        fb.append(fb[-1] + len(n))
        at += len(s)
    blob = np.frombuffer(b"".join(bytes(s) for s in streams), np.uint8)
    n_runs, nf = len(streams), fb[-1]
    with (N.SbrDeviceParser if cfg.sbr else N.DeviceParser)(cfg, device) as gp, N.Context(cfg, n_runs, device) as ctx:
        if cfg.sbr:
            parsers = [N.Parser(cfg) for _ in range(n_runs)]
            for p, s0 in zip(parsers, np.broadcast_to(np.asarray(pns_state, np.uint32), (n_runs,))):
                p.pns_state = int(s0)
            state = parsers
        else:
            state = N.gparse_state(n_runs, pns_state)
        rec = gp.parse_blob(blob, np.concatenate(offs), np.concatenate(lens), np.array(fb, np.uint32), state)
        if rec.status:
            bad = int(np.flatnonzero((rec.frame_result != 0) & (rec.frame_result != N.ERR_EOS))[0])
            raise N.JaadError(rec.status, f"jaad_gparse_batch (frame {bad})")
        nb = N.lib().jaad_frame_pcm_bytes(C.byref(cfg), flags)
        pcm = torch.zeros((nf, nb), dtype=torch.uint8, device=torch.device("cuda", device))
        # the kernel choice only: byte 0 of jaad_ics_info is window_sequence
        short = bool((rec.tensors["ics"][:, 0] == N.EIGHT_SHORT_SEQUENCE).any().item())
        torch.cuda.synchronize(pcm.device)  # the zeroed PCM is there before the decode writes into it
        ctx.decode_device(rec.dev, rec.batch, pcm.data_ptr(), nf * nb, flags | (N.HINT_SHORT_WINDOWS if short else 0))
        ctx.wait()
        host = pcm.cpu().numpy()
    return [np.ascontiguousarray(host[fb[r]:fb[r + 1]]) for r in range(n_runs)]
