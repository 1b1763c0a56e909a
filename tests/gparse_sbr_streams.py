"""Synthetic HE-AAC streams as raw_data_blocks for the device front end's SBR tests
(test_gparse_sbr_core.py, test_gparse_sbr_gpu.py): the C4 (stereo SBR) and C5 (mono SBR + PS)
generator configurations written by the test writer, with frames that carry no payload."""
from functools import lru_cache

from jaadec_amd import native as N
from oracle import oracle as O


@lru_cache(maxsize=None)
def streams(cfgid, extras=0, frames=12, n_streams=2, seed=0x5EED40, tns_mode=N.TNS_COMPAT, upsample_percent=20):
    """(cfg, per run: (frames, pns0), the generator's batch): n_streams runs of `frames` frames.
    upsample_percent of the frames have no SBR payload (JAAD_SBR_UPSAMPLE), some are coupled, and
    the first frames come before the first SBR header."""
    p = N.synth_params(cfgid, n_streams=n_streams, frames_per_stream=frames, coupling_percent=50,
                       upsample_percent=upsample_percent, nohdr_frames=1, seed=seed + cfgid)
    b = N.synth_batch(p)
    cfg = N.cfg_for(p, tns_mode)
    runs = []
    for r in range(n_streams):
        one = b.select_runs([r])
        w = O.SbrWriter(cfg.ext_sf_index, seed + r)
        runs.append((tuple(O.write_frames(one, p.sf_index, extras=extras, sbr_writer=w)), int(one.ics["pns_state"][0])))
    return cfg, tuple(runs), b
