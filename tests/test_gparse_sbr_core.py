"""Device bitstream front end for HE-AAC, the parts that need no GPU (include/jaad_gparse.h).

* the C-ABI: exports, and the refusals jaad_gparse_create_sbr makes before it looks for a device;
* the split parse against the host parser: tools/gparse_sbr_diff.cpp, a stand-alone program built
  with ASan + UBSan, runs the SBR variant of the shared core, a scalar link pass, the shared
  bit-shift copy and the host tail stage over C4 / C5 streams and 20 000 bit-flipped / truncated
  mutants of their frames, and requires the statuses, records and parser state of jaad_parse_frame;
  it also checks the bit-shift copy against a bit-by-bit one."""
import ctypes as C
import re
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import pytest

from jaadec_amd import native as N

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
from gparse_sbr_streams import streams  # noqa: E402


def test_library_exports_the_sbr_entries_of_the_gparse_header():
    from test_abi import header_functions
    declared = header_functions(ROOT / "include" / "jaad_gparse.h")
    new = {"jaad_gparse_create_sbr", "jaad_gparse_batch_sbr", "jaad_gparse_last_ms_sbr"}
    assert new <= set(declared) and new <= set(N.GPARSE_EXPORTS)
    assert set(declared) == set(N.GPARSE_EXPORTS), declared
    for name in new:
        assert hasattr(N.lib(), name), name


def _create(cfg):
    h = C.c_void_p()
    rc = N.lib().jaad_gparse_create_sbr(C.byref(cfg), 0, C.byref(h))
    if rc == 0:
        N.lib().jaad_gparse_destroy(h)
    return rc


def test_create_sbr_refuses_before_it_looks_for_a_device():
    assert _create(N.make_cfg(sf_index=6, channel_config=2)) == N.ERR_UNSUPPORTED            # sbr = 0
    assert _create(N.make_cfg(sf_index=6, channel_config=2, sbr=True, ps=True)) == N.ERR_UNSUPPORTED  # PS on a CPE
    for chc in (3, 4, 5, 6, 7):
        assert _create(N.make_cfg(sf_index=6, channel_config=chc, sbr=True)) == N.ERR_UNSUPPORTED
    bad = N.make_cfg(sf_index=6, channel_config=2, sbr=True)
    bad.abi_version = N.ABI_VERSION + 1
    assert _create(bad) == N.ERR_ABI
    assert N.lib().jaad_gparse_create_sbr(None, 0, None) == N.ERR_INVALID_ARG


def test_create_sbr_without_a_device_reports_no_device():
    try:  # the same rule as jaad_ctx_create: a gfx950 device, or JAAD_ERR_NO_DEVICE
        N.Context(N.make_cfg(sf_index=3, channel_config=2), 1).close()
        want = N.OK
    except N.JaadError as e:
        assert e.status == N.ERR_NO_DEVICE
        want = N.ERR_NO_DEVICE
    # every configuration the call accepts, every ext_sf_index included
    for cfg in (N.make_cfg(sf_index=6, channel_config=2, sbr=True), N.make_cfg(sf_index=6, channel_config=1, sbr=True),
                N.make_cfg(sf_index=6, channel_config=1, sbr=True, ps=True)):
        for ext in (0, 3, 6, 11, 15):
            cfg.ext_sf_index = ext
            p = C.c_void_p()
            assert N.lib().jaad_parser_create(C.byref(cfg), C.byref(p)) == N.OK
            N.lib().jaad_parser_destroy(p)
            assert _create(cfg) == want
    if want:
        with pytest.raises(N.JaadError) as e:
            N.SbrDeviceParser(N.make_cfg(sf_index=6, channel_config=1, sbr=True, ps=True))
        assert e.value.status == N.ERR_NO_DEVICE


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_split_parse_equals_the_host_parser_under_sanitizers(tmp_path):
    seeds = tmp_path / "seeds.bin"
    run = 0
    with open(seeds, "wb") as out:
        for cfgid in (4, 5):
            for extras in (0, 3):
                # extras carry pulse data: once with the reference's parse (pulses dropped), once
                # with the spec-mode pulse tool
                for tns_mode in ((N.TNS_COMPAT, N.TNS_SPEC) if extras else (N.TNS_COMPAT,)):
                    cfg, runs, b = streams(cfgid, extras, tns_mode=tns_mode)
                    assert (b.sbr["status"] == N.SBR_UPSAMPLE).any() and (b.sbr["status"] == N.SBR_OK).any()
                    for frames, _ in runs:
                        for f in frames:
                            out.write(struct.pack("<BBBBBBI", cfg.sf_index, cfg.channel_config, tns_mode, cfg.ps,
                                                  cfg.ext_sf_index, run, len(f)) + f)
                        run += 1
    exe = tmp_path / "gparse_sbr_diff"
    csrc = ROOT / "jaadec_amd" / "csrc"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{csrc}",
                    str(ROOT / "tools" / "gparse_sbr_diff.cpp"), str(csrc / "jaad_parse.cpp"), str(csrc / "jaad_parse_sbr.cpp"),
                    str(csrc / "jaad_parse_tail.cpp"), str(csrc / "jaad_sbr_host.cpp"), "-pthread", "-o", str(exe)],
                   check=True, timeout=300)
    r = subprocess.run([str(exe), str(seeds), "20000"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "mismatches: 0" in r.stdout
    assert "tail copy: ok" in r.stdout  # 8 bit phases x 4 byte phases x 7 lengths, at the buffer's end too
    # not vacuous: every status the parser can end with occurs among the mutants, and OK, EOS and
    # UNSUPPORTED occur as decided by the host tail stage; no mutant is left out
    counts = {int(m.group(1)): (int(m.group(2)), int(m.group(3)))
              for m in re.finditer(r"status (-?\d+): (\d+), in the tail (\d+)", r.stdout)}
    for st in (N.OK, N.ERR_EOS, N.ERR_BITSTREAM, N.ERR_UNSUPPORTED):
        assert counts.get(st, (0, 0))[0] > 0, (st, counts)
    for st in (N.OK, N.ERR_EOS, N.ERR_UNSUPPORTED):
        assert counts.get(st, (0, 0))[1] > 0, (st, counts)
    assert sum(c[0] for c in counts.values()) == 20000
    assert int(re.search(r"seed frames without a payload: (\d+)", r.stdout).group(1)) > 0
