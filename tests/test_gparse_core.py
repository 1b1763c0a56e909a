"""Device bitstream front end, the parts that need no GPU (include/jaad_gparse.h).

* the C-ABI: exports, and the refusals jaad_gparse_create makes before it looks for a device;
* the parse core shared by host and device (jaadec_amd/csrc/jaad_parse_core.h) against the host
  parser: tools/gparse_diff.cpp, a stand-alone program built with ASan + UBSan, runs both over the
  round-trip cases of tests/test_parse.py and 20 000 bit-flipped / truncated mutants of them and
  requires the same status, records and state; it also checks the LCG jump of the link pass."""
import ctypes as C
import re
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import pytest

from jaadec_amd import native as N
from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))


def test_library_exports_the_gparse_header():
    from test_abi import header_functions
    declared = header_functions(ROOT / "include" / "jaad_gparse.h")
    assert set(declared) == set(N.GPARSE_EXPORTS), declared
    lib = N.lib()
    for name in declared:
        assert hasattr(lib, name), name


def _create(cfg):
    h = C.c_void_p()
    rc = N.lib().jaad_gparse_create(C.byref(cfg), 0, C.byref(h))
    if rc == 0:
        N.lib().jaad_gparse_destroy(h)
    return rc


def test_create_refuses_what_stays_on_the_host_parser_before_it_looks_for_a_device():
    assert _create(N.make_cfg(sf_index=6, channel_config=2, sbr=True)) == N.ERR_UNSUPPORTED
    assert _create(N.make_cfg(sf_index=6, channel_config=1, ps=True)) == N.ERR_UNSUPPORTED
    assert _create(N.make_cfg(sf_index=3, channel_config=3)) == N.ERR_UNSUPPORTED
    bad = N.make_cfg()
    bad.abi_version = N.ABI_VERSION + 1
    assert _create(bad) == N.ERR_ABI
    assert N.lib().jaad_gparse_create(None, 0, None) == N.ERR_INVALID_ARG


def test_create_without_a_device_reports_no_device():
    cfg = N.make_cfg(sf_index=3, channel_config=2)
    try:  # the same rule as jaad_ctx_create: a gfx950 device, or JAAD_ERR_NO_DEVICE
        N.Context(cfg, 1).close()
        want = N.OK
    except N.JaadError as e:
        assert e.status == N.ERR_NO_DEVICE
        want = N.ERR_NO_DEVICE
    assert _create(cfg) == want
    if want:
        with pytest.raises(N.JaadError) as e:
            N.DeviceParser(N.make_cfg(sf_index=4, channel_config=1))
        assert e.value.status == N.ERR_NO_DEVICE


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_shared_core_equals_the_host_parser_under_sanitizers(tmp_path):
    from test_parse import CASES
    seeds = tmp_path / "seeds.bin"
    with open(seeds, "wb") as out:
        for case in sorted(CASES):
            cfgid, over = CASES[case]
            p = N.synth_params(cfgid, **over)
            b = N.synth_batch(p)
            for extras in (0, 3):
                # extras carry pulse data: once with the reference's parse (pulses dropped), once
                # with the spec-mode pulse tool
                for tns_mode in ((N.TNS_COMPAT, N.TNS_SPEC) if extras else (N.TNS_COMPAT,)):
                    for f in O.write_frames(b, p.sf_index, extras=extras):
                        out.write(struct.pack("<BBBI", p.sf_index, p.channel_config, tns_mode, len(f)) + f)
    exe = tmp_path / "gparse_diff"
    csrc = ROOT / "jaadec_amd" / "csrc"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{csrc}",
                    str(ROOT / "tools" / "gparse_diff.cpp"), str(csrc / "jaad_parse.cpp"), str(csrc / "jaad_parse_sbr.cpp"),
                    str(csrc / "jaad_sbr_host.cpp"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe), str(seeds), "20000"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "mismatches: 0" in r.stdout
    assert "lcg jump: ok" in r.stdout  # n steps by the power table == n single steps
    # every status the parser can end with occurs among the mutants: the comparison is not vacuous
    counts = {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"status (-?\d+): (\d+)", r.stdout)}
    for st in (N.OK, N.ERR_EOS, N.ERR_BITSTREAM, N.ERR_UNSUPPORTED):
        assert counts.get(st, 0) > 0, (st, counts)
    assert sum(counts.values()) == 20000
