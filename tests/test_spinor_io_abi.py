"""CPU: the propagator / source I/O is exported and declared -- the core C-ABI (include/tmlqcd_hip.h), read_spinor under its reference
name and the tmlqcd_hip_* additions in the drop-in (include/tmlqcd_dropin.h), the Python mirror, the resource guard -- and the drop-in
still loads next to a host program that has none of the globals it newly reads."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
CORE = ["tmhip_spinor_pack", "tmhip_spinor_unpack", "tmhip_read_spinor", "tmhip_write_spinor", "tmhip_source_point"]
DROPIN = ["read_spinor", "tmlqcd_hip_write_spinor", "tmlqcd_hip_write_lime_message", "tmlqcd_hip_source_spinor_field",
          "tmlqcd_hip_source_spinor_field_point_from_file"]


def _nm(so, *flags):
    out = subprocess.run(["nm", "-D"] + list(flags) + [so], stdout=subprocess.PIPE, text=True, check=True).stdout
    return [l.split() for l in out.splitlines() if l.strip()]


def test_core_symbols_exported_and_declared():
    syms = {l[-1] for l in _nm(os.path.join(LIB, "libtmlqcd_hip.so"), "--defined-only")}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read(), flags=re.S)
    for n in CORE:
        assert n in syms, n
        assert re.search(r"\bint\s+%s\(tmhip_ctx \*ctx" % n, hdr), n
    assert "tmhip_write_lime_message" in syms and re.search(r"\bint\s+tmhip_write_lime_message\(const char \*filename", hdr)
    assert re.search(r"\}\s*tmhip_spinor_info\s*;", hdr)


def test_header_cites_the_reference_lines():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    for cite in ("io/spinor_write_binary.c:145-224", "io/dml.c:49-60", "io/spinor_read.c:27-150", "io/utils_parse_propagator_type.c:22-91",
                 "io/spinor_write.c:23-47", "start.c:707-741", "start.c:743-830", "tmhip_field_even(full), tmhip_field_odd(full)"):
        assert cite in hdr, cite


def test_dropin_symbols():
    so = os.path.join(LIB, "libtmlqcd_dropin.so")
    defined = {l[-1]: l[-2] for l in _nm(so, "--defined-only")}
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    for n in DROPIN:
        assert defined.get(n) == "T", n
        assert re.search(r"\b%s\(" % n, hdr), n
    assert re.search(r"int\s+read_spinor\(spinor\s*\*\s*const\s+s\s*,\s*spinor\s*\*\s*const\s+r\s*,\s*char\s*\*\s*filename\s*,\s*const\s+int\s+position\s*\)\s*;", hdr)
    # PropInfo and SourceInfo stay with io/spinor_read.o of the host program
    assert "PropInfo" not in defined and "SourceInfo" not in defined
    # every host global that read_spinor newly reads is a weak reference
    undefined = {l[-1]: l[-2] for l in _nm(so, "--undefined-only")}
    for g in ("g_disable_src_IO_checks", "g_debug_level", "g_cart_id"):
        assert undefined.get(g) == "w", g


def test_dropin_loads_next_to_the_host_stub(host_stub):
    stub, d = host_stub
    src = open(os.path.join(ROOT, "tests", "host_stub", "globals.c")).read()
    assert "g_disable_src_IO_checks" not in src          # the stub has none of them: the weak references are what lets this load
    for n in DROPIN:
        assert getattr(d, n) is not None


def test_python_mirror_declares_them():
    from tmlqcd_amd import hip
    lib = hip.load_library()
    for n in CORE + ["tmhip_write_lime_message"]:
        assert getattr(lib, n).argtypes is not None, n
    for m in ("spinor_pack", "spinor_unpack", "read_spinor", "write_spinor", "source_point"):
        assert callable(getattr(hip.Lattice, m)), m
    assert callable(hip.write_lime_message)


def test_write_lime_message_needs_no_device(tmp_path):
    """Host code only: two records, the second appended; the bytes are the restatement's."""
    from tests import spinor_io_restate as sr
    from tmlqcd_amd import hip
    p = tmp_path / "m.lime"
    hip.write_lime_message(p, "propagator-type", "DiracFermion_Sink", 1, 1, append=False)
    hip.write_lime_message(p, "inversion-info", "solver = CG\n epssq = 1e-18\n", 1, 0)
    want = sr.lime_record(1, 1, "propagator-type", "DiracFermion_Sink") + sr.lime_record(1, 0, "inversion-info", "solver = CG\n epssq = 1e-18\n")
    assert p.read_bytes() == want


def test_resource_guard_lists_the_kernels():
    table = open(os.path.join(LIB, "resource_usage.txt")).read()
    rows = [l for l in table.splitlines() if l.startswith("void spinor_io_kernel<")]
    assert len(rows) == 4 and all("spinor record pack / unpack" in l and l.rstrip().endswith("ok") for l in rows)
    for l in rows:                                            # columns: name, VGPR, AGPR, scratch, occ, LDS, guard
        m = re.search(r">\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s", l)
        assert m and int(m.group(3)) == 0, l                  # no scratch
