"""CPU: the entry points of the online measurements are declared in both headers with the agreed signatures and exported by the
built libraries (core C-ABI: tmhip_slice_correlators, tmhip_polyakov_loop, tmhip_measure_oriented_plaquettes; drop-in:
tmlqcd_hip_slice_correlators, the reference's measure_oriented_plaquettes / oriented_plaquettes_measurement, tmlqcd_hip_polyakov_loop
and tmlqcd_hip_polyakov_loop_dir), the Python binding exposes them, the new unit is part of the library and every one of its kernels
is guarded by the resource check of the build."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
CORE = ["tmhip_slice_correlators", "tmhip_polyakov_loop", "tmhip_measure_oriented_plaquettes"]
DROPIN = ["tmlqcd_hip_slice_correlators", "measure_oriented_plaquettes", "oriented_plaquettes_measurement", "tmlqcd_hip_polyakov_loop",
          "tmlqcd_hip_polyakov_loop_dir"]


def _exports(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def _has(hdr, pattern):
    return re.search(re.sub(r" +", r"\\s*", pattern), hdr) is not None


def test_core_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    assert _has(hdr, r"int tmhip_slice_correlators\( tmhip_ctx \*\w* , const tmhip_field \*\w+ , const tmhip_field \*\w+ , int \w+ , "
                     r"double \*\w+ , double \*\w+ , double \*\w+ \) ;")
    assert _has(hdr, r"int tmhip_polyakov_loop\( tmhip_ctx \*\w* , int \w+ , double \*\w+ , double \*\w+ \) ;")
    assert _has(hdr, r"int tmhip_measure_oriented_plaquettes\( tmhip_ctx \*\w* , double \w+\[6\] \) ;")


def test_core_symbols_exported():
    assert set(CORE) <= _exports(os.path.join(LIB, "libtmlqcd_hip.so"))


def test_dropin_declares_and_exports_the_names():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    assert _has(hdr, r"void tmlqcd_hip_slice_correlators\( const spinor \* const even , const spinor \* const odd , const int dir , "
                     r"double \* const pp , double \* const pa , double \* const p4 \) ;")
    assert _has(hdr, r"void measure_oriented_plaquettes\( const su3 \*\* const gf , double \*plaq \) ;")               # meas/oriented_plaquettes.h
    assert _has(hdr, r"void oriented_plaquettes_measurement\( const int traj , const int id , const int ieo \) ;")
    assert _has(hdr, r"void tmlqcd_hip_polyakov_loop\( double pl\[2\] , const int dir \) ;")
    assert _has(hdr, r"int tmlqcd_hip_polyakov_loop_dir\( const int nstore , const int dir \) ;")
    assert set(DROPIN) <= _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))


def test_python_binding_has_the_methods():
    from tmlqcd_amd.hip import Lattice
    for m in ("slice_correlators", "polyakov_loop", "measure_oriented_plaquettes"):
        assert callable(getattr(Lattice, m))


def test_the_unit_is_built_and_its_kernels_are_guarded():
    mk = open(os.path.join(ROOT, "tmlqcd_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bmeas\.hip\b", mk, re.M) and re.search(r"^RU\s*=.*meas\.ru\.txt", mk, re.M)
    table = open(os.path.join(LIB, "resource_usage.txt")).read()
    rows = [l for l in table.splitlines() if re.match(r"(void )?meaship::", l)]
    names = " ".join(rows)
    for k in ("slice_t_kernel<true>", "slice_t_kernel<false>", "slice_z_kernel<true>", "slice_z_kernel<false>", "polyakov_kernel",
              "oriented_plaquette_kernel", "meas_final_kernel"):
        assert "meaship::" + k in names, k
    for l in rows:                                                             # no scratch, at least two waves per SIMD, verdict ok
        assert "(>= 2 waves)" in l and l.rstrip().endswith("ok"), l
