"""CPU: the gradient flow's entry points are declared in both headers with the agreed signatures and exported by the built
libraries (core C-ABI: tmhip_measure_field_strength, the tmhip_flow_* family and tmhip_gradient_flow; drop-in: the reference's
measure_clover_field_strength_observables and tmlqcd_hip_gradient_flow_measurement), the Python binding exposes them, the new
kernels are guarded by the resource check of the build, and the new unit is part of the library."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
CORE = ["tmhip_measure_field_strength", "tmhip_flow_begin", "tmhip_flow_step", "tmhip_flow_observables", "tmhip_flow_download",
        "tmhip_flow_end", "tmhip_gradient_flow"]


def _exports(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def _has(hdr, pattern):
    return re.search(re.sub(r" +", r"\\s*", pattern), hdr) is not None


def test_core_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    assert _has(hdr, r"int tmhip_measure_field_strength\( tmhip_ctx \*\w* , double \*\w+ , double \*\w+ \) ;")
    assert _has(hdr, r"int tmhip_flow_begin\( tmhip_ctx \*\w* \) ;")
    assert _has(hdr, r"int tmhip_flow_step\( tmhip_ctx \*\w* , double \w+ \) ;")
    assert _has(hdr, r"int tmhip_flow_observables\( tmhip_ctx \*\w* , double \*\w+ , double \*\w+ , double \*\w+ \) ;")
    assert _has(hdr, r"int tmhip_flow_download\( tmhip_ctx \*\w* , void \*\w+ \) ;")
    assert _has(hdr, r"int tmhip_flow_end\( tmhip_ctx \*\w* \) ;")
    assert _has(hdr, r"int tmhip_gradient_flow\( tmhip_ctx \*\w* , double \w+ , double \w+ , int \w+ , double \*\w+ , int \*\w+ \) ;")


def test_core_symbols_exported():
    assert set(CORE) <= _exports(os.path.join(LIB, "libtmlqcd_hip.so"))


def test_dropin_declares_and_exports_the_names():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    assert _has(hdr, r"typedef struct \{ double E ; double Q ; \} field_strength_obs_t ;")
    # meas/measure_clover_field_strength_observables.h
    assert _has(hdr, r"void measure_clover_field_strength_observables\( const su3 \*\* const gf , field_strength_obs_t \* const \w+ \) ;")
    assert _has(hdr, r"void tmlqcd_hip_gradient_flow_measurement\( const int traj , const double eps , const double tmax \) ;")
    syms = _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))
    assert {"measure_clover_field_strength_observables", "tmlqcd_hip_gradient_flow_measurement"} <= syms


def test_python_binding_has_the_methods():
    from tmlqcd_amd.hip import Lattice
    for m in ("measure_field_strength", "flow_begin", "flow_step", "flow_observables", "flow_links", "flow_end", "gradient_flow"):
        assert callable(getattr(Lattice, m))


def test_the_unit_is_built_and_its_kernels_are_guarded():
    mk = open(os.path.join(ROOT, "tmlqcd_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bflow\.hip\b", mk, re.M) and re.search(r"^RU\s*=.*flow\.ru\.txt", mk, re.M)
    table = open(os.path.join(LIB, "resource_usage.txt")).read()
    rows = [l for l in table.splitlines() if re.match(r"(void )?flowhip::(flow_stage_kernel<[012]>|field_strength_kernel)\s", l)]
    assert len(rows) == 4, rows
    for l in rows:                                                             # no scratch, at least two waves per SIMD, verdict ok
        assert "(>= 2 waves)" in l and l.rstrip().endswith("ok"), l
