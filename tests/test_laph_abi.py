"""CPU: the LapH entry points are exported, declared and mirrored -- the core C-ABI (include/tmlqcd_hip.h) with its Python mirror,
Jacobi in the drop-in with the prototype of the reference's jacobi.h, the new unit and its register-usage file in the Makefile, the
resource rules of its kernels, and fixtures that say how they were made."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
CORE = ("tmhip_cvfield_alloc", "tmhip_cvfield_upload", "tmhip_cvfield_download", "tmhip_cvfield_upload_slices", "tmhip_cvfield_download_slices",
        "tmhip_cvfield_zero", "tmhip_laph_apply", "tmhip_laph_apply_dot", "tmhip_laph_apply_filter", "tmhip_laph_dots", "tmhip_laph_project",
        "tmhip_laph_normalise", "tmhip_laph_rotate", "tmhip_laph_set_interval", "tmhip_laph_eigensystem", "tmhip_laph_write", "tmhip_laph_timing")
PYTHON = ("cvfield", "laph_apply", "laph_dots", "laph_project", "laph_normalise", "laph_rotate", "laph_eigensystem", "laph_set_interval",
          "laph_write", "laph_timing")


def _exports(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_core_symbols_exported_declared_and_mirrored():
    import tmlqcd_amd
    syms, hdr = _exports(os.path.join(LIB, "libtmlqcd_hip.so")), _read("include", "tmlqcd_hip.h")
    lib = tmlqcd_amd.load_library()
    for name in CORE:
        assert name in syms, name
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(getattr(lib, name).argtypes) == len(args.split(",")), name
    assert "tmhip_cvfield_free" in syms and re.search(r"\bvoid\s+tmhip_cvfield_free\s*\(", hdr)
    assert re.search(r"#define\s+TMHIP_LAPH_MAX_BASIS\s+128\b", hdr)
    for name in PYTHON:
        assert callable(getattr(tmlqcd_amd.Lattice, name)), name
    from tmlqcd_amd.hip import CvField
    for name in ("upload", "download", "zero", "free"):
        assert callable(getattr(CvField, name)), name


def test_options_are_known_to_the_library_and_the_documents():
    src = _read("tmlqcd_amd", "csrc", "context.hip")
    for opt in ("laph_fused", "laph_cheb", "laph_basis"):
        assert len(re.findall(r'strcmp\(name, "%s"\)' % opt, src)) == 2, opt      # tmhip_set_option and tmhip_get_option
        assert opt in _read("include", "tmlqcd_hip.h") and opt in _read("README.md")


def test_dropin_declares_jacobi_as_the_reference_does():
    hdr = _read("include", "tmlqcd_dropin.h")
    proto = r"void\s+Jacobi\(\s*su3_vector\s*\*\s*const\s+l\s*,\s*su3_vector\s*\*\s*const\s+k\s*,\s*int\s+t\s*\)\s*;"
    assert re.search(proto, hdr)
    ref = os.path.join(os.environ.get("TMLQCD_REF", "/root/reference"), "jacobi.h")
    if os.path.exists(ref):                                     # the same expression finds the reference's own declaration
        assert re.search(proto, open(ref).read())
    assert re.search(r"int\s+tmlqcd_hip_laph_eigensystem\(\s*const\s+int\s+nev\s*,\s*const\s+double\s+prec\s*,\s*const\s+int\s+max_apps\s*,\s*const\s+int\s+nstore\s*\)\s*;", hdr)
    syms = _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))
    assert "Jacobi" in syms and "tmlqcd_hip_laph_eigensystem" in syms


def test_the_unit_is_built_and_its_kernels_are_guarded():
    mk = _read("tmlqcd_amd", "csrc", "Makefile")
    assert re.search(r"^SRCS\s*=.*\blaph\.hip\b", mk, re.M) and re.search(r"^RU\s*=.*laph\.ru\.txt", mk, re.M)
    table = _read("tmlqcd_amd", "lib", "resource_usage.txt")
    rows = [l for l in table.splitlines() if re.match(r"(void )?laphhip::", l)]
    floors = {"laph_kernel<0>": 3, "laph_kernel<1>": 3, "laph_kernel<2>": 3, "laph_dots_kernel": 8, "laph_project_kernel": 8, "laph_scale_kernel": 8,
              "laph_comb_kernel": 8, "laph_final_kernel": 8, "laph_fill_kernel": 8, "laph_rotate_kernel": 4, "cv_layout_kernel<true>": 8,
              "cv_layout_kernel<false>": 8}
    for k, floor in floors.items():
        row = [l for l in rows if "laphhip::" + k in l]
        assert row and "(>= %d waves)" % floor in row[0] and row[0].rstrip().endswith("ok"), k
    assert len(rows) == len(floors)                             # no kernel of the unit without a rule


def test_fixtures_describe_their_runs():
    for tag, dims in (("4x4", (4, 4, 4, 4)), ("8x6x4x12", (8, 6, 4, 12))):
        z = np.load(os.path.join(ROOT, "tests", "golden", "ref_laph_%s.npz" % tag))
        T, S3 = dims[0], dims[1] * dims[2] * dims[3]
        assert tuple(z["dims"]) == dims and z["k"].shape == z["l"].shape == (T, S3, 3, 2)
        assert z["iup3d"].shape == z["idn3d"].shape == (S3, 4)
        assert "Jacobi" in str(z["run"]) and "WITHLAPH" in str(z["run"]) and str(z["gauge_from"])
        k = np.random.default_rng(int(z["seed"])).standard_normal((T, S3, 3, 2))
        assert np.array_equal(k, z["k"])                        # the input can be made again from the seed
