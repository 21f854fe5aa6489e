"""The host program in miniature behind every tests/*_child.py and every tests/mp_*_worker.py that drives libtmlqcd_dropin.so.

How to add a drop-in child:
  1. tests/NAME_dropin_child.py puts the repository root on sys.path and says `from tests import hostprog`.
  2. `stub, extra, d = hostprog.load()`; globals the stub lacks go in as C source, `load(extra_c=hostprog.ND_GLOBALS)`.
  3. Every symbol it calls gets one line in PROTOTYPES below (tests/test_hostprog.py holds the table against the header);
     functions of its own C source go to load() as extra_prototypes, a table of the same form.  No child assigns .argtypes or .restype.
  4. `hostprog.init_lattice(stub, T, LX, LY, LZ, gauge, kappa)` makes the geometry and copies the links in.
  5. `with hostprog.HostFields(stub, d, mode) as hf:` sets the residency mode and resets it on the way out; `hf.arr(sites, init)`
     is a host spinor array as (numpy view, pointer), `hf.copy(a)` its content once the device's result is on the host.
  6. `hostprog.emit(results)` prints the one JSON line; the parent test gets it back from `hostprog.run_child("NAME_dropin_child.py", mode)`.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB_DIR = os.path.join(ROOT, "tests", "host_stub")
DROPIN = os.path.join(ROOT, "tmlqcd_amd", "lib", "libtmlqcd_dropin.so")
MODES = {"coherent": 0, "resident": 1, "lazy": 2}

VP, D, I, S, UL = C.c_void_p, C.c_double, C.c_int, C.c_char_p, C.c_ulong
PD, PI, PVP, PUL = C.POINTER(D), C.POINTER(I), C.POINTER(VP), C.POINTER(UL)

# ---- globals of a host program that tests/host_stub/globals.c does not have
ND_GLOBALS = """
double g_mubar = 0.0, g_epsbar = 0.0, phmc_invmaxev = 1.0;
void nd_set(double a, double b, double c) { g_mubar = a; g_epsbar = b; phmc_invmaxev = c; }
"""
SLOPPY_GLOBALS = """
int g_sloppy_precision = 0;
void set_sloppy(int v) { g_sloppy_precision = v; }
int get_sloppy(void) { return g_sloppy_precision; }
"""
WRAPPED_QTM_PM_PSI = """
extern void Qtm_pm_psi(void *, void *);
void wrapped_Qtm_pm_psi(void *l, void *k) { Qtm_pm_psi(l, k); }
"""


class SolverParams(C.Structure):   # include/tmlqcd_dropin.h: tmlqcd_solver_params (solver/solver_params.h:46-109)
    _fields_ = [("eigcg_i", I * 5), ("eigcg_d", D * 3), ("eigcg_rand_guess_opt", I), ("mcg_delta", C.c_float),
                ("type", I), ("max_iter", I), ("rel_prec", I), ("no_shifts", I), ("sdim", I),
                ("squared_solver_prec", D), ("M_psi", VP), ("M_psi32", VP), ("M_ndpsi", VP), ("M_ndpsi32", VP),
                ("shifts", PD), ("solution_type", I), ("compression_type", I), ("sloppy_precision", I), ("external_inverter", I)]


class HF(C.Structure):        # hamiltonian_field.h:26-32
    _fields_ = [("gaugefield", VP), ("momenta", VP), ("derivative", VP), ("update_gauge_copy", I), ("traj_counter", I)]


class FSO(C.Structure):       # meas/field_strength_types.h
    _fields_ = [("E", D), ("Q", D)]


class Cplx(C.Structure):      # _Complex double returned by value
    _fields_ = [("re", D), ("im", D)]


class GaugeInfo(C.Structure):  # io/params.h:98-104, first member
    _fields_ = [("plaquetteEnergy", D)]


PHF, PSP = C.POINTER(HF), C.POINTER(SolverParams)
_OP1 = (None, [VP, VP])                                    # void f(spinor *l, spinor *k)
_OP2 = (None, [VP] * 4)                                    # void f(spinor *l_s, spinor *l_c, spinor *k_s, spinor *k_c)
_SOLVER = (I, [VP, VP, I, D, I, I, VP])
_RAT = (I, [VP, PD, PD, I, I, D, I, PD])
_RATCOR = (I, [VP, PD, PD, D, I, I, D, I, PD, PI])
_NDRATCOR = (I, [VP, VP, PD, PD, D, I, I, D, I, PD, PI])

# name -> (restype, argtypes).  stub_*: tests/host_stub/globals.c; the rest: include/tmlqcd_dropin.h.  A _Complex double passed by
# value is its (re, im) pair in two SSE registers: two doubles here.
PROTOTYPES = {
    "stub_init": (VP, [I] * 4), "stub_init_rank": (VP, [I] * 6), "stub_boundary": (None, [D] * 5),
    "stub_set_mu": (None, [D]), "stub_get_mu": (D, []), "stub_calloc": (VP, [C.c_size_t]), "stub_init_clover": (VP, [I]),
    "stub_mark_gauge_dirty": (None, []), "stub_gauge_flag": (I, []), "stub_install_segv_probe": (I, []), "stub_touch_guard": (I, []),
    # residency and bookkeeping
    "tmlqcd_hip_set_residency": (None, [I]), "tmlqcd_hip_sync_to_host": (None, [VP]), "tmlqcd_hip_host_modified": (None, [VP]),
    "tmlqcd_hip_lazy_stats": (None, [PUL]), "tmlqcd_hip_transfer_counts": (None, [PUL]), "tmlqcd_hip_calls": (UL, []),
    "tmlqcd_hip_finalize": (None, []), "tmlqcd_hip_comm_init_shm": (None, [S]), "tmlqcd_hip_comm_init_ipc": (I, []),
    # operators
    "Hopping_Matrix": (None, [I, VP, VP]), "D_psi": _OP1, "Q_pm_psi": _OP1, "Qtm_pm_psi": _OP1, "Qtm_plus_psi": _OP1, "Qtm_minus_psi": _OP1,
    "Mtm_plus_sym_psi": _OP1, "Qsw_pm_psi": _OP1, "H_eo_tm_inv_psi": (None, [VP, VP, I, D]),
    "Qtm_ndpsi": _OP2, "Qtm_dagger_ndpsi": _OP2, "Qtm_pm_ndpsi": _OP2, "Qsw_pm_ndpsi": _OP2,
    "M_ee_inv_ndpsi": (None, [VP] * 4 + [D] * 2), "H_eo_tm_ndpsi": (None, [VP] * 4 + [I]), "mul_one_pm_itau2": (None, [VP] * 4 + [D, I]),
    # linalg
    "square_norm": (D, [VP, I, I]), "scalar_prod_r": (D, [VP, VP, I, I]), "scalar_prod": (Cplx, [VP, VP, I, I]),
    "assign_diff_mul": (None, [VP, VP, D, D, I]), "mul": (None, [VP, D, D, VP, I]),
    "assign_add_mul_add_mul": (None, [VP, VP, VP, D, D, D, D, I]), "assign_mul_bra_add_mul_ket_add": (None, [VP, VP, VP, D, D, D, D, I]),
    "assign_mul_add_mul_add_mul_add_mul_r": (None, [VP] * 4 + [D] * 4 + [I]),
    # solvers
    "cg_her": _SOLVER, "bicgstab_complex": _SOLVER, "cg_her_nd": (I, [VP] * 4 + [I, D, I, I, VP]),
    "cg_mms_tm": (I, [PVP, VP, PSP, PD]), "cg_mms_tm_nd": (I, [PVP, PVP, VP, VP, PSP]),
    "chrono_guess": (I, [VP, VP, PVP, PI, I, I, I, VP]), "chrono_add_solution": (None, [VP, PVP, PI, I, PI, I]),
    "eigenvalues_bi": (D, [PI, I, D, I, VP]), "tmlqcd_hip_eigenvalues": (D, [PI, I, D, I, VP, PD]),
    "tmlqcd_hip_phmc_compute_ev": (I, [I, I, S, D, I, D, PD, PD]),
    # clover term
    "tmlqcd_hip_sw_term": (None, [D, D]), "tmlqcd_hip_sw_invert": (None, [I, D]), "sw_invert_nd": (None, [D]),
    "tmlqcd_hip_sw_invert_failures": (I, []), "tmlqcd_hip_update_clover": (None, []),
    "sw_trace": (D, [I, D]), "sw_trace_nd": (D, [I, D, D]), "tmlqcd_hip_sw_trace_failures": (I, []),
    # molecular dynamics and the trajectory frame
    "deriv_Sb": (None, [I, VP, VP, PHF, D]), "tmlqcd_hip_gauge_derivative": (None, [PHF, D, D, D, I, D]),
    "tmlqcd_hip_flush_derivative": (None, [PHF]), "tmlqcd_hip_update_gauge": (None, [D, PHF]), "tmlqcd_hip_update_momenta": (None, [D, PHF]),
    "tmlqcd_hip_sync_gauge_to_host": (None, [PHF]), "tmlqcd_hip_sync_momenta_to_host": (None, [PHF]),
    "tmlqcd_hip_gauge_snapshot": (None, [PHF]), "tmlqcd_hip_gauge_snapshot_diff": (D, [PHF]), "tmlqcd_hip_moment_energy": (D, [PHF]),
    "tmlqcd_hip_accept_links": (None, [PHF, I]), "tmlqcd_hip_reject_links": (None, [PHF]), "tmlqcd_hip_force_norms": (None, [PHF, PD, PD]),
    # monomials
    "tmlqcd_hip_cloverrat_derivative": (I, [PHF, VP, PD, PD, I, D, D, I, I, D, I]),
    "tmlqcd_hip_cloverrat_heatbath": _RAT, "tmlqcd_hip_cloverrat_acc": _RAT,
    "tmlqcd_hip_ndcloverrat_derivative": (I, [PHF, VP, VP, PD, PD, I, D, D, D, I, I, D, I]),
    "tmlqcd_hip_ratcor_heatbath": _RATCOR, "tmlqcd_hip_ratcor_acc": _RATCOR,
    "tmlqcd_hip_cloverratcor_heatbath": _RATCOR, "tmlqcd_hip_cloverratcor_acc": _RATCOR,
    "tmlqcd_hip_ndratcor_heatbath": _NDRATCOR, "tmlqcd_hip_ndratcor_acc": _NDRATCOR,
    "tmlqcd_hip_ndcloverratcor_heatbath": _NDRATCOR, "tmlqcd_hip_ndcloverratcor_acc": _NDRATCOR,
    "Ptilde_ndpsi": (None, [VP, VP, PD, I, VP, VP, VP]), "tmlqcd_hip_ndpoly_derivative": (I, [PHF, VP, VP, PD, I, D, D]),
    "tmlqcd_hip_ndpoly_heatbath": (I, [VP, VP, PD, I, D, D, PD, I, D, PD]),
    "tmlqcd_hip_ndpoly_acc": (I, [VP, VP, PD, I, D, D, PD, PD, I, D, D, PD]),
    # measurements and I/O
    "measure_plaquette": (D, [VP]), "measure_gauge_action": (D, [VP, D]),
    "measure_clover_field_strength_observables": (None, [VP, C.POINTER(FSO)]), "tmlqcd_hip_gradient_flow_measurement": (None, [I, D, D]),
    "tmlqcd_hip_slice_correlators": (None, [VP, VP, I, PD, PD, PD]), "measure_oriented_plaquettes": (None, [VP, PD]),
    "oriented_plaquettes_measurement": (None, [I, I, I]), "tmlqcd_hip_polyakov_loop": (None, [PD, I]), "tmlqcd_hip_polyakov_loop_dir": (I, [I, I]),
    "tmlqcd_hip_source_spinor_field": (None, [VP, VP, I, I]), "tmlqcd_hip_source_spinor_field_point_from_file": (None, [VP, VP, I, I, I]),
    "read_spinor": (I, [VP, VP, S, I]), "tmlqcd_hip_write_spinor": (I, [S, I, PVP, PVP, I, I]),
    "tmlqcd_hip_write_lime_message": (I, [S, I, S, S, I, I]),
}
# functions of the snippets above: applied to those an extra source defines
SNIPPET_PROTOTYPES = {"nd_set": (None, [D] * 3), "set_sloppy": (None, [I]), "get_sloppy": (I, [])}


def set_prototypes(lib, table):
    """restype and argtypes of every name in table (name -> (restype, argtypes)); a name the library lacks is an AttributeError"""
    for name, proto in table.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = proto


def build_stub():
    """tests/host_stub/libtmhost.so, rebuilt when older than globals.c: the file and the rule of the host_stub fixture."""
    so, src = os.path.join(STUB_DIR, "libtmhost.so"), os.path.join(STUB_DIR, "globals.c")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        mine = so + ".%d" % os.getpid()
        try:
            subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-shared", "-o", mine, src, "-lm"])
            os.replace(mine, so)       # (several ranks may get here at once)
        finally:
            if os.path.exists(mine):   # gcc failed half way
                os.remove(mine)
    return so


def load(extra_c=None, core_first=False, extra_prototypes=None):
    """(stub, extra, dropin), loaded RTLD_GLOBAL in this order so that the drop-in's weak references bind to the host program's
    globals -- which needs a fresh process.  extra is None without extra_c; extra_prototypes is the table of the functions that a
    child's own extra_c defines."""
    stub = C.CDLL(build_stub(), mode=C.RTLD_GLOBAL)
    extra = None
    if extra_c:
        with tempfile.TemporaryDirectory() as tmp:       # a loaded object may be unlinked
            src, so = os.path.join(tmp, "extra.c"), os.path.join(tmp, "libextra.so")
            open(src, "w").write(extra_c)
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-o", so, src])
            extra = C.CDLL(so, mode=C.RTLD_GLOBAL | os.RTLD_LAZY)     # lazy: it may call into the drop-in, which comes next
    if core_first:
        import tmlqcd_amd
        tmlqcd_amd.load_library()
    dropin = C.CDLL(DROPIN, mode=C.RTLD_GLOBAL)
    set_prototypes(stub, {n: p for n, p in PROTOTYPES.items() if n.startswith("stub_")})
    set_prototypes(dropin, {n: p for n, p in PROTOTYPES.items() if not n.startswith("stub_")})
    if extra is not None:
        set_prototypes(extra, {n: p for n, p in SNIPPET_PROTOTYPES.items() if hasattr(extra, n)})
        set_prototypes(extra, extra_prototypes or {})
    return stub, extra, dropin


def init_lattice(stub, T, LX, LY, LZ, gauge, kappa, theta=(0., 0., 0., 0.), rank=None):
    """Geometry (rank = (nproc_t, proc_t) on a T-split lattice), the links copied into g_gauge_field, kappa and the boundary
    phases.  Returns the address of g_gauge_field[0]."""
    g = stub.stub_init(T, LX, LY, LZ) if rank is None else stub.stub_init_rank(T, LX, LY, LZ, *rank)
    gauge = np.ascontiguousarray(gauge)
    C.memmove(g, gauge.ctypes.data, gauge.nbytes)
    stub.stub_boundary(kappa, *theta)
    return g


class HostFields:
    """The host program's spinor arrays in one residency mode.  `with HostFields(...)` sets the mode and sets it back to coherent
    on the way out; a child that ends with tmlqcd_hip_finalize() instead sets the mode itself (MODES) and uses arr / copy alone."""

    def __init__(self, stub, dropin, mode, modes=tuple(MODES)):
        assert mode in modes, "%r is not one of %r" % (mode, modes)
        self.stub, self.dropin, self.mode = stub, dropin, mode

    def __enter__(self):
        self.dropin.tmlqcd_hip_set_residency(MODES[self.mode])
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            self.dropin.tmlqcd_hip_set_residency(0)

    def arr(self, sites, init=None, dtype=np.float64):
        """(numpy view [sites][4][3][2], pointer) on page-aligned memory (watchable in lazy mode), as a host program's own fields"""
        nbytes = sites * 24 * np.dtype(dtype).itemsize
        p = self.stub.stub_calloc(nbytes)
        a = np.frombuffer((C.c_char * nbytes).from_address(p), dtype=dtype).reshape(sites, 4, 3, 2)
        if init is not None:
            a[:] = init
        return a, p

    def copy(self, a):
        if self.mode == "resident":
            self.dropin.tmlqcd_hip_sync_to_host(a[1])
        return a[0].copy()


def rel_l2(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def rel_max(a, b):
    """max |a-b| / max |b|: tests.util.rel_err without its floor on the denominator"""
    return float(np.abs(a - b).max() / np.abs(b).max())


def emit(results):
    print(json.dumps(results))
    sys.stdout.flush()


def last_json(r):
    return json.loads(r.stdout.strip().splitlines()[-1])


def run_child(script, *args, cwd=ROOT, timeout=300, env=None, check=True):
    """tests/<script> in a fresh interpreter.  check: exit status 0 is asserted and the parsed last line of its output returned;
    otherwise the CompletedProcess, for the caller to judge."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script)] + list(args), cwd=cwd, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    if not check:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    return last_json(r)
