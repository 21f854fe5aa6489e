"""CPU: the harness of the drop-in children (tests/hostprog.py): its prototype table against libtmlqcd_dropin.so and
include/tmlqcd_dropin.h, its SolverParams against tmlqcd_solver_params, build_stub() from two processes at once, and the temporary
directory of load(extra_c=...)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from tests import hostprog
from tests.test_abi import exported

ROOT = hostprog.ROOT
# in the table, not in include/tmlqcd_dropin.h: nothing at present (a reference symbol declared elsewhere would go here, with a word why)
NOT_IN_HEADER = ()
DROPIN_NAMES = sorted(n for n in hostprog.PROTOTYPES if not n.startswith("stub_"))


def declarations():
    """name -> (return type, [parameter, ...]) of include/tmlqcd_dropin.h, after the stripping of test_abi.py::declared_functions"""
    txt = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//.*", "", txt)
    txt = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", txt, flags=re.S)
    txt = re.sub(r"typedef[^;]*;", "", txt)
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t]*?[ \t*]+)([A-Za-z_][A-Za-z0-9_]*)\s*\(([^;{()]*)\)\s*;", txt):
        params = [p.strip() for p in params.split(",")]
        out[name] = (" ".join(ret.replace("const", " ").split()), [] if params == ["void"] else params)
    return out


def test_every_drop_in_name_of_the_table_is_exported():
    if not os.path.exists(hostprog.DROPIN):
        pytest.skip("libtmlqcd_dropin.so is not built")
    exp = exported(hostprog.DROPIN)
    missing = [n for n in DROPIN_NAMES if n not in exp]
    assert not missing, missing


def test_table_agrees_with_the_header():
    decl = declarations()
    assert len(decl) > 100 and decl["cg_her"][0] == "int" and len(decl["cg_her"][1]) == 7
    assert sorted(n for n in DROPIN_NAMES if n not in decl) == sorted(NOT_IN_HEADER)
    for name in DROPIN_NAMES:
        if name in NOT_IN_HEADER:
            continue
        restype, argtypes = hostprog.PROTOTYPES[name]
        ret, params = decl[name]
        # a _Complex double by value travels as two doubles
        want = sum(2 if "_Complex" in p and "*" not in p else 1 for p in params)
        assert len(argtypes) == want, (name, len(argtypes), params)
        is_pointer = restype is not None and issubclass(restype, (C._Pointer, C.c_void_p, C.c_char_p))
        assert (restype is C.c_double or is_pointer) == (ret == "double" or ret.endswith("*")), (name, restype, ret)
        assert (restype is None) == (ret == "void"), (name, restype, ret)


def test_solver_params_has_the_layout_of_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tmlqcd_dropin.h"\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(tmlqcd_solver_params), offsetof(tmlqcd_solver_params, M_psi),\n'
                   '         offsetof(tmlqcd_solver_params, shifts), offsetof(tmlqcd_solver_params, sdim));\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=gnu99", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    sp = hostprog.SolverParams
    assert got == [C.sizeof(sp), sp.M_psi.offset, sp.shifts.offset, sp.sdim.offset]


def test_build_stub_from_two_processes_at_once(tmp_path):
    """both build a copy of tests/host_stub in a directory of their own and move it into place; each loads what is there"""
    stub_dir = tmp_path / "host_stub"
    stub_dir.mkdir()
    (stub_dir / "globals.c").write_text(open(os.path.join(hostprog.STUB_DIR, "globals.c")).read())
    code = ("import ctypes, sys; sys.path.insert(0, %r); from tests import hostprog; hostprog.STUB_DIR = %r; "
            "so = hostprog.build_stub(); assert ctypes.CDLL(so).stub_calloc; print(so)" % (ROOT, str(stub_dir)))
    procs = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for _ in range(2)]
    for p in procs:
        out, err = p.communicate(timeout=120)
        assert p.returncode == 0 and out.strip() == str(stub_dir / "libtmhost.so"), err[-2000:]
    assert sorted(os.listdir(stub_dir)) == ["globals.c", "libtmhost.so"]
    assert C.CDLL(str(stub_dir / "libtmhost.so")).stub_calloc


def test_build_stub_compiles_under_its_own_name_and_moves_it_into_place(tmp_path, monkeypatch):
    stub_dir = tmp_path / "host_stub"
    stub_dir.mkdir()
    (stub_dir / "globals.c").write_text(open(os.path.join(hostprog.STUB_DIR, "globals.c")).read())
    monkeypatch.setattr(hostprog, "STUB_DIR", str(stub_dir))
    so, moves, real = str(stub_dir / "libtmhost.so"), [], os.replace

    def replace(a, b):
        moves.append((a, b, os.path.exists(b)))
        real(a, b)
    monkeypatch.setattr(os, "replace", replace)
    assert hostprog.build_stub() == so
    assert moves == [(so + ".%d" % os.getpid(), so, False)]       # nothing under the final name before the finished file is moved there
    assert hostprog.build_stub() == so and len(moves) == 1        # up to date: not built again
    (stub_dir / "globals.c").write_text("#error broken\n")
    os.utime(stub_dir / "globals.c", (os.path.getmtime(so) + 10,) * 2)
    with pytest.raises(subprocess.CalledProcessError):
        hostprog.build_stub()
    assert sorted(os.listdir(stub_dir)) == ["globals.c", "libtmhost.so"]      # a failed build leaves nothing behind


def test_load_with_extra_globals_leaves_no_directory_behind(tmp_path):
    if not os.path.exists(hostprog.DROPIN):
        pytest.skip("libtmlqcd_dropin.so is not built")
    tmpdir = tmp_path / "tmp"
    tmpdir.mkdir()
    code = ("import sys; sys.path.insert(0, %r); from tests import hostprog; "
            "stub, nd, d = hostprog.load(extra_c=hostprog.ND_GLOBALS); nd.nd_set(0.1, 0.2, 0.3); "
            "import ctypes; assert ctypes.c_double.in_dll(nd, 'g_epsbar').value == 0.2; print('loaded')" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TMPDIR=str(tmpdir)), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "loaded" in r.stdout, r.stderr[-2000:]
    assert os.listdir(tmpdir) == []
