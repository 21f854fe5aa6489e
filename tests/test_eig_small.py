"""CPU: the small symmetric eigensolver of the eigenvalue measurement (tmlqcd_amd/csrc/eig_small.h, cyclic Jacobi) as host code.

tests/c_host/eig_small_main.cpp includes the header eig.hip includes and is compiled here into a plain program with the
undefined-behaviour and address sanitizers (nothing is preloaded: it has its own main).  Bounds, from the backward stability
of Jacobi rotations: eigenvalues to 64 eps |A| against numpy.linalg.eigvalsh, |Y^T Y - 1| and |A Y - Y Lambda| to the same
scale (max norm, |A| = the spectral norm)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "eig_small_main.cpp")
INC = os.path.join(ROOT, "tmlqcd_amd", "csrc")
EPS = np.finfo(np.float64).eps


def _sym(rng, n):
    a = rng.standard_normal((n, n))
    return 0.5 * (a + a.T)


def _matrices():
    rng = np.random.default_rng(20)
    out = {"random%d" % n: _sym(rng, n) for n in (1, 2, 3, 17, 64)}
    # what a restart leaves: diag(theta) with an arrow in row / column k, then the tridiagonal of the new steps
    n, k = 24, 12
    a = np.diag(np.sort(rng.uniform(0.01, 1.0, n)))
    a[:k, k] = a[k, :k] = 1e-3 * rng.standard_normal(k)
    for j in range(k, n - 1):
        a[j, j + 1] = a[j + 1, j] = rng.uniform(0.05, 0.3)
    out["arrowhead24"] = a
    q, _ = np.linalg.qr(rng.standard_normal((9, 9)))
    out["repeated"] = q @ np.diag([0.5, 0.5, 0.5, 1.0, 2.0, 2.0, 3.0, 3.0, 3.0]) @ q.T
    out["repeated"] = 0.5 * (out["repeated"] + out["repeated"].T)
    out["diagonal"] = np.diag([3.0, -1.0, 2.0, 2.0, 0.0, 7.5])
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("eigsmall") / "eig_small_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-static-libasan", "-static-libubsan",
           "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe, "-lm"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    mats = _matrices()
    text = "".join("%d\n%s\n" % (a.shape[0], " ".join(float(x).hex() for x in a.reshape(-1))) for a in mats.values())
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 3 * len(mats)
    out = {}
    for i, (name, a) in enumerate(mats.items()):
        n = int(lines[3 * i])
        assert n == a.shape[0]
        w = np.array([float.fromhex(t) for t in lines[3 * i + 1].split()])
        y = np.array([float.fromhex(t) for t in lines[3 * i + 2].split()]).reshape(n, n)
        out[name] = (a, w, y)
    return out


@pytest.mark.parametrize("name", list(_matrices()))
def test_eigenpairs(results, name):
    a, w, y = results[name]
    n = a.shape[0]
    norm = max(np.linalg.norm(a, 2), np.finfo(np.float64).tiny)
    ref = np.linalg.eigvalsh(a)
    errs = (np.abs(w - ref).max(), np.abs(y.T @ y - np.eye(n)).max(), np.abs(a @ y - y * w).max())
    print(name, "n", n, "errors / (eps |A|):", [e / (EPS * norm) for e in errs[::2]], "orthonormality / eps:", errs[1] / EPS)
    assert np.all(np.diff(w) >= 0)
    assert errs[0] <= 64 * EPS * norm
    assert errs[1] <= 64 * EPS
    assert errs[2] <= 64 * EPS * norm


def test_library_entry_point_meets_the_same_bounds(results):
    """tmhip_eig_small of the built library (host code: no device needed) is the header behind a range check"""
    import tmlqcd_amd.hip as h
    for name in ("random17", "arrowhead24", "repeated"):
        a, _, _ = results[name]
        n = a.shape[0]
        norm = np.linalg.norm(a, 2)
        w, y = h.eig_small(a)
        assert np.abs(w - np.linalg.eigvalsh(a)).max() <= 64 * EPS * norm, name
        assert np.abs(y.T @ y - np.eye(n)).max() <= 64 * EPS and np.abs(a @ y - y * w).max() <= 64 * EPS * norm, name
    with pytest.raises(h.TmHipError):
        h.eig_small(np.eye(65))
