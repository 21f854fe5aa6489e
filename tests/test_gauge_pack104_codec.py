"""The compact form of the two kept rows of the packed link read (104 bytes per link; tmlqcd_amd/csrc/gauge_pack_codec.h) as host
code, no GPU.

tests/c_host/gauge_pack104_check.cpp includes the header the build kernel and the stencil include, and is compiled here into a plain
program with the undefined-behaviour and address sanitizers (nothing is preloaded: it has its own main).  Its selftest prints one
line of counts per property; the counts are asserted here.  Every comparison is equality of bits or of counts.  The Python model of
"fits compact" in tests/gauge_pack104_host.py, from which the GPU test of the format takes its expectations, is held against the
same program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gauge_pack104_host as g104
from tests import gauge_pack_host as gph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "gauge_pack104_check.cpp")
INC = os.path.join(ROOT, "tmlqcd_amd", "csrc")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gpack104") / "gauge_pack104_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=undefined,address",
           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe, "-lm"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def _run(exe, mode, text=""):
    r = subprocess.run([exe, mode], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def selftest(prog):
    out = {}
    for line in _run(prog, "selftest"):
        print(line)
        name, *kv = line.split()
        out[name] = {k: v for k, v in (x.split("=") for x in kv)}
    return out


def _counts(r):
    return int(r["cases"]), int(r["fits"]), int(r["same"]), int(r["escaped"])


def test_round_trip_of_a_million_kept_row_pairs_of_random_su3_links(selftest):
    r = selftest["roundtrip"]
    assert int(r["pairs"]) == 1000000
    assert int(r["notfit"]) == 0 and int(r["mismatch"]) == 0


def test_limits_of_the_window_in_every_position(selftest):
    n = 24                                                      # twelve positions, either sign
    assert _counts(selftest["window_low"]) == (n, n, n, 0)      # 2^-30 fits without the escape
    assert _counts(selftest["window_low_escape"]) == (n, n, n, n)   # the double just below it only with it
    assert _counts(selftest["two_small"]) == (n, 0, 0, 0)       # two such reals do not fit
    assert _counts(selftest["one"]) == (n, n, n, 0)
    assert _counts(selftest["below_two"]) == (n, n, n, 0)
    assert _counts(selftest["two"]) == (n, 0, 0, 0)
    assert _counts(selftest["escape_min"]) == (n, n, n, n)      # the smallest escapable binade
    assert _counts(selftest["escape_below"]) == (n, 0, 0, 0)    # ... and the one below it
    assert _counts(selftest["subnormal"]) == (2 * n, 0, 0, 0)
    assert _counts(selftest["nan"]) == (n, 0, 0, 0)
    assert _counts(selftest["inf"]) == (n, 0, 0, 0)


def test_zeros_fit_and_keep_their_sign(selftest):
    r = selftest["zero"]
    assert int(r["cases"]) == 24 and int(r["fits"]) == 24 and int(r["same"]) == 24 and int(r["signs_kept"]) == 24


def test_mantissas_of_all_ones_and_all_zeros_in_every_position(selftest):
    r = selftest["mantissa"]
    cases = 4 * 12 * 3
    assert _counts(r) == (cases, cases, cases, 0)
    assert int(r["fields_ok"]) == 12 * cases
    # the layout itself: twelve fields of ones (sign, code 31, twenty mantissa bits) below the escape byte "none": index 15, ext 0
    assert int(selftest["allones"]["h"], 16) == (0x0F << 312) | ((1 << 312) - 1)


def test_escape_in_every_position_with_ext_1_and_15(selftest):
    r = selftest["escape"]
    cases = 12 * 2 * 4
    assert _counts(r) == (cases, cases, cases, cases)
    assert int(r["index_and_ext_ok"]) == cases


def _hex(x):
    return "%016x" % gph.bits(float(x))


def test_python_model_agrees_with_the_header(prog):
    """fits_compact() against the encoder's verdict: rows of random magnitudes around both ends of the window and of the escape's
    reach, with zeros of either sign, a second small real, values at and above 2, subnormals, infinities and NaNs mixed in."""
    rng = np.random.default_rng(5)
    rows = rng.uniform(0.3, 1.0, (6000, 12)) * np.where(rng.random((6000, 12)) < 0.5, -1.0, 1.0)
    rows *= np.where(rng.random((6000, 12)) < 0.1, 2.0 ** rng.integers(-40, 2, (6000, 12)), 1.0)   # a tenth of the reals leave O(1)
    special = np.array([0.0, -0.0, 2.0, -2.0, 2.0 ** -30, np.nextafter(2.0 ** -30, 0.0), np.nextafter(2.0, 0.0), 2.0 ** -495,
                        np.nextafter(2.0 ** -495, 0.0), 1e-12, -3e-200, 5e-324, -1e-310, np.inf, -np.inf, np.nan, 1e-100, 1.0])
    for n in range(0, 6000, 2):
        rows[n, rng.integers(12)] = special[rng.integers(len(special))]
    for n in range(0, 6000, 10):
        rows[n, rng.integers(12)] = special[rng.integers(len(special))]
    got = [line.split() for line in _run(prog, "fits", "".join(" ".join(_hex(x) for x in r) + "\n" for r in rows))]
    want = g104.fits_compact(rows)
    assert len(got) == len(rows)
    assert [g[0] for g in got] == ["1" if w else "0" for w in want]
    assert all(g[1] == "1" for g, w in zip(got, want) if w)          # what fits comes back bit for bit
    assert 1500 < int(want.sum()) < 5000
