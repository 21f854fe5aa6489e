"""The codec of the 112-byte packed link read (tmlqcd_amd/csrc/gauge_pack_codec.h) as host code, no GPU.

tests/c_host/gauge_pack_codec_check.cpp includes the header the build kernel and the stencil include, and is compiled here into a
plain program with the undefined-behaviour and address sanitizers (nothing is preloaded: it has its own main).  Its selftest prints
one line of counts per property; the counts are asserted here.  The Python model of tests/gauge_pack_host.py, which the GPU test
of the format relies on for its expected counts, is held against the same program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gauge_pack_host as gph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "gauge_pack_codec_check.cpp")
INC = os.path.join(ROOT, "tmlqcd_amd", "csrc")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gpack") / "gauge_pack_codec_check")
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
        out.setdefault(name, []).append(dict(x.split("=") for x in kv))
    return out


def test_round_trip_of_a_million_random_rows(selftest):
    (r,) = selftest["roundtrip"]
    assert int(r["tails"]) == 1000000 and int(r["pairs"]) == 6000000
    assert int(r["notfit"]) == 0 and int(r["mismatch"]) == 0


def test_limits_of_the_offset(selftest):
    rows = {int(r["d"]): r for r in selftest["limit"]}
    assert sorted(rows) == [-2 ** 20 - 1, -2 ** 20, 2 ** 20 - 1, 2 ** 20]
    for d, r in rows.items():
        cases = int(r["cases"])
        assert cases == 12
        if -2 ** 20 <= d <= 2 ** 20 - 1:
            assert int(r["fits"]) == cases and int(r["same"]) == cases, r
        else:
            assert int(r["fits"]) == 0 and int(r["same"]) == 0, r      # reported as not fitting, and the tail does not pretend otherwise


def test_pairs_across_a_binade_boundary(selftest):
    (r,) = selftest["binade"]
    assert int(r["cases"]) == 240 and int(r["fits"]) == 240 and int(r["same"]) == 240


def test_zero_against_a_tiny_value_of_either_sign(selftest):
    seen = 0
    for r in selftest["zero"]:
        if "near_fits" not in r:
            assert r["w"] == "+0" and r["c"] == "-0" and r["fits"] == "0"
            continue
        same_sign = r["w"][0] == r["c"][0]
        assert int(r["near_fits"]) == (1 if same_sign else 0), r
        assert int(r["near_same"]) == (1 if same_sign else 0), r
        assert int(r["far_fits"]) == 0, r
        seen += 1
    assert seen == 4


def test_extreme_patterns_in_every_field(selftest):
    (r,) = selftest["extreme"]
    assert int(r["cases"]) == 48 and int(r["fits"]) == 48 and int(r["same"]) == 48 and int(r["fields_ok"]) == 6 * 48
    # the layout itself: six fields of ones below the two rotation bits, and the two fields that straddle words 0|1 and 1|2 alone
    assert selftest["allones"][0]["tail"] == "f" * 32
    want = ((2 ** 21 - 1) << 21) | ((2 ** 21 - 1) << 63)
    assert int(selftest["straddle"][0]["tail"], 16) == want


def _hex(x):
    return "%016x" % gph.bits(float(x))


def test_python_model_agrees_with_the_header(prog):
    """offset(): random pairs around the limits and across signs; rebuild_row(): random rows, some with tiny elements."""
    rng = np.random.default_rng(3)
    pairs = []
    for n in range(4000):
        w = float(rng.standard_normal() * 10.0 ** rng.integers(-12, 1))
        k = int(rng.choice([0, 1, -1, 2 ** 20 - 1, -2 ** 20, 2 ** 20, -2 ** 20 - 1, int(rng.integers(-2 ** 22, 2 ** 22))]))
        c = gph.add_ulps(w, k)
        if n % 50 == 0:
            c = -c
        pairs.append((c, w))
    got = _run(prog, "fits", "".join("%s %s\n" % (_hex(c), _hex(w)) for c, w in pairs))
    want = ["0" if gph.offset(c, w) is None else "1" for c, w in pairs]
    assert got == want
    assert 1000 < want.count("1") < 3500

    rows = rng.standard_normal((300, 2, 3, 2))
    rows[::7, 0, 1] *= 1e-9
    rows[::11, 1, 2, 0] *= 1e-14
    text = "".join(" ".join(_hex(x) for x in r.reshape(-1)) + "\n" for r in rows)
    got = _run(prog, "rebuild", text)
    assert len(got) == len(rows)
    for r, line in zip(rows, got):
        w = gph.rebuild_row([tuple(x) for x in r[0]], [tuple(x) for x in r[1]])
        assert [_hex(x) for x in w] == line.split()
