"""CPU: the NumPy restatement of the propagator / source file code (tests/spinor_io_restate.py) against the committed fixtures, whose
site order, checksums and point sources come from the reference's object code (tools/make_golden_spinor_io.py), and against itself:
round trips, the T-split checksum rule, read_spinor's position and error rules."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import spinor_io_restate as sr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = list(sr.SHAPES)


def gold(tag):
    return json.load(open(os.path.join(GOLD, "ref_spinor_io_%s.json" % tag)))


def as32(a):
    with np.errstate(over="ignore"):
        return a.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_fixture(tag):
    g, dims = gold(tag), sr.SHAPES[tag]
    assert tuple(g["dims"]) == dims and g["seed"] == sr.FIELD_SEED
    even, odd = sr.fields(dims)
    for prec in (64, 32):
        rec, sums = sr.pack(even, odd, dims, prec)
        want = g["prec%d" % prec]
        assert rec.size == sr.volume(dims) * (192 if prec == 64 else 96)
        assert ("%08x" % sums[0], "%08x" % sums[1]) == (want["suma"], want["sumb"])
        assert hashlib.sha256(rec.tobytes()).hexdigest() == want["sha256"]
    src = g["point_sources"]
    assert src["odd_site_index"] == sr.odd_site(dims)
    for k in range(12):
        p = sr.source_point(dims, k // 3, k % 3, 0)
        assert [p[0], p[1], p[2], 0, 1.0] == src["site0"][k]
        p = sr.source_point(dims, k // 3, k % 3, sr.odd_site(dims))
        assert [p[0], p[1], p[2], 0, 1.0] == src["odd_site"][k] and p[0] == 1


@pytest.mark.parametrize("tag", TAGS)
def test_checksum_is_the_references_own_code(tag):
    from oracle import ildgbind as ib
    if not ib.ref_available():
        pytest.skip("oracle/_ref/libtmref_dml.so (the reference's io/dml.c compiled in place) is not built here")
    dims = sr.SHAPES[tag]
    even, odd = sr.fields(dims)
    for prec in (64, 32):
        rec, sums = sr.pack(even, odd, dims, prec, rank0=12345)
        assert ib.ref_checksum(rec, 192 if prec == 64 else 96, rank0=12345) == sums


@pytest.mark.parametrize("tag", TAGS)
def test_unpack_inverts_pack(tag):
    dims = sr.SHAPES[tag]
    even, odd = sr.fields(dims)
    for prec in (64, 32):
        rec, sums = sr.pack(even, odd, dims, prec)
        e, o, s2 = sr.unpack(rec, dims, prec)
        assert s2 == sums
        assert np.array_equal(e, even if prec == 64 else as32(even)) and np.array_equal(o, odd if prec == 64 else as32(odd))
        assert np.array_equal(np.signbit(e), np.signbit(even))          # -0.0 stays -0.0


@pytest.mark.parametrize("world", [2, 4])
def test_t_slabs_concatenate_and_their_checksums_xor(world):
    dims = (8, 4, 4, 4)
    local = (8 // world, 4, 4, 4)
    even, odd = sr.fields(dims)
    for prec in (64, 32):
        rec, sums = sr.pack(even, odd, dims, prec)
        parts, xa, xb = [], 0, 0
        for r in range(world):
            part, s = sr.pack(sr.slab(even, world, r), sr.slab(odd, world, r), local, prec, rank0=r * sr.volume(local), toff=r * local[0])
            parts.append(part); xa ^= s[0]; xb ^= s[1]
        assert np.array_equal(np.concatenate(parts), rec) and (xa, xb) == sums


def _file(dims, prec=64):
    """propagator-type + inversion-info, then three (source, sink) style data records: a Source_Sink_Pairs file with four records."""
    fl = [sr.fields(dims, seed=sr.FIELD_SEED + k) for k in range(4)]
    head = sr.lime_record(1, 1, "propagator-type", "DiracFermion_Source_Sink_Pairs") + sr.lime_record(1, 1, "inversion-info", "solver = CG\n")
    return head, fl, head + sr.spinor_records(fl, dims, prec)


def test_reader_position_rule_and_return_values():
    dims = sr.SHAPES["2x2x2x6"]
    head, fl, blob = _file(dims)
    rc, e, o, info = sr.read_spinor(blob, dims, 1)
    assert rc == 0 and info["position"] == 3 and info["prec"] == 64 and info["calculated"] == info["stored"]
    assert np.array_equal(e, fl[3][0]) and np.array_equal(o, fl[3][1])                  # position 1 of Source_Sink_Pairs = data record 3
    rc, e, o, info = sr.read_spinor(blob, dims, 0)
    assert rc == 0 and info["position"] == 1 and np.array_equal(e, fl[1][0])
    plain = sr.lime_record(1, 1, "propagator-type", "DiracFermion_Sink") + sr.spinor_records(fl, dims, 32)
    rc, e, o, info = sr.read_spinor(plain, dims, 2)
    assert rc == 0 and info["position"] == 2 and info["prec"] == 32 and np.array_equal(e, as32(fl[2][0]))
    # -5: the file ends behind its header records; -6: a record of another lattice; -1: no scidac-checksum behind the data
    assert sr.read_spinor(head, dims, 0)[0] == -5
    assert sr.read_spinor(blob, dims, 2)[0] == -5                                         # data record 5 of 4
    assert sr.read_spinor(blob, (2, 2, 2, 8), 0)[0] == -6
    rec, _ = sr.pack(fl[0][0], fl[0][1], dims, 64)
    nosum = sr.lime_record(1, 0, "scidac-binary-data", rec)
    assert sr.read_spinor(nosum, dims, 0)[0] == -1
    assert sr.read_spinor(nosum + nosum, dims, 0)[0] == -1                                # more binary data ends the search
    assert sr.read_spinor(nosum, dims, 0, io_checks=False)[0] == 0
    assert sr.read_spinor(sr.lime_record(1, 1, "propagator-type", "DiracFermion_ScalarSource_TwelveSink") + blob, dims, 0)[0] == -2
    assert sr.read_spinor(sr.lime_record(1, 1, "source-type", "DiracFermion_ScalarSource") + blob, dims, 0)[0] == -3


def test_point_source_on_a_t_split():
    local = (4, 4, 4, 4)
    g = sr.odd_site((8, 4, 4, 4))
    assert sr.source_point(local, 2, 1, g, world=2, r=0) is None
    par, idx, comp = sr.source_point(local, 2, 1, g, world=2, r=1)
    whole = sr.source_point((8, 4, 4, 4), 2, 1, g)
    assert (par, idx + sr.volume(local) // 2, comp) == whole
