"""GPU: propagator and source I/O through the HIP path (spinor_io.hip) -- pack / unpack kernels, read_spinor / write_spinor with the
LIME framing, point sources -- bit for bit against the NumPy restatement (tests/spinor_io_restate.py) and the committed fixtures,
whose site order, checksums and point sources come from the reference's object code (tools/make_golden_spinor_io.py).

Shapes: 4^4 plain; 8x6x4x12 LX != LZ and LX no multiple of the 4-wide x tile (4 + 2); 2x2x2x6 VOLUME/2 = 24, a partial wave, a
tile narrower than the x group and a plane stride padded beyond the field; 4x12x2x6 LX > LZ with three x tiles and rows of three
entries per parity; 2x2x2x34 LZ beyond the 32 z a tile holds: the z loop, second range of two sites."""
import functools
import json
import os

import numpy as np
import pytest

from tests import spinor_io_restate as sr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = list(sr.SHAPES)
SENTINEL = -7.25


def as32(a):
    with np.errstate(over="ignore"):
        return a.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(tag):
    """(fixture, even, odd, {prec: (record, sums)}) of a shape: computed once, shared, never written to."""
    dims = sr.SHAPES[tag]
    even, odd = sr.fields(dims)
    recs = {prec: sr.pack(even, odd, dims, prec) for prec in (64, 32)}
    for a in (even, odd, recs[64][0], recs[32][0]):
        a.setflags(write=False)
    return json.load(open(os.path.join(GOLD, "ref_spinor_io_%s.json" % tag))), even, odd, recs


def fixture_sums(g, prec):
    return int(g["prec%d" % prec]["suma"], 16), int(g["prec%d" % prec]["sumb"], 16)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("tag", TAGS)
def test_pack(tag, prec):
    from tmlqcd_amd import Lattice
    g, even, odd, recs = case(tag)
    lat = Lattice(*sr.SHAPES[tag])
    out, sums = lat.spinor_pack(lat.field(even), lat.field(odd), prec)
    assert np.array_equal(out, recs[prec][0])
    assert sums == recs[prec][1] == fixture_sums(g, prec)
    lat.close()


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("tag", TAGS)
def test_unpack(tag, prec):
    from tmlqcd_amd import Lattice
    g, even, odd, recs = case(tag)
    lat = Lattice(*sr.SHAPES[tag])
    fe, fo = lat.field(), lat.field()
    sums = lat.spinor_unpack(fe, fo, recs[prec][0], prec)
    assert sums == fixture_sums(g, prec)
    assert same_bits(fe.download(), even if prec == 64 else as32(even))          # bit for bit: signed zeros, denormals, infinities
    assert same_bits(fo.download(), odd if prec == 64 else as32(odd))
    lat.close()


@pytest.mark.parametrize("tag", TAGS)
def test_pack_then_unpack_is_the_identity_and_leaves_the_padding_alone(tag):
    from tmlqcd_amd import Lattice
    g, even, odd, recs = case(tag)
    lat = Lattice(*sr.SHAPES[tag])
    rec, sums = lat.spinor_pack(lat.field(even), lat.field(odd), 64)
    fe, fo = lat.field(), lat.field()
    ns = fe.raw().shape[1]
    assert ns % 64 == 0 and ns >= lat.Vh and (tag != "2x2x2x6" or ns == 64 > lat.Vh)
    fill = np.full((12, ns, 2), SENTINEL)
    fe.raw(fill); fo.raw(fill)
    assert lat.spinor_unpack(fe, fo, rec, 64) == sums
    for f, want in ((fe, even), (fo, odd)):
        planes = f.raw()
        assert same_bits(planes[:, :lat.Vh].transpose(1, 0, 2).reshape(lat.Vh, 4, 3, 2), want)
        assert np.all(planes[:, lat.Vh:] == SENTINEL)                               # entries [Vh, ns) as they were
    lat.close()


@pytest.mark.parametrize("tag", ["8x6x4x12", "2x2x2x6"])
def test_full_field_as_its_two_views(tag):
    """The `_l` forms of the reference: a lexicographic field is the same record."""
    from tmlqcd_amd import Lattice
    g, even, odd, recs = case(tag)
    dims = sr.SHAPES[tag]
    T, LX, LY, LZ = dims
    lat = Lattice(*dims)
    lex = np.zeros((lat.V, 4, 3, 2))
    ix = np.arange(lat.V)
    par = (ix % LZ + ix // LZ % LY + ix // (LZ * LY) % LX + ix // (LZ * LY * LX)) & 1
    lex[par == 0] = even[ix[par == 0] >> 1]
    lex[par == 1] = odd[ix[par == 1] >> 1]
    full = lat.full_field(lex)
    for prec in (64, 32):
        out, sums = lat.spinor_pack(full.even(), full.odd(), prec)
        assert np.array_equal(out, recs[prec][0]) and sums == recs[prec][1]
    back = lat.full_field()
    lat.spinor_unpack(back.even(), back.odd(), recs[64][0], 64)
    assert same_bits(back.download(), lex)
    lat.close()


@pytest.mark.parametrize("world", [2, 4])
def test_t_split_ranks_handle_their_part_of_the_record(world):
    from tmlqcd_amd import Lattice
    dims = (8, 4, 4, 4)
    local = (8 // world, 4, 4, 4)
    even, odd = sr.fields(dims)
    for prec in (64, 32):
        rec, sums = sr.pack(even, odd, dims, prec)
        share = rec.size // world
        xa = xb = 0
        for r in range(world):
            lat = Lattice(*local, nproc_t=world, proc_t=r)
            e, o = np.ascontiguousarray(sr.slab(even, world, r)), np.ascontiguousarray(sr.slab(odd, world, r))
            out, s = lat.spinor_pack(lat.field(e), lat.field(o), prec)
            assert np.array_equal(out, rec[r * share:(r + 1) * share])
            xa ^= s[0]; xb ^= s[1]
            fe, fo = lat.field(), lat.field()
            assert lat.spinor_unpack(fe, fo, rec[r * share:(r + 1) * share], prec) == s
            assert same_bits(fe.download(), e if prec == 64 else as32(e)) and same_bits(fo.download(), o if prec == 64 else as32(o))
            lat.close()
        assert (xa, xb) == sums


def test_files(tmp_path, capfd):
    """write_spinor with one flavour, with two, appended; read_spinor at every position; precision recognised; the error cases of the
    CPU test with the same codes and untouched fields; a flipped byte is read with status 0 and shows in the checksums."""
    from tmlqcd_amd import Lattice, hip
    tag = "2x2x2x6"
    dims = sr.SHAPES[tag]
    fl = [sr.fields(dims, seed=sr.FIELD_SEED + k) for k in range(3)]
    lat = Lattice(*dims)
    dev = [(lat.field(e), lat.field(o)) for e, o in fl]
    for prec in (64, 32):
        p = tmp_path / ("w%d.lime" % prec)
        hip.write_lime_message(p, "propagator-type", "DiracFermion_Sink", 1, 1, append=False)
        s1 = lat.write_spinor(p, dev[0][0], dev[0][1], prec, append=True)
        s2 = lat.write_spinor(p, [dev[1][0], dev[2][0]], [dev[1][1], dev[2][1]], prec, append=True)
        want = sr.lime_record(1, 1, "propagator-type", "DiracFermion_Sink") + sr.spinor_records(fl, dims, prec)
        assert p.read_bytes() == want                                                # byte for byte the restatement's file
        assert s1 + s2 == [sr.pack(e, o, dims, prec)[1] for e, o in fl]
        fe, fo = lat.field(), lat.field()
        for pos in range(3):
            rc, info = lat.read_spinor(fe, fo, p, pos)
            assert rc == 0 and info.prec == prec and info.position == pos and info.prop_type == 0 and info.checksum_read == 1
            assert (info.suma, info.sumb) == (info.suma_stored, info.sumb_stored) == (s1 + s2)[pos]
            assert same_bits(fe.download(), fl[pos][0] if prec == 64 else as32(fl[pos][0]))
            assert same_bits(fo.download(), fl[pos][1] if prec == 64 else as32(fl[pos][1]))
    # a file that starts with the data (append = False creates it)
    q = tmp_path / "plain.lime"
    lat.write_spinor(q, dev[0][0], dev[0][1], 64)
    assert q.read_bytes() == sr.spinor_records(fl[:1], dims, 64)
    # Source_Sink_Pairs: position 1 is data record 3
    fl4 = fl + [sr.fields(dims, seed=sr.FIELD_SEED + 3)]
    head = sr.lime_record(1, 1, "propagator-type", "DiracFermion_Source_Sink_Pairs") + sr.lime_record(1, 1, "inversion-info", "solver = CG\n")
    pairs = tmp_path / "pairs.lime"
    pairs.write_bytes(head + sr.spinor_records(fl4, dims, 64))
    fe, fo = lat.field(), lat.field()
    rc, info = lat.read_spinor(fe, fo, pairs, 1)
    assert rc == 0 and info.position == 3 and info.prop_type == 1 and same_bits(fe.download(), fl4[3][0]) and same_bits(fo.download(), fl4[3][1])
    # error cases: same codes as the restatement, the reference's messages, fields as they were
    keep_e, keep_o = fe.download(), fo.download()
    capfd.readouterr()
    rec0 = sr.pack(fl[0][0], fl[0][1], dims, 64)[0]
    cases = {"cut": (head, 0, -5, "End of file reached before record was found"),
             "beyond": (head + sr.spinor_records(fl4, dims, 64), 2, -5, "Unable to find requested LIME record scidac-binary-data"),
             "length": (sr.lime_record(1, 0, "scidac-binary-data", rec0[:-192]) + sr.lime_record(0, 1, "scidac-checksum", sr.checksum_xml((1, 2))), 0, -6,
                        "does not match input parameters"),
             "nosum": (sr.lime_record(1, 0, "scidac-binary-data", rec0), 0, -1, "\"scidac-checksum\", in gauge file"),
             "twelve": (sr.lime_record(1, 1, "propagator-type", "DiracFermion_ScalarSource_TwelveSink") + sr.spinor_records(fl[:1], dims, 64), 0, -2, ""),
             "scalar": (sr.lime_record(1, 1, "source-type", "DiracFermion_ScalarSource") + sr.spinor_records(fl[:1], dims, 64), 0, -3, "")}
    for name, (blob, pos, code, text) in cases.items():
        f = tmp_path / (name + ".lime")
        f.write_bytes(blob)
        assert sr.read_spinor(blob, dims, pos)[0] == code, name
        rc, _ = lat.read_spinor(fe, fo, f, pos)
        assert rc == code, name
        assert text in capfd.readouterr().err, name
        assert same_bits(fe.download(), keep_e) and same_bits(fo.download(), keep_o), name
    # ... and with the checks off the file without a checksum record is read
    rc, info = lat.read_spinor(fe, fo, tmp_path / "nosum.lime", 0, io_checks=False)
    assert rc == 0 and info.checksum_read == 0 and same_bits(fe.download(), fl[0][0])
    # one flipped byte in the record: status 0 (the reference only prints the two pairs), calculated != stored
    raw = bytearray((tmp_path / "plain.lime").read_bytes())
    raw[144 + 1000] ^= 0x10
    (tmp_path / "flipped.lime").write_bytes(raw)
    rc, info = lat.read_spinor(fe, fo, tmp_path / "flipped.lime", 0)
    assert rc == 0 and (info.suma, info.sumb) != (info.suma_stored, info.sumb_stored)
    assert (info.suma_stored, info.sumb_stored) == sr.pack(fl[0][0], fl[0][1], dims, 64)[1]
    lat.close()


def test_file_calls_refuse_a_t_split_context(tmp_path, capfd):
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    lat = Lattice(2, 2, 2, 6, nproc_t=2, proc_t=1)
    fe, fo = lat.field(), lat.field()
    with pytest.raises(TmHipError):
        lat.write_spinor(tmp_path / "x.lime", fe, fo)
    with pytest.raises(TmHipError):
        lat.read_spinor(fe, fo, tmp_path / "x.lime")
    assert "unsplit lattices only" in capfd.readouterr().err
    lat.close()


@pytest.mark.parametrize("tag", TAGS)
def test_point_sources(tag):
    from tmlqcd_amd import Lattice
    g = case(tag)[0]["point_sources"]
    lat = Lattice(*sr.SHAPES[tag])
    fe, fo = lat.field(np.ones((lat.Vh, 4, 3, 2))), lat.field(np.ones((lat.Vh, 4, 3, 2)))
    for key, site in (("site0", 0), ("odd_site", g["odd_site_index"])):
        for k in range(12):
            lat.source_point(fe, fo, k // 3, k % 3, site)
            both = np.stack([fe.download(), fo.download()]).reshape(2, lat.Vh, 12, 2)
            nz = np.argwhere(both != 0.0)
            assert len(nz) == 1                                                          # exactly one non-zero
            a, b, c, d = (int(v) for v in nz[0])
            assert [a, b, c, d, float(both[a, b, c, d])] == g[key][k]
    lat.close()


def test_point_source_on_a_t_split_lives_on_the_owning_rank():
    from tmlqcd_amd import Lattice
    local, world = (4, 4, 4, 4), 2
    site = sr.odd_site((8, 4, 4, 4))
    for r in range(world):
        lat = Lattice(*local, nproc_t=world, proc_t=r)
        fe, fo = lat.field(np.ones((lat.Vh, 4, 3, 2))), lat.field(np.ones((lat.Vh, 4, 3, 2)))
        lat.source_point(fe, fo, 3, 2, site)
        both = np.stack([fe.download(), fo.download()]).reshape(2, lat.Vh, 12, 2)
        want = sr.source_point(local, 3, 2, site, world=world, r=r)
        nz = [tuple(int(v) for v in x) for x in np.argwhere(both != 0.0)]
        assert nz == ([] if want is None else [(want[0], want[1], want[2], 0)])
        lat.close()
