"""TEST INFRASTRUCTURE ONLY.  NumPy restatement of the reference's propagator / source file code:

  pack / unpack      io/spinor_write_binary.c:145-224, io/spinor_read_binary.c: the "scidac-binary-data" record of two e/o fields
  checksum           io/dml.c:49-60 on zlib.crc32 (= io/DML_crc32.c)
  spinor_file        io/spinor_write.c:23-47 inside the LIME framing of c-lime 1.3.x (144-byte headers, data padded to 8 bytes)
  read_spinor        io/spinor_read.c:27-150 with io/utils_parse_propagator_type.c:22-91: position rule and return values
  source_point       start.c:707-741 (site 0) and start.c:743-830 (any global site, z fastest)

Fields are float64 [VOLUME/2][4][3][2] per parity (su3.h:60-63), entry = g_lexic2eosub = lexicographic index / 2 for even extents.
Inputs are seeded here, so the fixtures (tests/golden/ref_spinor_io_<shape>.json, tools/make_golden_spinor_io.py) hold results only.
"""
import struct
import zlib

import numpy as np

# the last shape is longer in z than the 32 sites a block of the device kernels holds at a time
SHAPES = {"4x4x4x4": (4, 4, 4, 4), "8x6x4x12": (8, 6, 4, 12), "2x2x2x6": (2, 2, 2, 6), "4x12x2x6": (4, 12, 2, 6), "2x2x2x34": (2, 2, 2, 34)}
FIELD_SEED = 20260


def volume(dims):
    T, LX, LY, LZ = dims
    return T * LX * LY * LZ


def fields(dims, seed=FIELD_SEED):
    """The seeded (even, odd) pair of a lattice.  A few entries are edge cases of the 32-bit conversion: signed zeros, a value that
    becomes a float denormal, one that underflows to zero, one that overflows to infinity, one that rounds to even."""
    Vh = volume(dims) // 2
    f = np.random.default_rng(seed).standard_normal((2, Vh, 4, 3, 2))
    special = [0.0, -0.0, 1.0e-40, -1.0e-50, 1.0e39, 1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, -3.0e38]
    flat = f.reshape(2, -1)
    for k, v in enumerate(special):
        flat[k & 1, (7 * k + 3) % flat.shape[1]] = v
        flat[1 - (k & 1), flat.shape[1] - 1 - 5 * k] = v
    return f[0], f[1]


def slab(field, world, r):
    """Rank r's part of a global one-parity field on a T split into `world` slabs: lexicographic order has t slowest."""
    n = field.shape[0] // world
    return field[r * n:(r + 1) * n]


def site_tables(dims, toff=0):
    """For the sites of a record in file order ((t LZ + z) LY + y) LX + x: (parity, entry) of the field that holds them."""
    T, LX, LY, LZ = dims
    t, z, y, x = np.meshgrid(np.arange(T), np.arange(LZ), np.arange(LY), np.arange(LX), indexing="ij")
    lexic = ((t * LX + x) * LY + y) * LZ + z
    par = (t + toff + x + y + z) & 1
    return par.ravel(), (lexic >> 1).ravel()


def checksum(record, site_bytes, rank0=0):
    """DML_checksum_accum over the sites of a record: crc32 of the site's bytes rotated by rank % 29 and rank % 31 (rank: uint32_t)."""
    b = bytes(record)
    a = bb = 0
    for f in range(len(b) // site_bytes):
        crc = zlib.crc32(b[f * site_bytes:(f + 1) * site_bytes]) & 0xffffffff
        rank = (rank0 + f) & 0xffffffff
        r29, r31 = rank % 29, rank % 31
        a ^= ((crc << r29) | (crc >> (32 - r29))) & 0xffffffff
        bb ^= ((crc << r31) | (crc >> (32 - r31))) & 0xffffffff
    return a, bb


def pack(even, odd, dims, prec, rank0=0, toff=0):
    """(record as a uint8 array, (suma, sumb)) of this rank's sites."""
    par, idx = site_tables(dims, toff)
    sites = np.where((par == 0)[:, None], even.reshape(-1, 24)[idx], odd.reshape(-1, 24)[idx])
    with np.errstate(over="ignore"):
        rec = np.frombuffer(sites.astype(">f8" if prec == 64 else ">f4").tobytes(), dtype=np.uint8)
    return rec, checksum(rec, 192 if prec == 64 else 96, rank0)


def unpack(record, dims, prec, rank0=0, toff=0):
    """(even, odd, (suma, sumb)) from this rank's part of a record."""
    par, idx = site_tables(dims, toff)
    rec = np.ascontiguousarray(np.frombuffer(bytes(record), dtype=np.uint8))
    sites = rec.view(">f8" if prec == 64 else ">f4").astype(np.float64).reshape(-1, 24)
    Vh = volume(dims) // 2
    out = np.zeros((2, Vh, 24))
    out[par, idx] = sites
    return out[0].reshape(Vh, 4, 3, 2), out[1].reshape(Vh, 4, 3, 2), checksum(rec, 192 if prec == 64 else 96, rank0)


# ---- LIME framing
def lime_record(mb, me, rtype, data):
    data = data.encode() if isinstance(data, str) else bytes(data)
    head = struct.pack(">IHBBQ", 0x456789ab, 1, (0x80 if mb else 0) | (0x40 if me else 0), 0, len(data)) + rtype.encode().ljust(128, b"\0")
    return head + data + b"\0" * (-len(data) % 8)


def checksum_xml(sums):
    return ("<?xml version=\"1.0\" encoding=\"UTF-8\"?>\n<scidacChecksum>\n  <version>1.0</version>\n  <suma>%08x</suma>\n  <sumb>%08x</sumb>\n</scidacChecksum>"
            % (sums[0], sums[1]))


def spinor_records(pairs, dims, prec):
    """What write_spinor puts on a writer for the flavours `pairs` = [(even, odd), ...]."""
    out = b""
    for even, odd in pairs:
        rec, sums = pack(even, odd, dims, prec)
        out += lime_record(1, 0, "scidac-binary-data", rec) + lime_record(0, 1, "scidac-checksum", checksum_xml(sums))
    return out


def records(blob):
    """[(type, mb, me, data)] of a LIME file's bytes; a malformed or cut header ends the walk."""
    out, pos = [], 0
    while pos + 144 <= len(blob):
        magic, version, flags, _, n = struct.unpack(">IHBBQ", blob[pos:pos + 16])
        if magic != 0x456789ab or version != 1:
            break
        rtype = blob[pos + 16:pos + 144].split(b"\0")[0].decode()
        out.append((rtype, (flags >> 7) & 1, (flags >> 6) & 1, blob[pos + 144:pos + 144 + n]))
        pos += 144 + (n + 7) // 8 * 8
    return out


PROP_TYPES = {"DiracFermion_Sink": 0, "DiracFermion_Source_Sink_Pairs": 1, "DiracFermion_ScalarSource_TwelveSink": 2,
              "DiracFermion_ScalarSource_FourSink": 3, "DiracFermion_Deflation_Field": 4}
SOURCE_TYPES = {"DiracFermion_Source": 10, "DiracFermion_ScalarSource": 11, "DiracFermion_FourScalarSource": 12, "DiracFermion_TwelveScalarSource": 13}


def parse_propagator_type(recs):
    for rtype, _, _, data in recs:
        if rtype == "propagator-type":
            return PROP_TYPES.get(data.decode(), -1)
        if rtype == "source-type":
            return SOURCE_TYPES.get(data.decode(), -1)
    return -1


def xml_value(msg, tag):
    tok = msg.replace("<", " ").replace(">", " ").split()
    for k in range(len(tok) - 1):
        if tok[k].startswith(tag):
            return tok[k + 1]
    return None


def read_spinor(blob, dims, position, io_checks=True):
    """(status, even, odd, info): status and the data-record rule of io/spinor_read.c; info = dict(prec, position, calculated, stored)."""
    recs = records(blob)
    ptype = parse_propagator_type(recs)
    if ptype == 1:
        position = 2 * position + 1
    elif ptype in (2, 3):
        return -2, None, None, None
    elif ptype in (11, 12, 13):
        return -3, None, None, None
    data = [k for k, r in enumerate(recs) if r[0] == "scidac-binary-data"]
    if position < 0 or position >= len(data):
        return -5, None, None, None
    at = data[position]
    n = len(recs[at][3])
    if n == volume(dims) * 192:
        prec = 64
    elif n == volume(dims) * 96:
        prec = 32
    else:
        return -6, None, None, None
    stored = None
    if io_checks:
        for r in recs[at + 1:]:
            if r[0] == "scidac-checksum":
                a, b = xml_value(r[3].decode(), "suma"), xml_value(r[3].decode(), "sumb")
                if a is not None and b is not None:
                    stored = (int(a, 16), int(b, 16))
                break
            if r[0] in ("scidac-binary-data", "ildg-binary-data"):
                break
        if stored is None:
            return -1, None, None, None
    even, odd, sums = unpack(recs[at][3], dims, prec)
    return 0, even, odd, {"prec": prec, "position": position, "calculated": sums, "stored": stored}


# ---- point sources
def source_point(dims, is_, ic, global_site=0, world=1, r=0):
    """(parity, entry, component) of the one non-zero (1.0 + 0.0 i) on rank r of a T split of the LOCAL dims, or None on other ranks."""
    T, LX, LY, LZ = dims
    z = global_site % LZ
    y = global_site // LZ % LY
    x = global_site // (LZ * LY) % LX
    tg = global_site // (LZ * LY * LX)
    assert 0 <= tg < T * world
    if tg // T != r:
        return None
    lexic = (((tg - r * T) * LX + x) * LY + y) * LZ + z
    return (tg + x + y + z) & 1, lexic >> 1, 3 * is_ + ic


def odd_site(dims):
    """The global index of (T-1, LX-1, LY-1, LZ-2): an odd site for even extents, far from site 0."""
    return volume(dims) - 2
