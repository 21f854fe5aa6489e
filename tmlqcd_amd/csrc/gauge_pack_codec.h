// The codec of the packed link read (TmhipGaugePack, tmhip_internal.h): the third row of an SU(3) link from the
// other two, the 16-byte tail that says how far the stored row lies from that rebuild, and the compact form of the two kept rows
// (88 instead of 96 bytes: the end of this file).  Plain inline functions, host and device: gauge_pack_kernel (md_update.hip)
// encodes and verifies with them, hop_dir<.., GAUX 15 | 16, ..> (hopping_impl.inc) decodes with them, tests/test_gauge_pack_codec.py
// and tests/test_gauge_pack104_codec.py compile them into host programs.  Nothing here depends on HIP.
//
// Tail, 128 bits as four 32-bit words, bit n of the tail = bit n % 32 of word n / 32:
//   bits 21 k .. 21 k + 20, k = 0..5 : d_k, a 21-bit two's-complement integer; k = 2 e + (0: re, 1: im) of element e of the rebuilt row
//   bits 126 .. 127                  : the rotation r -- rows r and r + 1 (mod 3) are kept, row r + 2 is rebuilt
// The stored real is the double whose 64-bit pattern is bits(w) + d_k in plain 64-bit integer addition, w the rebuilt real: a
// distance in ulps that is monotone across binade boundaries.  A stored real whose sign differs from w's has no offset.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TMHIP_HD __host__ __device__ __forceinline__
#else
#define TMHIP_HD inline
#endif

constexpr int TMHIP_GPACK_BITS = 21;
constexpr int64_t TMHIP_GPACK_DMAX = ((int64_t)1 << (TMHIP_GPACK_BITS - 1)) - 1, TMHIP_GPACK_DMIN = -((int64_t)1 << (TMHIP_GPACK_BITS - 1));

// c = conj(a x b): ONE sequence of operations for the kernel that builds the packed copy (and verifies every link bit for bit) and for
// the stencil that reads it.  Explicit fma() calls and no contraction: both callers round exactly alike.  (The 121-byte format
// ended with "+ residual", which turned a -0.0 into +0.0; this one may return either zero.  Both sides call this function and every
// link is verified against the stored row, so the sign of a zero is encoded like any other bit.)  C: any type with members x (re), y (im).
template <class C>
TMHIP_HD void tmhip_su3_row_rebuild(const C (&a)[3], const C (&b)[3], C (&c)[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 3; k++) {
    const int i = (k + 1) % 3, j = (k + 2) % 3;   // (a x b)_k = a_i b_j - a_j b_i
    double re = a[i].x * b[j].x;
    re = fma(-a[i].y, b[j].y, re);
    re = fma(-a[j].x, b[i].x, re);
    re = fma(a[j].y, b[i].y, re);
    double im = a[i].x * b[j].y;
    im = fma(a[i].y, b[j].x, im);
    im = fma(-a[j].x, b[i].y, im);
    im = fma(-a[j].y, b[i].x, im);
    c[k].x = re;
    c[k].y = -im;
  }
}

TMHIP_HD uint64_t tmhip_gpack_bits(double v) { uint64_t u; __builtin_memcpy(&u, &v, 8); return u; }
TMHIP_HD double tmhip_gpack_real(uint64_t u) { double v; __builtin_memcpy(&v, &u, 8); return v; }

// the offset of one real; false: it does not fit (too far, or the signs differ)
TMHIP_HD bool tmhip_gpack_offset(double stored, double rebuilt, int32_t &d) {
  const uint64_t s = tmhip_gpack_bits(stored), w = tmhip_gpack_bits(rebuilt);
  const int64_t diff = (int64_t)(s - w);
  d = (int32_t)diff;
  return ((s ^ w) >> 63) == 0 && diff >= TMHIP_GPACK_DMIN && diff <= TMHIP_GPACK_DMAX;
}
TMHIP_HD double tmhip_gpack_apply(double rebuilt, int32_t d) { return tmhip_gpack_real(tmhip_gpack_bits(rebuilt) + (uint64_t)(int64_t)d); }

// field k of the tail, sign-extended (k is a constant wherever this is called from an unrolled loop: two shifts, an or, a bit-field extract)
TMHIP_HD int32_t tmhip_gpack_field(const uint32_t (&t)[4], int k) {
  const int o = TMHIP_GPACK_BITS * k, w = o >> 5, sh = o & 31;
  uint32_t v = t[w] >> sh;
  if (sh + TMHIP_GPACK_BITS > 32) v |= t[w + 1] << (32 - sh);
  return (int32_t)(v << (32 - TMHIP_GPACK_BITS)) >> (32 - TMHIP_GPACK_BITS);
}
TMHIP_HD int tmhip_gpack_rot(const uint32_t (&t)[4]) { return (int)(t[3] >> 30); }

TMHIP_HD void tmhip_gpack_tail(const int32_t (&d)[6], int rot, uint32_t (&t)[4]) {
  t[0] = t[1] = t[2] = 0u;
  t[3] = (uint32_t)rot << 30;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 6; k++) {
    const int o = TMHIP_GPACK_BITS * k, w = o >> 5, sh = o & 31;
    const uint32_t v = (uint32_t)d[k] & ((1u << TMHIP_GPACK_BITS) - 1u);
    t[w] |= v << sh;
    if (sh + TMHIP_GPACK_BITS > 32) t[w + 1] |= v >> (32 - sh);
  }
}

// stored row c, rebuilt row w (re, im of elements 0..2), rotation -> tail; false: some real does not fit (the tail is then the
// rotation with offsets of zero: defined, and wrong)
TMHIP_HD bool tmhip_gpack_encode(const double (&c)[6], const double (&w)[6], int rot, uint32_t (&t)[4]) {
  int32_t d[6];
  bool fits = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 6; k++) fits = tmhip_gpack_offset(c[k], w[k], d[k]) && fits;
  if (!fits)
    for (int k = 0; k < 6; k++) d[k] = 0;
  tmhip_gpack_tail(d, rot, t);
  return fits;
}
// rebuilt row w, tail -> stored row c
TMHIP_HD void tmhip_gpack_decode(const double (&w)[6], const uint32_t (&t)[4], double (&c)[6]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 6; k++) c[k] = tmhip_gpack_apply(w[k], tmhip_gpack_field(t, k));
}

// ---- the compact form of the two kept rows: 88 bytes for twelve reals, exact ("gauge_pack_compact", the 104-byte read) ----
// Every real of a link that has a rotation is below 2 in magnitude, and all but a stray one are at or above 2^-30: five bits of
// exponent do the work of eleven.  The twelve reals, in the order a0.re a0.im a1.re .. a2.im b0.re .. b2.im:
//   lo[k]            bits 31..0 of real k as they are (three 16-byte planes)
//   h[0..9], 320 bits, bit n = bit n % 32 of word n / 32 (two 16-byte planes and one 8-byte plane):
//     bits 26 k .. 26 k + 25 : the field of real k -- bit 25 the sign, bits 24..20 the exponent code c, bits 19..0 bits 51..32 of the double
//                              c = 0: biased exponent 0 (+-0.0);  c = 1..31: biased exponent 992 + c, magnitudes in [2^-30, 2)
//     bits 312 .. 315        : the index of the one escaped real of the link, 15: none
//     bits 316 .. 319        : ext = 1..15 -- the escaped real's biased exponent is 992 + c - 31 ext, down to 528 (2^-495)
// A rebuilt real below about 5e-7 never fits the tail (its offset is about 0.5 / |x| ulps), so a tiny real always sits in a kept
// row: the escape is what keeps a field with one such real compact.  A pair of rows "fits compact" when every real is +-0.0 or lies
// in [2^-30, 2), except at most one in [2^-495, 2^-30); anything else -- a value at or above 2, a subnormal, a NaN, an infinity, a
// second small real -- does not, and tmhip_gpack104_encode says so.  Integer operations only.
constexpr int TMHIP_GPACK104_FIELD = 26;
constexpr uint32_t TMHIP_GPACK104_EBASE = 992, TMHIP_GPACK104_ESTEP = 31, TMHIP_GPACK104_EXTMAX = 15;

// field k of h (k is a constant wherever this is called from an unrolled loop)
TMHIP_HD uint32_t tmhip_gpack104_field(const uint32_t (&h)[10], int k) {
  const int o = TMHIP_GPACK104_FIELD * k, w = o >> 5, sh = o & 31;
  uint32_t v = h[w] >> sh;
  if (sh + TMHIP_GPACK104_FIELD > 32) v |= h[w + 1] << (32 - sh);
  return v & ((1u << TMHIP_GPACK104_FIELD) - 1u);
}
// the high word of a real from its field; base: what a non-zero exponent code is lifted by, 992 << 20 for a real without the escape
TMHIP_HD uint32_t tmhip_gpack104_high(uint32_t f, uint32_t base = TMHIP_GPACK104_EBASE << 20) {
  const uint32_t x = f & 0x1FFFFFFu;
  return (x + ((x >> 20) ? base : 0u)) | ((f >> 25) << 31);
}

// twelve reals -> lo, h; false: the rows do not fit compact (the planes are then defined, and wrong)
TMHIP_HD bool tmhip_gpack104_encode(const double (&v)[12], uint32_t (&lo)[12], uint32_t (&h)[10]) {
  bool fits = true;
  uint32_t esc = 15u, ext = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int w = 0; w < 10; w++) h[w] = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 12; k++) {
    const uint64_t u = tmhip_gpack_bits(v[k]);
    lo[k] = (uint32_t)u;
    const uint32_t hi = (uint32_t)(u >> 32), e = (hi >> 20) & 0x7FFu, m = hi & 0xFFFFFu;
    uint32_t c = 0u;
    if (e == 0u) fits = fits && m == 0u && lo[k] == 0u;                                  // +-0.0; a subnormal does not fit
    else if (e > TMHIP_GPACK104_EBASE && e <= TMHIP_GPACK104_EBASE + 31u) c = e - TMHIP_GPACK104_EBASE;
    else if (e <= TMHIP_GPACK104_EBASE && e + TMHIP_GPACK104_ESTEP * TMHIP_GPACK104_EXTMAX > TMHIP_GPACK104_EBASE && esc == 15u) {
      esc = (uint32_t)k;
      ext = (TMHIP_GPACK104_EBASE + 31u - e) / TMHIP_GPACK104_ESTEP;                      // the smallest ext that brings c to 1..31
      c = e + TMHIP_GPACK104_ESTEP * ext - TMHIP_GPACK104_EBASE;
    } else fits = false;                                                                 // >= 2, inf, NaN, below 2^-495, or a second small real
    const uint32_t f = (hi >> 31) << 25 | c << 20 | m;
    const int o = TMHIP_GPACK104_FIELD * k, w = o >> 5, sh = o & 31;
    h[w] |= f << sh;
    if (sh + TMHIP_GPACK104_FIELD > 32) h[w + 1] |= f >> (32 - sh);
  }
  h[9] |= (esc | ext << 4) << 24;
  return fits;
}

// lo, h -> twelve reals.  The escape is a select per real on what its exponent code is lifted by -- a compare and a select, no
// branch: behind a wave-uniform branch (a ballot of "index != 15") it would cost one scalar branch per link, but the branch cuts
// every hop of the stencil into basic blocks, and the instance then spills 1.6 kB per lane under its bound of three waves per SIMD
// (256 registers left to itself), where the straight-line form takes 144 registers.
TMHIP_HD void tmhip_gpack104_decode(const uint32_t (&lo)[12], const uint32_t (&h)[10], double (&v)[12]) {
  const uint32_t esc = (h[9] >> 24) & 15u, plain = TMHIP_GPACK104_EBASE << 20, escaped = plain - ((TMHIP_GPACK104_ESTEP * (h[9] >> 28)) << 20);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 12; k++) {
    const uint32_t hi = tmhip_gpack104_high(tmhip_gpack104_field(h, k), esc == (uint32_t)k ? escaped : plain);
    v[k] = tmhip_gpack_real((uint64_t)hi << 32 | lo[k]);
  }
}
