// Host program around tmlqcd_amd/csrc/gauge_pack_codec.h (tests/test_gauge_pack_codec.py builds and runs it).
//   gauge_pack_codec_check selftest   the round trips and edge cases, one "name key=value ..." line each
//   gauge_pack_codec_check fits       stdin: "stored rebuilt" as 16-digit hex bit patterns per line -> "1" / "0" per line
//   gauge_pack_codec_check rebuild    stdin: 12 hex patterns per line (rows a, b: re im of elements 0..2) -> 6 patterns of conj(a x b)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "gauge_pack_codec.h"

struct cplx { double x, y; };

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// a finite, normal double of either sign with an exponent field in [lo, hi]
static double rnd_double(int lo, int hi) {
  const uint64_t r = rnd();
  const uint64_t e = (uint64_t)lo + rnd() % (uint64_t)(hi - lo + 1);
  return tmhip_gpack_real((r & 0x800fffffffffffffull) | (e << 52));
}

// one real through encode and decode in slot k of a tail whose other slots hold `fill`; returns fits, *same = the decode gave c's bits
static bool one(double c, double w, int k, int rot, int32_t fill, bool *same) {
  double c6[6], w6[6], o6[6];
  for (int e = 0; e < 6; e++) { w6[e] = 1.0 + e; c6[e] = tmhip_gpack_apply(w6[e], fill); }
  c6[k] = c; w6[k] = w;
  uint32_t t[4];
  const bool fits = tmhip_gpack_encode(c6, w6, rot, t);
  tmhip_gpack_decode(w6, t, o6);
  *same = tmhip_gpack_rot(t) == rot;
  for (int e = 0; e < 6; e++) *same = *same && tmhip_gpack_bits(o6[e]) == tmhip_gpack_bits(c6[e]);
  return fits;
}

static int selftest() {
  // 1. round trip of random rows: every offset within [-2^20, 2^20 - 1], any exponent, either sign
  long long tails = 0, pairs = 0, notfit = 0, mismatch = 0;
  for (int n = 0; n < 1000000; n++) {
    double c6[6], w6[6], o6[6];
    for (int e = 0; e < 6; e++) {
      w6[e] = rnd_double(1, 2045);
      const int64_t d = (int64_t)(rnd() % (1u << 21)) - (1 << 20);
      c6[e] = tmhip_gpack_real(tmhip_gpack_bits(w6[e]) + (uint64_t)d);
    }
    const int rot = (int)(rnd() % 3);
    uint32_t t[4];
    if (!tmhip_gpack_encode(c6, w6, rot, t)) notfit++;
    tmhip_gpack_decode(w6, t, o6);
    if (tmhip_gpack_rot(t) != rot) mismatch++;
    for (int e = 0; e < 6; e++) { pairs++; if (tmhip_gpack_bits(o6[e]) != tmhip_gpack_bits(c6[e])) mismatch++; }
    tails++;
  }
  printf("roundtrip tails=%lld pairs=%lld notfit=%lld mismatch=%lld\n", tails, pairs, notfit, mismatch);

  // 2. the limits, in every slot, on a positive and a negative rebuilt real
  const int64_t lim[4] = {(1 << 20) - 1, -(1 << 20), 1 << 20, -(1 << 20) - 1};
  for (int l = 0; l < 4; l++) {
    int fits = 0, same = 0, cases = 0;
    for (int k = 0; k < 6; k++)
      for (int s = 0; s < 2; s++) {
        const double w = s ? -0.3718 : 0.3718, c = tmhip_gpack_real(tmhip_gpack_bits(w) + (uint64_t)lim[l]);
        bool sm;
        fits += one(c, w, k, k % 3, 0, &sm) ? 1 : 0; same += sm ? 1 : 0; cases++;
      }
    printf("limit d=%" PRId64 " cases=%d fits=%d same=%d\n", lim[l], cases, fits, same);
  }

  // 3. across a binade boundary: w just below 2^-k, c just above, and the other way round
  {
    int fits = 0, same = 0, cases = 0;
    for (int k = 1; k <= 60; k++)
      for (int s = 0; s < 2; s++)
        for (int dir = 0; dir < 2; dir++) {
          const double p = ldexp(s ? -1.0 : 1.0, -k);
          const double below = tmhip_gpack_real(tmhip_gpack_bits(p) - 1000u), above = tmhip_gpack_real(tmhip_gpack_bits(p) + 1000u);
          bool sm;
          fits += one(dir ? below : above, dir ? above : below, (k + s) % 6, k % 3, -1, &sm) ? 1 : 0; same += sm ? 1 : 0; cases++;
        }
    printf("binade cases=%d fits=%d same=%d\n", cases, fits, same);
  }

  // 4. zeros: w = +-0.0 against a tiny (denormal) c of either sign
  {
    const double wz[2] = {0.0, -0.0};
    for (int a = 0; a < 2; a++)
      for (int b = 0; b < 2; b++) {
        const double c_in = tmhip_gpack_real(tmhip_gpack_bits(wz[b]) + 12345u), c_far = tmhip_gpack_real(tmhip_gpack_bits(wz[b]) + (1u << 20));
        bool s1, s2;
        const bool f1 = one(c_in, wz[a], 3, 1, 0, &s1), f2 = one(c_far, wz[a], 3, 1, 0, &s2);
        printf("zero w=%s c=%s near_fits=%d near_same=%d far_fits=%d\n", a ? "-0" : "+0", b ? "-tiny" : "+tiny", f1 ? 1 : 0, s1 ? 1 : 0, f2 ? 1 : 0);
      }
    bool s;
    const bool f = one(-0.0, 0.0, 0, 0, 0, &s);
    printf("zero w=+0 c=-0 fits=%d\n", f ? 1 : 0);
  }

  // 5. all six fields at the extreme patterns (fields 1, 3 and 4 straddle a 32-bit word), every rotation
  {
    const int32_t ext[4] = {(1 << 20) - 1, -(1 << 20), -1, 0x55555 /* 0b0_0101... */};
    int fits = 0, same = 0, cases = 0, fields = 0;
    for (int p = 0; p < 4; p++)
      for (int q = 0; q < 4; q++)
        for (int rot = 0; rot < 3; rot++) {
          double c6[6], w6[6], o6[6];
          int32_t d[6];
          for (int e = 0; e < 6; e++) { d[e] = (e & 1) ? ext[q] : ext[p]; w6[e] = (e & 2) ? -0.0625 * (e + 1) : 3.0e-7 * (e + 1); c6[e] = tmhip_gpack_apply(w6[e], d[e]); }
          uint32_t t[4];
          fits += tmhip_gpack_encode(c6, w6, rot, t) ? 1 : 0;
          tmhip_gpack_decode(w6, t, o6);
          bool sm = tmhip_gpack_rot(t) == rot;
          for (int e = 0; e < 6; e++) { sm = sm && tmhip_gpack_bits(o6[e]) == tmhip_gpack_bits(c6[e]); fields += tmhip_gpack_field(t, e) == d[e] ? 1 : 0; }
          same += sm ? 1 : 0; cases++;
        }
    printf("extreme cases=%d fits=%d same=%d fields_ok=%d\n", cases, fits, same, fields);
    const int32_t all1[6] = {-1, -1, -1, -1, -1, -1};
    uint32_t t[4];
    tmhip_gpack_tail(all1, 3, t);
    printf("allones tail=%08x%08x%08x%08x\n", t[3], t[2], t[1], t[0]);
    const int32_t mid[6] = {0, -1, 0, -1, 0, 0};   // fields at bits 21-41 and 63-83 alone
    tmhip_gpack_tail(mid, 0, t);
    printf("straddle tail=%08x%08x%08x%08x\n", t[3], t[2], t[1], t[0]);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "selftest")) return selftest();
  if (argc == 2 && !strcmp(argv[1], "fits")) {
    uint64_t s, w;
    while (scanf("%" SCNx64 " %" SCNx64, &s, &w) == 2) {
      int32_t d;
      printf("%d\n", tmhip_gpack_offset(tmhip_gpack_real(s), tmhip_gpack_real(w), d) ? 1 : 0);
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "rebuild")) {
    for (;;) {
      cplx a[3], b[3], c[3];
      uint64_t v[12];
      for (int e = 0; e < 12; e++)
        if (scanf("%" SCNx64, &v[e]) != 1) return 0;
      for (int e = 0; e < 3; e++) {
        a[e].x = tmhip_gpack_real(v[2 * e]); a[e].y = tmhip_gpack_real(v[2 * e + 1]);
        b[e].x = tmhip_gpack_real(v[6 + 2 * e]); b[e].y = tmhip_gpack_real(v[6 + 2 * e + 1]);
      }
      tmhip_su3_row_rebuild(a, b, c);
      for (int e = 0; e < 3; e++) printf("%016" PRIx64 " %016" PRIx64 "%s", tmhip_gpack_bits(c[e].x), tmhip_gpack_bits(c[e].y), e == 2 ? "\n" : " ");
    }
  }
  fprintf(stderr, "usage: gauge_pack_codec_check selftest | fits | rebuild\n");
  return 2;
}
