// Host program around the compact-row half of tmlqcd_amd/csrc/gauge_pack_codec.h (tests/test_gauge_pack104_codec.py builds and runs it).
//   gauge_pack104_check selftest   the round trips and edge cases, one "name key=value ..." line each
//   gauge_pack104_check fits       stdin: twelve reals as 16-digit hex bit patterns per line -> "fits same" (1 / 0 each) per line:
//                                  the encoder's verdict, and whether the decode of what it wrote gives the twelve patterns back
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "gauge_pack_codec.h"

struct cplx { double x, y; };

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static double uniform() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
static double gauss() {   // sum of twelve uniforms: any smooth distribution will do for a random matrix
  double s = -6.0;
  for (int k = 0; k < 12; k++) s += uniform();
  return s;
}

// a random SU(3) link: Gram-Schmidt on two random complex rows, the third row their rebuild
static void random_su3(cplx (&u)[3][3]) {
  for (int r = 0; r < 2; r++)
    for (int c = 0; c < 3; c++) { u[r][c].x = gauss(); u[r][c].y = gauss(); }
  auto norm = [](cplx (&a)[3]) {
    double n = 0.0;
    for (int c = 0; c < 3; c++) n += a[c].x * a[c].x + a[c].y * a[c].y;
    n = 1.0 / sqrt(n);
    for (int c = 0; c < 3; c++) { a[c].x *= n; a[c].y *= n; }
  };
  norm(u[0]);
  double pr = 0.0, pi = 0.0;   // <row0, row1>
  for (int c = 0; c < 3; c++) { pr += u[0][c].x * u[1][c].x + u[0][c].y * u[1][c].y; pi += u[0][c].x * u[1][c].y - u[0][c].y * u[1][c].x; }
  for (int c = 0; c < 3; c++) { u[1][c].x -= pr * u[0][c].x - pi * u[0][c].y; u[1][c].y -= pr * u[0][c].y + pi * u[0][c].x; }
  norm(u[1]);
  tmhip_su3_row_rebuild(u[0], u[1], u[2]);
}

// encode, decode, compare; returns the encoder's verdict
static bool trip(const double (&v)[12], bool *same, uint32_t (*h_out)[10] = nullptr) {
  uint32_t lo[12], h[10];
  double o[12];
  const bool fits = tmhip_gpack104_encode(v, lo, h);
  tmhip_gpack104_decode(lo, h, o);
  *same = true;
  for (int k = 0; k < 12; k++) *same = *same && tmhip_gpack_bits(o[k]) == tmhip_gpack_bits(v[k]);
  if (h_out) memcpy(*h_out, h, sizeof(h));
  return fits;
}

// twelve harmless reals of mixed sign and exponent, real k replaced by x
static void filled(double (&v)[12], int k, double x) {
  for (int e = 0; e < 12; e++) v[e] = ((e & 1) ? -1.0 : 1.0) * ldexp(0.6 + 0.03 * e, -(e % 5));
  v[k] = x;
}
static double from_parts(unsigned sign, unsigned e, uint64_t mant) { return tmhip_gpack_real((uint64_t)sign << 63 | (uint64_t)e << 52 | mant); }

struct Tally { int cases = 0, fits = 0, same = 0, esc = 0; };
static void count(Tally &t, const double (&v)[12]) {
  bool sm;
  uint32_t h[10];
  const bool f = trip(v, &sm, &h);
  t.cases++; t.fits += f ? 1 : 0; t.same += (f && sm) ? 1 : 0; t.esc += (f && ((h[9] >> 24) & 15u) != 15u) ? 1 : 0;
}
static void report(const char *name, const Tally &t) { printf("%s cases=%d fits=%d same=%d escaped=%d\n", name, t.cases, t.fits, t.same, t.esc); }

static int selftest() {
  // 1. round trip of the kept rows of random SU(3) links, every rotation in turn
  {
    long long pairs = 0, notfit = 0, mismatch = 0, escaped = 0;
    for (int n = 0; n < 1000000; n++) {
      cplx u[3][3];
      random_su3(u);
      const int r = n % 3;
      double v[12];
      for (int c = 0; c < 3; c++) { v[2 * c] = u[r][c].x; v[2 * c + 1] = u[r][c].y; v[6 + 2 * c] = u[(r + 1) % 3][c].x; v[7 + 2 * c] = u[(r + 1) % 3][c].y; }
      bool sm;
      uint32_t h[10];
      if (!trip(v, &sm, &h)) notfit++;
      if (!sm) mismatch++;
      if (((h[9] >> 24) & 15u) != 15u) escaped++;
      pairs++;
    }
    printf("roundtrip pairs=%lld notfit=%lld mismatch=%lld escaped=%lld\n", pairs, notfit, mismatch, escaped);
  }
  // 2. the limits of the window, in each of the twelve positions and with either sign
  Tally lo_in, lo_esc, two_small, one, below2, two, zero, esc_min, esc_below, subn, nan, inf;
  int zero_signs = 0;
  for (int k = 0; k < 12; k++)
    for (unsigned s = 0; s < 2; s++) {
      double v[12];
      const double sg = s ? -1.0 : 1.0;
      filled(v, k, sg * ldexp(1.0, -30)); count(lo_in, v);
      filled(v, k, from_parts(s, 992, 0xFFFFFFFFFFFFFull)); count(lo_esc, v);                 // the double just below 2^-30
      v[(k + 5) % 12] = from_parts(1 - s, 992, 0xFFFFFFFFFFFFFull); count(two_small, v);      // ... and a second one
      filled(v, k, sg * 1.0); count(one, v);
      filled(v, k, from_parts(s, 1023, 0xFFFFFFFFFFFFFull)); count(below2, v);                // the largest double below 2
      filled(v, k, sg * 2.0); count(two, v);
      filled(v, k, s ? -0.0 : 0.0);
      {
        uint32_t lo[12], h[10];
        double o[12];
        const bool f = tmhip_gpack104_encode(v, lo, h);
        tmhip_gpack104_decode(lo, h, o);
        zero.cases++; zero.fits += f ? 1 : 0; zero.same += tmhip_gpack_bits(o[k]) == (uint64_t)s << 63 ? 1 : 0;
        zero_signs += (tmhip_gpack_bits(o[k]) >> 63) == s ? 1 : 0;
      }
      filled(v, k, from_parts(s, 528, 0x8000000000001ull)); count(esc_min, v);                // the smallest escapable binade
      filled(v, k, from_parts(s, 527, 0xFFFFFFFFFFFFFull)); count(esc_below, v);              // the one below it
      filled(v, k, from_parts(s, 0, 0x0000000000001ull)); count(subn, v);
      filled(v, k, from_parts(s, 0, 0x8000000000000ull)); count(subn, v);                     // (a subnormal whose low word is zero)
      filled(v, k, from_parts(s, 2047, 0x8000000000000ull)); count(nan, v);
      filled(v, k, from_parts(s, 2047, 0)); count(inf, v);
    }
  report("window_low", lo_in); report("window_low_escape", lo_esc); report("two_small", two_small); report("one", one);
  report("below_two", below2); report("two", two);
  printf("zero cases=%d fits=%d same=%d signs_kept=%d\n", zero.cases, zero.fits, zero.same, zero_signs);
  report("escape_min", esc_min); report("escape_below", esc_below); report("subnormal", subn); report("nan", nan); report("inf", inf);

  // 3. mantissas of all ones and all zeros in every position, against neighbours of the opposite pattern: every field that straddles
  // a word boundary carries a run of ones next to a run of zeros
  {
    Tally t;
    int fields_ok = 0;
    for (int pat = 0; pat < 4; pat++)
      for (int k = 0; k < 12; k++)
        for (unsigned e : {993u, 1008u, 1023u}) {
          double v[12];
          const uint64_t ones = 0xFFFFFFFFFFFFFull;
          for (int j = 0; j < 12; j++) {
            const bool on = pat == 0 ? j == k : pat == 1 ? j != k : pat == 2 ? ((j ^ k) & 1) == 0 : true;
            v[j] = from_parts(on ? 1u : 0u, on ? e : 1023u + 993u - e, on ? ones : 0ull);
          }
          count(t, v);
          uint32_t lo[12], h[10];
          tmhip_gpack104_encode(v, lo, h);
          for (int j = 0; j < 12; j++) fields_ok += tmhip_gpack104_high(tmhip_gpack104_field(h, j)) == (uint32_t)(tmhip_gpack_bits(v[j]) >> 32) ? 1 : 0;
        }
    printf("mantissa cases=%d fits=%d same=%d escaped=%d fields_ok=%d\n", t.cases, t.fits, t.same, t.esc, fields_ok);
    double v[12];
    for (int j = 0; j < 12; j++) v[j] = from_parts(1, 1023, 0xFFFFFFFFFFFFFull);
    uint32_t lo[12], h[10];
    tmhip_gpack104_encode(v, lo, h);
    printf("allones h=");
    for (int w = 9; w >= 0; w--) printf("%08x", h[w]);
    printf("\n");
  }
  // 4. the escape in every position, ext = 1 and 15 (both ends of each step), either sign
  {
    Tally t;
    int ext_ok = 0;
    for (int k = 0; k < 12; k++)
      for (unsigned s = 0; s < 2; s++)
        for (unsigned e : {992u, 962u, 558u, 528u}) {
          double v[12];
          filled(v, k, from_parts(s, e, 0xABCDE12345678ull));
          count(t, v);
          uint32_t lo[12], h[10];
          tmhip_gpack104_encode(v, lo, h);
          ext_ok += ((h[9] >> 24) & 15u) == (uint32_t)k && (h[9] >> 28) == (e >= 962u ? 1u : 15u) ? 1 : 0;
        }
    printf("escape cases=%d fits=%d same=%d escaped=%d index_and_ext_ok=%d\n", t.cases, t.fits, t.same, t.esc, ext_ok);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "selftest")) return selftest();
  if (argc == 2 && !strcmp(argv[1], "fits")) {
    for (;;) {
      double v[12];
      for (int k = 0; k < 12; k++) {
        uint64_t u;
        if (scanf("%" SCNx64, &u) != 1) return 0;
        v[k] = tmhip_gpack_real(u);
      }
      bool sm;
      const bool f = trip(v, &sm);
      printf("%d %d\n", f ? 1 : 0, sm ? 1 : 0);
    }
  }
  fprintf(stderr, "usage: gauge_pack104_check selftest | fits\n");
  return 2;
}
