/* TEST / MEASUREMENT INFRASTRUCTURE ONLY (tools/spinor_io_speed.py): the host loop that the device path replaces, written here on the
 * layout rules of io/spinor_write_binary.c:145-224 and io/spinor_read_binary.c -- one thread, site by site: pick the half by parity,
 * gather the site from its e/o entry, swap the bytes of 24 reals, hand the site's bytes to the checksum routine.  The checksum
 * routine is passed in: the tool gives the reference's own DML_checksum_accum (oracle/_ref/libtmref_dml.so). */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

typedef struct { uint32_t suma, sumb; } spio_checksum;
typedef void (*spio_accum)(spio_checksum *, uint32_t rank, char *buf, size_t size);

static inline uint64_t swap64(uint64_t v) { return __builtin_bswap64(v); }
static inline uint32_t swap32(uint32_t v) { return __builtin_bswap32(v); }

/* even, odd: double [V/2][24]; record: V sites of 192 (prec 64) or 96 bytes, file order ((t LZ + z) LY + y) LX + x */
void spio_host_write(const double *even, const double *odd, int T, int LX, int LY, int LZ, int prec, unsigned char *record, spio_accum accum, uint32_t sums[2]) {
  spio_checksum cs = {0, 0};
  uint32_t rank = 0;
  const size_t bytes = prec == 64 ? 192 : 96;
  for (int t = 0; t < T; t++)
    for (int z = 0; z < LZ; z++)
      for (int y = 0; y < LY; y++)
        for (int x = 0; x < LX; x++, rank++) {
          const size_t ix = (((size_t)t * LX + x) * LY + y) * LZ + z;
          const double *p = ((t + x + y + z) % 2 == 0 ? even : odd) + 24 * (ix / 2);
          unsigned char *out = record + bytes * rank;
          if (prec == 64) {
            for (int k = 0; k < 24; k++) { uint64_t v; memcpy(&v, p + k, 8); v = swap64(v); memcpy(out + 8 * k, &v, 8); }
          } else {
            for (int k = 0; k < 24; k++) { const float f = (float)p[k]; uint32_t v; memcpy(&v, &f, 4); v = swap32(v); memcpy(out + 4 * k, &v, 4); }
          }
          accum(&cs, rank, (char *)out, bytes);
        }
  sums[0] = cs.suma; sums[1] = cs.sumb;
}

void spio_host_read(double *even, double *odd, int T, int LX, int LY, int LZ, int prec, unsigned char *record, spio_accum accum, uint32_t sums[2]) {
  spio_checksum cs = {0, 0};
  uint32_t rank = 0;
  const size_t bytes = prec == 64 ? 192 : 96;
  for (int t = 0; t < T; t++)
    for (int z = 0; z < LZ; z++)
      for (int y = 0; y < LY; y++)
        for (int x = 0; x < LX; x++, rank++) {
          const size_t ix = (((size_t)t * LX + x) * LY + y) * LZ + z;
          double *p = ((t + x + y + z) % 2 == 0 ? even : odd) + 24 * (ix / 2);
          unsigned char *in = record + bytes * rank;
          accum(&cs, rank, (char *)in, bytes);
          if (prec == 64) {
            for (int k = 0; k < 24; k++) { uint64_t v; memcpy(&v, in + 8 * k, 8); v = swap64(v); memcpy(p + k, &v, 8); }
          } else {
            for (int k = 0; k < 24; k++) { uint32_t v; float f; memcpy(&v, in + 4 * k, 4); v = swap32(v); memcpy(&f, &v, 4); p[k] = (double)f; }
          }
        }
  sums[0] = cs.suma; sums[1] = cs.sumb;
}
