// What the two file-format translation units (ildg.hip: gauge configurations, spinor_io.hip: propagators and sources) share:
// the CRC-32 of io/DML_crc32.c with compile-time tables, the zero-byte operator that joins chunk CRCs, the SciDAC checksum
// accumulators (io/dml.c:49-60), and the LIME framing on the host.  Everything sits in an anonymous namespace: each translation
// unit gets its own copy of the constant tables, nothing is exported.
#pragma once
#include "tmhip_internal.h"

#include <string>
#include <vector>

namespace {

#define ILDG_BS 256            /* threads per block of every kernel that uses these tables */
#define ILDG_SLOTS 1024        /* checksum accumulators (pairs of words) the waves spread their atomics over */

typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned bswap32(unsigned v) { return __builtin_bswap32(v); }

// ------------------------------------------------------------------ CRC-32 (io/DML_crc32.c = zlib's crc32: reflected 0xedb88320)
// Checksum: DML_crc32 over a site's bytes = its four chunks in order.  CRC(A || B) = Z_|B|(CRC(A)) xor CRC(B), Z_n = the
// CRC register advanced by n zero bytes (linear over GF(2): a 32 x 32 bit matrix), so lane j computes the CRC of its chunk (four
// bytes per step, four independent table look-ups: "slicing by 4"), applies Z_chunk (3 - j) times and the four lanes of a site
// XOR their results; the site's rank rotations and the XOR over sites follow io/dml.c:49-60.
// The tables are compile-time constants (building them per block -- above all the dependent steps of the zero operator -- cost a
// quarter of the gauge kernel); a block copies them from constant memory into LDS, where 64 lanes can index them independently.
// Any LDS structure that begins with these two members serves the functions below.
struct CrcLds { unsigned tab[4][256]; unsigned zop[32]; };
enum { CRC_ZOP_144 = 0, CRC_ZOP_72 = 1 };   // chunk sizes of the bit-serial zero operator: a 64 / 32-bit link
struct CrcConst { unsigned tab[4][256]; unsigned zop[2][32]; };
constexpr unsigned crc_entry_c(unsigned n) {
  unsigned c = n;
  for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
  return c;
}
constexpr CrcConst crc_make_const() {
  CrcConst t{};
  const int zbytes[2] = {144, 72};
  for (unsigned n = 0; n < 256; n++) {
    unsigned c = crc_entry_c(n);
    t.tab[0][n] = c;
    for (int k = 1; k < 4; k++) { c = crc_entry_c(c & 0xff) ^ (c >> 8); t.tab[k][n] = c; }
  }
  for (int w = 0; w < 2; w++)
    for (unsigned b = 0; b < 32; b++) {
      unsigned c = 1u << b;
      for (int n = 0; n < zbytes[w]; n++) c = t.tab[0][c & 0xff] ^ (c >> 8);
      t.zop[w][b] = c;
    }
  return t;
}
__constant__ CrcConst c_crc = crc_make_const();
template <class Lds>
__device__ __forceinline__ void crc_tables(Lds &L, int zsel) {
  for (int n = threadIdx.x; n < 1024; n += ILDG_BS) (&L.tab[0][0])[n] = (&c_crc.tab[0][0])[n];
  if (threadIdx.x < 32) L.zop[threadIdx.x] = c_crc.zop[zsel][threadIdx.x];
  __syncthreads();
}
template <class Lds>
__device__ __forceinline__ unsigned ildg_crc_step(unsigned c, unsigned w, const Lds &L) {
  const unsigned v = c ^ w;
  return L.tab[3][v & 0xff] ^ L.tab[2][(v >> 8) & 0xff] ^ L.tab[1][(v >> 16) & 0xff] ^ L.tab[0][v >> 24];
}
template <class Lds>
__device__ __forceinline__ unsigned ildg_zero_op(unsigned c, const Lds &L) {
  unsigned r = 0;
#pragma unroll 8
  for (int b = 0; b < 32; b++) r ^= ((c >> b) & 1u) ? L.zop[b] : 0u;
  return r;
}
// chunk CRC of lane j (already final, i.e. with DML_crc32's pre / post inversion) -> site CRC in the site's four lanes -> the site's
// two rotated words XOR-ed into (a, b) of the site's lead lane
template <class Lds>
__device__ __forceinline__ void crc_site_words(unsigned crc, int j, unsigned long long rank64, bool active, const Lds &L, unsigned &a, unsigned &b) {
  if (j < 3) crc = ildg_zero_op(crc, L);
  if (j < 2) crc = ildg_zero_op(crc, L);
  if (j < 1) crc = ildg_zero_op(crc, L);
  crc ^= __shfl_xor(crc, 1, 64);
  crc ^= __shfl_xor(crc, 2, 64);               // every lane of the site now holds DML_crc32(0, site bytes)
  const unsigned rank = (unsigned)rank64;      // DML_SiteRank is uint32_t (io/dml.h:40)
  const unsigned r29 = rank % 29, r31 = rank % 31;
  const bool lead = active && j == 0;
  a ^= lead ? (r29 ? (crc << r29 | crc >> (32 - r29)) : crc) : 0u;
  b ^= lead ? (r31 ? (crc << r31 | crc >> (32 - r31)) : crc) : 0u;
}
// the wave's words into its slot
__device__ __forceinline__ void crc_wave_flush(unsigned a, unsigned b, unsigned *sums) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a ^= __shfl_xor(a, off, 64); b ^= __shfl_xor(b, off, 64); }
  // XOR is associative and commutative: any order gives the same words.  One address would serialise the atomics of all waves
  // (measured: 131 072 atomics on one word = 1.5 ms, the whole kernel): ILDG_SLOTS pairs, folded on the host.
  if ((threadIdx.x & 63) == 0) {
    unsigned *slot = sums + 2 * ((blockIdx.x * (ILDG_BS / 64) + (threadIdx.x >> 6)) & (ILDG_SLOTS - 1));
    atomicXor(slot, a); atomicXor(slot + 1, b);
  }
}
template <class Lds>
__device__ __forceinline__ void ildg_checksum_accum(unsigned crc, int j, unsigned long long rank64, bool active, const Lds &L, unsigned *sums) {
  unsigned a = 0, b = 0;
  crc_site_words(crc, j, rank64, active, L, a, b);
  crc_wave_flush(a, b, sums);
}

// ------------------------------------------------------------------ LIME framing (host)
// written from the published format of c-lime 1.3.x (not part of the reference tree): 144-byte record headers
//   0: magic 0x456789ab (be32)  4: version 1 (be16)  6: MB 0x80 | ME 0x40  8: data length (be64)  16: type, 128 bytes, NUL-padded
// followed by the data padded to a multiple of 8 bytes
const unsigned LIME_MAGIC = 0x456789abu;
struct LimeRecord { std::string type; unsigned long long bytes; long data_pos; int mb, me; };

unsigned long long be64(const unsigned char *p) { unsigned long long v = 0; for (int i = 0; i < 8; i++) v = (v << 8) | p[i]; return v; }
void put_be(unsigned char *p, unsigned long long v, int n) { for (int i = n - 1; i >= 0; i--) { p[i] = (unsigned char)(v & 0xff); v >>= 8; } }

// the records of a LIME file in order; -1 on a malformed header
int lime_scan(FILE *fp, std::vector<LimeRecord> &recs) {
  unsigned char h[144];
  long pos = 0;
  for (;;) {
    if (fseek(fp, pos, SEEK_SET)) return -1;
    const size_t n = fread(h, 1, 144, fp);
    if (n == 0) return 0;                       // LIME_EOF
    if (n != 144) return -1;
    const unsigned magic = ((unsigned)h[0] << 24) | ((unsigned)h[1] << 16) | ((unsigned)h[2] << 8) | h[3];
    const unsigned version = ((unsigned)h[4] << 8) | h[5];
    if (magic != LIME_MAGIC || version != 1) return -1;
    LimeRecord r;
    r.mb = (h[6] & 0x80) != 0; r.me = (h[6] & 0x40) != 0;
    r.bytes = be64(h + 8);
    h[143] = 0;
    r.type = std::string(reinterpret_cast<const char *>(h + 16));
    r.data_pos = pos + 144;
    recs.push_back(r);
    pos += 144 + (long)((r.bytes + 7) / 8 * 8);
  }
}
int lime_write_header(FILE *fp, int mb, int me, const char *type, unsigned long long bytes) {
  unsigned char h[144];
  memset(h, 0, sizeof(h));
  put_be(h, LIME_MAGIC, 4);
  put_be(h + 4, 1, 2);
  h[6] = (unsigned char)((mb ? 0x80 : 0) | (me ? 0x40 : 0));
  put_be(h + 8, bytes, 8);
  strncpy(reinterpret_cast<char *>(h + 16), type, 127);
  return fwrite(h, 1, 144, fp) == 144 ? 0 : -1;
}
int lime_write_data(FILE *fp, const void *data, unsigned long long bytes) {
  static const unsigned char zero[8] = {0};
  if (bytes && fwrite(data, 1, bytes, fp) != bytes) return -1;
  const unsigned long long pad = (8 - bytes % 8) % 8;
  if (pad && fwrite(zero, 1, pad, fp) != pad) return -1;
  return 0;
}
int lime_write_message(FILE *fp, int mb, int me, const char *type, const std::string &msg) {
  return lime_write_header(fp, mb, me, type, msg.size()) || lime_write_data(fp, msg.data(), msg.size());
}
int lime_read_string(FILE *fp, const LimeRecord &r, std::string &out) {
  out.resize(r.bytes);
  if (fseek(fp, r.data_pos, SEEK_SET)) return -1;
  return r.bytes == 0 || fread(&out[0], 1, r.bytes, fp) == r.bytes ? 0 : -1;
}
// io/utils_parse_ildgformat_xml.c / utils_parse_checksum_xml.c: tokens separated by "<> \n\t", the value is the token behind the tag
bool xml_value(const std::string &msg, const char *tag, std::string &val) {
  std::vector<std::string> tok;
  size_t i = 0;
  const std::string sep = "<> \n\t";
  while (i < msg.size()) {
    const size_t b = msg.find_first_not_of(sep, i);
    if (b == std::string::npos) break;
    size_t e = msg.find_first_of(sep, b);
    if (e == std::string::npos) e = msg.size();
    tok.push_back(msg.substr(b, e - b));
    i = e;
  }
  const size_t n = strlen(tag);
  for (size_t k = 0; k + 1 < tok.size(); k++)
    if (!strncmp(tok[k].c_str(), tag, n)) { val = tok[k + 1]; return true; }
  return false;
}
// io/utils_write_checksum.c:30-35
std::string checksum_message(const unsigned cs[2]) {
  char chk[512];
  snprintf(chk, sizeof(chk), "<?xml version=\"1.0\" encoding=\"UTF-8\"?>\n<scidacChecksum>\n  <version>1.0</version>\n  <suma>%08x</suma>\n  <sumb>%08x</sumb>\n</scidacChecksum>",
           cs[0], cs[1]);
  return std::string(chk);
}

int sums_reserve(tmhip_ctx *ctx) {
  if (!ctx->io_sums) TMHIP_CHECK(hipMalloc((void **)&ctx->io_sums, 2 * ILDG_SLOTS * sizeof(unsigned)));
  TMHIP_CHECK(hipMemsetAsync(ctx->io_sums, 0, 2 * ILDG_SLOTS * sizeof(unsigned), ctx->stream));
  return 0;
}
// the checksum words of the launch that has just been enqueued (synchronises the stream)
int sums_fetch(tmhip_ctx *ctx, unsigned out[2]) {
  static unsigned h[2 * ILDG_SLOTS];
  TMHIP_CHECK(hipMemcpyAsync(h, ctx->io_sums, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  out[0] = out[1] = 0;
  for (int k = 0; k < ILDG_SLOTS; k++) { out[0] ^= h[2 * k]; out[1] ^= h[2 * k + 1]; }
  return 0;
}

}  // namespace
