// Propagators and sources in and out of HBM (io/spinor_read.c, io/spinor_write.c, io/spinor_{read,write}_binary.c, start.c:707-830).
//
// The reference walks a "scidac-binary-data" record site by site on one thread (io/spinor_write_binary.c:145-224: loops t, z, y, x;
// per site it picks the even or the odd field by (t + x + y + z) % 2, looks up g_lexic2eosub[g_ipt[t][x][y][z]], byte-swaps 24 reals
// and feeds 192 or 96 bytes to DML_checksum_accum).  Here the record travels as it lies in the file and ONE kernel per direction does
// the rest in HBM.  The two sides want different things: the device field is SoA, v2d d[12][ns] per parity, site = lexicographic
// index / 2, so a row (t, x, y, .) is LZ / 2 consecutive entries in each of 24 planes; the file has x fastest, so a run (t, z, y, .)
// is LX * 192 contiguous bytes.  The x <-> z transposition happens in LDS.
//
// Tile: a block owns one (t, y), SPIO_XG = 4 consecutive x and up to SPIO_ZC = 32 consecutive z (longer LZ: looped), held in LDS as
// the file's bytes, [z][x][192 or 96].  4 x-values make the file side runs of 768 (384) bytes = 6 (3) whole 128-byte lines, and 32 z
// the device side rows of 16 entries = 256 bytes per plane and parity; 4 x 32 x 192 B = 24.5 KB with the padding, five blocks per CU
// beside the 5 KB of CRC tables.  (Measured at 32^4, 64 bit, pack / unpack: 8 x-values, 49 KB and three blocks per CU 0.247 / 0.222 ms;
// 4 x-values 0.152 / 0.131; 8 x-values with 16 z the same as 4 with 32.  The three phases of a block -- field rows, checksum, file
// runs -- are separated by barriers, so what hides the latency of one block's loads is the other blocks of the CU.)
// Bank rules (64 banks of 4 bytes; a 16-byte LDS store is serviced in groups of 8 consecutive lanes over 32 banks, an 8-byte one
// in groups of 16): in the transposing phase consecutive lanes are consecutive z, i.e. one tile row apart, and a row of 4 x 48
// words would put them on six banks only.  Rows are therefore padded by one element (4 words for 64-bit data, 2 for 32-bit): row
// stride = 4 (2) mod 32 words, the 8 (16) lanes of a group cover the 32 banks exactly once.  The row-wise phase (whole runs to or
// from the file) has consecutive lanes on consecutive elements and is conflict-free by itself.
// Checksum: four lanes per site, each the CRC of a quarter of the site's bytes (c = 48 or 24 bytes, read from the LDS image: lane
// stride 12 (6) words = 3 elements, and 3 is prime to the 16 (32) element-banks a 16-byte (8-byte) read sees).  The quarters are
// joined pairwise -- CRC(A || B) = Z_|B|(CRC(A)) xor CRC(B) -- with Z_c, then Z_2c.  The bit-serial zero operator of io_common.h
// (32 steps, three times per site for these short chunks) took a third of the kernel; here Z is eight look-ups in 16-entry tables,
// one per nibble of the register (Z is linear over GF(2)).  A wave keeps its two words in registers over the whole tile and issues
// one pair of atomics.
#include "io_common.h"

namespace {

#define SPIO_XG 4
#define SPIO_ZC 32

struct SpioGeom { int T, LX, LY, LZ, toff, ns; unsigned long long rank0; };   // local extents; global t of local t = 0; plane stride; DML rank of the first file site

// PW = 32-bit words per complex number in the file: 4 (64-bit data) or 2.  One element = one complex number = Piece.
template <int PW> struct SpioPiece;
template <> struct SpioPiece<4> { typedef v4u type; };
template <> struct SpioPiece<2> { typedef v2u type; };

template <int PW> __device__ __forceinline__ typename SpioPiece<PW>::type spio_to_file(v2d v);
template <> __device__ __forceinline__ v4u spio_to_file<4>(v2d v) {
  const unsigned long long re = (unsigned long long)__double_as_longlong(v.x), im = (unsigned long long)__double_as_longlong(v.y);
  return v4u{bswap32((unsigned)(re >> 32)), bswap32((unsigned)re), bswap32((unsigned)(im >> 32)), bswap32((unsigned)im)};
}
template <> __device__ __forceinline__ v2u spio_to_file<2>(v2d v) {                                   // be_to_cpu_assign_double2single (io/utils.h)
  return v2u{bswap32(__float_as_uint((float)v.x)), bswap32(__float_as_uint((float)v.y))};
}
__device__ __forceinline__ v2d spio_from_file(v4u w) {
  const unsigned long long re = ((unsigned long long)bswap32(w.x) << 32) | bswap32(w.y), im = ((unsigned long long)bswap32(w.z) << 32) | bswap32(w.w);
  return v2d{__longlong_as_double((long long)re), __longlong_as_double((long long)im)};
}
__device__ __forceinline__ v2d spio_from_file(v2u w) {                                                // be_to_cpu_assign_single2double
  return v2d{(double)__uint_as_float(bswap32(w.x)), (double)__uint_as_float(bswap32(w.y))};
}

// Z_n as nibble tables: Z_n(c) = xor over k of nib[k][(c >> 4k) & 15], nib[k][v] = Z_n(v << 4k).  Sizes 24, 48 and 96 bytes:
// 32-bit data joins with (24, 48), 64-bit data with (48, 96).
struct SpioZop { unsigned nib[3][8][16]; };
constexpr SpioZop spio_make_zop() {
  SpioZop t{};
  const int zbytes[3] = {24, 48, 96};
  for (int w = 0; w < 3; w++)
    for (int k = 0; k < 8; k++)
      for (unsigned v = 0; v < 16; v++) {
        unsigned c = v << (4 * k);
        for (int n = 0; n < zbytes[w]; n++) c = crc_entry_c(c & 0xff) ^ (c >> 8);
        t.nib[w][k][v] = c;
      }
  return t;
}
__constant__ SpioZop c_spio_zop = spio_make_zop();
struct SpioLds { CrcLds crc; unsigned nib[2][8][16]; };       // [0]: Z over one quarter of a site, [1]: over two
__device__ __forceinline__ unsigned spio_zero_op(unsigned c, const unsigned (&nib)[8][16]) {
  unsigned r = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) r ^= nib[k][(c >> (4 * k)) & 15u];
  return r;
}
// the final CRC of lane j's quarter -> the site's CRC in its four lanes -> the site's two rotated words XOR-ed into (a, b) of its
// lead lane (io/dml.c:49-60; DML_SiteRank is uint32_t)
__device__ __forceinline__ void spio_site_words(unsigned crc, int j, unsigned long long rank64, bool active, const SpioLds &L, unsigned &a, unsigned &b) {
  if (!(j & 1)) crc = spio_zero_op(crc, L.nib[0]);
  crc ^= __shfl_xor(crc, 1, 64);               // both lanes of a pair: the CRC of its half of the site
  if (j < 2) crc = spio_zero_op(crc, L.nib[1]);
  crc ^= __shfl_xor(crc, 2, 64);               // all four: DML_crc32(0, site bytes)
  const unsigned rank = (unsigned)rank64;
  const unsigned r29 = rank % 29, r31 = rank % 31;
  const bool lead = active && j == 0;
  a ^= lead ? (r29 ? (crc << r29 | crc >> (32 - r29)) : crc) : 0u;
  b ^= lead ? (r31 ? (crc << r31 | crc >> (32 - r31)) : crc) : 0u;
}

// PACK: fields -> file bytes; else file bytes -> fields.  Grid: T * LY * ceil(LX / SPIO_XG) blocks of ILDG_BS threads.
// Dynamic LDS: SpioLds, then min(LZ, SPIO_ZC) rows of SPIO_XG * 12 + 1 elements.
template <int PW, bool PACK>
__global__ __launch_bounds__(ILDG_BS) void spinor_io_kernel(typename SpioPiece<PW>::type *__restrict__ file, v2d *__restrict__ even, v2d *__restrict__ odd,
                                                            SpioGeom g, unsigned *sums) {
  typedef typename SpioPiece<PW>::type Piece;
  extern __shared__ v4u spio_lds[];
  SpioLds &S = *reinterpret_cast<SpioLds *>(spio_lds);
  CrcLds &L = S.crc;
  Piece *tile = reinterpret_cast<Piece *>(spio_lds + sizeof(SpioLds) / sizeof(v4u));
  constexpr int ROW = SPIO_XG * 12 + 1;        // elements per tile row, one of them padding
  (&S.nib[0][0][0])[threadIdx.x] = (&c_spio_zop.nib[PW == 4 ? 1 : 0][0][0])[threadIdx.x];      // 256 threads, 2 x 128 words: two consecutive sizes
  crc_tables(L, CRC_ZOP_144);                  // (the byte tables; its bit-serial operator is not used here)
  const int nxg = (g.LX + SPIO_XG - 1) / SPIO_XG;
  int bid = blockIdx.x;
  const int xg = bid % nxg; bid /= nxg;
  const int y = bid % g.LY, t = bid / g.LY;
  const int x0 = xg * SPIO_XG, nx = g.LX - x0 < SPIO_XG ? g.LX - x0 : SPIO_XG;
  const int j = threadIdx.x & 3;
  unsigned suma = 0, sumb = 0;
  for (int z0 = 0; z0 < g.LZ; z0 += SPIO_ZC) {
    const int nz = g.LZ - z0 < SPIO_ZC ? g.LZ - z0 : SPIO_ZC;
    if (z0) __syncthreads();                   // the tile of the previous z range has been used up
    // 1. the tile as the file's bytes
    if (PACK) {
      // rows of the fields in: consecutive lanes = consecutive z of one (x, component), alternating between the two parities
      for (int e = threadIdx.x; e < nx * 12 * nz; e += ILDG_BS) {
        const int zl = e % nz, c = (e / nz) % 12, xl = e / (nz * 12);
        const int x = x0 + xl, z = z0 + zl;
        const size_t ix = (((size_t)t * g.LX + x) * g.LY + y) * g.LZ + z;
        const v2d *src = ((g.toff + t + x + y + z) & 1) ? odd : even;
        tile[zl * ROW + xl * 12 + c] = spio_to_file<PW>(src[(size_t)c * g.ns + (ix >> 1)]);
      }
    } else {
      // runs of the file in: row zl of the tile = the nx * 12 elements that follow file site (t, z, y, x0)
      for (int q = threadIdx.x; q < nz * nx * 12; q += ILDG_BS) {
        const int zl = q / (nx * 12), k = q - zl * (nx * 12);
        const size_t f = (((size_t)t * g.LZ + z0 + zl) * g.LY + y) * g.LX + x0;
        tile[zl * ROW + k] = __builtin_nontemporal_load(file + f * 12 + k);
      }
    }
    __syncthreads();
    // 2. checksum from the LDS image: four lanes per site
    for (int s0 = 0; s0 < nz * nx; s0 += ILDG_BS / 4) {       // the same trip count in every lane: the shuffles below are wave-wide
      const int s = s0 + (threadIdx.x >> 2);
      const bool active = s < nz * nx;
      const int zl = active ? s / nx : 0, xl = active ? s - zl * nx : 0;
      unsigned crc = 0xffffffffu;
      if (active) {
        const Piece *p = tile + zl * ROW + xl * 12 + j * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const Piece w = p[k];
          crc = ildg_crc_step(ildg_crc_step(crc, w.x, L), w.y, L);
          if constexpr (PW == 4) crc = ildg_crc_step(ildg_crc_step(crc, w.z, L), w.w, L);
        }
      }
      const unsigned long long f = (((unsigned long long)t * g.LZ + z0 + zl) * g.LY + y) * g.LX + x0 + xl;
      spio_site_words(crc ^ 0xffffffffu, j, g.rank0 + f, active, S, suma, sumb);
    }
    // 3. the tile out (both read it: no barrier between 2 and 3)
    if (PACK) {
      for (int q = threadIdx.x; q < nz * nx * 12; q += ILDG_BS) {
        const int zl = q / (nx * 12), k = q - zl * (nx * 12);
        const size_t f = (((size_t)t * g.LZ + z0 + zl) * g.LY + y) * g.LX + x0;
        file[f * 12 + k] = tile[zl * ROW + k];
      }
    } else {
      for (int e = threadIdx.x; e < nx * 12 * nz; e += ILDG_BS) {
        const int zl = e % nz, c = (e / nz) % 12, xl = e / (nz * 12);
        const int x = x0 + xl, z = z0 + zl;
        const size_t ix = (((size_t)t * g.LX + x) * g.LY + y) * g.LZ + z;
        v2d *dst = ((g.toff + t + x + y + z) & 1) ? odd : even;
        dst[(size_t)c * g.ns + (ix >> 1)] = spio_from_file(tile[zl * ROW + xl * 12 + c]);
      }
    }
  }
  crc_wave_flush(suma, sumb, sums);
}

bool spio_field_ok(const tmhip_ctx *ctx, const tmhip_field *f) { return f && f->kind == TMHIP_FIELD_EO && f->prec == 0 && f->d && f->ns == ctx->ns; }

// the kernel on the record in ctx->stage (this rank's sites)
template <bool PACK>
int spio_launch(tmhip_ctx *ctx, tmhip_field *even, tmhip_field *odd, int prec) {
  const SpioGeom g{ctx->g.T, ctx->g.LX, ctx->g.LY, ctx->g.LZ, ctx->g.proc_t * ctx->g.T, ctx->ns,
                   (unsigned long long)ctx->g.proc_t * ctx->g.T * ctx->g.LX * ctx->g.LY * ctx->g.LZ};
  const int rows = g.LZ < SPIO_ZC ? g.LZ : SPIO_ZC;
  const size_t lds = sizeof(SpioLds) + (size_t)rows * (SPIO_XG * 12 + 1) * (prec == 64 ? 16 : 8);
  const dim3 grid((unsigned)(g.T * g.LY * ((g.LX + SPIO_XG - 1) / SPIO_XG)));
  if (prec == 64) hipLaunchKernelGGL((spinor_io_kernel<4, PACK>), grid, dim3(ILDG_BS), lds, ctx->stream, (v4u *)ctx->stage, even->d, odd->d, g, ctx->io_sums);
  else hipLaunchKernelGGL((spinor_io_kernel<2, PACK>), grid, dim3(ILDG_BS), lds, ctx->stream, (v2u *)ctx->stage, even->d, odd->d, g, ctx->io_sums);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

// io/utils_parse_propagator_type.c:22-91 on the scanned records
int parse_propagator_type(FILE *fp, const std::vector<LimeRecord> &recs) {
  int prop_type = -1, found = 0;
  for (const LimeRecord &r : recs) {
    const bool is_prop = r.type == "propagator-type", is_src = r.type == "source-type";
    if (!is_prop && !is_src) continue;
    std::string msg;
    if (lime_read_string(fp, r, msg)) break;
    const char *s = msg.c_str();
    if (is_prop) {
      if (!strcmp("DiracFermion_Sink", s)) prop_type = 0;
      else if (!strcmp("DiracFermion_Source_Sink_Pairs", s)) prop_type = 1;
      else if (!strcmp("DiracFermion_ScalarSource_TwelveSink", s)) prop_type = 2;
      else if (!strcmp("DiracFermion_ScalarSource_FourSink", s)) prop_type = 3;
      else if (!strcmp("DiracFermion_Deflation_Field", s)) prop_type = 4;
      else { fprintf(stderr, "Unrecognized propagator-type, found type: %s.\n", s); break; }
    } else {
      if (!strcmp("DiracFermion_Source", s)) prop_type = 10;
      else if (!strcmp("DiracFermion_ScalarSource", s)) prop_type = 11;
      else if (!strcmp("DiracFermion_FourScalarSource", s)) prop_type = 12;
      else if (!strcmp("DiracFermion_TwelveScalarSource", s)) prop_type = 13;
      else { fprintf(stderr, "Unrecognized source-type, found type: %s\n", s); break; }
    }
    found = 1;
    break;
  }
  if (!found) fprintf(stderr, "Unable to find either source-type or propagator-type record.\nWARNING: Continuing in blind faith.\n");
  return prop_type;
}

}  // namespace

extern "C" {

/* io/spinor_write_binary.c:145-224 + io/dml.c:49-60: see include/tmlqcd_hip.h */
int tmhip_spinor_pack(tmhip_ctx *ctx, tmhip_field *even, tmhip_field *odd, void *file_bytes, int prec, unsigned *sums) {
  if (!file_bytes || (prec != 32 && prec != 64)) TMHIP_FAIL("tmhip_spinor_pack: null buffer or precision %d (32 or 64)", prec);
  if (!spio_field_ok(ctx, even) || !spio_field_ok(ctx, odd) || even == odd) TMHIP_FAIL("tmhip_spinor_pack: needs two distinct fp64 one-parity fields (a FULL field is passed as its two views)");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const size_t fbytes = (size_t)ctx->V * (prec == 64 ? 192 : 96);
  if (tmhip_stage_reserve(ctx, fbytes) || sums_reserve(ctx)) return 1;
  if (spio_launch<true>(ctx, even, odd, prec)) return 1;
  unsigned h[2];
  TMHIP_CHECK(hipMemcpyAsync(file_bytes, ctx->stage, fbytes, hipMemcpyDeviceToHost, ctx->stream));
  if (sums_fetch(ctx, h)) return 1;
  if (sums) { sums[0] = h[0]; sums[1] = h[1]; }
  return 0;
}

/* io/spinor_read_binary.c + io/dml.c:49-60 */
int tmhip_spinor_unpack(tmhip_ctx *ctx, tmhip_field *even, tmhip_field *odd, const void *file_bytes, int prec, unsigned *sums) {
  if (!file_bytes || (prec != 32 && prec != 64)) TMHIP_FAIL("tmhip_spinor_unpack: null data or precision %d (32 or 64)", prec);
  if (!spio_field_ok(ctx, even) || !spio_field_ok(ctx, odd) || even == odd) TMHIP_FAIL("tmhip_spinor_unpack: needs two distinct fp64 one-parity fields (a FULL field is passed as its two views)");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const size_t fbytes = (size_t)ctx->V * (prec == 64 ? 192 : 96);
  if (tmhip_stage_reserve(ctx, fbytes) || sums_reserve(ctx)) return 1;
  TMHIP_CHECK(hipMemcpyAsync(ctx->stage, file_bytes, fbytes, hipMemcpyHostToDevice, ctx->stream));
  if (spio_launch<false>(ctx, even, odd, prec)) return 1;
  unsigned h[2];
  if (sums_fetch(ctx, h)) return 1;
  if (sums) { sums[0] = h[0]; sums[1] = h[1]; }
  return 0;
}

/* `reps` launches of the pack (pack != 0) or unpack kernel alone between two HIP events, on the record a first pack leaves in the
 * staging buffer: no host copy, no checksum fetch (tools/spinor_io_speed.py).  An unpack rewrites the fields with their own values. */
int tmhip_bench_spinor_io(tmhip_ctx *ctx, tmhip_field *even, tmhip_field *odd, int prec, int pack, int reps, double *ms_total) {
  if (!ms_total || reps < 1 || (prec != 32 && prec != 64)) TMHIP_FAIL("tmhip_bench_spinor_io: reps >= 1, precision 32 or 64");
  if (!spio_field_ok(ctx, even) || !spio_field_ok(ctx, odd) || even == odd) TMHIP_FAIL("tmhip_bench_spinor_io: needs two distinct fp64 one-parity fields");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (tmhip_stage_reserve(ctx, (size_t)ctx->V * (prec == 64 ? 192 : 96)) || sums_reserve(ctx)) return 1;
  if (spio_launch<true>(ctx, even, odd, prec)) return 1;
  if (tmhip_event_record(ctx, 14)) return 1;
  for (int k = 0; k < reps; k++)
    if (pack ? spio_launch<true>(ctx, even, odd, prec) : spio_launch<false>(ctx, even, odd, prec)) return 1;
  if (tmhip_event_record(ctx, 15)) return 1;
  return tmhip_event_elapsed_ms(ctx, 14, 15, ms_total);
}

/* io/spinor_read.c:27-150 */
int tmhip_read_spinor(tmhip_ctx *ctx, tmhip_field *even, tmhip_field *odd, const char *filename, int position_, int io_checks, tmhip_spinor_info *info) {
  if (ctx->g.nproc_t > 1) TMHIP_FAIL("tmhip_read_spinor: file-level spinor I/O runs on unsplit lattices only (a T-split rank unpacks its part with tmhip_spinor_unpack)");
  if (!filename || !spio_field_ok(ctx, even) || !spio_field_ok(ctx, odd) || even == odd) TMHIP_FAIL("tmhip_read_spinor: needs a file name and two distinct fp64 one-parity fields");
  if (info) memset(info, 0, sizeof(*info));
  FILE *fp = fopen(filename, "rb");
  if (!fp) TMHIP_FAIL("read_spinor: cannot open %s", filename);
  std::vector<LimeRecord> recs;
  // a malformed header ends the walk as the `break` of spinor_read.c:63-66 does; the records in front of it are still looked at
  if (lime_scan(fp, recs)) fprintf(stderr, "ReaderNextRecord returned status %d.\n", -1);
  int prop_type = parse_propagator_type(fp, recs), position = position_;
  switch (prop_type) {
    case 1: position = 2 * position_ + 1; break;   /* strictly speaking this depends on whether a source or a propagator is read */
    case 2: case 3: fclose(fp); return -2;
    case 11: case 12: case 13: fclose(fp); return -3;
    case -1: case 4: prop_type = 0;
  }
  size_t at = recs.size();
  for (size_t k = 0, getpos = 0; k < recs.size(); k++)
    if (recs[k].type == "scidac-binary-data" && (int)getpos++ == position) { at = k; break; }
  if (at == recs.size()) {
    fprintf(stderr, "Unable to find requested LIME record scidac-binary-data in file %s.\nEnd of file reached before record was found.\n", filename);
    fclose(fp); return -5;
  }
  const unsigned long long bytes = recs[at].bytes, full = (unsigned long long)ctx->V * 192;
  int prec = 0;
  if (bytes == full) prec = 64;
  else if (bytes == full / 2) prec = 32;
  else {
    fprintf(stderr, "Length of scidac-binary-data record in %s does not match input parameters.\n", filename);
    fprintf(stderr, "Found %llu bytes.\n", bytes);
    fclose(fp); return -6;
  }
  if (info) { info->prec = prec; info->prop_type = prop_type; info->position = position; }   // (known from here on, whatever follows: the reference prints the precision now)
  // the checksum record directly behind the data, looked for until more binary data is found (spinor_read.c:114-132).  It is looked
  // for BEFORE the data go to the device, so that a file refused with -1 leaves the fields as they were
  unsigned stored[2] = {0, 0};
  int have_stored = 0;
  if (io_checks) {
    for (size_t k = at + 1; k < recs.size(); k++) {
      if (recs[k].type == "scidac-checksum") {
        std::string msg, a, b;
        if (!lime_read_string(fp, recs[k], msg))     // io/utils_parse_checksum_xml.c
          have_stored = xml_value(msg, "suma", a) && xml_value(msg, "sumb", b) && sscanf(a.c_str(), "%x", &stored[0]) == 1 && sscanf(b.c_str(), "%x", &stored[1]) == 1;
        break;
      }
      if (recs[k].type == "scidac-binary-data" || recs[k].type == "ildg-binary-data") break;
    }
    if (!have_stored) {
      fprintf(stderr, "LIME record with name: \"scidac-checksum\", in gauge file %s either missing or malformed.\n", filename);
      fprintf(stderr, "Unable to verify integrity of gauge field data.\n");
      fclose(fp); return -1;
    }
  }
  void *buf = nullptr;
  if (hipHostMalloc(&buf, bytes, hipHostMallocDefault) != hipSuccess) { fclose(fp); TMHIP_FAIL("read_spinor: no page-locked buffer of %llu bytes", bytes); }
  unsigned calc[2] = {0, 0};
  const bool got = !fseek(fp, recs[at].data_pos, SEEK_SET) && fread(buf, 1, bytes, fp) == bytes;
  fclose(fp);
  const int rstat = got ? tmhip_spinor_unpack(ctx, even, odd, buf, prec, calc) : 1;
  (void)hipHostFree(buf);
  if (rstat) { fprintf(stderr, "read_binary_spinor_data failed with return value %d", rstat); return -7; }
  if (info) {
    info->checksum_read = have_stored;
    info->suma = calc[0]; info->sumb = calc[1]; info->suma_stored = stored[0]; info->sumb_stored = stored[1];
  }
  return 0;
}

/* io/spinor_write.c:23-47 */
int tmhip_write_spinor(tmhip_ctx *ctx, const char *filename, int append, tmhip_field *const *even, tmhip_field *const *odd, int flavours, int prec, unsigned *sums) {
  if (ctx->g.nproc_t > 1) TMHIP_FAIL("tmhip_write_spinor: file-level spinor I/O runs on unsplit lattices only (a T-split rank packs its part with tmhip_spinor_pack)");
  if (!filename || !even || !odd || flavours < 1 || (prec != 32 && prec != 64)) TMHIP_FAIL("tmhip_write_spinor: needs a file name, %d >= 1 flavours and precision %d in (32, 64)", flavours, prec);
  for (int i = 0; i < flavours; i++)
    if (!spio_field_ok(ctx, even[i]) || !spio_field_ok(ctx, odd[i]) || even[i] == odd[i]) TMHIP_FAIL("tmhip_write_spinor: flavour %d needs two distinct fp64 one-parity fields", i);
  const unsigned long long bytes = (unsigned long long)ctx->V * 192 * prec / 64;
  void *buf = nullptr;
  TMHIP_CHECK(hipHostMalloc(&buf, bytes, hipHostMallocDefault));
  FILE *fp = fopen(filename, append ? "ab" : "wb");
  if (!fp) { (void)hipHostFree(buf); TMHIP_FAIL("write_spinor: cannot open %s for writing", filename); }
  int bad = 0;
  for (int i = 0; i < flavours && !bad; i++) {
    unsigned cs[2] = {0, 0};
    bad = tmhip_spinor_pack(ctx, even[i], odd[i], buf, prec, cs);
    bad = bad || lime_write_header(fp, 1, 0, "scidac-binary-data", bytes) || lime_write_data(fp, buf, bytes);
    bad = bad || lime_write_message(fp, 0, 1, "scidac-checksum", checksum_message(cs));          // io/utils_write_checksum.c:30-44
    if (sums) { sums[2 * i] = cs[0]; sums[2 * i + 1] = cs[1]; }
  }
  bad = fclose(fp) || bad;
  (void)hipHostFree(buf);
  if (bad) TMHIP_FAIL("write_spinor: error while writing %s", filename);
  return 0;
}

/* one record of a message: write_header + write_message + close_writer_record of io/utils.h, on a file of its own handle */
int tmhip_write_lime_message(const char *filename, int append, const char *type, const char *text, int mb, int me) {
  if (!filename || !type || !text) TMHIP_FAIL("tmhip_write_lime_message: null argument");
  if (strlen(type) > 127) TMHIP_FAIL("tmhip_write_lime_message: record type longer than 127 characters");
  FILE *fp = fopen(filename, append ? "ab" : "wb");
  if (!fp) TMHIP_FAIL("write_lime_message: cannot open %s for writing", filename);
  int bad = lime_write_message(fp, mb, me, type, std::string(text));
  bad = fclose(fp) || bad;
  if (bad) TMHIP_FAIL("write_lime_message: error while writing %s", filename);
  return 0;
}

/* start.c:707-741 (global_site 0) and start.c:743-830: global_site = ((t L + x) L + y) L + z over the GLOBAL extents */
int tmhip_source_point(tmhip_ctx *ctx, tmhip_field *even, tmhip_field *odd, int is, int ic, long long global_site) {
  if (!spio_field_ok(ctx, even) || !spio_field_ok(ctx, odd) || even == odd) TMHIP_FAIL("tmhip_source_point: needs two distinct fp64 one-parity fields");
  const long long Vg = (long long)ctx->V * ctx->g.nproc_t;
  if (is < 0 || is > 3 || ic < 0 || ic > 2) TMHIP_FAIL("tmhip_source_point: spin %d, colour %d outside [0, 3] x [0, 2]", is, ic);
  if (global_site < 0 || global_site >= Vg) TMHIP_FAIL("tmhip_source_point: SourceLocation %lld must be in [0, VOLUME - 1 = %lld]", global_site, Vg - 1);
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (tmhip_field_zero(ctx, even) || tmhip_field_zero(ctx, odd)) return 1;
  long long r = global_site;
  const int z = (int)(r % ctx->g.LZ); r /= ctx->g.LZ;
  const int y = (int)(r % ctx->g.LY); r /= ctx->g.LY;
  const int x = (int)(r % ctx->g.LX);
  const int tg = (int)(r / ctx->g.LX);
  if (tg / ctx->g.T != ctx->g.proc_t) return 0;   // another rank's site
  const int t = tg - ctx->g.proc_t * ctx->g.T;
  const size_t ix = (((size_t)t * ctx->g.LX + x) * ctx->g.LY + y) * ctx->g.LZ + z;
  tmhip_field *f = ((tg + x + y + z) & 1) ? odd : even;
  static const double one[2] = {1.0, 0.0};
  TMHIP_CHECK(hipMemcpyAsync(f->d + (size_t)(3 * is + ic) * f->ns + (ix >> 1), one, sizeof(one), hipMemcpyHostToDevice, ctx->stream));
  return 0;
}

}  // extern "C"
