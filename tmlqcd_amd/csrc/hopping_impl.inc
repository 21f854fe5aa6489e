// Stencil kernels and launchers, compiled three times by hopping.hip (not a stand-alone translation unit):
//   hop64  : ET = V2T = double2, one site per thread                       (Hopping_Matrix and its fused variants)
//   hop32  : ET = V2T = float2,  one site per thread                       (Hopping_Matrix_32, any even LZ)
//   hop32p : ET = float2, V2T = two complex floats, TWO sites per thread   (same, LZ % 4 == 0: every load except
//            the +-z neighbours is a 16-byte access, the widest a lane can issue)
// The including namespace provides: ET (element in memory), V2T (complex value(s) a thread computes with, with
// members x = re, y = im), HOP_SITES, ldc<NT>/stc<NT> (HOP_SITES consecutive sites), ldc2 (two separate sites),
// czero, cbcast(re, im), cdotd(w, r) = sum over the thread's sites of Re(conj(w) r) in double.
struct HopArgs {
  ET *out;
  const ET *in;
  const ET *p;
  const ET *gauge;  // already offset to the parity of the output sites
  TmhipGaugePack pack;   // GAUX 15 / 16 instances: the packed twin of the gauge copy, offset to the parity like `gauge`
  const ET *halo_up, *halo_dn;
  const ET *cw;      // clover epilogues: sw (6 blocks) or sw_inv (8 blocks) of the output sites, [blk][9][gs]
  const ET *dotv;   // EPI_TM_SUB_G5_DOT: field whose real scalar product with the output is accumulated
  double *partials;  // EPI_TM_SUB_G5_DOT: one partial per block
  ET *resid; const double *scal;   // EPI_TM_SUB_G5_RES: the residual field and the address of alpha in the device-side CG state
  int ns, gs;
  int T, LX, LY, LZh;
  int Vh, face, YZh;
  int i_begin, i_end;
  int par_off;  // (proc_t*T + ieo) & 1
  int nxcd_chunk;  // >0: XCD-aware block remap, blocks per XCD chunk
  int map_tc;      // >0: within an XCD chunk walk t fastest over map_tc time-slices (tile order)
  int map_bpt;     // blocks per time-slice (face / BS) for the tile order; exterior kernel: blocks per face
  int map_nb;      // real number of blocks of this launch (the grid is padded to a multiple of 8)
  int map_slab;    // >0: slab order -- XCD j owns blocks [j*map_slab, (j+1)*map_slab) of EVERY time-slice and marches through t
  // T-split rank.  wait_up / wait_dn: the words that tell that the faces this stencil gathers have arrived (>= wait_seq, wrap-safe
  // signed difference): the exterior kernel waits for both at its head, the boundary waves of a TSKIP 3 launch each for their own, before
  // they read the received half-spinors; nullptr: the faces are already there (Hopping_Matrix_nocom, events, the single-process
  // ring).  Carriers that exchange on the comm stream publish ONE word behind the exchange (both
  // pointers name it); with the direct carrier (tmhip_comm_init_ipc) each neighbour writes its own word into this rank's memory.
  // start_flag: the stencil kernel's first thread publishes start_seq = "the main stream has reached this stencil", which the pack
  // kernel on the comm stream waits for.
  const unsigned int *wait_up, *wait_dn; unsigned int wait_seq; unsigned int *err_flag; unsigned long long wait_ticks;
  int wait_sys;    // 1: the words (and the faces) are written by another agent (direct carrier): system-scope polls
  unsigned int *start_flag; unsigned int start_seq;
  int ext_sites;   // exterior kernel: 2 * face
  HopSelfAlpha self;   // hop_split4_kernel, EPI_TM_SUB_G5_RES: partials != nullptr => alpha = *normsq / sum(partials) computed by every block
  // t_rot: order of the time-slices of a whole-range TSKIP 1 / 3 launch: 1 = 1, .., T-1, 0 (boundary slices last), 2 = T-1, 0, 1, .. (first)
  int t_rot;
  // pp_dn / pp_up != nullptr: whoever completes the boundary slices of `out` (the exterior kernel; the boundary waves of a TSKIP 3
  // launch) also projects them to half-spinors for the neighbours -- the faces of the NEXT stencil of a chain -- into the send buffers
  // or, with the direct carrier, straight into the neighbours' receive buffers (pp_through: write-through stores, system scope)
  ET *pp_dn, *pp_up; int pp_through;
  // pipe != 0 (TSKIP 3 launches of the direct carrier): the boundary waves count in when their stores have left (*bcount reaches
  // bcount_target with the last of them), and that wave publishes *rflag_up = *rflag_dn = rflag_seq (words in the neighbours' memory:
  // "your faces of push rflag_seq are complete").
  int pipe;
  unsigned int *bcount; unsigned int bcount_target;
  unsigned int *rflag_up, *rflag_dn; unsigned int rflag_seq;
  // pub_after != nullptr: this stencil's own faces were pushed by a pack kernel on the comm stream (push pub_after_seq = rflag_seq - 1);
  // the wave that publishes rflag_seq first waits until that kernel has published ITS number (*pub_after >= pub_after_seq, a local
  // word): the words in the neighbours' memory never run backwards and never announce push n + 1 before the faces of push n are complete
  const unsigned int *pub_after; unsigned int pub_after_seq;
  double ka[4][2];
  double cre, cim;
};

#ifdef HOP_COMPLEX_COMPONENTWISE
// (two-sites-per-thread variant: V2T is a pair of two-lane vectors, .x = real parts, .y = imaginary parts of both sites)
__device__ __forceinline__ V2T cmul(V2T a, V2T b) { return V2T{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ V2T cmulc(V2T a, V2T b) {  // conj(a) * b
  return V2T{a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ V2T cfma(V2T a, V2T b, V2T c) {  // c + a*b
  return V2T{c.x + a.x * b.x - a.y * b.y, c.y + a.x * b.y + a.y * b.x};
}
__device__ __forceinline__ V2T cfmac(V2T a, V2T b, V2T c) {  // c + conj(a)*b
  return V2T{c.x + a.x * b.x + a.y * b.y, c.y + a.x * b.y - a.y * b.x};
}
#else
// Complex arithmetic on (re, im) pairs written as two-lane vector FMAs: (a.x, a.x) * b  then  (-a.y, a.y) * (b.y, b.x).  In fp32
// each line is ONE v_pk_fma_f32 (broadcast, swap and sign are operand modifiers), i.e. two instructions per complex
// multiply-add instead of the four to six the component-wise form compiles to; in fp64 it is the same four v_fma_f64 as before.
__device__ __forceinline__ V2T cfma(V2T a, V2T b, V2T c) {  // c + a*b
  const V2T t = __builtin_elementwise_fma(V2T{a.x, a.x}, b, c);
  return __builtin_elementwise_fma(V2T{-a.y, a.y}, V2T{b.y, b.x}, t);
}
__device__ __forceinline__ V2T cfmac(V2T a, V2T b, V2T c) {  // c + conj(a)*b
  const V2T t = __builtin_elementwise_fma(V2T{a.x, a.x}, b, c);
  return __builtin_elementwise_fma(V2T{a.y, -a.y}, V2T{b.y, b.x}, t);
}
__device__ __forceinline__ V2T cmul(V2T a, V2T b) {
  return __builtin_elementwise_fma(V2T{-a.y, a.y}, V2T{b.y, b.x}, V2T{a.x, a.x} * b);
}
__device__ __forceinline__ V2T cmulc(V2T a, V2T b) {  // conj(a) * b
  return __builtin_elementwise_fma(V2T{a.y, -a.y}, V2T{b.y, b.x}, V2T{a.x, a.x} * b);
}
#endif

// r = W s  (or W^dagger s) / r += W s for one 3x3 block `blk` of the site-local clover arrays [blk][9][gs]
__device__ __forceinline__ void su3_block_mul(V2T (&r)[3], const ET *__restrict__ w, size_t gs, int i, int blk, const V2T *s, bool dagger) {
  V2T u[9];
#pragma unroll
  for (int e = 0; e < 9; e++) u[e] = ldc<true>(w + ((size_t)blk * 9 + e) * gs + i);
#pragma unroll
  for (int row = 0; row < 3; row++)
    r[row] = dagger ? cfmac(u[6 + row], s[2], cfmac(u[3 + row], s[1], cmulc(u[row], s[0])))
                    : cfma(u[3 * row + 2], s[2], cfma(u[3 * row + 1], s[1], cmul(u[3 * row], s[0])));
}
__device__ __forceinline__ void su3_block_mac(V2T (&r)[3], const ET *__restrict__ w, size_t gs, int i, int blk, const V2T *s, bool dagger) {
  V2T t[3];
  su3_block_mul(t, w, gs, i, blk, s, dagger);
#pragma unroll
  for (int row = 0; row < 3; row++) r[row] += t[row];
}

// epilogues that end in a block reduction into a.partials[blockIdx.x]
#define HOP_EPI_REDUCES(E) ((E) == EPI_TM_SUB_G5_DOT || (E) == EPI_TM_SUB_G5_NRM || (E) == EPI_TM_SUB_G5_RES || (E) == EPI_CLOVER_G5_NRM || (E) == EPI_CLOVER_G5_RES || \
                            (E) == EPI_TM_SUB_G5_RSH || (E) == EPI_CLOVER_G5_RSH)
#define HOP_EPI_CLOVER_G5(E) ((E) == EPI_CLOVER_G5 || (E) == EPI_CLOVER_G5_NRM || (E) == EPI_CLOVER_G5_RES || (E) == EPI_CLOVER_G5_RSH)

// SM: where the neighbour spinor comes from in the LDS-staged variant (the wave has copied the input spinors of its own 64
// consecutive sites to its LDS region):
//   0 global loads (gather kernel; +-t, +-x)   1 every lane's neighbour is in the region (+-z: a wave holds whole z-rows)
//   2 per lane: region if the index falls inside it, else a global load (+-y: all rows of the wave but one edge row)
// One of the 8 hops.  D = 2*mu + (0: +mu, 1: -mu), mu = t,x,y,z.
// HALO: the projected half-spinor comes from an exchanged face buffer [6][face] instead of `in`.
template <int D, bool HALO, bool NT, int GAUX = -1, int SM = 0>
__device__ __forceinline__ void hop_dir(V2T (&acc)[12], const ET *__restrict__ in, int ns, int j, int j2,
                                        const ET *__restrict__ halo, int face,
                                        const ET *__restrict__ g, size_t gs, int i, V2T ka,
                                        const unsigned char *lds = nullptr, int jl = 0, const TmhipGaugePack &pk = TmhipGaugePack{}) {
  (void)j2; (void)pk;
  V2T pa[3], pb[3];
  constexpr bool PACKED = GAUX == 15 || GAUX == 16;   // 15: the 112-byte form, 16: the 104-byte form (compact rows)
  V2T ra[3], rb[3], rc[3]; v4u tl = {};   // PACKED: the two stored rows, the rebuilt one, the tail (its offsets and the rotation)
  v4u cl[3] = {}, ch[2] = {}; v2u ch2 = {};   // GAUX 16: the compact rows as loaded -- low words, packed high words
  (void)ra; (void)rb; (void)rc; (void)tl; (void)cl; (void)ch; (void)ch2;
  static_assert(!PACKED || !HALO, "the packed link read has no boundary form");
  if (HALO) {
    V2T h[6];
    ld6_fresh(h, halo, (size_t)face, j, 0);   // written by the exchange while this kernel may already have been running: never from L1
#pragma unroll
    for (int c = 0; c < 3; c++) { pa[c] = h[c]; pb[c] = h[3 + c]; }
  } else {
    V2T s[12];
    if constexpr (SM == 1) {
      stage_get6(s, lds, jl, 0); stage_get6(s + 6, lds, jl, 1);
    } else if constexpr (SM == 2) {
      const bool inb = (unsigned)jl < 64u;   // word by word: an LDS read under one half of the exec mask, a global load under the other
#pragma unroll
      for (int w = 0; w < HOP_SW; w++) {
        const SWT v = inb ? sw_stage(lds, jl, w) : sw_ld(in, (size_t)ns, j, w);
        sw_unpack(s, w, v);
      }
    } else {
      ld6<false>(s, in, (size_t)ns, j, 0); ld6<false>(s + 6, in, (size_t)ns, j, 1);
    }
    if constexpr (PACKED) {
      // Packed link read: the link's seven loads are requested right behind the spinor's, and the spinor is projected (48 -> 24
      // registers) while they are in flight; the rebuild and the selects below then have the room they need.  Left to itself
      // the compiler asks for the link first and rebuilds it with the whole neighbour spinor outstanding: 176 registers for EPI_TM_SUB_G5
      // when the instance is compiled with __launch_bounds__(256, 1) (tools/micro/regprobe.hip), scratch under the bound of three waves.
      __builtin_amdgcn_sched_barrier(0);
      // (scalar plane base + one 32-bit lane offset per load: a direction's planes of one parity span < 4 GiB, pack_setup)
      const unsigned int ugs = (unsigned int)gs, ui = (unsigned int)i;
      if constexpr (GAUX == 16) {
        // the compact rows: three planes of low words, two and a half of packed high words -- 88 bytes in six loads
        const char *plo = reinterpret_cast<const char *>(pk.lo + (size_t)D * 3 * gs), *phi = reinterpret_cast<const char *>(pk.hi + (size_t)D * 2 * gs);
  #pragma unroll
        for (int e = 0; e < 3; e++) {
          const v4u *q = reinterpret_cast<const v4u *>(plo + (size_t)(((unsigned int)e * ugs + ui) * 16u));
          cl[e] = NT ? __builtin_nontemporal_load(q) : *q;
        }
  #pragma unroll
        for (int e = 0; e < 2; e++) {
          const v4u *q = reinterpret_cast<const v4u *>(phi + (size_t)(((unsigned int)e * ugs + ui) * 16u));
          ch[e] = NT ? __builtin_nontemporal_load(q) : *q;
        }
        const v2u *q2 = reinterpret_cast<const v2u *>(reinterpret_cast<const char *>(pk.hi2 + (size_t)D * gs) + (size_t)(ui * 8u));
        ch2 = NT ? __builtin_nontemporal_load(q2) : *q2;
      } else {
        const char *prow = reinterpret_cast<const char *>(pk.rows + (size_t)D * 6 * gs);
  #pragma unroll
        for (int e = 0; e < 3; e++) {
          ra[e] = ldc<NT>(reinterpret_cast<const v2d *>(prow + (size_t)(((unsigned int)e * ugs + ui) * 16u)));
          rb[e] = ldc<NT>(reinterpret_cast<const v2d *>(prow + (size_t)(((unsigned int)(3 + e) * ugs + ui) * 16u)));
        }
      }
      const v4u *pt = reinterpret_cast<const v4u *>(reinterpret_cast<const char *>(pk.tail + (size_t)D * gs) + (size_t)(ui * 16u));
      tl = NT ? __builtin_nontemporal_load(pt) : *pt;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const V2T s0 = s[c], s1 = s[3 + c], s2 = s[6 + c], s3 = s[9 + c];
      if (D == 0) { pa[c] = s0 + s2; pb[c] = s1 + s3; }                                           // hopping.h:579,584
      if (D == 1) { pa[c] = s0 - s2; pb[c] = s1 - s3; }                                           // hopping.h:591,596
      if (D == 2) { pa[c] = V2T{s0.x - s3.y, s0.y + s3.x}; pb[c] = V2T{s1.x - s2.y, s1.y + s2.x}; }  // s0+i s3, s1+i s2
      if (D == 3) { pa[c] = V2T{s0.x + s3.y, s0.y - s3.x}; pb[c] = V2T{s1.x + s2.y, s1.y - s2.x}; }  // s0-i s3, s1-i s2
      if (D == 4) { pa[c] = s0 + s3; pb[c] = s1 - s2; }                                           // hopping.h:627,632
      if (D == 5) { pa[c] = s0 - s3; pb[c] = s1 + s2; }                                           // hopping.h:639,644
      if (D == 6) { pa[c] = V2T{s0.x - s2.y, s0.y + s2.x}; pb[c] = V2T{s1.x + s3.y, s1.y - s3.x}; }  // s0+i s2, s1-i s3
      if (D == 7) { pa[c] = V2T{s0.x + s2.y, s0.y - s2.x}; pb[c] = V2T{s1.x - s3.y, s1.y + s3.x}; }  // s0-i s2, s1+i s3
    }
    if constexpr (PACKED) {
      // (the projected half-spinor is pinned here: an empty statement the compiler cannot move the additions past)
#pragma unroll
      for (int c = 0; c < 3; c++) asm volatile("" : "+v"(pa[c]), "+v"(pb[c]));
      __builtin_amdgcn_sched_barrier(0);
    }
#ifndef HOP_GAUGE_PACKED
    if constexpr (GAUX == 16) {
      // the twelve kept reals from their compact form, directly behind the projection: the neighbour spinor is down to 24 registers
      // before these 24 are made of the 22 that were loaded (integer work, gauge_pack_codec.h)
      const uint32_t lo[12] = {cl[0].x, cl[0].y, cl[0].z, cl[0].w, cl[1].x, cl[1].y, cl[1].z, cl[1].w, cl[2].x, cl[2].y, cl[2].z, cl[2].w};
      const uint32_t hw[10] = {ch[0].x, ch[0].y, ch[0].z, ch[0].w, ch[1].x, ch[1].y, ch[1].z, ch[1].w, ch2.x, ch2.y};
      double v12[12];
      tmhip_gpack104_decode(lo, hw, v12);
#pragma unroll
      for (int e = 0; e < 3; e++) { ra[e] = V2T{v12[2 * e], v12[2 * e + 1]}; rb[e] = V2T{v12[6 + 2 * e], v12[7 + 2 * e]}; }
    }
#endif
  }
  const ET *gd = g + (size_t)D * 9 * gs + i;
  V2T u[9];
#ifdef HOP_GAUGE_PACKED
  {
    // packed fp32 links: element pairs (0,1) (2,3) (4,5) (6,7) as float4 planes, element 8 as a float2 plane
    const ET *gp = g + (size_t)D * 9 * gs;
    constexpr int NP = GAUX == 12 ? 3 : 4;
#pragma unroll
    for (int m = 0; m < NP; m++) {
      const vf4 v = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(gp + (size_t)m * 2 * gs) + i);
      u[2 * m] = V2T{v.x, v.y}; u[2 * m + 1] = V2T{v.z, v.w};
    }
    if constexpr (GAUX == 12) {
      const V2T a0 = cmul(u[1], u[5]) - cmul(u[2], u[4]), a1 = cmul(u[2], u[3]) - cmul(u[0], u[5]), a2 = cmul(u[0], u[4]) - cmul(u[1], u[3]);
      u[6] = V2T{a0.x, -a0.y}; u[7] = V2T{a1.x, -a1.y}; u[8] = V2T{a2.x, -a2.y};
    } else {
      u[8] = ldc<NT>(gp + (size_t)8 * gs + i);
    }
  }
#else
  if constexpr (PACKED) {
    // packed read ("gauge_pack"): two rows (GAUX 16: decoded from their compact form above) and the 16-byte tail -- 112 or 104 bytes; the third row is rebuilt and moved by the tail's
    // offsets (integer additions on the bit patterns) by the functions that verified it bit for bit when the copy was built
    // (gauge_pack_codec.h, gauge_pack_kernel in md_update.hip), and the rows go back to their places by selects on the tail's
    // rotation: every load is uniform across the wave, the result is the stored link
    tmhip_su3_row_rebuild(ra, rb, rc);
    const uint32_t t[4] = {tl.x, tl.y, tl.z, tl.w};
    const double w6[6] = {rc[0].x, rc[0].y, rc[1].x, rc[1].y, rc[2].x, rc[2].y};
    double c6[6];
    tmhip_gpack_decode(w6, t, c6);
#pragma unroll
    for (int e = 0; e < 3; e++) rc[e] = V2T{c6[2 * e], c6[2 * e + 1]};
    const int rot = tmhip_gpack_rot(t);
#pragma unroll
    for (int e = 0; e < 3; e++) {
      u[e] = rot == 0 ? ra[e] : (rot == 1 ? rc[e] : rb[e]);
      u[3 + e] = rot == 0 ? rb[e] : (rot == 1 ? ra[e] : rc[e]);
      u[6 + e] = rot == 0 ? rc[e] : (rot == 1 ? rb[e] : ra[e]);
    }
  } else if constexpr (GAUX == 12) {
    // opt-in 12-real storage read ("gauge_recon" = 12): rows 0 and 1 are loaded, row 2 = conj(row0 x row1) is rebuilt
    // in registers -- exact for SU(3) links up to rounding; the third of the link bytes is never fetched.
#pragma unroll
    for (int e = 0; e < 6; e++) u[e] = ldc<NT>(gd + (size_t)e * gs);
    const V2T a0 = cmul(u[1], u[5]) - cmul(u[2], u[4]), a1 = cmul(u[2], u[3]) - cmul(u[0], u[5]), a2 = cmul(u[0], u[4]) - cmul(u[1], u[3]);
    u[6] = V2T{a0.x, -a0.y}; u[7] = V2T{a1.x, -a1.y}; u[8] = V2T{a2.x, -a2.y};
  } else {
#pragma unroll
    for (int e = 0; e < 9; e++) u[e] = ldc<NT>(gd + (size_t)e * gs);
  }
#endif
  (void)gd;
  V2T ca[3], cb[3];
  if ((D & 1) == 0) {  // chi = U psi           (su3.h:308-311)
#pragma unroll
    for (int r = 0; r < 3; r++) {
      ca[r] = cfma(u[3 * r + 2], pa[2], cfma(u[3 * r + 1], pa[1], cmul(u[3 * r], pa[0])));
      cb[r] = cfma(u[3 * r + 2], pb[2], cfma(u[3 * r + 1], pb[1], cmul(u[3 * r], pb[0])));
    }
#pragma unroll
    for (int r = 0; r < 3; r++) { ca[r] = cmul(ka, ca[r]); cb[r] = cmul(ka, cb[r]); }
  } else {  // chi = U^dagger psi     (su3.h:313-316)
#pragma unroll
    for (int r = 0; r < 3; r++) {
      ca[r] = cfmac(u[6 + r], pa[2], cfmac(u[3 + r], pa[1], cmulc(u[r], pa[0])));
      cb[r] = cfmac(u[6 + r], pb[2], cfmac(u[3 + r], pb[1], cmulc(u[r], pb[0])));
    }
#pragma unroll
    for (int r = 0; r < 3; r++) { ca[r] = cmulc(ka, ca[r]); cb[r] = cmulc(ka, cb[r]); }
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const V2T a = ca[c], b = cb[c];
    acc[c] += a;      // s0 += a
    acc[3 + c] += b;  // s1 += b
    if (D == 0) { acc[6 + c] += a; acc[9 + c] += b; }
    if (D == 1) { acc[6 + c] -= a; acc[9 + c] -= b; }
    if (D == 2) { acc[9 + c] += V2T{a.y, -a.x}; acc[6 + c] += V2T{b.y, -b.x}; }   // s3 -= i a ; s2 -= i b
    if (D == 3) { acc[9 + c] += V2T{-a.y, a.x}; acc[6 + c] += V2T{-b.y, b.x}; }   // s3 += i a ; s2 += i b
    if (D == 4) { acc[9 + c] += a; acc[6 + c] -= b; }
    if (D == 5) { acc[9 + c] -= a; acc[6 + c] += b; }
    if (D == 6) { acc[6 + c] += V2T{a.y, -a.x}; acc[9 + c] += V2T{-b.y, b.x}; }   // s2 -= i a ; s3 += i b
    if (D == 7) { acc[6 + c] += V2T{-a.y, a.x}; acc[9 + c] += V2T{b.y, -b.x}; }   // s2 += i a ; s3 -= i b
  }
  // (packed link read: nothing of the next hop is requested before this one is added up -- as in the other instances, there by the
  // compiler's own choice -- so that the registers of the rebuild are free again)
  if constexpr (PACKED) __builtin_amdgcn_sched_barrier(0);
}

// TSKIP (T-split rank, DESIGN.md section 7): the launch still covers ALL sites of the rank, but the one hop that crosses the rank
// boundary -- -t on the t = 0 slice, +t on the t = T-1 slice -- is left out; hop_exterior_kernel adds it once the neighbours'
// half-spinor faces have arrived.  Every epilogue is linear in the accumulator, so the exterior kernel only has to push its one
// term through the same factors; the reducing epilogues leave the face sites' partial sums to it.  This kernel never waits for
// anything: whatever the exchange needs of the chip (RCCL's send / recv kernels want whole CUs) becomes free as its blocks retire.
// (Tried and dropped, profiles/r03_split_forms.md: the boundary hop inside this kernel, its waves waiting for the faces after their
// seven local hops -- one kernel per stencil, but the waiting waves hold the CUs RCCL's kernels need: every stencil ran into the
// deadline on 8 x 32^3 with a one-rank RCCL communicator; reserving CUs with a CU-masked stream cost 5-12 % of the stencil.)
// TSKIP 1: every wave lies inside one time-slice (LX LY LZ / 2 a multiple of 64), the choice is a scalar branch -- the form every
// production lattice takes; written as a per-lane branch the same kernel needs up to 256 VGPRs instead of 126-160.  TSKIP 2: per lane,
// any shape (the small lattices of the tests).
extern __shared__ __align__(16) unsigned char hop_dyn_smem[];   // occupancy cap (unused bytes) / staging area of the STG variant

// Consumer side of a cross-stream hand-off, per WAVE (cdna guide G16: relaxed polls of one word, then ONE agent-scope acquire; the
// acquiring wave's own later loads need neither a wait nor a barrier).  The producer is a whole kernel / copy on the other stream
// that completed before the flag was stored.  The spin is bounded by wait_ticks of the 100 MHz clock
// (tmhip_set_option "flag_timeout_ms"; 0 = unbounded): a neighbour that is merely late -- seconds are routine in an MPI run,
// xchange_field's MPI_Waitall just waits (xchange/xchange_field.c:98-250) -- is waited for; only a dead one trips the deadline,
// which sets *err (reported and cleared by tmhip_check_async_error) instead of hanging the GPU for good.
// SLEEP: pause between two polls in units of 64 clocks.  Hundreds of waves polling ONE word every quarter microsecond are ~2 G requests
// per second on one L2 channel: harmless while nothing else runs, but beside a running stencil kernel it held up every wave of that
// kernel -- 95 us instead of 43 (the round-3 "split_pipe" form, removed in round 4); waves that wait beside others look less often.
// SYS: the word is written by another agent -- a neighbour GPU's (or, on a shared GPU, another process's) kernel through an IPC mapping
// of this rank's memory (direct carrier): polled at system scope.  All comparisons are signed differences: sequence numbers may wrap.
template <bool SYS>
__device__ __forceinline__ unsigned int flag_load(const unsigned int *flag) {
  if (SYS) return __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool ACQUIRE = true, int SLEEP = 8, bool SYS = false>
__device__ __forceinline__ void wave_wait_flag(const unsigned int *flag, unsigned int seq, unsigned int *err, unsigned long long ticks) {
  if ((int)(flag_load<SYS>(flag) - seq) < 0) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while ((int)(flag_load<SYS>(flag) - seq) < 0) {
      __builtin_amdgcn_s_sleep(SLEEP);
      if (ticks && __builtin_amdgcn_s_memrealtime() - t0 > ticks) {
        __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
  }
  // ACQUIRE false: the caller reads what the flag guards with agent-scope loads only (ld6_fresh) and needs no invalidate of the CU's L1
  // (~4 us of a 10 us exterior kernel when all four waves of every block fence, profiles/r03_split_forms.md) -- only the order
  if (ACQUIRE) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A wave (lane 0 acts) whose stores of projected faces have left (the caller drained them: s_waitcnt vmcnt(0)) counts in; the wave
// that completes the count publishes into the neighbours' memory (direct carrier: their faces of push rflag_seq are complete).  Every counted wave had its write-through
// stores acknowledged before its add, the publishing wave's stores of the words come after its own add returned: whoever sees the
// word and then loads the faces at system scope sees all of them.
// The count is SHARDED -- wave number `ordinal` of the bcount_target waves of this launch adds to shard
// ordinal % 32 (each on a 128-byte line of its own), the wave that completes a shard adds to the top word, the wave that completes
// that one zeroes everything again (the next counting kernel is behind this one on the same stream) and publishes.  All boundary waves
// of a grid the chip holds at once finish within a microsecond of each other, and device-scope atomics on ONE word are served one
// at a time by the memory side (~70 ns each): 512 of them were 35 us at the end of an 8 x 32^3 stencil (profiles/r04_split_forms.md).
#define HOP_COUNT_SHARDS 32
__device__ __forceinline__ void faces_publish(const HopArgs &a) {
  if (a.rflag_up) {
    if (a.pub_after) wave_wait_flag<false>(a.pub_after, a.pub_after_seq, a.err_flag, a.wait_ticks);
    __hip_atomic_store(a.rflag_up, a.rflag_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(a.rflag_dn, a.rflag_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
__device__ __forceinline__ void faces_count_in(const HopArgs &a, unsigned int ordinal) {
  const unsigned int n = a.bcount_target, sh = ordinal % HOP_COUNT_SHARDS;
  const unsigned int expect = n / HOP_COUNT_SHARDS + (sh < n % HOP_COUNT_SHARDS ? 1u : 0u);
  if (__hip_atomic_fetch_add(a.bcount + 32 * (1 + sh), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u != expect) return;
  const unsigned int shards = n < HOP_COUNT_SHARDS ? n : HOP_COUNT_SHARDS;
  if (__hip_atomic_fetch_add(a.bcount, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u != shards) return;
  for (unsigned int k = 0; k <= HOP_COUNT_SHARDS; k++) __hip_atomic_store(a.bcount + 32 * k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  faces_publish(a);
}

template <int EPI, int TSKIP, bool NTIO, int BS, int MINW, int GAUX = -1, int STG = 0>
__global__ __launch_bounds__(BS, MINW) void hop_kernel(const HopArgs a) {
  static_assert(STG == 0 || (STG == 64 && HOP_SITES == 1), "the LDS-staged variant: one site per thread, whole blocks");
  static_assert((GAUX != 15 && GAUX != 16) || (STG == 64 && TSKIP == 0), "the packed link read exists in the staged kernel of unsplit lattices only");
  // gauge links: used once per call -> non-temporal (0.19 -> 0.16 ms at 32^4).  GAUX = -2 (small unsplit lattices, 64-thread blocks, the
  // gauge copy under ~200 MB: launch_variant): NOT marked streaming, so the links stay in the 256 MiB Infinity Cache from one call to
  // the next: 12^4 10.5 -> 8.8, 16^4 15.3 -> 12.1, 20^4 25.3 -> 21.9 us per launch; beyond the cache it is a loss (24^4 53 -> 62,
  // 8 x 32^3 41 -> 50 us; profiles/r02_gauge_nt_small_ab.log, r02_loopback_direct_ab.log)
  constexpr bool NT = HOP_GAUGE_NT && GAUX != -2;
  int bid = blockIdx.x;
  int i = 0;
  // wave-uniform, kept in a scalar register: what the end of the kernel needs of threadIdx (partial-sum slot, count-in lane) must not
  // cost a vector register carried through the eight hops (tools/check_resources.py: that register was the one that spilled)
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (TSKIP && a.start_flag && blockIdx.x == 0 && threadIdx.x == 0)
    // This kernel running means everything enqueued before it on its stream has completed, which is exactly what the
    // comm stream waits for before it packs the faces of `in`: no separate one-thread flag kernel per stencil.
    __hip_atomic_store(a.start_flag, a.start_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  if (a.map_slab > 0) {
    // slab order (large lattices): blocks b, b+8, .. share an XCD; XCD j takes the j-th eighth of every time-slice
    // (a slab of x-planes) and walks t.  +-x/y/z neighbours stay in the XCD's L2; the +-t neighbours of slice t are
    // the slab's own lines of slices t-1 / t+1, and what falls out of L2 is caught by the Infinity Cache, which holds
    // the three active time-slices of all eight slabs.
    // map_slab = ceil(map_bpt / 8): when the slice does not split evenly the last slab is shorter and its spare
    // block slots exit at once.
    const int xcd = bid & 7, q = bid >> 3;
    const int tt = q / a.map_slab, rr = xcd * a.map_slab + (q - tt * a.map_slab);
    if (rr >= a.map_bpt) {
      if (HOP_EPI_REDUCES(EPI) && (threadIdx.x & 63) == 0) a.partials[blockIdx.x * (BS / 64) + wave_in_block] = 0.0;
      return;
    }
    bid = tt * a.map_bpt + rr;
  } else if (a.nxcd_chunk > 0) {
    // XCD-aware remap: blocks b, b+8, b+16.. share an XCD (and its L2); give each XCD a
    // contiguous chunk of the lattice so neighbouring tiles hit the same L2.
    const int xcd = bid & 7;
    int q = bid >> 3;
    bid = xcd * a.nxcd_chunk + q;
    if (bid >= a.map_nb) {
      if (HOP_EPI_REDUCES(EPI) && (threadIdx.x & 63) == 0) a.partials[blockIdx.x * (BS / 64) + wave_in_block] = 0.0;
      return;
    }
    if (a.map_tc > 0) {
      // tile order: time-slices are taken in groups of map_tc; inside a group the same spatial
      // tile at t, t+1, .. is dispatched back to back, so the +-t (and +-x) users of an input
      // line run close in time on the same XCD.
      const int per_group = a.map_tc * a.map_bpt;
      const int g = bid / per_group, rem = bid - g * per_group;
      const int sp = rem / a.map_tc, tl = rem - sp * a.map_tc;
      bid = (g * a.map_tc + tl) * a.map_bpt + sp;
    }
  }
  i = a.i_begin + bid * (BS * HOP_SITES) + threadIdx.x * HOP_SITES;
  if (i >= a.i_end) return;  // (the fused-reduction variant is only launched on lattices with V/2 % BS == 0: no partial blocks)
  if constexpr (TSKIP == 1 || TSKIP == 3) {
    if (a.t_rot == 1) { i += a.face; if (i >= a.Vh) i -= a.Vh; }        // time-slices in the order 1, .., T-1, 0: the boundary slices come last (whole range only)
    else if (a.t_rot == 2) { i -= a.face; if (i < 0) i += a.Vh; }       // ... T-1, 0, 1, .., T-2: the boundary slices come first
  }

  const int LZh = a.LZh;
  const int k = i % LZh;
  int r = i / LZh;
  const int y = r % a.LY;
  r /= a.LY;
  const int x = r % a.LX;
  const int t = r / a.LX;
  const int o = (t + x + y + a.par_off) & 1;  // z = 2k + o  (geometry_eo.c:807-811)
  const int XYZh = a.face, YZh = a.YZh;

  const int jtp = (t + 1 < a.T) ? i + XYZh : i - (a.T - 1) * XYZh;
  const int jtm = (t > 0) ? i - XYZh : i + (a.T - 1) * XYZh;
  const int jxp = (x + 1 < a.LX) ? i + YZh : i - (a.LX - 1) * YZh;
  const int jxm = (x > 0) ? i - YZh : i + (a.LX - 1) * YZh;
  const int jyp = (y + 1 < a.LY) ? i + LZh : i - (a.LY - 1) * LZh;
  const int jym = (y > 0) ? i - LZh : i + (a.LY - 1) * LZh;
  const int jzp = o ? ((k + 1 < LZh) ? i + 1 : i - (LZh - 1)) : i;
  const int jzm = o ? i : ((k > 0) ? i - 1 : i + (LZh - 1));
  // two-site variant: the thread owns sites (i, i+1) of one z-row (k even); +-z neighbours of the second site
  const int jzp2 = o ? ((k + 2 < LZh) ? i + 2 : i + 1 - (LZh - 1)) : i + 1;
  const int jzm2 = o ? i + 1 : i;

  V2T acc[12];
#pragma unroll
  for (int c = 0; c < 12; c++) acc[c] = czero();

  const V2T ka0 = cbcast(a.ka[0][0], a.ka[0][1]), ka1 = cbcast(a.ka[1][0], a.ka[1][1]);
  const V2T ka2 = cbcast(a.ka[2][0], a.ka[2][1]), ka3 = cbcast(a.ka[3][0], a.ka[3][1]);
  const ET *__restrict__ in = a.in;
  const ET *__restrict__ g = a.gauge;
  // T-split rank: the hop across the rank boundary belongs to hop_exterior_kernel (block-uniform whenever a time-slice is whole blocks)
  const int tu = (TSKIP == 1 || TSKIP == 3) ? __builtin_amdgcn_readfirstlane(t) : t;
  const bool do_tp = !(TSKIP && tu == a.T - 1), do_tm = !(TSKIP && tu == 0);

  if constexpr (STG > 0) {
    // LDS-staged variant.  The input spinors of the wave's own 64 consecutive sites (one load per component: the only time these
    // lines are requested by this wave) go to the wave's LDS region first thing; the +-z hops then read both neighbours from
    // there and the +-y hops all but one edge row, instead of asking L2 for the same lines a second and third time while the
    // first request is still in flight.  No block barrier: the LDS operations of one wave execute in order.  launch_one
    // guarantees whole blocks (no thread has left) and a lattice shape with 64 % (LZ/2) == 0 and LY*LZ/2 >= 64.
    const int lid = (int)(threadIdx.x & 63);
    unsigned char *st = hop_dyn_smem + (size_t)wave_in_block * HOP_STAGE_BYTES;
    const int i0 = i - lid;
    stage_put(st, lid, in, (size_t)a.ns, i);
    __builtin_amdgcn_wave_barrier();
    if (do_tp) hop_dir<0, false, NT, GAUX>(acc, in, a.ns, jtp, 0, nullptr, 0, g, a.gs, i, ka0, nullptr, 0, a.pack);
    if (do_tm) hop_dir<1, false, NT, GAUX>(acc, in, a.ns, jtm, 0, nullptr, 0, g, a.gs, i, ka0, nullptr, 0, a.pack);
    hop_dir<2, false, NT, GAUX>(acc, in, a.ns, jxp, 0, nullptr, 0, g, a.gs, i, ka1, nullptr, 0, a.pack);
    hop_dir<3, false, NT, GAUX>(acc, in, a.ns, jxm, 0, nullptr, 0, g, a.gs, i, ka1, nullptr, 0, a.pack);
    hop_dir<4, false, NT, GAUX, 2>(acc, in, a.ns, jyp, 0, nullptr, 0, g, a.gs, i, ka2, st, jyp - i0, a.pack);
    hop_dir<5, false, NT, GAUX, 2>(acc, in, a.ns, jym, 0, nullptr, 0, g, a.gs, i, ka2, st, jym - i0, a.pack);
    hop_dir<6, false, NT, GAUX, 1>(acc, in, a.ns, jzp, 0, nullptr, 0, g, a.gs, i, ka3, st, jzp - i0, a.pack);
    hop_dir<7, false, NT, GAUX, 1>(acc, in, a.ns, jzm, 0, nullptr, 0, g, a.gs, i, ka3, st, jzm - i0, a.pack);
  } else {
    if (do_tp) hop_dir<0, false, NT, GAUX>(acc, in, a.ns, jtp, 0, nullptr, 0, g, a.gs, i, ka0);
    if (do_tm) hop_dir<1, false, NT, GAUX>(acc, in, a.ns, jtm, 0, nullptr, 0, g, a.gs, i, ka0);
    hop_dir<2, false, NT, GAUX>(acc, in, a.ns, jxp, 0, nullptr, 0, g, a.gs, i, ka1);
    hop_dir<3, false, NT, GAUX>(acc, in, a.ns, jxm, 0, nullptr, 0, g, a.gs, i, ka1);
    hop_dir<4, false, NT, GAUX>(acc, in, a.ns, jyp, 0, nullptr, 0, g, a.gs, i, ka2);
    hop_dir<5, false, NT, GAUX>(acc, in, a.ns, jym, 0, nullptr, 0, g, a.gs, i, ka2);
    hop_dir<6, false, NT, GAUX>(acc, in, a.ns, jzp, jzp2, nullptr, 0, g, a.gs, i, ka3);
    hop_dir<7, false, NT, GAUX>(acc, in, a.ns, jzm, jzm2, nullptr, 0, g, a.gs, i, ka3);
  }
  if constexpr (TSKIP == 3) {
    // The hop across the cut, taken from the received half-spinors AFTER the seven local ones: a boundary wave whose faces are not
    // there yet (wait_up / wait_dn != nullptr: the one-kernel form of the direct carrier) has done all its other work before it
    // waits.  Nothing it waits for needs a compute unit of this GPU: the neighbour's waves store the faces and the word straight
    // into this rank's memory (launch_direct).  Wave-uniform (a wave never straddles a time-slice here).
    __builtin_amdgcn_sched_barrier(0);
    if (!do_tp) {
      if (a.wait_up) { if (a.wait_sys) wave_wait_flag<false, 8, true>(a.wait_up, a.wait_seq, a.err_flag, a.wait_ticks); else wave_wait_flag<false>(a.wait_up, a.wait_seq, a.err_flag, a.wait_ticks); }
      hop_dir<0, true, NT, GAUX>(acc, in, a.ns, i - tu * XYZh, 0, a.halo_up, a.face, g, a.gs, i, ka0);
    } else if (!do_tm) {
      if (a.wait_dn) { if (a.wait_sys) wave_wait_flag<false, 8, true>(a.wait_dn, a.wait_seq, a.err_flag, a.wait_ticks); else wave_wait_flag<false>(a.wait_dn, a.wait_seq, a.err_flag, a.wait_ticks); }
      hop_dir<1, true, NT, GAUX>(acc, in, a.ns, i - tu * XYZh, 0, a.halo_dn, a.face, g, a.gs, i, ka0);
    }
  }
  // reducing epilogues on a T-split rank: the face sites' terms are summed by the exterior kernel, after it has completed them
  const bool own_sum = (do_tp && do_tm) || TSKIP == 3;   // (TSKIP 3: every site is complete in this kernel)
  const bool bwave = TSKIP == 3 && a.pipe && !(do_tp && do_tm);   // a boundary-slice wave of a launch whose boundary waves count in (wave-uniform)
  (void)own_sum;

  ET *__restrict__ out = a.out;
  const V2T cf = cbcast(a.cre, a.cim);
  const size_t ns = (size_t)a.ns;
  V2T fin[TSKIP == 3 ? 12 : 1];   // TSKIP 3: what was stored to `out` (projected for the neighbours below)
  auto put = [&](ET *f, int b, const V2T *o) {
    if constexpr (TSKIP == 3) {
#pragma unroll
      for (int c = 0; c < 6; c++) fin[6 * b + c] = o[c];
    }
    st6<NTIO>(f, ns, i, b, o);   // ONE store path for every wave: a second, write-through one for boundary waves (round 3) cost the whole kernel 90 VGPRs (tools/check_resources.py)
  };
  if (EPI == EPI_STORE) {  // hopping.h:690-694
    put(out, 0, acc); put(out, 1, acc + 6);
  } else if (EPI == EPI_TM_TIMES) {  // hopping.h:674-678
    V2T o[12];
#pragma unroll
    for (int c = 0; c < 6; c++) o[c] = cmul(cf, acc[c]);
#pragma unroll
    for (int c = 6; c < 12; c++) o[c] = cmulc(cf, acc[c]);
    put(out, 0, o); put(out, 1, o + 6);
  } else if (EPI == EPI_CLOVER_INV) {
    // clover_inv (clovertm_operators.c:287-350) fused behind the stencil: per chirality b
    //   s_a' = W[0][b] s_a + W[1][b] s_b ,  s_b' = W[3][b] s_a + W[2][b] s_b     with W = sw_inv (8 blocks = [4][2])
#pragma unroll
    for (int b = 0; b < 2; b++) {
      V2T ra[3], rb[3], o[6];
      su3_block_mul(ra, a.cw, a.gs, i, 0 * 2 + b, acc + 6 * b, false);
      su3_block_mul(rb, a.cw, a.gs, i, 3 * 2 + b, acc + 6 * b, false);
      su3_block_mac(ra, a.cw, a.gs, i, 1 * 2 + b, acc + 6 * b + 3, false);
      su3_block_mac(rb, a.cw, a.gs, i, 2 * 2 + b, acc + 6 * b + 3, false);
#pragma unroll
      for (int c = 0; c < 3; c++) { o[c] = ra[c]; o[3 + c] = rb[c]; }
      put(out, b, o);
    }
  } else if (HOP_EPI_CLOVER_G5(EPI) || EPI == EPI_CLOVER) {
    // clover_gamma5 / clover (clovertm_operators.c:448-520, 535-600): l = [g5] ( (1 + T + i mu g5) p - H k ),
    // T = sw (6 blocks = [3][2]): psi1 = A s_a + B s_b, psi2 = B^dag s_a + C s_b
    // _NRM / _RES: the CG reductions of cg_enqueue_fused (cg.hip) on top, as for the twisted-mass epilogue below
    // _RSH (multi-shift CG, mms.hip): resid -= alpha (out + sigma0 dotv), alpha = scal[0], sigma0 = scal[1]
    constexpr bool CRES = EPI == EPI_CLOVER_G5_RES || EPI == EPI_CLOVER_G5_RSH;
    const ET *__restrict__ p = a.p;
    double d = 0.0;
    V2T malpha = cbcast(0.0, 0.0), csig = cbcast(0.0, 0.0);
    if (CRES) malpha = cbcast(-*a.scal, 0.0);
    if (EPI == EPI_CLOVER_G5_RSH) csig = cbcast(a.scal[1], 0.0);
#pragma unroll
    for (int b = 0; b < 2; b++) {
      V2T sab[6], r1[3], r2[3], o[6];
      ld6<NTIO>(sab, p, ns, i, b);
      const V2T *sa = sab, *sb = sab + 3;
      su3_block_mul(r1, a.cw, a.gs, i, 0 * 2 + b, sa, false);
      su3_block_mac(r1, a.cw, a.gs, i, 1 * 2 + b, sb, false);
      su3_block_mul(r2, a.cw, a.gs, i, 1 * 2 + b, sa, true);
      su3_block_mac(r2, a.cw, a.gs, i, 2 * 2 + b, sb, false);
      const V2T imu = cbcast(0.0, b == 0 ? a.cim : -a.cim);   // + i mu on the upper, - i mu on the lower components
      V2T rs[6], pw[6];
      if (CRES) ld6<NTIO>(rs, a.resid, ns, i, b);
      if (EPI == EPI_CLOVER_G5_RSH) ld6<NTIO>(pw, a.dotv, ns, i, b);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        r1[c] = cfma(imu, sa[c], r1[c]);
        r2[c] = cfma(imu, sb[c], r2[c]);
        const bool flip = HOP_EPI_CLOVER_G5(EPI) && b == 1;
        V2T v1 = flip ? acc[6 * b + c] - r1[c] : r1[c] - acc[6 * b + c];
        V2T v2 = flip ? acc[6 * b + 3 + c] - r2[c] : r2[c] - acc[6 * b + 3 + c];
        if (EPI == EPI_CLOVER_G5_RSH) { v1 = cfma(csig, pw[c], v1); v2 = cfma(csig, pw[3 + c], v2); }
        if (CRES) {
          const V2T n1 = cfma(malpha, v1, rs[c]);
          const V2T n2 = cfma(malpha, v2, rs[3 + c]);
          o[c] = n1; o[3 + c] = n2;
          d += cdotd(n1, n1) + cdotd(n2, n2);
        } else {
          o[c] = v1; o[3 + c] = v2;
          if (EPI == EPI_CLOVER_G5_NRM) d += cdotd(v1, v1) + cdotd(v2, v2);
        }
      }
      if (CRES) put(a.resid, b, o);
      else put(out, b, o);
    }
    if (HOP_EPI_REDUCES(EPI)) {
      if (!own_sum) d = 0.0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
      if (__lane_id() == 0) a.partials[blockIdx.x * (BS / 64) + wave_in_block] = d;
    }
  } else {
    // EPI_TM_SUB_G5[_DOT]: hopping.h:680-688  l = g5[(cf,cf*) p - H k];  EPI_TM_SUB: same without g5
    // _RSH (multi-shift CG, mms.hip): resid -= alpha (out + sigma0 dotv), alpha = scal[0], sigma0 = scal[1]
    constexpr bool TRES = EPI == EPI_TM_SUB_G5_RES || EPI == EPI_TM_SUB_G5_RSH;
    const ET *__restrict__ p = a.p;
    double d = 0.0;
    V2T malpha = cbcast(0.0, 0.0), msig = cbcast(0.0, 0.0);
    if (TRES) malpha = cbcast(-*a.scal, 0.0);
    if (EPI == EPI_TM_SUB_G5_RSH) msig = cbcast(-a.scal[0] * a.scal[1], 0.0);
#pragma unroll
    for (int b = 0; b < 2; b++) {
      // _RSH: one chirality at a time (its three input fields are 18 complex values; both at once do not fit three waves per SIMD)
      if (EPI == EPI_TM_SUB_G5_RSH) __builtin_amdgcn_sched_barrier(0);
      V2T pv[6], o[6], ex[6];
      ld6<NTIO>(pv, p, ns, i, b);
      if (TRES) ld6<NTIO>(ex, a.resid, ns, i, b);
      if (EPI == EPI_TM_SUB_G5_RSH) {
        // the sigma0 term first (resid - alpha sigma0 dotv): dotv is dead before the stencil's own terms are combined
        V2T pw[6];
        ld6<NTIO>(pw, a.dotv, ns, i, b);
#pragma unroll
        for (int cc = 0; cc < 6; cc++) ex[cc] = cfma(msig, pw[cc], ex[cc]);
      }
      if (EPI == EPI_TM_SUB_G5_DOT) ld6<NTIO>(ex, a.dotv, ns, i, b);
#pragma unroll
      for (int cc = 0; cc < 6; cc++) {
        const int c = 6 * b + cc;
        V2T r;
        if (b == 0) r = cmul(cf, pv[cc]) - acc[c];
        else { const V2T zp = cmulc(cf, pv[cc]); r = (EPI == EPI_TM_SUB) ? zp - acc[c] : acc[c] - zp; }
        if (TRES) {
          // cg_her.c:95-101 fused behind the last stencil of Qtm_pm_psi: r <- r - alpha (A p), err = |r|^2; A p is never stored
          const V2T rn = cfma(malpha, r, ex[cc]);
          o[cc] = rn;
          d += cdotd(rn, rn);
        } else {
          o[cc] = r;
          if (EPI == EPI_TM_SUB_G5_NRM) d += cdotd(r, r);   // |Q_- p|^2 = <p, Q_+ Q_- p>: the pro of cg_her.c:93 without re-reading anything
          if (EPI == EPI_TM_SUB_G5_DOT) d += cdotd(ex[cc], r);   // fused scalar_prod_r(dotv, out), cg_her.c:93
        }
      }
      if (TRES) put(a.resid, b, o);
      else put(out, b, o);
      if (EPI == EPI_TM_SUB_G5_RSH) __builtin_amdgcn_sched_barrier(0);
    }
    if (HOP_EPI_REDUCES(EPI)) {
      // one partial per WAVE (no LDS, no block barrier: a barrier here keeps the CU slots of the fast waves occupied
      // until the slowest wave of the block has finished its epilogue); the fixed-order sum kernel adds them up
      if (!own_sum) d = 0.0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
      if (__lane_id() == 0) a.partials[blockIdx.x * (BS / 64) + wave_in_block] = d;
    }
  }
  if constexpr (TSKIP == 3) {
    if (bwave) {
      {
        if (a.pp_dn) {   // the faces of the NEXT stencil: pack_faces_kernel's arithmetic on what this wave has just stored
          V2T h[6];
#pragma unroll
          for (int c = 0; c < 3; c++) {
            h[c] = do_tp ? fin[c] + fin[6 + c] : fin[c] - fin[6 + c];          // do_tp: the t = 0 slice -> send_dn; else t = T-1 -> send_up
            h[3 + c] = do_tp ? fin[3 + c] + fin[9 + c] : fin[3 + c] - fin[9 + c];
          }
          st6_through(do_tp ? a.pp_dn : a.pp_up, (size_t)a.face, i - tu * XYZh, 0, h);
        }
      }
      if (a.bcount) {
        // this wave's stores have left before it counts in: the projections are write-through stores and only need draining
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (__lane_id() == 0) faces_count_in(a, (unsigned int)((do_tp ? 0 : a.face / 64) + (i - tu * XYZh) / 64));   // (the lane number is recomputed from the exec mask here: carried from the top of the kernel it was a spilled register)
      }
    }
  }
}

// The eight hops of a site SPLIT OVER THE FOUR WAVES of a block (wave w does +-mu for mu = w), for SMALL unsplit lattices: a
// launch of one thread per site is a few hundred waves walking eight dependent hops each -- latency, not bandwidth (16^4: 13.8 us
// per launch for 50 MB).  Here a block of 256 threads owns 64 sites: each wave accumulates two hops, the four partial spinors
// meet in LDS (48 KB in fp64), and wave w finishes components 3w .. 3w+2 (epilogue and, for the CG epilogues, its own partial
// sum).  Four times the waves, a quarter of the chain (DESIGN.md section 4, "hopsplit").  Epilogues that act component by
// component only.  Links are served by the Infinity Cache at these sizes: no streaming hint (see hop_kernel).
#ifndef HOP_SPINOR_PACKED
template <int EPI, bool NTIO>
__global__ __launch_bounds__(256) void hop_split4_kernel(const HopArgs a) {
  constexpr bool NT = false;
  __shared__ V2T part[4][12][64];
  __shared__ double wsum[4];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double self_acc = 0.0;
  if (EPI == EPI_TM_SUB_G5_RES && a.self.partials) {
    // requested first, needed last: the previous stencil's per-wave partial sums (see HopSelfAlpha); strided per thread here, the rest
    // of tmhip_block_sum256's order (wave butterfly, four wave sums) around the barrier this kernel has anyway
    for (int j = threadIdx.x; j < a.self.n; j += 256) self_acc += a.self.partials[j];
  }
  const int jl = (int)blockIdx.x * 64 + lane;
  const bool active = a.i_begin + jl < a.i_end;
  const int i = active ? a.i_begin + jl : a.i_begin;
  const int LZh = a.LZh;
  const int k = i % LZh;
  int r = i / LZh;
  const int y = r % a.LY;
  r /= a.LY;
  const int x = r % a.LX;
  const int t = r / a.LX;
  const int o = (t + x + y + a.par_off) & 1;
  const int XYZh = a.face, YZh = a.YZh;
  V2T acc[12];
#pragma unroll
  for (int c = 0; c < 12; c++) acc[c] = czero();
  const ET *__restrict__ in = a.in;
  const ET *__restrict__ g = a.gauge;
  // the epilogue's own operands (p, the residual) of this wave's three components are requested up front: behind the barrier they would be
  // one more dependent trip to memory in a kernel that is latency from end to end
  constexpr bool HAS_P = !(EPI == EPI_STORE || EPI == EPI_TM_TIMES);
  V2T pv3[3], rs3[3];
  if (HAS_P && active) {
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
      pv3[cc] = ldc<NTIO>(a.p + (size_t)(3 * w + cc) * a.ns + i);
      if (EPI == EPI_TM_SUB_G5_RES) rs3[cc] = ldc<NTIO>(a.resid + (size_t)(3 * w + cc) * a.ns + i);
    }
  }
  if (active) {
    if (w == 0) {
      const V2T ka0 = cbcast(a.ka[0][0], a.ka[0][1]);
      const int jtp = (t + 1 < a.T) ? i + XYZh : i - (a.T - 1) * XYZh, jtm = (t > 0) ? i - XYZh : i + (a.T - 1) * XYZh;
      hop_dir<0, false, NT>(acc, in, a.ns, jtp, 0, nullptr, 0, g, a.gs, i, ka0);
      hop_dir<1, false, NT>(acc, in, a.ns, jtm, 0, nullptr, 0, g, a.gs, i, ka0);
    } else if (w == 1) {
      const V2T ka1 = cbcast(a.ka[1][0], a.ka[1][1]);
      const int jxp = (x + 1 < a.LX) ? i + YZh : i - (a.LX - 1) * YZh, jxm = (x > 0) ? i - YZh : i + (a.LX - 1) * YZh;
      hop_dir<2, false, NT>(acc, in, a.ns, jxp, 0, nullptr, 0, g, a.gs, i, ka1);
      hop_dir<3, false, NT>(acc, in, a.ns, jxm, 0, nullptr, 0, g, a.gs, i, ka1);
    } else if (w == 2) {
      const V2T ka2 = cbcast(a.ka[2][0], a.ka[2][1]);
      const int jyp = (y + 1 < a.LY) ? i + LZh : i - (a.LY - 1) * LZh, jym = (y > 0) ? i - LZh : i + (a.LY - 1) * LZh;
      hop_dir<4, false, NT>(acc, in, a.ns, jyp, 0, nullptr, 0, g, a.gs, i, ka2);
      hop_dir<5, false, NT>(acc, in, a.ns, jym, 0, nullptr, 0, g, a.gs, i, ka2);
    } else {
      const V2T ka3 = cbcast(a.ka[3][0], a.ka[3][1]);
      const int jzp = o ? ((k + 1 < LZh) ? i + 1 : i - (LZh - 1)) : i, jzm = o ? i : ((k > 0) ? i - 1 : i + (LZh - 1));
      hop_dir<6, false, NT>(acc, in, a.ns, jzp, 0, nullptr, 0, g, a.gs, i, ka3);
      hop_dir<7, false, NT>(acc, in, a.ns, jzm, 0, nullptr, 0, g, a.gs, i, ka3);
    }
  }
#pragma unroll
  for (int c = 0; c < 12; c++) part[w][c][lane] = acc[c];
  if (EPI == EPI_TM_SUB_G5_RES && a.self.partials) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) self_acc += __shfl_xor(self_acc, off, 64);
    if (lane == 0) wsum[w] = self_acc;
  }
  __syncthreads();
  double alpha_self = 0.0;
  if (EPI == EPI_TM_SUB_G5_RES && a.self.partials) {
    const double pro = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    alpha_self = *a.self.normsq / pro;                                  // cg_her.c:93-94
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.self.out2[0] = pro; a.self.out2[1] = alpha_self; }
  }
  double d = 0.0;
  if (active) {
    ET *__restrict__ out = a.out;
    const V2T cf = cbcast(a.cre, a.cim);
    V2T malpha = cbcast(0.0, 0.0);
    if (EPI == EPI_TM_SUB_G5_RES) malpha = cbcast(a.self.partials ? -alpha_self : -*a.scal, 0.0);
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
      const int c = 3 * w + cc;                                  // wave-uniform: components 3w .. 3w+2
      const V2T h = (part[0][c][lane] + part[1][c][lane]) + (part[2][c][lane] + part[3][c][lane]);
      if (EPI == EPI_STORE) {
        stc<NTIO>(out + (size_t)c * a.ns + i, h);
      } else if (EPI == EPI_TM_TIMES) {
        stc<NTIO>(out + (size_t)c * a.ns + i, c < 6 ? cmul(cf, h) : cmulc(cf, h));
      } else {                                                   // TM_SUB family, as in hop_kernel
        const V2T pv = pv3[cc];
        V2T rr;
        if (c < 6) rr = cmul(cf, pv) - h;
        else { const V2T zp = cmulc(cf, pv); rr = (EPI == EPI_TM_SUB) ? zp - h : h - zp; }
        if (EPI == EPI_TM_SUB_G5_RES) {
          const V2T rn = cfma(malpha, rr, rs3[cc]);
          stc<NTIO>(a.resid + (size_t)c * a.ns + i, rn);
          d += cdotd(rn, rn);
        } else {
          stc<NTIO>(out + (size_t)c * a.ns + i, rr);
          if (EPI == EPI_TM_SUB_G5_NRM) d += cdotd(rr, rr);
        }
      }
    }
  }
  if (HOP_EPI_REDUCES(EPI)) {
    // ONE partial per block (the four wave sums meet in LDS): a quarter of the values whoever adds them up has to read -- on these
    // small lattices that is every block of the next kernels (HopSelfAlpha, cg_xp_self_kernel)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
    __syncthreads();                                   // (wsum may still be read by the coefficient above)
    if (lane == 0) wsum[w] = d;
    __syncthreads();
    if (threadIdx.x == 0) a.partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
  }
}
#endif  // !HOP_SPINOR_PACKED

// Project the two t-faces of the input field to half-spinors for the neighbours
// (what xchange_halffield ships, xchange/xchange_halffield.c:199-255; projections of
// operator/halfspinor_hopping.h:1279-1293):
//   dst_dn[j] = (s0+s2, s1+s3)(t=0)      -> down neighbour, consumed by its +t hop at t=T-1
//   dst_up[j] = (s0-s2, s1-s3)(t=T-1)    -> up neighbour,   consumed by its -t hop at t=0
// start_flag != null: every block first waits until *start_flag >= start_seq ("`in` is final": the stencil kernel on the main stream
// has started), one launch less in the comm-stream chain than a one-thread wait kernel in front.
// Direct carrier (launch_direct): dst_* are the NEIGHBOURS' receive buffers (IPC mappings; write-through stores).  The block then
// also waits until both neighbours' pushes number fc_seq have arrived here -- which proves that they are done with the buffer
// this push overwrites (flow control, see launch_direct) --, and the last block to count in publishes rflag_seq into the neighbours'
// arrival words.
struct PackArgs {
  const ET *in; int ns, Vh, face;
  ET *dst_dn, *dst_up; int through;
  const unsigned int *start_flag; unsigned int start_seq;
  const unsigned int *fc_up, *fc_dn; unsigned int fc_seq;
  unsigned int *err; unsigned long long ticks;
  unsigned int *count; unsigned int count_target; unsigned int *rflag_up, *rflag_dn; unsigned int rflag_seq;
  unsigned int *done_flag;   // local word that receives rflag_seq behind the two remote ones (HopArgs::pub_after)
};
__global__ __launch_bounds__(256) void pack_faces_kernel(const PackArgs a) {
  if (a.start_flag || a.fc_up) {
    if (threadIdx.x < 64) {
      if (a.start_flag) wave_wait_flag(a.start_flag, a.start_seq, a.err, a.ticks);
      if (a.fc_up) { wave_wait_flag<false, 8, true>(a.fc_up, a.fc_seq, a.err, a.ticks); wave_wait_flag<false, 8, true>(a.fc_dn, a.fc_seq, a.err, a.ticks); }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the acquire's invalidate has completed before the other waves pass the barrier)
    __syncthreads();
  }
  const int which = blockIdx.y;  // 0: t=0 face -> dst_dn, 1: t=T-1 face -> dst_up
  ET *dst = which ? a.dst_up : a.dst_dn;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < a.face; j += gridDim.x * 256) {
    const int i = which ? a.Vh - a.face + j : j;
    V2T s[12], h[6];
    ld6<false>(s, a.in, (size_t)a.ns, i, 0); ld6<false>(s + 6, a.in, (size_t)a.ns, i, 1);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      h[c] = which ? s[c] - s[6 + c] : s[c] + s[6 + c];
      h[3 + c] = which ? s[3 + c] - s[9 + c] : s[3 + c] + s[9 + c];
    }
    if (a.through) st6_through(dst, (size_t)a.face, j, 0, h);
    else st6<false>(dst, (size_t)a.face, j, 0, h);
  }
  if (a.count) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave's stores have left ...
    __syncthreads();                                    // ... before the block counts in
    if (threadIdx.x == 0) {
      const unsigned int old = __hip_atomic_fetch_add(a.count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old + 1u == a.count_target) {
        __hip_atomic_store(a.rflag_up, a.rflag_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(a.rflag_dn, a.rflag_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(a.done_flag, a.rflag_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// The exterior kernel of a T-split rank: the ONE hop a TSKIP launch of hop_kernel left out at the sites of the two boundary
// time-slices, added once the neighbours' half-spinor faces have arrived (the reference's own split into project / exchange /
// reconstruct, operator/halfspinor_body.c:239-311).  Sites j < face: the t = 0 slice (-t hop, half-spinors from halo_dn), the
// others the t = T-1 slice (+t hop, halo_up).  Per site: the half-spinor (96 B), one link (144 B) and a read-modify-write of the
// output (384 B) instead of a second full stencil.  With chi the hop's term of the accumulator, the epilogues of hop_kernel continue as
//   STORE            out += chi
//   TM_TIMES         out += (cf, cf*) chi
//   TM_SUB[_G5]      out -= chi              (_G5: += on the lower two spin components)
//   CLOVER_INV       out += sw_inv chi       (6x6 blocks per chirality)
//   CLOVER[_G5]      as TM_SUB[_G5]
//   .._NRM           and the partial of |out|^2 over the face sites, now that they are complete
//   .._RES           resid -= alpha (-+ chi), partial of |resid|^2     (out itself is not stored by this epilogue)
// One partial per wave at a.partials[4 blockIdx.x + wave]; the launcher hands hop_kernel the range behind them.
// At most HOP_EXT_MAX_BLOCKS blocks (grid-stride loop): this is the kernel that WAITS for the exchange (wait_up / wait_dn, head of
// every wave), and blocks that wait must leave most of the chip to what they wait for.
#define HOP_EXT_MAX_BLOCKS 128
template <int EPI, bool NTIO>
__global__ __launch_bounds__(256) void hop_exterior_kernel(const HopArgs a) {
  constexpr bool NT = HOP_GAUGE_NT;
  constexpr bool RES = EPI == EPI_TM_SUB_G5_RES || EPI == EPI_CLOVER_G5_RES;
  constexpr bool NRM = EPI == EPI_TM_SUB_G5_NRM || EPI == EPI_CLOVER_G5_NRM;
  constexpr bool G5 = EPI == EPI_TM_SUB_G5 || EPI == EPI_CLOVER_G5 || RES || NRM;
  const size_t ns = (size_t)a.ns;
  ET *__restrict__ dst = RES ? a.resid : a.out;
  double d = 0.0;
  bool waited = a.wait_up == nullptr;
  auto wait_faces = [&]() {   // both faces: a wave's sites may lie in either slice
    if (a.wait_sys) { wave_wait_flag<false, 8, true>(a.wait_up, a.wait_seq, a.err_flag, a.wait_ticks); wave_wait_flag<false, 8, true>(a.wait_dn, a.wait_seq, a.err_flag, a.wait_ticks); }
    else { wave_wait_flag<false>(a.wait_up, a.wait_seq, a.err_flag, a.wait_ticks); if (a.wait_dn != a.wait_up) wave_wait_flag<false>(a.wait_dn, a.wait_seq, a.err_flag, a.wait_ticks); }
  };
  for (int j = (int)blockIdx.x * 256 + (int)threadIdx.x; j < a.ext_sites; j += (int)gridDim.x * 256) {
    const int second = j >= a.face;
    const int jf = second ? j - a.face : j;
    const int i = second ? a.Vh - a.face + jf : jf;
    // what does not depend on the exchange is requested first: the output of the stencil kernel (complete: same stream) ...
    V2T o[12];
    ld6<false>(o, dst, ns, i, 0); ld6<false>(o + 6, dst, ns, i, 1);
    if (!waited) {
      // ... then every wave waits for the faces itself (no block barrier; a wave's own loads behind its acquire are safe)
      wait_faces();
      waited = true;
    }
    const V2T ka0 = cbcast(a.ka[0][0], a.ka[0][1]);
    V2T chi[12];
#pragma unroll
    for (int c = 0; c < 12; c++) chi[c] = czero();
    if (second) hop_dir<0, true, NT>(chi, nullptr, a.ns, jf, 0, a.halo_up, a.face, a.gauge, a.gs, i, ka0);
    else        hop_dir<1, true, NT>(chi, nullptr, a.ns, jf, 0, a.halo_dn, a.face, a.gauge, a.gs, i, ka0);
    const V2T cf = cbcast(a.cre, a.cim);
    V2T malpha = cbcast(0.0, 0.0);
    if (RES) malpha = cbcast(-*a.scal, 0.0);
#pragma unroll
    for (int b = 0; b < 2; b++) {
      V2T v[6];
      if (EPI == EPI_STORE) {
#pragma unroll
        for (int c = 0; c < 6; c++) v[c] = chi[6 * b + c];
      } else if (EPI == EPI_TM_TIMES) {
#pragma unroll
        for (int c = 0; c < 6; c++) v[c] = b == 0 ? cmul(cf, chi[c]) : cmulc(cf, chi[6 + c]);
      } else if (EPI == EPI_CLOVER_INV) {
        V2T ra[3], rb[3];
        su3_block_mul(ra, a.cw, a.gs, i, 0 * 2 + b, chi + 6 * b, false);
        su3_block_mul(rb, a.cw, a.gs, i, 3 * 2 + b, chi + 6 * b, false);
        su3_block_mac(ra, a.cw, a.gs, i, 1 * 2 + b, chi + 6 * b + 3, false);
        su3_block_mac(rb, a.cw, a.gs, i, 2 * 2 + b, chi + 6 * b + 3, false);
#pragma unroll
        for (int c = 0; c < 3; c++) { v[c] = ra[c]; v[3 + c] = rb[c]; }
      } else {   // TM_SUB / CLOVER and their gamma5 forms: p-term minus the accumulator, gamma5 flips the lower half back
        const bool plus = G5 && b == 1;
#pragma unroll
        for (int c = 0; c < 6; c++) v[c] = plus ? chi[6 * b + c] : czero() - chi[6 * b + c];
      }
#pragma unroll
      for (int c = 0; c < 6; c++) {
        o[6 * b + c] = RES ? cfma(malpha, v[c], o[6 * b + c]) : o[6 * b + c] + v[c];
        if (RES || NRM) d += cdotd(o[6 * b + c], o[6 * b + c]);
      }
      st6<NTIO>(dst, ns, i, b, o + 6 * b);
    }
    if (!RES && a.pp_dn) {
      // The boundary slices of `out` are complete HERE and nowhere earlier: project them for the neighbours now (pack_faces_kernel's
      // arithmetic), and the next stencil of a chain -- whose input is this output -- starts its exchange without a pack kernel.
      // The send buffers are free: this kernel waited for the exchange that last read them.
      V2T h[6];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        h[c] = second ? o[c] - o[6 + c] : o[c] + o[6 + c];
        h[3 + c] = second ? o[3 + c] - o[9 + c] : o[3 + c] + o[9 + c];
      }
      if (a.pp_through) st6_through(second ? a.pp_up : a.pp_dn, (size_t)a.face, jf, 0, h);
      else st6<false>(second ? a.pp_up : a.pp_dn, (size_t)a.face, jf, 0, h);
    }
  }
  if (!waited && a.wait_up) wait_faces();   // (a wave without sites still leaves only after the exchange: nothing may overtake it)
  if (a.bcount) {   // direct carrier: the projections went straight into the neighbours' receive buffers; every wave of the grid counts in
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if ((threadIdx.x & 63) == 0) faces_count_in(a, blockIdx.x * 4 + (threadIdx.x >> 6));
  }
  if (HOP_EPI_REDUCES(EPI)) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
    if ((threadIdx.x & 63) == 0) a.partials[blockIdx.x * 4 + (threadIdx.x >> 6)] = d;
  }
}

#ifndef HOP_KERNELS_ONLY   /* (tools/micro/regprobe.hip instantiates single kernels to look at their register budget) */
struct HopLaunch { int block; int minw; int xcd; int occ; int tgrp; int recon; int *grid_out /* receives the number of waves = partial sums */; int stg; int split4; int gcache; int pack /* a.pack is valid: the staged twisted-mass instances read the packed links */; long long *pack_count /* counts the launches that do */; };
// Block order ("xcd" option): 0 none (hardware round-robin), 1 one contiguous chunk per XCD, 2 = default: automatic choice
// between the tile order and the slab order, 3 slab order, 4 tile order.
//   tile order: contiguous chunk of time-slices per XCD, inside it t runs fastest over a small group of slices, so +-t AND
//               +-x users of a line meet in the XCD's L2.  Best while map_tc x-planes' worth of traffic fits the 4 MiB L2
//               (L <= 32: 32^4 147 us vs 158 chunk / 235 none).
//   slab order: XCD j owns the j-th eighth of every time-slice and marches through t.  +-x/y/z reuse in L2, +-t reuse out of
//               the 256 MiB Infinity Cache (three active time-slices).  Wins once an x-plane times the t-group no longer
//               fits L2: 48^3x96 1467 us vs 1575 tile / 1572 none; 64^4 2361 us vs 2977 tile (profiles/r01_variants_sizes*.log).

template <int EPI, int TSKIP, bool NTIO, int BS, int MINW, int GAUX = -1, int STG = 0>
static void launch_one(const HopArgs &a, hipStream_t st, const HopLaunch &o) {
  constexpr int SPB = BS * HOP_SITES;  // sites per block
  const int n = a.i_end - a.i_begin;
  if (n <= 0) return;
  int nb = (n + SPB - 1) / SPB;
  HopArgs b = a;
  b.nxcd_chunk = 0; b.map_tc = 0; b.map_bpt = 0; b.map_nb = nb; b.map_slab = 0;
  const bool whole_slices = a.face % SPB == 0 && a.i_begin % a.face == 0 && n % a.face == 0;
  // automatic choice (xcd = 2): the tile order keeps map_tc (= 4 typ.) x-planes' worth of spinor + gauge traffic between the
  // two uses of a line; past ~4 MiB of that the slab order does better
  // fp32: the slab order already wins at 32^4 (Qtm_pm_psi_32 79.0 against 82.5 us per launch, profiles/r03_fp32_opts_ab.log; 48^3 x 96: 855 against 888)
  const size_t slab_from = sizeof(ET) == 8 ? (size_t)2 << 20 : (size_t)4 << 20;
  // ... and so it does on SHORT lattices with large time-slices (one rank's share of a T split: 8 x 32^3, 16 x 32^3): with fewer than ~24
  // time-slices an XCD's contiguous eighth of the blocks is one or two whole slices, whose +-t neighbours live in other XCDs' L2s
  // (8 x 32^3: 78.6 -> 75.2 us per {H_eo, H_oe}, 16 x 32^3 154.8 -> 149.3; from 24 slices on no difference: profiles/r04_shape_sweep.log)
  const bool short_t = whole_slices && n / a.face < 24 && (size_t)a.YZh * 4 * 1536 > ((size_t)1 << 20);
  const bool want_slab = o.xcd == 3 || (o.xcd == 2 && ((size_t)a.YZh * 4 * 1536 > slab_from || short_t));
  if (want_slab && nb >= 64 && whole_slices && a.face / SPB >= 8) {
    b.map_bpt = a.face / SPB;          // whole time-slices in whole blocks, eight slabs per slice
    b.map_slab = (b.map_bpt + 7) / 8;
    nb = 8 * b.map_slab * (n / a.face);
  } else if (o.xcd && nb >= 64) {
    const int chunk = (nb + 7) / 8;
    b.nxcd_chunk = chunk;
    // tile order needs whole time-slices in whole blocks: range = k time-slices, face % BS == 0
    if (o.xcd >= 2 && whole_slices) {
      const int nt = n / a.face;  // time-slices in this launch
      int grp = 0;
      for (int cand : {4, 5, 6, 3, 2}) if (nt % cand == 0) { grp = cand; break; }
      if (o.tgrp > 0 && nt % o.tgrp == 0) grp = o.tgrp;
      if (grp) { b.map_tc = grp; b.map_bpt = a.face / SPB; }
    }
    nb = chunk * 8;  // blocks past i_end exit immediately
  }
  // occupancy cap: dynamic LDS sized so that only `occ` waves per SIMD fit on a CU
  size_t lds = 0;
  if (o.occ > 0) {
    const int blocks_per_cu = o.occ * 4 * 64 / BS;
    lds = (size_t)(163840 / (blocks_per_cu > 0 ? blocks_per_cu : 1)) / 256 * 256;
    if (lds > 65536) lds = 65536;  // default dynamic-LDS limit without an attribute opt-in
  }
  if (o.grid_out) *o.grid_out = nb * (BS / 64);   // = partial sums the reducing epilogues write: one per wave of the padded grid
  if (STG > 0 && lds < (size_t)(BS / 64) * HOP_STAGE_BYTES) lds = (size_t)(BS / 64) * HOP_STAGE_BYTES;   // the per-wave staging regions double as the occupancy cap
  hipLaunchKernelGGL((hop_kernel<EPI, TSKIP, NTIO, BS, MINW, GAUX, STG>), dim3(nb), dim3(BS), lds, st, b);
}

// The LDS-staged kernel needs blocks of 256 consecutive sites that never straddle a time-slice and a range made of whole blocks
static inline bool stg_ok(const HopArgs &a, const HopLaunch &o) {
  return HOP_SITES == 1 && o.stg && o.block == 256 && a.face % 256 == 0 && a.i_begin % 256 == 0 && (a.i_end - a.i_begin) % 256 == 0 &&
         64 % a.LZh == 0 && a.YZh >= 64;   // a wave = whole z-rows of one x-plane (or whole x-planes are never split): +-z in the wave, +-x never
}

// the whole gauge copy (both parities) small enough to live in the Infinity Cache next to the fields of a CG iteration
// ("gauge_cache" -1 automatic, 0 / 1 force the streaming hint on / off for these launches: A/B)
static inline bool gauge_fits_cache(const HopArgs &a, const HopLaunch &o) { return o.gcache < 0 ? (size_t)2 * 72 * a.gs * sizeof(ET) <= (size_t)200 << 20 : o.gcache != 0; }

template <int EPI, int TSKIP>
static void launch_variant(const HopArgs &a, hipStream_t st, const HopLaunch &o) {
  if constexpr (TSKIP) {
    if (a.face % 64 != 0) { launch_one<EPI, 2, true, 64, 1>(a, st, o); return; }   // waves straddle time-slices: per-lane choice of the skipped hop
  }
  constexpr bool TM_EPI = EPI == EPI_STORE || EPI == EPI_TM_TIMES || EPI == EPI_TM_SUB_G5 || EPI == EPI_TM_SUB || (HOP_EPI_REDUCES(EPI) && !HOP_EPI_CLOVER_G5(EPI));
#ifndef HOP_SPINOR_PACKED
  if constexpr (!TSKIP && (EPI == EPI_STORE || EPI == EPI_TM_TIMES || EPI == EPI_TM_SUB_G5 || EPI == EPI_TM_SUB || EPI == EPI_TM_SUB_G5_NRM || EPI == EPI_TM_SUB_G5_RES)) {
    if (o.split4 && o.recon != 12) {   // small lattices: 64 sites per 256-thread block, the eight hops spread over its four waves
      const int n = a.i_end - a.i_begin;
      if (n <= 0) return;
      const int nb = (n + 63) / 64;
      if (o.grid_out) *o.grid_out = nb;   // one partial per block
      hipLaunchKernelGGL((hop_split4_kernel<EPI, true>), dim3(nb), dim3(256), 0, st, a);
      return;
    }
  }
#endif
  if constexpr (HOP_SITES == 1) {
    if (stg_ok(a, o)) {
      if constexpr (TM_EPI) {
        if (o.recon == 12) { launch_one<EPI, TSKIP, true, 256, 3, 12, 64>(a, st, o); return; }
#ifndef HOP_GAUGE_PACKED
        if constexpr (!TSKIP) {
          if (o.pack) {   // bit-exact packed link read ("gauge_pack"): 104 bytes where the twin was built compact, else 112
            if (o.pack == 16) launch_one<EPI, 0, true, 256, 3, 16, 64>(a, st, o); else launch_one<EPI, 0, true, 256, 3, 15, 64>(a, st, o);
            if (o.pack_count) ++*o.pack_count;
            return;
          }
        }
#endif
      }
      // __launch_bounds__(256, 3) keeps the twisted-mass instances at the gather kernel's three waves per SIMD (146-164 VGPRs, no
      // scratch; left alone the compiler takes 190 for the plain store epilogue); the clover epilogues would spill under that bound
      constexpr int MW = (EPI == EPI_CLOVER_INV || EPI == EPI_CLOVER || HOP_EPI_CLOVER_G5(EPI)) ? 1 : (sizeof(V2T) == 8 ? 4 : 3);   // fp32: four waves (<= 128 VGPRs) like its gather kernel
      launch_one<EPI, TSKIP, true, 256, MW, -1, 64>(a, st, o);
      return;
    }
  }
  // opt-in 12-real gauge read on the launches that cover the bulk of the lattice (twisted-mass epilogues), all precisions
  if constexpr (TM_EPI) {
    if (o.recon == 12 && o.block == 256) {
      launch_one<EPI, TSKIP, true, 256, 1, 12>(a, st, o);
      return;
    }
  }
  // The gather kernel of a T-split rank (TSKIP != 0) with a twisted-mass epilogue is BOUND to three waves per SIMD in fp64 (<= 168 VGPRs),
  // like the staged kernel above: left to itself the allocator lands anywhere between 130 and 250 registers depending on which of the
  // split forms' few extra lines it sees (tools/check_resources.py keeps watch).  Unsplit instances and fp32 stay unbounded (126-146 / <= 128).
  constexpr int GW = (TSKIP != 0 && TSKIP != 2 && TM_EPI && sizeof(V2T) == 16) ? 3 : 1;
  if constexpr (HOP_EPI_REDUCES(EPI)) {   // only reached through launch_hopping_dot: one variant per block size
    if constexpr (!TSKIP) {
      if (o.block == 64) {   // small unsplit lattices
        if (gauge_fits_cache(a, o)) launch_one<EPI, false, true, 64, 1, -2>(a, st, o);
        else launch_one<EPI, false, true, 64, 1>(a, st, o);
        return;
      }
    }
    if constexpr (TSKIP == 1 || TSKIP == 3) {
      // a T-split rank whose gauge copy fits the Infinity Cache (4 x 32^3 per rank: 151 MB) keeps its links there from one stencil to the
      // next, like the small unsplit lattices above -- the unsplit kernel it is measured against does (profiles/r04_split_forms.md)
      if (gauge_fits_cache(a, o)) { launch_one<EPI, TSKIP, true, 256, GW, -2>(a, st, o); return; }
    }
    launch_one<EPI, TSKIP, true, 256, GW>(a, st, o);
    return;
  } else {
    if (o.block == 64) {
      if constexpr (!TSKIP) {
        if (o.minw < 4 && gauge_fits_cache(a, o)) { launch_one<EPI, false, true, 64, 1, -2>(a, st, o); return; }
      }
      if constexpr (TSKIP == 1 || TSKIP == 3) {
        if (o.minw < 4 && gauge_fits_cache(a, o)) { launch_one<EPI, TSKIP, true, 64, GW, -2>(a, st, o); return; }
      }
      if (o.minw >= 4) launch_one<EPI, TSKIP, true, 64, 4>(a, st, o); else launch_one<EPI, TSKIP, true, 64, GW>(a, st, o);
    } else {
      if (o.minw >= 4) launch_one<EPI, TSKIP, true, 256, 4>(a, st, o); else launch_one<EPI, TSKIP, true, 256, GW>(a, st, o);
    }
  }
}

template <int TSKIP>
static void launch_epi(const HopArgs &a, int epi, hipStream_t st, const HopLaunch &o) {
  switch (epi) {
    case EPI_STORE: launch_variant<EPI_STORE, TSKIP>(a, st, o); break;
    case EPI_TM_TIMES: launch_variant<EPI_TM_TIMES, TSKIP>(a, st, o); break;
    case EPI_TM_SUB_G5: launch_variant<EPI_TM_SUB_G5, TSKIP>(a, st, o); break;
    case EPI_TM_SUB_G5_DOT: if constexpr (!TSKIP) launch_variant<EPI_TM_SUB_G5_DOT, 0>(a, st, o); break;   // (unsplit only: launch_hopping_dot refuses it on a T-split rank)
    case EPI_TM_SUB_G5_NRM: launch_variant<EPI_TM_SUB_G5_NRM, TSKIP>(a, st, o); break;
    case EPI_TM_SUB_G5_RES: launch_variant<EPI_TM_SUB_G5_RES, TSKIP>(a, st, o); break;
    case EPI_CLOVER_G5_NRM: launch_variant<EPI_CLOVER_G5_NRM, TSKIP>(a, st, o); break;
    case EPI_CLOVER_G5_RES: launch_variant<EPI_CLOVER_G5_RES, TSKIP>(a, st, o); break;
    // the shifted residual updates exist for unsplit fp64 lattices only (launch_hopping_dot refuses them elsewhere)
    case EPI_TM_SUB_G5_RSH: if constexpr (!TSKIP && sizeof(ET) == 16) launch_variant<EPI_TM_SUB_G5_RSH, 0>(a, st, o); break;
    case EPI_CLOVER_G5_RSH: if constexpr (!TSKIP && sizeof(ET) == 16) launch_variant<EPI_CLOVER_G5_RSH, 0>(a, st, o); break;
    case EPI_CLOVER_INV: launch_variant<EPI_CLOVER_INV, TSKIP>(a, st, o); break;
    case EPI_CLOVER_G5: launch_variant<EPI_CLOVER_G5, TSKIP>(a, st, o); break;
    case EPI_CLOVER: launch_variant<EPI_CLOVER, TSKIP>(a, st, o); break;
    default: launch_variant<EPI_TM_SUB, TSKIP>(a, st, o); break;
  }
}

// "hopsplit": -1 automatic (unsplit fp64 lattices up to HOP_SPLIT4_MAX_SITES sites per parity with the automatic block size), 0 never, 1 always
#define HOP_SPLIT4_MAX_SITES 40000   /* 16^4: 12.8 vs 15.4 us per launch; 20^4 (80 000 sites): 29.4 vs 25.4 -- profiles/r02_hopsplit_ab.log */
static inline int use_split4(const tmhip_ctx *ctx) {
#ifdef HOP_SPINOR_PACKED
  (void)ctx;
  return 0;
#else
  if (ctx->g.nproc_t > 1 || ctx->loopback) return 0;
  if (ctx->opt_hopsplit >= 0) return ctx->opt_hopsplit;
  return ctx->opt_block == 0 && ctx->Vh <= HOP_SPLIT4_MAX_SITES;
#endif
}

static void fill_args(HopArgs &a, tmhip_ctx *ctx, int ieo, ET *out, const ET *in, const ET *p, double cre, double cim) {
  memset(&a, 0, sizeof(a));   // every mapping / fusion field starts from "off": a field added later can never reach a kernel uninitialised
  a.out = out; a.in = in; a.p = p;
  a.gauge = HOP_CTX_GAUGE(ctx) + (size_t)(ieo ? 1 : 0) * 72 * ctx->gs;
  a.halo_up = (const ET *)ctx->recv_up; a.halo_dn = (const ET *)ctx->recv_dn;
  a.ns = ctx->ns; a.gs = ctx->gs;
  a.T = ctx->g.T; a.LX = ctx->g.LX; a.LY = ctx->g.LY; a.LZh = ctx->g.LZ / 2;
  a.Vh = ctx->Vh; a.face = ctx->face; a.YZh = ctx->g.LY * ctx->g.LZ / 2;
  a.par_off = (ctx->g.proc_t * ctx->g.T + ieo) & 1;
  for (int m = 0; m < 4; m++) { a.ka[m][0] = ctx->ka[m][0]; a.ka[m][1] = ctx->ka[m][1]; }
  a.cre = cre; a.cim = cim;
  a.i_begin = 0; a.i_end = ctx->Vh;
}

static HopLaunch launch_opts(const tmhip_ctx *ctx, int block) {
  return HopLaunch{block, ctx->opt_minw, ctx->opt_xcd, HOP_CTX_OCC(ctx), ctx->opt_tgrp, ctx->opt_recon, nullptr, HOP_CTX_STG(ctx), use_split4(ctx), ctx->opt_gauge_cache, 0, nullptr};
}

// "gauge_pack": where this launch would take the staged twisted-mass instance of an unsplit fp64 lattice, make sure the packed twin
// of the gauge copy is current (built on ctx->stream by the first such launch after the links changed) and hand it to the kernel
// if every link of the field has an exact rotation; otherwise the launch reads the 18-real copy as before.
static int pack_setup(tmhip_ctx *ctx, HopArgs &a, HopLaunch &o, int ieo, int epi, bool split) {
#ifndef HOP_GAUGE_PACKED
  const bool clover = epi == EPI_CLOVER_INV || epi == EPI_CLOVER || HOP_EPI_CLOVER_G5(epi);
  if (split || clover || ctx->opt_gauge_pack == 0 || o.recon == 12 || o.split4 || !stg_ok(a, o)) return 0;
  if ((size_t)ctx->gs * 96 >= ((size_t)1 << 32)) return 0;   // the kernel addresses a direction's planes with 32-bit lane offsets
  bool usable = false;
  if (tmhip_gauge_pack_prepare(ctx, &usable)) return 1;
  if (!usable) return 0;
  const size_t off = (size_t)(ieo ? 1 : 0) * 8 * ctx->gs;
  a.pack.rows = ctx->gpack.rows + off * 6; a.pack.tail = ctx->gpack.tail + off;
  a.pack.lo = ctx->gpack.lo + off * 3; a.pack.hi = ctx->gpack.hi + off * 2; a.pack.hi2 = ctx->gpack.hi2 + off;
  o.pack = ctx->gpack_bytes == 104 ? 16 : 15; o.pack_count = &ctx->gpack_launches;   // the GAUX value of the instance that reads the twin as built
#else
  (void)ctx; (void)a; (void)o; (void)ieo; (void)epi; (void)split;
#endif
  return 0;
}

// (a kernel that may wait at its head: at most 2 x 32 blocks)
static int pack_blocks(const tmhip_ctx *ctx) { const int nb = (ctx->face + 255) / 256; return nb < 32 ? nb : 32; }
static void launch_pack(tmhip_ctx *ctx, const ET *in, hipStream_t st, const unsigned int *start_flag = nullptr, unsigned int start_seq = 0) {
  PackArgs p;
  memset(&p, 0, sizeof(p));
  p.in = in; p.ns = ctx->ns; p.Vh = ctx->Vh; p.face = ctx->face;
  p.dst_dn = (ET *)ctx->send_dn; p.dst_up = (ET *)ctx->send_up;
  p.start_flag = start_flag; p.start_seq = start_seq; p.err = ctx->sync_flags + 2; p.ticks = ctx->flag_timeout_ticks;
  hipLaunchKernelGGL(pack_faces_kernel, dim3(pack_blocks(ctx), 2), dim3(256), 0, st, p);
}

// one wave that waits for a flag of the other stream (bounded like every device-side wait here); what follows it in its stream starts behind it
__global__ __launch_bounds__(64) void flag_wait_kernel(const unsigned int *flag, unsigned int seq, unsigned int *err, unsigned long long ticks) {
  wave_wait_flag(flag, seq, err, ticks);
}
__global__ void flag_set_kernel(unsigned int *flag, unsigned int seq) {
  __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// blocks of the exterior launch, and the partials it writes for the reducing epilogues (one per wave)
static int exterior_blocks(const tmhip_ctx *ctx) { const int nb = (2 * ctx->face + 255) / 256; return nb < HOP_EXT_MAX_BLOCKS ? nb : HOP_EXT_MAX_BLOCKS; }
static int exterior_partials(const tmhip_ctx *ctx) { return 4 * exterior_blocks(ctx); }

static void launch_exterior(tmhip_ctx *ctx, const HopArgs &a, int epi, hipStream_t st) {
  HopArgs b = a;
  b.ext_sites = 2 * ctx->face;
  const dim3 grid(exterior_blocks(ctx)), blk(256);
#define TMHIP_X(EPI) hipLaunchKernelGGL((hop_exterior_kernel<EPI, true>), grid, blk, 0, st, b)
  switch (epi) {
    case EPI_STORE: TMHIP_X(EPI_STORE); break;
    case EPI_TM_TIMES: TMHIP_X(EPI_TM_TIMES); break;
    case EPI_TM_SUB_G5: TMHIP_X(EPI_TM_SUB_G5); break;
    case EPI_TM_SUB_G5_NRM: TMHIP_X(EPI_TM_SUB_G5_NRM); break;
    case EPI_TM_SUB_G5_RES: TMHIP_X(EPI_TM_SUB_G5_RES); break;
    case EPI_CLOVER_INV: TMHIP_X(EPI_CLOVER_INV); break;
    case EPI_CLOVER_G5: TMHIP_X(EPI_CLOVER_G5); break;
    case EPI_CLOVER: TMHIP_X(EPI_CLOVER); break;
    case EPI_CLOVER_G5_NRM: TMHIP_X(EPI_CLOVER_G5_NRM); break;
    case EPI_CLOVER_G5_RES: TMHIP_X(EPI_CLOVER_G5_RES); break;
    default: TMHIP_X(EPI_TM_SUB); break;
  }
#undef TMHIP_X
}

#include "hopping_split.inc"   // launch_direct, launch_split: the split-phase launchers

int launch_hopping(tmhip_ctx *ctx, int ieo, ET *out, const ET *in, const ET *p, int epi,
                   double cre, double cim, int comm, const ET *cw = nullptr) {
  if (!HOP_CTX_GAUGE_READY(ctx)) TMHIP_FAIL("Hopping_Matrix called before tmhip_set_gauge");
  if (out == in) TMHIP_FAIL("Hopping_Matrix: l and k must differ (operator/D_psi_body.c:267-272 convention)");
  HopArgs a;
  fill_args(a, ctx, ieo, out, in, p, cre, cim);
  a.cw = cw;
  if ((epi == EPI_CLOVER_INV || epi == EPI_CLOVER_G5 || epi == EPI_CLOVER) && !cw) TMHIP_FAIL("clover operator called before tmhip_set_clover");
  HopLaunch o = launch_opts(ctx, tmhip_hop_block(ctx));
  const bool split = ctx->g.nproc_t > 1 || ctx->loopback;
  if (pack_setup(ctx, a, o, ieo, epi, split)) return 1;
  if (!split) launch_epi<0>(a, epi, ctx->stream, o);
  else if (launch_split(ctx, a, epi, o, comm)) return 1;
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

// tm_sub_Hopping_Matrix / clover_gamma5 with a CG reduction accumulated in the epilogue (partials in ctx->partials, *npartials of them):
// mode 0 <dotv, l> (unsplit lattices only), 1 |l|^2, 2 resid -= (*scal) l without storing l, |resid|^2, 3 (unsplit fp64 only)
// resid -= scal[0] (l + scal[1] dotv) without storing l, |resid|^2 (the shifted residual of the multi-shift CG, mms.hip).
int launch_hopping_dot(tmhip_ctx *ctx, int ieo, ET *out, const ET *in, const ET *p, const ET *dotv,
                             double cre, double cim, int *npartials, int mode, ET *resid, const double *scal, const ET *cw, int chained = 0, const HopSelfAlpha *self = nullptr) {
  if (cw && mode == 0) TMHIP_FAIL("launch_hopping_dot: the clover epilogue has modes 1 and 2 only");
  const bool rmode = mode == 2 || mode == 3;
  if (mode < 0 || mode > 3 || (mode == 0 && !dotv) || (mode == 2 && (!resid || !(scal || self))) || (mode == 3 && (!resid || !scal || !dotv || self)) ||
      (!rmode && !out)) TMHIP_FAIL("launch_hopping_dot: bad arguments for mode %d", mode);
  if (rmode && (const ET *)resid == in) TMHIP_FAIL("launch_hopping_dot: the residual must not be the gathered field");
  if (!HOP_CTX_GAUGE_READY(ctx)) TMHIP_FAIL("Hopping_Matrix called before tmhip_set_gauge");
  const bool split = ctx->g.nproc_t > 1 || ctx->loopback;
  if (mode == 3 && (split || sizeof(ET) != 16)) TMHIP_FAIL("launch_hopping_dot: mode 3 exists for unsplit fp64 lattices only");
  const int blk = split ? 256 : tmhip_hop_block(ctx);   // T-split ranks: the 256-thread kernels only
  const bool s4 = use_split4(ctx) && mode != 0 && mode != 3 && !cw && ctx->opt_recon != 12;   // (the hop-split kernel: 64 sites and four partials per block)
  if (ctx->Vh % ((s4 ? 64 : blk) * HOP_SITES) != 0 || (split && mode == 0))
    TMHIP_FAIL("stencil with fused reduction: needs whole blocks (and mode 1 or 2 on a split lattice)");
  if (out == in) TMHIP_FAIL("Hopping_Matrix: l and k must differ");
  HopArgs a;
  fill_args(a, ctx, ieo, out, in, p, cre, cim);
  a.dotv = dotv; a.partials = ctx->partials; a.resid = resid; a.scal = scal; a.cw = cw;
  if (self) {
    if (!s4 || mode != 2 || split) TMHIP_FAIL("launch_hopping_dot: the self-computed coefficient exists in the hop-split kernel only (tmhip_hopping_self_alpha_ok)");
    a.self = *self;
    a.partials = ctx->partials + ctx->max_partials / 2;   // this launch's own partials go behind the ones it adds up (tmhip_hopping_self_alpha_ok: both halves fit)
    if (self->partials != ctx->partials) TMHIP_FAIL("launch_hopping_dot: the partials to add up are the ones the previous reducing stencil left at the start of the buffer");
  }
  HopLaunch o = launch_opts(ctx, blk);
  o.minw = 0;
  const int epi = cw ? (mode == 1 ? EPI_CLOVER_G5_NRM : (mode == 2 ? EPI_CLOVER_G5_RES : EPI_CLOVER_G5_RSH))
                     : (mode == 0 ? EPI_TM_SUB_G5_DOT : (mode == 1 ? EPI_TM_SUB_G5_NRM : (mode == 2 ? EPI_TM_SUB_G5_RES : EPI_TM_SUB_G5_RSH)));
  const int nbnd = split ? exterior_partials(ctx) : 0;
  // one partial per wave of the grid launch_one chooses (padded by the block orders: at most 8 + 7 * T extra blocks)
  {
    const int nbr = ctx->Vh / (blk * HOP_SITES);
    const int need = s4 ? (ctx->Vh / 64) : (blk / 64) * (nbr + 8 + (nbr >= 64 ? 7 * ctx->g.T : 0)) + nbnd;
    if (need > ctx->max_partials) TMHIP_FAIL("partials buffer too small");
  }
  int nwave = 0;
  o.grid_out = &nwave;
  if (pack_setup(ctx, a, o, ieo, epi, split)) return 1;
  if (!split) launch_epi<0>(a, epi, ctx->stream, o);
  else if (launch_split(ctx, a, epi, o, HOP_COMM | ((chained & 1) ? HOP_CHAINED : 0) | ((chained & 2) ? HOP_FEED : 0))) return 1;   // chained: bit 0 HOP_CHAINED, bit 1 HOP_FEED
  *npartials = (split ? ctx->last_ext_partials : 0) + nwave;
  TMHIP_CHECK(hipGetLastError());
  return 0;
}
#endif  // !HOP_KERNELS_ONLY
