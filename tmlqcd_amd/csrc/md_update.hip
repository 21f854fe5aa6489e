// Molecular-dynamics updates with the links resident in HBM ("gauge-copy refresh per MD step"):
//   update_gauge   (update_gauge.c:51-110)   U_mu(x) <- restoresu3(exposu3(step * P_mu(x))) U_mu(x) for every link
//   update_momenta (update_momenta.c:67-72)  P -= step * derivative
// The lexicographic gauge field ([VPR][4][9] complex, what tmhip_set_gauge received) stays on the device, the momenta
// ([V][4][8] doubles, hamiltonian_field_t::momenta) are uploaded once per trajectory or kept resident, and the stencil's
// gauge copy is re-sorted from the updated links on the device: no host <-> device copy of the gauge field per MD step.
#include "tmhip_internal.h"

namespace {
typedef v2d cd;   // .x = re, .y = im
__device__ __forceinline__ cd cmul(cd a, cd b) { return cd{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cd cconj(cd a) { return cd{a.x, -a.y}; }
__device__ __forceinline__ cd rmul(double r, cd a) { return cd{r * a.x, r * a.y}; }

// u = v w   (su3.h:583-592: each element the sum of three products, left to right)
__device__ __forceinline__ void m3mul(cd (&u)[9], const cd (&v)[9], const cd (&w)[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) u[3 * i + j] = cmul(v[3 * i], w[j]) + cmul(v[3 * i + 1], w[3 + j]) + cmul(v[3 * i + 2], w[6 + j]);
}

// expo.c:56-97 (Cayley-Hamilton form of exp(v), v anti-hermitian traceless from the su3adj vector p = d1..d8)
__device__ __forceinline__ void exposu3(cd (&vr)[9], const double (&p)[8]) {
  cd v[9], v2[9];
  const double d1 = p[0], d2 = p[1], d3 = p[2], d4 = p[3], d5 = p[4], d6 = p[5], d7 = p[6], d8 = p[7];
  v[0] = cd{0.0, 0.5773502691896258 * d8 + d3};     // _make_su3, su3adj.h:45-54
  v[1] = cd{d2, d1};
  v[2] = cd{d5, d4};
  v[3] = cd{-d2, d1};
  v[4] = cd{0.0, 0.5773502691896258 * d8 - d3};
  v[5] = cd{d7, d6};
  v[6] = cd{-d5, d4};
  v[7] = cd{-d7, d6};
  v[8] = cd{0.0, -(1.154700538379252 * d8)};
  m3mul(v2, v, v);
  const double a = 0.5 * (v2[0].x + v2[4].x + v2[8].x);
  // 1/3 Im tr(v v2): the nine products in the order of expo.c:70-72
  const cd tr = cmul(v[0], v2[0]) + cmul(v[1], v2[3]) + cmul(v[2], v2[6]) + cmul(v[3], v2[1]) + cmul(v[4], v2[4]) + cmul(v[5], v2[7]) +
                cmul(v[6], v2[2]) + cmul(v[7], v2[5]) + cmul(v[8], v2[8]);
  const double b = 0.33333333333333333 * tr.y;
  cd a0 = cd{0.16059043836821615e-9, 0.0}, a1 = cd{0.11470745597729725e-10, 0.0}, a2 = cd{0.76471637318198165e-12, 0.0};
  double fac = 0.20876756987868099e-8, r = 12.0;
#pragma unroll
  for (int i = 3; i <= 15; ++i) {
    const cd a1p = a0 + rmul(a, a2);
    a0 = cd{fac - b * a2.y, b * a2.x};              // fac + (b i) a2
    a2 = a1;
    a1 = a1p;
    fac *= r;
    r -= 1.0;
  }
#pragma unroll
  for (int e = 0; e < 9; e++) vr[e] = cmul(a1, v[e]) + cmul(a2, v2[e]);
  vr[0] += a0; vr[4] += a0; vr[8] += a0;
}

// expo.c:118-137: rows 0 and 1 normalised, row 2 = conj(row0 x row1)
__device__ __forceinline__ void restoresu3(cd (&vr)[9], const cd (&u)[9]) {
  const double n0 = 1.0 / sqrt((u[0].x * u[0].x + u[0].y * u[0].y) + (u[1].x * u[1].x + u[1].y * u[1].y) + (u[2].x * u[2].x + u[2].y * u[2].y));
  const double n1 = 1.0 / sqrt((u[3].x * u[3].x + u[3].y * u[3].y) + (u[4].x * u[4].x + u[4].y * u[4].y) + (u[5].x * u[5].x + u[5].y * u[5].y));
#pragma unroll
  for (int e = 0; e < 3; e++) { vr[e] = rmul(n0, u[e]); vr[3 + e] = rmul(n1, u[3 + e]); }
  vr[6] = cconj(cmul(vr[1], vr[5]) - cmul(vr[2], vr[4]));
  vr[7] = cconj(cmul(vr[2], vr[3]) - cmul(vr[0], vr[5]));
  vr[8] = cconj(cmul(vr[0], vr[4]) - cmul(vr[1], vr[3]));
}

// One kernel for "links -> stencil copy" with or without a transform of the links in front:
//   LINKS_UPDATE  U_mu(x) <- restoresu3(exposu3(step P_mu(x))) U_mu(x)  (update_gauge.c:51-110), written back to the lexicographic field
//   LINKS_REUNIT  U_mu(x) <- restoresu3(U_mu(x))  (restoresu3_in_place on every link after an accept, update_tm.c:313-328), written back;
//                 no momenta staged.  The halo slabs of a T-split rank are transformed with the own links (VT = VPR): restoresu3 is a
//                 function of the single link, so the slabs stay the neighbours' slices bit for bit without an exchange
//   LINKS_COPY    U_mu(x) <- the link of a second field in the same layout (aux: the snapshot, after a reject: update_tm.c:329-339),
//                 written to the lexicographic field, halo slabs included -- restore and re-sort in one pass over the snapshot
//   always        the link goes straight to its TWO slots of the stencil's gauge copy g[par][dir][e][site]: dir 2 mu of its own site and
//                 dir 2 mu + 1 of the site at x + mu (update_backward_gauge.c:185-242 turned from a gather into a scatter)
// so an MD step reads every link once and never re-reads the updated field for a separate re-sort (832 + 1152 -> 640 B per link
// site-direction).  A block owns 64 consecutive lexicographic sites = 256 links: the host-layout arrays (144-byte links, 64-byte
// momenta) are moved between HBM and LDS as whole contiguous rows, 16 bytes per lane (a lane-per-link access has a 144-byte lane
// stride: 363 us for 1.48 GB at 32^4, 0.51 of the peak); each thread then takes ONE link out of LDS (lane stride 36 words:
// conflict-free 16-byte reads; the momenta rows are padded to 80 bytes for the same reason).
// T-split ranks: the link U_t at t = T-1 is the backward link of a site of the up neighbour (not stored here), and the backward
// t-links of the t = 0 sites come from the t = -1 halo slab once the neighbours' slices have arrived (halo_backward_kernel).
// VT: the sites whose links are loaded (and transformed): V, or VPR in the LINKS_REUNIT form; only the V own sites are scattered.
// aux: the momenta (LINKS_UPDATE) or the field to copy from (LINKS_COPY).
enum { LINKS_RESORT = 0, LINKS_UPDATE = 1, LINKS_REUNIT = 2, LINKS_COPY = 3 };
template <int MODE>
__global__ __launch_bounds__(256) void links_kernel(v2d *__restrict__ raw, const double *__restrict__ aux, v2d *__restrict__ g, int gs, int V, int VT,
                                                    int T, int LX, int LY, int LZ, int toff, int split, double step) {
  constexpr bool UPDATE = MODE == LINKS_UPDATE;
  __shared__ v2d sl[256 * 9];
  __shared__ v2d sm[UPDATE ? 256 * 5 : 1];
  const int tid = threadIdx.x;
  const size_t l0 = (size_t)blockIdx.x * 256;            // first link of the block
  const int nl = (int)(((size_t)VT * 4 - l0) < 256 ? ((size_t)VT * 4 - l0) : 256);
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const int idx = j * 256 + tid;
    if (idx < nl * 9) sl[idx] = MODE == LINKS_COPY ? reinterpret_cast<const v2d *>(aux)[l0 * 9 + idx] : raw[l0 * 9 + idx];
  }
  if (UPDATE) {
    const v2d *m2 = reinterpret_cast<const v2d *>(aux) + l0 * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int idx = j * 256 + tid;
      if (idx < nl * 4) sm[(idx >> 2) * 5 + (idx & 3)] = m2[idx];
    }
  }
  __syncthreads();
  if (MODE == LINKS_UPDATE || MODE == LINKS_REUNIT) {
    if (tid < nl) {
      cd z[9], out[9];
#pragma unroll
      for (int e = 0; e < 9; e++) z[e] = sl[tid * 9 + e];
      if (UPDATE) {
        double d[8];
#pragma unroll
        for (int k = 0; k < 4; k++) { const v2d m = sm[tid * 5 + k]; d[2 * k] = step * m.x; d[2 * k + 1] = step * m.y; }   // _su3adj_assign_const_times_su3adj, update_gauge.c:85
        cd w[9], v[9];
        exposu3(w, d);
        restoresu3(v, w);
        m3mul(out, v, z);
      } else restoresu3(out, z);
#pragma unroll
      for (int e = 0; e < 9; e++) sl[tid * 9 + e] = out[e];
    }
    __syncthreads();
  }
  if (MODE != LINKS_RESORT) {
#pragma unroll
    for (int j = 0; j < 9; j++) {
      const int idx = j * 256 + tid;
      if (idx < nl * 9) raw[l0 * 9 + idx] = sl[idx];
    }
  }
  // scatter into the stencil copy, re-mapped: thread = (parity p, direction mu, pair s) so that the 32 lanes of one (p, mu) write 32
  // consecutive sites of ONE plane -- 512 contiguous bytes per plane and store instruction instead of 128
  const int p = tid >> 7, mu = (tid >> 5) & 3, sp = tid & 31;
  const int ix0 = (int)(l0 >> 2);
  const int ie = ix0 + 2 * sp;                              // even member of the pair (z even)
  if (ie >= V) return;
  const int z0 = ie % LZ;
  int r = ie / LZ;
  const int y = r % LY;
  r /= LY;
  const int x = r % LX, t = r / LX;
  const int rp = (t + x + y + z0 + toff) & 1;               // parity of the even member
  const int ix = ie + (p ^ rp), z = z0 + (p ^ rp);          // the pair's site of parity p
  const v2d *src = sl + ((ix - ix0) * 4 + mu) * 9;
  cd out[9];
#pragma unroll
  for (int e = 0; e < 9; e++) out[e] = src[e];
  v2d *gf = g + ((size_t)p * 72 + (size_t)(2 * mu) * 9) * gs + (ix >> 1);
#pragma unroll
  for (int e = 0; e < 9; e++) __builtin_nontemporal_store(out[e], gf + (size_t)e * gs);   // (written once, read by the next stencil at the earliest)
  int jx;                                                  // x + mu, periodic
  if (mu == 0) {
    if (t + 1 < T) jx = ix + LX * LY * LZ;
    else { if (split) return; jx = ix - (T - 1) * LX * LY * LZ; }
  } else if (mu == 1) jx = (x + 1 < LX) ? ix + LY * LZ : ix - (LX - 1) * LY * LZ;
  else if (mu == 2) jx = (y + 1 < LY) ? ix + LZ : ix - (LY - 1) * LZ;
  else jx = (z + 1 < LZ) ? ix + 1 : ix - (LZ - 1);
  v2d *gb = g + ((size_t)(1 - p) * 72 + (size_t)(2 * mu + 1) * 9) * gs + (jx >> 1);
#pragma unroll
  for (int e = 0; e < 9; e++) __builtin_nontemporal_store(out[e], gb + (size_t)e * gs);
}

// restoresu3 on every link and nothing else: the first launch of the two-launch accept tmhip_bench_trajectory_forms measures against the
// LINKS_REUNIT form of links_kernel (same row loads through LDS, no scatter)
__global__ __launch_bounds__(256) void reunit_only_kernel(v2d *__restrict__ raw, size_t nlinks) {
  __shared__ v2d sl[256 * 9];
  const int tid = threadIdx.x;
  const size_t l0 = (size_t)blockIdx.x * 256;
  const int nl = (int)((nlinks - l0) < 256 ? (nlinks - l0) : 256);
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const int idx = j * 256 + tid;
    if (idx < nl * 9) sl[idx] = raw[l0 * 9 + idx];
  }
  __syncthreads();
  if (tid < nl) {
    cd z[9], out[9];
#pragma unroll
    for (int e = 0; e < 9; e++) z[e] = sl[tid * 9 + e];
    restoresu3(out, z);
#pragma unroll
    for (int e = 0; e < 9; e++) sl[tid * 9 + e] = out[e];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const int idx = j * 256 + tid;
    if (idx < nl * 9) raw[l0 * 9 + idx] = sl[idx];
  }
}

// T-split rank: dir 1 (U_t(x - t)) of the t = 0 sites <- the t = -1 halo slab of the lexicographic field (geometry_eo.c:296-298)
__global__ __launch_bounds__(256) void halo_backward_kernel(const v2d *__restrict__ raw, v2d *__restrict__ g, int gs, int V, int XYZ, int LX, int LY, int LZ, int toff) {
  const int j = blockIdx.x * 256 + threadIdx.x;          // site of the t = 0 slice, lexicographic
  if (j >= XYZ) return;
  const int z = j % LZ;
  int r = j / LZ;
  const int y = r % LY, x = r / LY;
  const int par = (x + y + z + toff) & 1;
  const v2d *u = raw + ((size_t)(V + XYZ + j) * 4 + 0) * 9;
  v2d *gb = g + ((size_t)par * 72 + 9) * gs + (j >> 1);
#pragma unroll
  for (int e = 0; e < 9; e++) gb[(size_t)e * gs] = u[e];
  (void)LX;
}

// momenta[ix][mu][8] -= step * deriv[par][mu][8][Vh]   (update_momenta.c:67-72).  A block owns 64 consecutive lexicographic sites =
// the e/o indices [32 b, 32 b + 32) of both parities: the derivative's 2 x 32 planes are read as 256-byte runs and transposed
// through LDS (rows padded to 33 doubles: conflict-free), the momenta -- 16 KB of the host layout -- are updated as one contiguous run.
__global__ __launch_bounds__(256) void update_momenta_kernel(double *__restrict__ mom, const double *__restrict__ d, int V, int Vh, int LX, int LY, int LZ, int toff, double step) {
  __shared__ double ld[2][32][33];
  const int tid = threadIdx.x;
  const int i0 = blockIdx.x * 32;
#pragma unroll
  for (int par = 0; par < 2; par++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int idx = j * 256 + tid, e = idx >> 5, sidx = idx & 31;
      if (i0 + sidx < Vh) ld[par][sidx][e] = d[((size_t)par * 32 + e) * Vh + i0 + sidx];
    }
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * 64 * 32;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int idx = j * 256 + tid;                         // double of the block's momenta run
    const int sl = idx >> 5, e = idx & 31;
    const int ix = blockIdx.x * 64 + sl;
    if (ix >= V) continue;
    const int z = ix % LZ;
    int r = ix / LZ;
    const int y = r % LY;
    r /= LY;
    const int x = r % LX, t = r / LX;
    const int par = (t + x + y + z + toff) & 1;
    mom[base + idx] -= step * ld[par][sl >> 1][e];
  }
}

// t = 0 and t = T-1 slices of the lexicographic field -> the neighbours' halo slabs (xchange_gauge, geometry_eo.c:292-299)
}  // namespace
int tmhip_exchange_gauge_halo(tmhip_ctx *ctx) {
  if (ctx->g.nproc_t < 2) return 0;
  if (!ctx->comm_ready) TMHIP_FAIL("nproc_t > 1 but tmhip_comm_init was not called");
  const size_t XYZ = (size_t)ctx->g.LX * ctx->g.LY * ctx->g.LZ, n = XYZ * 36 * 2;   // doubles per slice
  v2d *raw = ctx->gauge_raw;
  v2d *first = raw, *last = raw + (size_t)(ctx->g.T - 1) * XYZ * 36;
  v2d *slab_up = raw + (size_t)ctx->V * 36, *slab_dn = slab_up + XYZ * 36;        // t = T, t = -1
  const int np = ctx->g.nproc_t, up = (ctx->g.proc_t + 1) % np, dn = (ctx->g.proc_t + np - 1) % np;
  if (ctx->shm) return tmhip_shm_ring(ctx, ctx->stream, first, last, slab_up, slab_dn, n * sizeof(double));
  TMHIP_NCCL_CHECK(ncclGroupStart());
  TMHIP_NCCL_CHECK(ncclSend(first, n, ncclDouble, dn, ctx->comm_red, ctx->stream));    // our t = 0 is the down neighbour's t = T
  TMHIP_NCCL_CHECK(ncclRecv(slab_up, n, ncclDouble, up, ctx->comm_red, ctx->stream));
  TMHIP_NCCL_CHECK(ncclSend(last, n, ncclDouble, up, ctx->comm_red, ctx->stream));     // our t = T-1 is the up neighbour's t = -1
  TMHIP_NCCL_CHECK(ncclRecv(slab_dn, n, ncclDouble, dn, ctx->comm_red, ctx->stream));
  TMHIP_NCCL_CHECK(ncclGroupEnd());
  return 0;
}

// links (-> updated links) -> stencil copy on ctx->stream; `halo`: the halo slabs of a T-split rank are current, finish the t = 0 sites
static int launch_links(tmhip_ctx *ctx, int mode, double step) {
  const int toff = ctx->g.proc_t * ctx->g.T, split = ctx->g.nproc_t > 1 ? 1 : 0;
  const int VT = mode == LINKS_REUNIT || mode == LINKS_COPY ? ctx->VPR : ctx->V;
  const unsigned nb = (unsigned)(((size_t)VT * 4 + 255) / 256);
  if (mode == LINKS_UPDATE)
    hipLaunchKernelGGL(links_kernel<LINKS_UPDATE>, dim3(nb), dim3(256), 0, ctx->stream, ctx->gauge_raw, (const double *)ctx->momenta, ctx->gauge, ctx->gs, ctx->V, VT,
                       ctx->g.T, ctx->g.LX, ctx->g.LY, ctx->g.LZ, toff, split, step);
  else if (mode == LINKS_REUNIT)
    hipLaunchKernelGGL(links_kernel<LINKS_REUNIT>, dim3(nb), dim3(256), 0, ctx->stream, ctx->gauge_raw, (const double *)nullptr, ctx->gauge, ctx->gs, ctx->V, VT,
                       ctx->g.T, ctx->g.LX, ctx->g.LY, ctx->g.LZ, toff, split, 0.0);
  else if (mode == LINKS_COPY)
    hipLaunchKernelGGL(links_kernel<LINKS_COPY>, dim3(nb), dim3(256), 0, ctx->stream, ctx->gauge_raw, (const double *)ctx->gauge_snap, ctx->gauge, ctx->gs, ctx->V, VT,
                       ctx->g.T, ctx->g.LX, ctx->g.LY, ctx->g.LZ, toff, split, 0.0);
  else
    hipLaunchKernelGGL(links_kernel<LINKS_RESORT>, dim3(nb), dim3(256), 0, ctx->stream, ctx->gauge_raw, (const double *)nullptr, ctx->gauge, ctx->gs, ctx->V, VT,
                       ctx->g.T, ctx->g.LX, ctx->g.LY, ctx->g.LZ, toff, split, 0.0);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}
static int launch_halo_backward(tmhip_ctx *ctx) {
  if (ctx->g.nproc_t < 2) return 0;
  const int XYZ = ctx->g.LX * ctx->g.LY * ctx->g.LZ;
  hipLaunchKernelGGL(halo_backward_kernel, dim3((XYZ + 255) / 256), dim3(256), 0, ctx->stream, (const v2d *)ctx->gauge_raw, ctx->gauge, ctx->gs, ctx->V, XYZ,
                     ctx->g.LX, ctx->g.LY, ctx->g.LZ, ctx->g.proc_t * ctx->g.T);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}
// Every path that puts new links into the stencil's gauge copy ends here (tmhip_resort_gauge -- behind tmhip_set_gauge, the ILDG reader and
// tmhip_sw_term / tmhip_sw_all with host links --, tmhip_update_gauge, tmhip_multi_update_gauge), with the copy complete on ctx->stream.
static int links_changed(tmhip_ctx *ctx) {
  ctx->gauge_set = true;
  ctx->gauge_copy_current = true;
  ctx->gauge32_set = false;       // the fp32 twin is rebuilt lazily from the new links
  ctx->gauge_recon_dev = -1.0;
  ctx->gpack_state = 0;           // ... and so is the packed twin, by the first stencil launch that can read it
  // "gauge_recon" 12 holds for SU(3) links only, and restoresu3 (rows 0 and 1 normalised, not orthogonalised) lets the updated links drift
  // away from it: the guard measures the new copy before any stencil can read 12 reals of it and gives the option up above 1e-13.  One
  // launch and one synchronisation per change of the links under the option; nothing with the default 18-real read.
  return ctx->opt_recon == 12 ? tmhip_check_gauge_recon(ctx) : 0;
}

// the stencil's gauge copy (and everything derived from the links) from the device-resident lexicographic field, halo slabs included
int tmhip_resort_gauge(tmhip_ctx *ctx) {
  if (!ctx->gauge_raw || !ctx->gauge_raw_valid) TMHIP_FAIL("no lexicographic gauge field on the device");
  if (launch_links(ctx, LINKS_RESORT, 0.0) || launch_halo_backward(ctx)) return 1;
  return links_changed(ctx);
}

// ---- the packed twin of the gauge copy (TmhipGaugePack, tmhip_internal.h) ----
// One thread per link slot of ctx->gauge (blockIdx.y = parity * 8 + direction).  The rotations r = first, first + 1, first + 2 (mod 3) are
// tried in turn: rows r and r + 1 are kept, row r + 2 is rebuilt from them, the distance of the stored row from the rebuild is encoded
// (gauge_pack_codec.h: six 21-bit offsets in ulps), decoded again by the function the stencil uses and compared with the stored row
// as 64-bit integers.  The first rotation that reproduces all six reals is stored; a link without one is counted in count[2] and the
// field is then not read packed at all.  count[0..1]: links on rotation 1 / 2 (one atomic per wave that has any).
// compact: the two kept rows are written in the 88-byte form of gauge_pack_codec.h instead (pk.lo, pk.hi, pk.hi2 in the place of
// pk.rows), decoded again by the stencil's function and compared as 64-bit integers; count[3]: links that have a rotation -- chosen
// exactly as without the flag -- but whose kept rows do not fit that form.
__global__ __launch_bounds__(256) void gauge_pack_kernel(const v2d *__restrict__ g, const TmhipGaugePack pk, int gs, int Vh, int first, unsigned int *count,
                                                         int compact) {
  v2d *__restrict__ rows = const_cast<v2d *>(pk.rows);
  v4u *__restrict__ tail = const_cast<v4u *>(pk.tail);
  const int i = blockIdx.x * 256 + threadIdx.x;
  int chosen = 0;   // 0..2: rotation, 3: none, -1: no link
  bool nofit = false;   // compact: the link has a rotation and its kept rows do not fit the 88-byte form
  if (i >= Vh) chosen = -1;
  else {
    const size_t slot = (size_t)blockIdx.y * gs + i;
    const v2d *gp = g + (size_t)blockIdx.y * 9 * gs + i;
    v2d u[9];
#pragma unroll
    for (int e = 0; e < 9; e++) u[e] = gp[(size_t)e * gs];
    v2d ka[3], kb[3];
    uint32_t kt[4];
    chosen = 3;
    for (int n = 0; n < 3 && chosen == 3; n++) {
      const int r = (first + n) % 3;
      v2d a[3], b[3], c[3], w[3];
#pragma unroll
      for (int e = 0; e < 3; e++) {   // selects, not indexed registers
        a[e] = r == 0 ? u[e] : (r == 1 ? u[3 + e] : u[6 + e]);
        b[e] = r == 0 ? u[3 + e] : (r == 1 ? u[6 + e] : u[e]);
        c[e] = r == 0 ? u[6 + e] : (r == 1 ? u[e] : u[3 + e]);
      }
      tmhip_su3_row_rebuild(a, b, w);
      const double c6[6] = {c[0].x, c[0].y, c[1].x, c[1].y, c[2].x, c[2].y}, w6[6] = {w[0].x, w[0].y, w[1].x, w[1].y, w[2].x, w[2].y};
      double t6[6];
      uint32_t t[4];
      bool same = tmhip_gpack_encode(c6, w6, r, t);
      tmhip_gpack_decode(w6, t, t6);
      same = same && tmhip_gpack_rot(t) == r;
#pragma unroll
      for (int e = 0; e < 6; e++) same = same && tmhip_gpack_bits(t6[e]) == tmhip_gpack_bits(c6[e]);
      if (same || n == 2) {   // (a link without an exact rotation still gets defined planes)
#pragma unroll
        for (int e = 0; e < 3; e++) { ka[e] = a[e]; kb[e] = b[e]; }
#pragma unroll
        for (int e = 0; e < 4; e++) kt[e] = t[e];
        if (same) chosen = r;
      }
    }
    if (compact) {
      const double k12[12] = {ka[0].x, ka[0].y, ka[1].x, ka[1].y, ka[2].x, ka[2].y, kb[0].x, kb[0].y, kb[1].x, kb[1].y, kb[2].x, kb[2].y};
      double t12[12];
      uint32_t lo[12], h[10];
      bool same = tmhip_gpack104_encode(k12, lo, h);
      tmhip_gpack104_decode(lo, h, t12);
#pragma unroll
      for (int e = 0; e < 12; e++) same = same && tmhip_gpack_bits(t12[e]) == tmhip_gpack_bits(k12[e]);
      nofit = chosen != 3 && !same;
      v4u *lop = const_cast<v4u *>(pk.lo) + (size_t)blockIdx.y * 3 * gs + i, *hip = const_cast<v4u *>(pk.hi) + (size_t)blockIdx.y * 2 * gs + i;
#pragma unroll
      for (int e = 0; e < 3; e++) lop[(size_t)e * gs] = v4u{lo[4 * e], lo[4 * e + 1], lo[4 * e + 2], lo[4 * e + 3]};
#pragma unroll
      for (int e = 0; e < 2; e++) hip[(size_t)e * gs] = v4u{h[4 * e], h[4 * e + 1], h[4 * e + 2], h[4 * e + 3]};
      const_cast<v2u *>(pk.hi2)[slot] = v2u{h[8], h[9]};
    } else {
#pragma unroll
      for (int e = 0; e < 3; e++) {
        rows[((size_t)blockIdx.y * 6 + e) * gs + i] = ka[e];
        rows[((size_t)blockIdx.y * 6 + 3 + e) * gs + i] = kb[e];
      }
    }
    tail[slot] = v4u{kt[0], kt[1], kt[2], kt[3]};
  }
#pragma unroll
  for (int v = 1; v <= 4; v++) {
    const unsigned long long m = __ballot(v == 4 ? nofit : chosen == v);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(count + (v - 1), (unsigned int)__popcll(m));
  }
}

int tmhip_gauge_pack_prepare(tmhip_ctx *ctx, bool *usable) {
  *usable = false;
  if (!ctx->gauge_set) return 0;
  if (ctx->gpack_unavailable) return 0;
  if (ctx->gpack_state == 0) {
    const size_t n = (size_t)16 * ctx->gs;   // link slots, padding included
    if (!ctx->gpack_mem) {
      if (!ctx->gpack_ev_made) {
        TMHIP_CHECK(hipEventCreate(&ctx->gpack_ev[0]));
        if (hipEventCreate(&ctx->gpack_ev[1]) != hipSuccess) { (void)hipEventDestroy(ctx->gpack_ev[0]); TMHIP_FAIL("tmhip_gauge_pack_prepare: hipEventCreate failed"); }
        ctx->gpack_ev_made = true;
      }
      // (out of memory is no error: the field is simply not read packed, and the allocation is not tried again)
      if (hipMalloc(&ctx->gpack_mem, n * 112 + 64) != hipSuccess) {
        (void)hipGetLastError();
        ctx->gpack_mem = nullptr; ctx->gpack_unavailable = true;
        for (int k = 0; k < 4; k++) ctx->gpack_stats[k] = 0;
        return 0;
      }
      unsigned char *m = (unsigned char *)ctx->gpack_mem;
      ctx->gpack.rows = (const v2d *)m;
      ctx->gpack.tail = (const v4u *)(m + n * 96);
      ctx->gpack.lo = (const v4u *)m;              // the compact rows lie where the six row planes do: 48 + 32 + 8 of their 96 bytes per link
      ctx->gpack.hi = (const v4u *)(m + n * 48);
      ctx->gpack.hi2 = (const v2u *)(m + n * 80);
      ctx->gpack_count = (unsigned int *)(m + n * 112);
    }
    const int first = ctx->opt_gauge_pack_rot < 0 ? 0 : ctx->opt_gauge_pack_rot;
    unsigned int h[4] = {0, 0, 0, 0};
    // the compact form first; a field with rotations throughout but a link that does not fit it is built once more in the 112-byte form
    // (the rotations, and with them the first three counters, are the same in both launches)
    int compact = ctx->opt_gauge_pack_compact != 0 ? 1 : 0;
    TMHIP_CHECK(hipEventRecord(ctx->gpack_ev[0], ctx->stream));
    for (;;) {
      TMHIP_CHECK(hipMemsetAsync(ctx->gpack_count, 0, sizeof(h), ctx->stream));
      hipLaunchKernelGGL(gauge_pack_kernel, dim3((ctx->Vh + 255) / 256, 16), dim3(256), 0, ctx->stream, (const v2d *)ctx->gauge, ctx->gpack, ctx->gs, ctx->Vh, first,
                         ctx->gpack_count, compact);
      TMHIP_CHECK(hipGetLastError());
      TMHIP_CHECK(hipEventRecord(ctx->gpack_ev[1], ctx->stream));
      TMHIP_CHECK(hipMemcpyAsync(h, ctx->gpack_count, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
      TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
      if (!(compact && h[2] == 0 && h[3] != 0)) break;
      compact = 0;
    }
    TMHIP_CHECK(hipEventElapsedTime(&ctx->gpack_build_ms, ctx->gpack_ev[0], ctx->gpack_ev[1]));
    ctx->gpack_stats[1] = h[0]; ctx->gpack_stats[2] = h[1]; ctx->gpack_stats[3] = h[2];
    ctx->gpack_stats[0] = (long long)16 * ctx->Vh - h[0] - h[1] - h[2];
    ctx->gpack_state = h[2] == 0 ? 1 : 2;
    ctx->gpack_bytes = h[2] != 0 ? 0 : (compact ? 104 : 112);
  }
  *usable = ctx->gpack_state == 1;
  return 0;
}

extern "C" {

int tmhip_gauge_pack_stats(tmhip_ctx *ctx, long long out[5]) {
  if (!out) TMHIP_FAIL("tmhip_gauge_pack_stats: null argument");
  if (!ctx->gauge_set) TMHIP_FAIL("tmhip_gauge_pack_stats called before tmhip_set_gauge");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  bool usable = false;
  if (tmhip_gauge_pack_prepare(ctx, &usable)) return 1;
  out[0] = usable ? 1 : 0;
  for (int k = 0; k < 4; k++) out[1 + k] = ctx->gpack_stats[k];
  return 0;
}

int tmhip_gauge_pack_format(tmhip_ctx *ctx, int *bytes_per_link) {
  if (!bytes_per_link) TMHIP_FAIL("tmhip_gauge_pack_format: null argument");
  if (!ctx->gauge_set) TMHIP_FAIL("tmhip_gauge_pack_format called before tmhip_set_gauge");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  bool usable = false;
  if (tmhip_gauge_pack_prepare(ctx, &usable)) return 1;
  *bytes_per_link = usable ? ctx->gpack_bytes : 0;
  return 0;
}

int tmhip_gauge_pack_launches(tmhip_ctx *ctx, long long *n) {
  if (!n) TMHIP_FAIL("tmhip_gauge_pack_launches: null argument");
  *n = ctx->gpack_launches;
  return 0;
}

int tmhip_gauge_pack_build_ms(tmhip_ctx *ctx, double *ms) {
  if (!ms) TMHIP_FAIL("tmhip_gauge_pack_build_ms: null argument");
  *ms = (double)ctx->gpack_build_ms;
  return 0;
}

int tmhip_momenta_upload(tmhip_ctx *ctx, const void *host) {
  if (!host) TMHIP_FAIL("tmhip_momenta_upload: null argument");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)ctx->V * 32 * sizeof(double);
  if (!ctx->momenta) TMHIP_CHECK(hipMalloc((void **)&ctx->momenta, bytes));
  TMHIP_CHECK(hipMemcpyAsync(ctx->momenta, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->xfer[2]++;
  return 0;
}

int tmhip_momenta_download(tmhip_ctx *ctx, void *host) {
  if (!host) TMHIP_FAIL("tmhip_momenta_download: null argument");
  if (!ctx->momenta) TMHIP_FAIL("tmhip_momenta_download: no momenta on the device");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  TMHIP_CHECK(hipMemcpyAsync(host, ctx->momenta, (size_t)ctx->V * 32 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->xfer[3]++;
  return 0;
}

/* update_momenta.c:67-72 with the derivative accumulated on the device by tmhip_deriv_Sb / tmhip_sw_all */
int tmhip_update_momenta(tmhip_ctx *ctx, double step) {
  if (!ctx->momenta) TMHIP_FAIL("tmhip_update_momenta: no momenta on the device (tmhip_momenta_upload)");
  if (!ctx->deriv) TMHIP_FAIL("tmhip_update_momenta: no derivative field on the device");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(update_momenta_kernel, dim3((ctx->V + 63) / 64), dim3(256), 0, ctx->stream, ctx->momenta, (const double *)ctx->deriv,
                     ctx->V, ctx->Vh, ctx->g.LX, ctx->g.LY, ctx->g.LZ, ctx->g.proc_t * ctx->g.T, step);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

/* update_gauge.c:51-110 on the device-resident links, then the halo slabs of a T-split rank (xchange_gauge) and the re-sort
 * of the stencil's gauge copy (update_backward_gauge.c:185-242) -- all in HBM */
int tmhip_update_gauge(tmhip_ctx *ctx, double step) {
  if (!ctx->gauge_raw || !ctx->gauge_raw_valid) TMHIP_FAIL("tmhip_update_gauge: the links are not resident (tmhip_set_gauge first)");
  if (!ctx->momenta) TMHIP_FAIL("tmhip_update_gauge: no momenta on the device (tmhip_momenta_upload)");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (launch_links(ctx, LINKS_UPDATE, step)) return 1;                 // exp(step P) U, back to the lexicographic field and into the stencil copy
  if (tmhip_exchange_gauge_halo(ctx)) return 1;
  if (launch_halo_backward(ctx)) return 1;                     // T-split: the backward t-links of the t = 0 sites from the neighbour's updated slice
  // clover blocks belong to the old links: tmhip_sw_term (gauge = NULL: from the resident links) / tmhip_sw_invert again
  ctx->sw_set = false; ctx->clover_set = false; ctx->sw_inv_ieo = -1; ctx->clover_nd_set = false; ctx->clover32_set = false;
  return links_changed(ctx);
}

/* ---- the links around a trajectory: gauge_tmp of update_tm.c on the device ---- */
/* update_tm.c:109-121: gauge_tmp <- links (halo slabs of a T-split rank included, so that a restore needs no exchange) */
int tmhip_gauge_snapshot(tmhip_ctx *ctx) {
  if (!ctx->gauge_raw || !ctx->gauge_raw_valid) TMHIP_FAIL("tmhip_gauge_snapshot: the links are not resident (tmhip_set_gauge first)");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)ctx->VPR * 36 * sizeof(v2d);
  if (!ctx->gauge_snap) TMHIP_CHECK(hipMalloc((void **)&ctx->gauge_snap, bytes));
  TMHIP_CHECK(hipMemcpyAsync(ctx->gauge_snap, ctx->gauge_raw, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}

int tmhip_gauge_snapshot_free(tmhip_ctx *ctx) {
  if (!ctx->gauge_snap) return 0;
  TMHIP_CHECK(hipSetDevice(ctx->device));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  TMHIP_CHECK(hipFree(ctx->gauge_snap));
  ctx->gauge_snap = nullptr;
  return 0;
}

// The two ways to put the snapshot back.  tmhip_bench_trajectory_forms measures both (profiles/r17_traj_speed.log: 0.572 against 0.445 ms at
// 32^4); tmhip_gauge_restore uses the one pass.
static int restore_two_launches(tmhip_ctx *ctx) {   // device-to-device copy, then the plain re-sort: 576 + 576 + 576 + 1152 bytes per site
  TMHIP_CHECK(hipMemcpyAsync(ctx->gauge_raw, ctx->gauge_snap, (size_t)ctx->VPR * 36 * sizeof(v2d), hipMemcpyDeviceToDevice, ctx->stream));
  return launch_links(ctx, LINKS_RESORT, 0.0);
}
static int restore_one_pass(tmhip_ctx *ctx) {       // the re-sort reads the snapshot and writes the links as well: 576 + 576 + 1152
  return launch_links(ctx, LINKS_COPY, 0.0);
}

/* update_tm.c:329-339 (reject): links <- gauge_tmp and the stencil's copy from them; everything derived from the links is left as
 * tmhip_update_gauge leaves it */
int tmhip_gauge_restore(tmhip_ctx *ctx) {
  if (!ctx->gauge_snap) TMHIP_FAIL("tmhip_gauge_restore: no snapshot (tmhip_gauge_snapshot first)");
  if (!ctx->gauge_raw) TMHIP_FAIL("tmhip_gauge_restore: the links are not resident (tmhip_set_gauge first)");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (restore_one_pass(ctx)) return 1;
  ctx->gauge_raw_valid = true;
  if (launch_halo_backward(ctx)) return 1;
  ctx->sw_set = false; ctx->clover_set = false; ctx->sw_inv_ieo = -1; ctx->clover_nd_set = false; ctx->clover32_set = false;
  return links_changed(ctx);
}

/* update_tm.c:313-328 (accept): restoresu3_in_place on every link, own and halo, and the stencil's copy from them, in one pass */
int tmhip_gauge_reunitarize(tmhip_ctx *ctx) {
  if (!ctx->gauge_raw || !ctx->gauge_raw_valid) TMHIP_FAIL("tmhip_gauge_reunitarize: the links are not resident (tmhip_set_gauge first)");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (launch_links(ctx, LINKS_REUNIT, 0.0) || launch_halo_backward(ctx)) return 1;
  ctx->sw_set = false; ctx->clover_set = false; ctx->sw_inv_ieo = -1; ctx->clover_nd_set = false; ctx->clover32_set = false;
  return links_changed(ctx);
}

/* Device time (HIP events, per call, over `reps` calls) of one form of the reject / accept pass, for tools/traj_speed.py:
 *   form 0  restore as a device-to-device copy + the plain re-sort      1  restore as one pass (the re-sort reads the snapshot)
 *   form 2  accept as restoresu3 pass + the plain re-sort               3  accept as one pass (LINKS_REUNIT)
 * Needs resident links and a snapshot.  The links end up restored (0, 1) or reunitarised (2, 3), the derived state as after the call
 * measured. */
int tmhip_bench_trajectory_forms(tmhip_ctx *ctx, int form, int reps, double *ms) {
  if (!ms || form < 0 || form > 3 || reps < 1) TMHIP_FAIL("tmhip_bench_trajectory_forms: bad argument");
  if (!ctx->gauge_raw || !ctx->gauge_raw_valid || !ctx->gauge_snap) TMHIP_FAIL("tmhip_bench_trajectory_forms: needs resident links and a snapshot");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const size_t nlinks = (size_t)ctx->VPR * 4;
  for (int r = -1; r < reps; r++) {   // (one warm call)
    if (r == 0) TMHIP_CHECK(hipEventRecord(ctx->ev_slots[14], ctx->stream));
    int rc = 0;
    if (form == 0) rc = restore_two_launches(ctx);
    else if (form == 1) rc = restore_one_pass(ctx);
    else if (form == 2) {
      hipLaunchKernelGGL(reunit_only_kernel, dim3((unsigned)((nlinks + 255) / 256)), dim3(256), 0, ctx->stream, ctx->gauge_raw, nlinks);
      rc = launch_links(ctx, LINKS_RESORT, 0.0);
    } else rc = launch_links(ctx, LINKS_REUNIT, 0.0);
    if (rc || launch_halo_backward(ctx)) return 1;
  }
  TMHIP_CHECK(hipEventRecord(ctx->ev_slots[15], ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  float t = 0.f;
  TMHIP_CHECK(hipEventElapsedTime(&t, ctx->ev_slots[14], ctx->ev_slots[15]));
  *ms = (double)t / reps;
  ctx->sw_set = false; ctx->clover_set = false; ctx->sw_inv_ieo = -1; ctx->clover_nd_set = false; ctx->clover32_set = false;
  return links_changed(ctx);
}

/* The same on a T-split lattice held by n contexts of one process (peer copies instead of RCCL, as tmhip_multi_sw_all): every
 * rank updates its links, the t = 0 / t = T-1 slices travel to the ring neighbours' halo slabs, the stencil copies are re-sorted. */
int tmhip_multi_update_gauge(int n, tmhip_ctx **ctxs, double step) {
  if (n < 2) TMHIP_FAIL("tmhip_multi_update_gauge needs >= 2 contexts");
  for (int r = 0; r < n; r++) {
    tmhip_ctx *c = ctxs[r];
    if (c->g.nproc_t != n || c->g.proc_t != r) TMHIP_FAIL("context %d is not rank %d of a %d-way T split", r, r, n);
    if (!c->gauge_raw || !c->gauge_raw_valid || !c->momenta) TMHIP_FAIL("tmhip_multi_update_gauge: rank %d has no resident links / momenta", r);
    TMHIP_CHECK(hipSetDevice(c->device));
    if (launch_links(c, LINKS_UPDATE, step)) return 1;
  }
  for (int r = 0; r < n; r++) { TMHIP_CHECK(hipSetDevice(ctxs[r]->device)); TMHIP_CHECK(hipStreamSynchronize(ctxs[r]->stream)); }
  const size_t XYZ = (size_t)ctxs[0]->g.LX * ctxs[0]->g.LY * ctxs[0]->g.LZ, sb = XYZ * 36 * sizeof(v2d);
  for (int r = 0; r < n; r++) {
    tmhip_ctx *c = ctxs[r], *up = ctxs[(r + 1) % n], *dn = ctxs[(r + n - 1) % n];
    TMHIP_CHECK(hipSetDevice(c->device));
    v2d *slab_up = c->gauge_raw + (size_t)c->V * 36, *slab_dn = slab_up + XYZ * 36;                                    // t = T, t = -1
    TMHIP_CHECK(hipMemcpyPeerAsync(slab_up, c->device, up->gauge_raw, up->device, sb, c->stream));                                            // the up neighbour's t = 0
    TMHIP_CHECK(hipMemcpyPeerAsync(slab_dn, c->device, dn->gauge_raw + (size_t)(dn->g.T - 1) * XYZ * 36, dn->device, sb, c->stream));         // the down neighbour's t = T-1
    c->sw_set = false; c->clover_set = false; c->sw_inv_ieo = -1; c->clover_nd_set = false; c->clover32_set = false;
    if (launch_halo_backward(c)) return 1;
    if (links_changed(c)) return 1;
  }
  for (int r = 0; r < n; r++) { TMHIP_CHECK(hipSetDevice(ctxs[r]->device)); TMHIP_CHECK(hipStreamSynchronize(ctxs[r]->stream)); }
  return 0;
}

/* the device-resident links in the host layout of g_gauge_field ([VOLUMEPLUSRAND][4] su3) */
int tmhip_gauge_download(tmhip_ctx *ctx, void *host) {
  if (!host) TMHIP_FAIL("tmhip_gauge_download: null argument");
  if (!ctx->gauge_raw || !ctx->gauge_raw_valid) TMHIP_FAIL("tmhip_gauge_download: the links are not resident");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  TMHIP_CHECK(hipMemcpyAsync(host, ctx->gauge_raw, (size_t)ctx->VPR * 36 * sizeof(v2d), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->xfer[1]++;
  return 0;
}

}  // extern "C"
