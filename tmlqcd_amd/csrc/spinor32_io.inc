// Access to the packed fp32 spinor fields -- six planes of float4 = components (0,1) (2,3) ... (10,11), [6][stride] -- by the kernels
// that work on complex floats: ld6 / st6 move the six components 6*blk .. 6*blk+5 of site j in three 16-byte accesses.  Included
// inside the namespace of a translation unit that has V2T = ET = v2f (hopping32.hip, nd32.hip).
typedef float vf4 __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ void ld6(V2T *s, const ET *f, size_t stride, int j, int blk) {
  const vf4 *p = reinterpret_cast<const vf4 *>(f);
#pragma unroll
  for (int m = 0; m < 3; m++) {
    const vf4 *q = p + (size_t)(3 * blk + m) * stride + j;
    const vf4 v = NT ? __builtin_nontemporal_load(q) : *q;
    s[2 * m] = V2T{v.x, v.y}; s[2 * m + 1] = V2T{v.z, v.w};
  }
}
template <bool NT> __device__ __forceinline__ void st6(ET *f, size_t stride, int j, int blk, const V2T *s) {
  vf4 *p = reinterpret_cast<vf4 *>(f);
#pragma unroll
  for (int m = 0; m < 3; m++) {
    const vf4 v = vf4{s[2 * m].x, s[2 * m].y, s[2 * m + 1].x, s[2 * m + 1].y};
    vf4 *q = p + (size_t)(3 * blk + m) * stride + j;
    if (NT) __builtin_nontemporal_store(v, q);
    else *q = v;
  }
}
