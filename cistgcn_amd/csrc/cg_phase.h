// Helpers of the kernels that walk (B,C,T,V) tensors in phases or tiles - dstd_tail.hip, map2adj_tail.hip, block_input.hip,
// collapse_rows.hip, tower_maps.hip, fpn_conv.hip, gate_head.hip, block_mid.hip: the BatchNorm constants of a chain (cg_bn.h),
// matrix-core fragment reads, the dropout factors of a quad.
#pragma once
#include "cg_common.h"
#include "cg_bn.h"

typedef float cg_f32x4 __attribute__((vector_size(16)));

// ======================================================================================================================
// matrix-core helpers (same fragment scheme as stgcn_domain_mfma.hip: inside a 16-wide k chunk step s takes k = 4*slot + s)
// ======================================================================================================================
template <int KIND>
__device__ __forceinline__ void cg_tfrag(const float* __restrict__ p, int rs, int k0, float v[4]) {
  if (KIND == 0) {
    const float4 t = *reinterpret_cast<const float4*>(p + k0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    const float* q = p + k0 * rs;
    v[0] = q[0]; v[1] = q[rs]; v[2] = q[2 * rs]; v[3] = q[3 * rs];
  }
}
template <int KIND>
__device__ __forceinline__ const float* cg_tfrag_ptr(const float* base, int rs, int l15, int slot) {
  return KIND == 0 ? base + l15 * rs + 4 * slot : base + l15 + 4 * slot * rs;
}


// keep factors of the four consecutive elements idx0 .. idx0 + 3 (idx0 % 4 == 0): one hash, as cg_norm_act's float4 path
static __device__ __forceinline__ void cg_keep4(bool on, float p, unsigned long long seed, unsigned int salt, unsigned long long idx0, float keep[4]) {
  if (!on) { keep[0] = keep[1] = keep[2] = keep[3] = 1.f; return; }
  const unsigned long long bits = cg_drop_bits(seed, salt, idx0 >> 2);
#pragma unroll
  for (int j = 0; j < 4; ++j) keep[j] = cg_drop_pick(bits, j, p);
}
