// Included by every source of the kernel library: the public C ABI (include/cistgcn_hip.h: every argument block, caller-facing limit and
// entry-point prototype - the kernels are compiled against it, nothing of it is repeated here), status codes, launcher limits, and
// the small device helpers more than one file needs - wave / block reductions, row-of-16 DPP exchange, fixed-width vector load / store,
// division by a run-time constant, the dropout hash.  (BatchNorm constants: cg_bn.h; fragment reads of the phase kernels: cg_phase.h.)
// Wavefront = 64 lanes (CDNA4); every reduction below is written for that width.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cistgcn_hip.h"      // by its place in the tree: found with or without include/ on the include path

#define CG_WAVE 64

// Makes a per-lane value opaque to the optimiser (no instruction is emitted).  Used at the top of long loop bodies so that the
// address arithmetic derived from it is recomputed per iteration instead of being hoisted into dozens of live registers.
// The CPU test shim (tests/hipemu) defines it as a no-op before this header is read.
#ifndef CG_OPAQUE_V
#define CG_OPAQUE_V(x) asm volatile("" : "+v"(x))
#endif

// ---- status codes returned through the C ABI (0 = ok, >0 = hipError_t, <0 = argument check) ----
#define CG_OK 0
#define CG_EARG (-1)
#define CG_ESHAPE (-2)

// Zero fill by a kernel (rowops.hip).  hipMemsetAsync is NOT used anywhere in this library: as a node of a captured HIP
// graph it was not reliably ordered against the neighbouring kernels (see cg_zero in rowops.hip).
int cg_zero_fill(void* p, long long bytes, hipStream_t stream);

// Dynamic LDS above the default limit needs hipFuncAttributeMaxDynamicSharedMemorySize raised on the kernel.  That is a driver call:
// it used to run in front of EVERY launch of the LDS-heavy kernels (invisible under graph replay, pure host overhead in eager
// small-batch steps).  The limit a kernel has been given is remembered here (per translation unit: kernels are file-local), the driver
// is called only when a launch needs more than was granted before.
#include <mutex>
static inline hipError_t cg_lds_limit(const void* fn, size_t bytes) {
  struct Slot { const void* fn; size_t bytes; };
  static Slot slots[64];
  static int used = 0;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  int at = -1;
  for (int i = 0; i < used; ++i) if (slots[i].fn == fn) { at = i; break; }
  if (at >= 0 && slots[at].bytes >= bytes) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  if (at < 0 && used < 64) at = used++;
  if (at >= 0) { slots[at].fn = fn; slots[at].bytes = bytes; }
  return hipSuccess;
}

// ---- limits of the glue launchers (stages.hip, optim.hip, rowops.hip), named so that cg_glue_geometry (stages.hip) answers from
// the numbers the launchers use: grids of the grid-stride kernels, the register budget of the sliced SE-gate backward, the
// dynamic LDS a kernel may take before cg_lds_limit has to raise its limit
#define CG_GLUE_THREADS 256
#define CG_MPJPE_MAX_BLOCKS 1024               // cg_mpjpe_fwd: one float atomic per workgroup onto the loss
// (cg_motion_loss_*, losses.hip: CG_LOSS_MAX_BLOCKS / CG_LOSS_THREADS are in cistgcn_hip.h - the caller sizes the scratch by them)
#define CG_LOSS_WAVES (CG_LOSS_THREADS / CG_WAVE)     // frames one workgroup of cg_motion_loss_* has in flight
#define CG_FLAT_MAX_BLOCKS 2048                // cg_adam_flat, cg_scale
#define CG_ZERO_MAX_BLOCKS 4096                // cg_zero_fill, 16 bytes per thread and pass
#define CG_SE_THREADS 256
#define CG_SE_MAXACC 8                         // sliced SE-gate backward: C * H <= CG_SE_THREADS * CG_SE_MAXACC
#define CG_SE_MAX_WORKGROUPS 64
#define CG_LDS_DEFAULT (64 * 1024)
#define CG_DSTD_THREADS 1024
#define CG_DSTD_ROWS_IN_FLIGHT 4
#define CG_DSTD_LDS_MAX (160 * 1024)

static inline int cg_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? CG_OK : (int)e;
}

// ---- wave / block reductions -------------------------------------------------------------------
// sum over the wavefront, result valid in lane 0
template <typename T>
__device__ __forceinline__ T cg_wave_sum(T v) {
#pragma unroll
  for (int off = CG_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, CG_WAVE);
  return v;
}
// maximum over the wavefront in every lane, T = float or double (a butterfly: every lane combines the same pairs)
template <typename T>
__device__ __forceinline__ T cg_wave_allmax(T v) {
#pragma unroll
  for (int off = CG_WAVE / 2; off > 0; off >>= 1) {
    if constexpr (sizeof(T) == sizeof(float)) v = fmaxf(v, __shfl_xor(v, off, CG_WAVE));
    else v = fmax(v, __shfl_xor(v, off, CG_WAVE));
  }
  return v;
}
// sum over the wavefront of N values at once, result in every lane (the same butterfly, so all lanes hold the same bits); the N
// exchanges of a level are independent
template <int N>
__device__ __forceinline__ void cg_wave_allsum(double (&v)[N]) {
#pragma unroll
  for (int off = CG_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], off, CG_WAVE);
  }
}

// Sum over the whole workgroup; result valid in thread 0. `scratch` holds >= 16 T's in LDS.
// Contains two barriers; every thread of the block must call it.
template <typename T>
__device__ __forceinline__ T cg_block_sum(T v, T* scratch) {
  const int lane = threadIdx.x & (CG_WAVE - 1);
  const int wave = threadIdx.x / CG_WAVE;
  const int nw = (blockDim.x + CG_WAVE - 1) / CG_WAVE;
  v = cg_wave_sum(v);
  __syncthreads();
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  T r = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < nw; ++w) r += scratch[w];
  return r;
}

// ---- VW consecutive floats (VW = 1, 2, 4; 4 * VW bytes aligned) memory <-> registers, unconditional ----------------
template <int VW>
__device__ __forceinline__ void cg_ldv(const float* p, float* v) {
  if constexpr (VW == 4) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  else if constexpr (VW == 2) { const float2 t = *reinterpret_cast<const float2*>(p); v[0] = t.x; v[1] = t.y; }
  else v[0] = *p;
}
template <int VW>
__device__ __forceinline__ void cg_stv(float* p, const float* v) {
  if constexpr (VW == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else if constexpr (VW == 2) *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  else *p = v[0];
}

// ---- n / d for a divisor known on the host, without the ~40-instruction 32-bit division -----------------------------
// magic = ceil(2^32 / d) (0 stands for d = 1), quotient = (n * magic) >> 32.  Exact while n * d < 2^32:
// magic * d = 2^32 + e with 0 <= e < d, so n * magic / 2^32 = n / d + n * e / (d * 2^32); the fractional part of n / d is at most
// (d - 1) / d, the floor is therefore the quotient as long as n * e / (d * 2^32) < 1 / d, i.e. n * e < 2^32 - and e < d.
// Every launcher that hands a magic number to a kernel bounds n and d by its geometry limits (DESIGN.md section 4 lists them).
static inline unsigned cg_div_magic(int d) { return d > 1 ? (unsigned)((0x100000000ULL + d - 1) / d) : 0u; }
__device__ __forceinline__ unsigned cg_div(unsigned n, unsigned magic) { return magic ? (unsigned)(((unsigned long long)n * magic) >> 32) : n; }
// the same without the d = 1 case, for divisors the launcher guarantees to be >= 2 (magic != 0): no select in a streaming loop
__device__ __forceinline__ unsigned cg_div_ge2(unsigned n, unsigned magic) { return (unsigned)(((unsigned long long)n * magic) >> 32); }

// ---- lane exchange inside a row of 16 lanes on the VALU (DPP), no LDS round trip -----------------------------------------------
// CTRL: 0x100 + n row_shl (lane i takes lane i + n), 0x110 + n row_shr (lane i takes lane i - n), 0x120 + n row_ror (rotation).
// A lane whose source falls outside its row keeps `old`.
template <int CTRL>
__device__ __forceinline__ float cg_dpp(float old, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ int cg_dpp(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false); }
// sum over the 16 lanes of a row, in every lane of the row
__device__ __forceinline__ float cg_row16_sum(float v) {
  v += cg_dpp<0x128>(0.f, v); v += cg_dpp<0x124>(0.f, v); v += cg_dpp<0x122>(0.f, v); v += cg_dpp<0x121>(0.f, v);
  return v;
}
// the same in f64 (BatchNorm channel sums are kept in f64 end to end: the variance is formed as E[x^2] - E[x]^2): the two 32-bit
// halves travel through the DPP rotation, the additions are f64
template <int CTRL>
__device__ __forceinline__ double cg_dpp_f64(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const int lo = cg_dpp<CTRL>(0, (int)(unsigned)(u & 0xFFFFFFFFull)), hi = cg_dpp<CTRL>(0, (int)(unsigned)(u >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}
__device__ __forceinline__ double cg_row16_sum(double v) {
  v += cg_dpp_f64<0x128>(v); v += cg_dpp_f64<0x124>(v); v += cg_dpp_f64<0x122>(v); v += cg_dpp_f64<0x121>(v);
  return v;
}

// the gradient of a shared PReLU slope: sum of its CG_ALPHA_SLOTS partial sums (cistgcn_hip.h), in slot order
__device__ __forceinline__ double cg_alpha_sum(const double* slots) {
  double s = 0.0;
  for (int i = 0; i < CG_ALPHA_SLOTS; ++i) s += slots[i];
  return s;
}

// ---- counter-based RNG for dropout: splitmix64 of (seed, site salt, index of a quad of elements) ---------------
// Dropout keep-scale: 0 (dropped) or 1/(1-p).  One 64-bit hash serves four consecutive elements (16 bits each), so
// the vectorised row kernels draw once per float4; the scalar path derives the same bits from (idx >> 2, idx & 3).
// The drop probability is therefore quantised to 1/65536.
__device__ __forceinline__ unsigned long long cg_drop_bits(unsigned long long seed, unsigned int salt, unsigned long long quad) {
  unsigned long long z = quad + seed * 0x9E3779B97F4A7C15ull + ((unsigned long long)salt << 40) + 0x632BE59BD9B4E019ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ float cg_drop_pick(unsigned long long bits, int j, float p) {
  const uint32_t thr = (uint32_t)(p * 65536.0f);
  return ((uint32_t)(bits >> (16 * j)) & 0xFFFFu) >= thr ? 1.0f / (1.0f - p) : 0.0f;
}
__device__ __forceinline__ float cg_drop_scale(float p, unsigned long long seed, unsigned int salt, unsigned long long idx) {
  return cg_drop_pick(cg_drop_bits(seed, salt, idx >> 2), (int)(idx & 3), p);
}
