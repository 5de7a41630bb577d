// Training losses other than plain MPJPE: what get_loss (environment/train.py:15-43 of the reference) selects, with the per-batch
// weights of train.py:62-71 - losses/losses.py: weighted_mpjpe :64-76, mpjpe_soft :241-252, weighted_mpjpe_soft :255-267, rmpjpe :36-47.
// (include/cistgcn_hip.h: CgMotionLoss lists the kinds, the weight formula, the conventions and the two deviations.)
//   cg_motion_loss_fwd_kernel      one wavefront per (b,t) frame, lanes over the joints (V > 64 loops): the maximum of the frame's speeds
//                                  is a wave reduction, no LDS and no barrier per frame; the wave keeps its sum of w * e in f64 over all its
//                                  frames, the workgroup's sum goes to part[blockIdx.x]
//   cg_motion_loss_finish_kernel   one wavefront: lane l adds part[l], part[l + 64], ... in order, the lanes are added in the fixed tree
//                                  of cg_wave_sum; stores the mean and the loss (its square root for rmpjpe)
//   cg_motion_loss_bwd_kernel      the forward layout again (the frame maximum is recomputed, no (B,T,V) weight tensor is kept), writes dpred
// The traffic is a few megabytes at most (B*T*V joints x 24 .. 36 bytes): these kernels are bound by their launches, so the layout is the
// one that needs neither a barrier nor a second pass for the frame maximum.  The weight is formed in fp32 in the reference's order without
// contraction into fma, e in fp32 as cg_mpjpe_fwd_kernel forms it; products and sums from there on are f64.  Nothing is accumulated
// with floating-point atomics: two calls give the same bits.  No input is written.
#include "cg_common.h"

#include <math.h>

__device__ __forceinline__ bool cg_loss_weighted(int kind) { return kind == CG_LOSS_WEIGHTED_MPJPE || kind == CG_LOSS_WEIGHTED_MPJPE_SOFT; }
__device__ __forceinline__ bool cg_loss_soft(int kind) { return kind == CG_LOSS_MPJPE_SOFT || kind == CG_LOSS_WEIGHTED_MPJPE_SOFT; }

// SmoothL1 with beta = 1 (torch.nn.SmoothL1Loss(reduction="none"), losses.py:10) and its derivative
__device__ __forceinline__ float cg_smooth_l1(float d) { const float a = fabsf(d); return a < 1.f ? 0.5f * d * d : a - 0.5f; }
__device__ __forceinline__ float cg_smooth_l1_grad(float d) { return fabsf(d) < 1.f ? d : d > 0.f ? 1.f : -1.f; }

// maximum over the V speeds of a frame, in every lane (all 64 lanes of the wave call it)
__device__ __forceinline__ float cg_loss_frame_max(const float* __restrict__ sp, int V, int lane) {
  float m = -INFINITY;
  for (int v = lane; v < V; v += CG_WAVE) m = fmaxf(m, sp[v]);
  return cg_wave_allmax(m);
}

// w(b,t,v) of joint j = f * V + v of frame f = b * T + t: train.py:62 (the tiled table), :66 (speeds / (max + 1e-6)), :68 / :70
__device__ __forceinline__ float cg_loss_weight(const CgMotionLoss& a, long long j, int t, float smax) {
#pragma clang fp contract(off)
  float w = a.w_full ? a.w_full[j] : a.w_frame ? a.w_frame[t] : 0.f;
  if (a.speeds) {
    const float sn = a.speeds[j] / (smax + 1e-6f);
    w = w + sn * a.speed_factor;
  }
  return w;
}

// d = pred - target of a joint; for the soft kinds s_c = SmoothL1(d_c) in s, else s = d; returns e = |s|_2
__device__ __forceinline__ float cg_loss_error(const float* __restrict__ p, const float* __restrict__ x, bool soft, float (&d)[3], float (&s)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    d[c] = p[c] - x[c];
    s[c] = soft ? cg_smooth_l1(d[c]) : d[c];
  }
  return sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
}

__global__ __launch_bounds__(CG_LOSS_THREADS) void cg_motion_loss_fwd_kernel(CgMotionLoss a) {
  __shared__ double red[16];
  const int lane = threadIdx.x & (CG_WAVE - 1), wave = threadIdx.x / CG_WAVE;
  const int V = a.V, T = a.T;
  const long long F = (long long)a.B * T;
  const bool weighted = cg_loss_weighted(a.kind), soft = cg_loss_soft(a.kind);
  double sum = 0.0;
  for (long long f = (long long)blockIdx.x * CG_LOSS_WAVES + wave; f < F; f += (long long)gridDim.x * CG_LOSS_WAVES) {      // wave-uniform
    const int t = (int)(f % T);
    const float smax = weighted && a.speeds ? cg_loss_frame_max(a.speeds + f * V, V, lane) : 0.f;
    for (int v = lane; v < V; v += CG_WAVE) {
      const long long j = f * V + v;
      float d[3], s[3];
      const float e = cg_loss_error(a.pred + 3 * j, a.target + 3 * j, soft, d, s);
      sum += weighted ? (double)cg_loss_weight(a, j, t, smax) * (double)e : (double)e;
    }
  }
  sum = cg_block_sum(sum, red);
  if (threadIdx.x == 0) a.part[blockIdx.x] = sum;
}

__global__ __launch_bounds__(CG_WAVE) void cg_motion_loss_finish_kernel(const double* __restrict__ part, int n, double count, int kind,
                                                                       float* __restrict__ loss, float* __restrict__ mean) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += CG_WAVE) s += part[i];
  s = cg_wave_sum(s);
  if (threadIdx.x == 0) {
    const double m = s / count;
    mean[0] = (float)m;
    loss[0] = (float)(kind == CG_LOSS_RMPJPE ? sqrt(m) : m);
  }
}

__global__ __launch_bounds__(CG_LOSS_THREADS) void cg_motion_loss_bwd_kernel(CgMotionLoss a) {
  const int lane = threadIdx.x & (CG_WAVE - 1), wave = threadIdx.x / CG_WAVE;
  const int V = a.V, T = a.T;
  const long long F = (long long)a.B * T;
  const bool weighted = cg_loss_weighted(a.kind), soft = cg_loss_soft(a.kind);
  // d loss / d (w e) of every joint: g / N; rmpjpe: g / (2 sqrt(M) N), and 0 where torch has NaN (M = 0)
  double k0 = (double)a.gloss[0] / ((double)F * (double)V);
  if (a.kind == CG_LOSS_RMPJPE) {
    const float M = a.mean[0];
    k0 = M > 0.f ? k0 / (2.0 * sqrt((double)M)) : 0.0;
  }
  for (long long f = (long long)blockIdx.x * CG_LOSS_WAVES + wave; f < F; f += (long long)gridDim.x * CG_LOSS_WAVES) {      // wave-uniform
    const int t = (int)(f % T);
    const float smax = weighted && a.speeds ? cg_loss_frame_max(a.speeds + f * V, V, lane) : 0.f;
    for (int v = lane; v < V; v += CG_WAVE) {
      const long long j = f * V + v;
      float d[3], s[3];
      const float e = cg_loss_error(a.pred + 3 * j, a.target + 3 * j, soft, d, s);
      const double k = weighted ? k0 * (double)cg_loss_weight(a, j, t, smax) : k0;
      const float r = e > 0.f ? (float)(k / (double)e) : 0.f;       // the gradient of a norm at 0 is 0
#pragma unroll
      for (int c = 0; c < 3; ++c) a.dpred[3 * j + c] = e > 0.f ? (soft ? s[c] * cg_smooth_l1_grad(d[c]) : d[c]) * r : 0.f;
    }
  }
}

static int cg_motion_loss_check(const CgMotionLoss* a) {
  if (!a || !a->pred || !a->target) return CG_EARG;
  if (a->kind < CG_LOSS_WEIGHTED_MPJPE || a->kind > CG_LOSS_RMPJPE || a->B < 1 || a->T < 1 || a->V < 1) return CG_ESHAPE;
  const bool weighted = a->kind == CG_LOSS_WEIGHTED_MPJPE || a->kind == CG_LOSS_WEIGHTED_MPJPE_SOFT;
  if (weighted && !a->w_full && !a->w_frame && !a->speeds) return CG_EARG;
  return CG_OK;
}

static unsigned cg_motion_loss_blocks(const CgMotionLoss* a) {
  const long long groups = ((long long)a->B * a->T + CG_LOSS_WAVES - 1) / CG_LOSS_WAVES;
  return (unsigned)min(groups, (long long)CG_LOSS_MAX_BLOCKS);
}

extern "C" int cg_motion_loss_fwd(const CgMotionLoss* a, void* stream_) {
  const int st = cg_motion_loss_check(a);
  if (st != CG_OK) return st;
  if (!a->part || !a->loss || !a->mean) return CG_EARG;
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned blocks = cg_motion_loss_blocks(a);
  hipLaunchKernelGGL(cg_motion_loss_fwd_kernel, dim3(blocks), dim3(CG_LOSS_THREADS), 0, stream, *a);
  hipLaunchKernelGGL(cg_motion_loss_finish_kernel, dim3(1), dim3(CG_WAVE), 0, stream, (const double*)a->part, (int)blocks,
                     (double)a->B * (double)a->T * (double)a->V, a->kind, a->loss, a->mean);
  return cg_launch_status();
}

extern "C" int cg_motion_loss_bwd(const CgMotionLoss* a, void* stream_) {
  const int st = cg_motion_loss_check(a);
  if (st != CG_OK) return st;
  if (!a->gloss || !a->dpred || (a->kind == CG_LOSS_RMPJPE && !a->mean)) return CG_EARG;
  hipLaunchKernelGGL(cg_motion_loss_bwd_kernel, dim3(cg_motion_loss_blocks(a)), dim3(CG_LOSS_THREADS), 0, (hipStream_t)stream_, *a);
  return cg_launch_status();
}
