// Input-space attacks on the eval-mode model (environment/adversarial_attacks.py of the reference: FGSM :375-437, IFGSM :442-548,
// MIFGSM :553-665) - everything an attack iteration does around the model call, without a host round trip:
//   cg_mpjpe_sample_fwd / _bwd   losses.mpjpe(reduce_axis=[1,2]) (losses/losses.py:50-61 as called at :175-178) and its adjoint with
//                                one upstream weight per sample (the fixed-shape form of the `[op_mask]` re-slicing of :518-521)
//   cg_attack_step               compute_gradient (:401-417, :469-496, :581-610) + the early-stop bookkeeping (:517, :529-538)
//   cg_deepfool_step             DEEPFOOL's compute_gradient (:697-717) + the same bookkeeping (:755-767)
// One workgroup per sample everywhere: a sample is T*V*3 floats (15 KB at T=50, V=25), its three reductions (y extent, |grad|_1,
// max |x_adv - x0|) never leave the workgroup, nothing is accumulated with floating-point atomics and every result is
// bit-reproducible from run to run (the bookkeeping compares losses with `>`).
#include "cg_common.h"

#include <limits.h>
#include <math.h>

#define CG_ATTACK_THREADS 256
#define CG_ATTACK_FGSM 0
#define CG_ATTACK_IFGSM 1
#define CG_ATTACK_MIFGSM 2

HIP_DYNAMIC_SHARED(unsigned char, cg_dyn_lds)

// ---------------------------------------------------------------------------------------------
// per-sample MPJPE: loss[b] = mean over the N = To*V joints of sample b of ||pred - target||_2
// ---------------------------------------------------------------------------------------------
__global__ void cg_mpjpe_sample_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, float* __restrict__ loss, int N) {
  __shared__ double red[16];
  const float* p = pred + (long long)blockIdx.x * N * 3;
  const float* t = tgt + (long long)blockIdx.x * N * 3;
  double s = 0.0;
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const float a = p[3 * i] - t[3 * i], b = p[3 * i + 1] - t[3 * i + 1], c = p[3 * i + 2] - t[3 * i + 2];
    s += (double)sqrtf(a * a + b * b + c * c);
  }
  s = cg_block_sum(s, red);       // fixed order: lanes, then waves
  if (threadIdx.x == 0) loss[blockIdx.x] = (float)(s / (double)N);
}

// dpred[b,i,:] = w[b] * (pred - target) / (N * ||pred - target||), 0 where the norm is 0.  grid (ceil(N / 256), B)
__global__ void cg_mpjpe_sample_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, const float* __restrict__ w,
                                           float* __restrict__ dpred, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const long long o = ((long long)blockIdx.y * N + i) * 3;
  const float a = pred[o] - tgt[o], b = pred[o + 1] - tgt[o + 1], c = pred[o + 2] - tgt[o + 2];
  const float n = sqrtf(a * a + b * b + c * c);
  const float k = n > 0.f ? w[blockIdx.y] / ((float)N * n) : 0.f;
  dpred[o] = a * k; dpred[o + 1] = b * k; dpred[o + 2] = c * k;
}

extern "C" int cg_mpjpe_sample_fwd(const float* pred, const float* tgt, float* loss, int B, int N, void* stream_) {
  if (!pred || !tgt || !loss) return CG_EARG;
  if (B <= 0 || N <= 0) return CG_ESHAPE;
  hipLaunchKernelGGL(cg_mpjpe_sample_fwd_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream_, pred, tgt, loss, N);
  return cg_launch_status();
}

extern "C" int cg_mpjpe_sample_bwd(const float* pred, const float* tgt, const float* w, float* dpred, int B, int N, void* stream_) {
  if (!pred || !tgt || !w || !dpred) return CG_EARG;
  if (B <= 0 || N <= 0 || B > 65535) return CG_ESHAPE;
  hipLaunchKernelGGL(cg_mpjpe_sample_bwd_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream_, pred, tgt, w,
                     dpred, N);
  return cg_launch_status();
}

// ---------------------------------------------------------------------------------------------
// the attack step (argument block CgAttackStep: include/cistgcn_hip.h)
// ---------------------------------------------------------------------------------------------
struct CgOpMin { __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); } };
struct CgOpMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct CgOpAdd { __device__ __forceinline__ double operator()(double a, double b) const { return a + b; } };

// Reduction over the workgroup in a fixed order, result in every thread.  `scratch`: one T per wave.  Two barriers.
template <typename T, typename Op>
__device__ __forceinline__ T cg_attack_reduce(T v, T* scratch, Op op) {
#pragma unroll
  for (int off = CG_WAVE / 2; off > 0; off >>= 1) v = op(v, __shfl_down(v, off, CG_WAVE));
  __syncthreads();
  if ((threadIdx.x & (CG_WAVE - 1)) == 0) scratch[threadIdx.x / CG_WAVE] = v;
  __syncthreads();
  T r = scratch[0];
  for (int k = 1; k < CG_ATTACK_THREADS / CG_WAVE; ++k) r = op(r, scratch[k]);
  return r;
}

__device__ __forceinline__ float cg_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// Dynamic LDS (floats): x[n] | x0[n] | d[n], n = T*V*3.  Every operand is read from memory once, every result written once.
// The roundings are those of the reference's fp32 tensor expressions: eps_b, the step alpha and the two edges of the box are each
// rounded on their own (they pass through LDS / a variable of their own, never through a fused multiply-add with another factor).
__global__ __launch_bounds__(CG_ATTACK_THREADS) void cg_attack_step_kernel(CgAttackStep a) {
  __shared__ float redf[CG_ATTACK_THREADS / CG_WAVE];
  __shared__ double redd[CG_ATTACK_THREADS / CG_WAVE];
  __shared__ float eps_sh;
  const int n = a.T * a.V * 3, b = blockIdx.x, tid = threadIdx.x;
  float* xs = reinterpret_cast<float*>(cg_dyn_lds);
  float* x0s = xs + n;
  float* ds = x0s + n;
  const long long base = (long long)b * n;
  const bool iter = a.mode != CG_ATTACK_FGSM;
  const bool act = iter ? a.active[b] != 0 : true;      // at the START of this iteration; thread 0 rewrites it behind several barriers
  int k = 0;
  if (iter) {
    // The reference leaves its loop once no sample is active (:540-541), so a step that starts with every sample frozen must change
    // nothing, not even through the reset.  Other workgroups of THIS launch may already have frozen their samples, so "active at the
    // start of step k" is read as frozen_at >= k, which a freeze during step k (frozen_at = k) does not change.
    k = a.steps[b];
    float alive = 0.f;
    for (int c = tid; c < a.B; c += CG_ATTACK_THREADS) alive = fmaxf(alive, a.frozen_at[c] >= k ? 1.f : 0.f);
    alive = cg_attack_reduce(alive, redf, CgOpMax());
    if (tid == 0) a.steps[b] = k + 1;
    if (alive == 0.f) return;
  }

  float lo = INFINITY, hi = -INFINITY;
  double l1 = 0.0;
  for (int i = tid; i < n; i += CG_ATTACK_THREADS) {
    const float xv = a.x[base + i];
    xs[i] = xv;
    x0s[i] = a.x0[base + i];
    if (i % 3 == 1) { lo = fminf(lo, xv); hi = fmaxf(hi, xv); }
    float gv = 0.f;
    if (act) { gv = a.grad[base + i]; l1 += (double)fabsf(gv); }
    ds[i] = gv;
  }
  lo = cg_attack_reduce(lo, redf, CgOpMin());
  hi = cg_attack_reduce(hi, redf, CgOpMax());
  if (tid == 0) eps_sh = a.epsilon * fabsf(hi - lo);      // eps_b = epsilon * len_y of the CURRENT iterate (:348-350, :471)
  float norm1 = 0.f;
  if (a.mode == CG_ATTACK_MIFGSM) norm1 = (float)cg_attack_reduce(l1, redd, CgOpAdd());
  __syncthreads();
  const float eps = eps_sh;
  const float alpha = iter ? eps / (float)a.iterations : eps;

  float far = 0.f;
  const bool move = act && !(a.mode == CG_ATTACK_MIFGSM && !(norm1 > 0.f));      // an all-zero gradient leaves g and x as they are
  for (int i = tid; i < n; i += CG_ATTACK_THREADS) {
    float xv = xs[i];
    if (move) {
      float d = ds[i];
      if (a.mode == CG_ATTACK_MIFGSM) {
        const float q = d / norm1;
        const float m = a.mu * a.g[base + i];
        d = m + q;
        a.g[base + i] = d;
      }
      const float m = a.mask ? a.mask[i / 3] : 1.f;
      const float r = m * (alpha * cg_sign(d));
      xv = xv + r;
      xs[i] = xv;
    }
    far = fmaxf(far, fabsf(xv - x0s[i]));
  }
  if (iter) far = cg_attack_reduce(far, redf, CgOpMax());
  // the reference's "projection" (:486-493): a RESET to x0 of what left [x0 - eps, x0 + eps), for every sample, frozen ones included
  const bool reset = iter && far > eps;
  for (int i = tid; i < n; i += CG_ATTACK_THREADS) {
    float xv = xs[i];
    if (reset) {
      const float o = x0s[i];
      const float lower = o - eps, upper = o + eps;
      if (xv < lower || xv >= upper) xv = o;
    }
    a.x[base + i] = xv;
  }

  if (iter && act && tid == 0) {       // bookkeeping with the loss of THIS iteration; it takes effect from the next one on
    a.queries[b] += 1;
    const float l = a.loss[b];
    int st = a.stall[b];
    if (l > a.best[b]) a.best[b] = l;
    else a.stall[b] = ++st;
    const bool freeze = st >= a.patience;
    a.w[b] = freeze ? 0.f : 1.f / (float)a.B;
    if (freeze) {
      a.active[b] = 0;
      a.frozen_at[b] = k;
      atomicAdd(a.n_active, -1);
    }
  }
}

extern "C" long long cg_attack_step_max_floats() { return (long long)((160 * 1024 - 256) / (3 * sizeof(float))); }      // 256 bytes of static LDS beside the sample

extern "C" int cg_attack_step(const CgAttackStep* a, void* stream_) {
  if (!a || !a->x0 || !a->x || !a->grad) return CG_EARG;
  if (a->mode < CG_ATTACK_FGSM || a->mode > CG_ATTACK_MIFGSM) return CG_EARG;
  if (a->mode == CG_ATTACK_MIFGSM && !a->g) return CG_EARG;
  if (a->mode != CG_ATTACK_FGSM && (!a->loss || !a->best || !a->stall || !a->active || !a->w || !a->queries || !a->n_active || !a->steps || !a->frozen_at)) return CG_EARG;
  if (a->B <= 0 || a->T <= 0 || a->V <= 0 || a->iterations <= 0 || a->patience <= 0) return CG_ESHAPE;
  const long long n = (long long)a->T * a->V * 3;
  if (n > cg_attack_step_max_floats()) return CG_ESHAPE;
  const size_t lds = (size_t)n * 3 * sizeof(float);
  if (cg_lds_limit((const void*)cg_attack_step_kernel, lds) != hipSuccess) return CG_ESHAPE;
  hipLaunchKernelGGL(cg_attack_step_kernel, dim3((unsigned)a->B), dim3(CG_ATTACK_THREADS), lds, (hipStream_t)stream_, *a);
  return cg_launch_status();
}

// ---------------------------------------------------------------------------------------------
// the DeepFool step (DEEPFOOL.compute_gradient, :697-717): x += mask * r,  r = -grad * mean_t(pred) / (||grad||_1 + 1e-10)
// (argument block CgDeepfoolStep: include/cistgcn_hip.h)
// ---------------------------------------------------------------------------------------------
// The To-means of the prediction's V*3 columns stay in LDS (f64) up to this many columns; a wider skeleton re-reads its column in
// every element, in the same order, so the two paths give the same bits.  Half the default dynamic LDS: no driver call to raise it.
#define CG_DEEPFOOL_LDS_COLS (CG_LDS_DEFAULT / 2 / (int)sizeof(double))

__device__ __forceinline__ double cg_deepfool_col_mean(const float* pred, int c, int cols, int To) {
  double s = 0.0;
  for (int t = 0; t < To; ++t) s += (double)pred[(long long)t * cols + c];
  return s / (double)To;
}

// The L1 norm and the column means are accumulated in f64 in a fixed order (lanes, then waves; frames in order); r is rounded to
// fp32 once and added once.  An element that does not move (frozen sample, mask 0, r = 0) is not written.
__global__ __launch_bounds__(CG_ATTACK_THREADS) void cg_deepfool_step_kernel(CgDeepfoolStep a, int staged) {
  __shared__ double redd[CG_ATTACK_THREADS / CG_WAVE];
  const int b = blockIdx.x, tid = threadIdx.x, cols = a.V * 3;
  const long long n = (long long)a.T * cols;
  const bool book = a.loss != nullptr;
  const bool act = book ? a.active[b] != 0 : true;      // at the START of this iteration; thread 0 rewrites it behind several barriers
  // A frozen sample is left alone entirely (there is no reset here), so a launch that starts with every sample frozen changes nothing
  // without the frozen_at >= k census of cg_attack_step_kernel; steps / frozen_at are kept up for the state's other users.
  if (!act) {
    if (tid == 0) a.steps[b] += 1;
    return;
  }

  const float* g = a.grad + (long long)b * n;
  const float* p = a.pred + (long long)b * a.To * cols;
  float* x = a.x + (long long)b * n;
  double* pm = reinterpret_cast<double*>(cg_dyn_lds);
  double l1 = 0.0;
  for (long long i = tid; i < n; i += CG_ATTACK_THREADS) l1 += (double)fabsf(g[i]);
  if (staged)
    for (int c = tid; c < cols; c += CG_ATTACK_THREADS) pm[c] = cg_deepfool_col_mean(p, c, cols, a.To);
  const double norm1 = cg_attack_reduce(l1, redd, CgOpAdd()) + 1e-10;      // its barriers also publish pm
  for (long long i = tid; i < n; i += CG_ATTACK_THREADS) {
    const float m = a.mask ? a.mask[i / 3] : 1.f;
    if (m == 0.f) continue;
    const int c = (int)(i % cols);
    const double mean = staged ? pm[c] : cg_deepfool_col_mean(p, c, cols, a.To);
    const float r = (float)(-((double)g[i] * mean) / norm1);      // an all-zero gradient: 0 / 1e-10 = 0, not NaN
    if (r != 0.f) x[i] = x[i] + m * r;
  }

  if (book && tid == 0) {       // the bookkeeping of cg_attack_step_kernel (:755-767 repeat :529-538)
    const int k = a.steps[b];
    a.steps[b] = k + 1;
    a.queries[b] += 1;
    const float l = a.loss[b];
    int st = a.stall[b];
    if (l > a.best[b]) a.best[b] = l;
    else a.stall[b] = ++st;
    const bool freeze = st >= a.patience;
    a.w[b] = freeze ? 0.f : 1.f / (float)a.B;
    if (freeze) {
      a.active[b] = 0;
      a.frozen_at[b] = k;
      atomicAdd(a.n_active, -1);
    }
  }
}

extern "C" int cg_deepfool_step(const CgDeepfoolStep* a, void* stream_) {
  if (!a || !a->x || !a->grad || !a->pred) return CG_EARG;
  const int given = !!a->loss + !!a->best + !!a->stall + !!a->active + !!a->w + !!a->queries + !!a->n_active + !!a->steps + !!a->frozen_at;
  if (given != 0 && given != 9) return CG_EARG;
  if (a->B <= 0 || a->T <= 0 || a->To <= 0 || a->V <= 0 || (given && a->patience <= 0)) return CG_ESHAPE;
  if (a->V > INT_MAX / 3) return CG_ESHAPE;
  const int cols = a->V * 3, staged = cols <= CG_DEEPFOOL_LDS_COLS;
  hipLaunchKernelGGL(cg_deepfool_step_kernel, dim3((unsigned)a->B), dim3(CG_ATTACK_THREADS), staged ? (size_t)cols * sizeof(double) : 0,
                     (hipStream_t)stream_, *a, staged);
  return cg_launch_status();
}
