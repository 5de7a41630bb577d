// Evaluation metrics of a batch (environment/test.py::Metrics.compute :65-94 of the reference with losses/losses.py: mpjpe :50-61,
// weighted_mpjpe :64-76, pa_mpjpe :79-144, n_mpjpe :147-160, mean_velocity_error :163-177, bone_length_error :199-215,
// weighted_bone_length_error :218-238) - nine metrics of pred / target (B,To,J,3) in one pass, without a host round trip:
//   cg_em_batch_max_kernel   max over the batch of (sn[b,t,j] + w_t), the denominator of `w_joints_t` (test.py:67-70)
//   cg_eval_metrics_kernel   one wavefront per (b,t) frame, one lane per joint: every sum over the joints of a frame (centroids,
//                            norms, the 3x3 correlation of the Procrustes fit, the scale of n_mpjpe) is a wave reduction, no barrier
//   cg_em_frames_kernel      `frames` mode only: the per-(b,t) sums over joints are added over b in a fixed order
// A frame is at most 64 joints x 3 floats; what a lane holds is widened to fp64 once and rounded to fp32 once, at the store, so the
// distance to an fp64 evaluation is the final rounding.  Nothing is accumulated with floating-point atomics: two calls give the same
// bits.  Neither pred, target nor speeds is written (the reference divides `speeds` in place, test.py:67).
#include "eval_frame.h"

#include <math.h>

#define CG_EM_THREADS 256
#define CG_EM_WAVES (CG_EM_THREADS / CG_WAVE)
#define CG_EM_PRE_THREADS 1024
#define CG_EM_PRE_WAVES (CG_EM_PRE_THREADS / CG_WAVE)
#define CG_EM_SUMS 7

// order of CgEvalMetrics.out (the list in include/cistgcn_hip.h, EVAL_METRICS of cistgcn_amd/ops.py)
enum { CG_EM_MPJPE = 0, CG_EM_PA, CG_EM_N, CG_EM_MVE, CG_EM_W, CG_EM_BONE, CG_EM_WBONE, CG_EM_WJ, CG_EM_WJT };
// the per-frame sums `frames` mode keeps: w_mpjpe and w_bone_l are w_t times the sums of mpjpe and bone_l
enum { CG_EM_S_E = 0, CG_EM_S_PA, CG_EM_S_N, CG_EM_S_MVE, CG_EM_S_BONE, CG_EM_S_WJ, CG_EM_S_WJT };

// w_t = (t + 1) / To in fp32, as `arange(1, To + 1) / To` gives it (test.py:301-302)
__device__ __forceinline__ double cg_em_wt(int t, int To) { return (double)((float)(t + 1) / (float)To); }

// sn + w_t of one joint: sn = speeds / (max over the joints of the frame + 1e-6) (test.py:67-69)
__device__ __forceinline__ double cg_em_sn(float s, float frame_max) { return (double)s / ((double)frame_max + 1e-6); }

// ---------------------------------------------------------------------------------------------
// bmax[t,j] = max_b (sn[b,t,j] + w_t): one workgroup per frame index t, its waves stride over the samples
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CG_EM_PRE_THREADS) void cg_em_batch_max_kernel(const float* __restrict__ speeds, double* __restrict__ bmax, int B,
                                                                            int To, int J) {
  __shared__ double red[CG_EM_PRE_WAVES][CG_WAVE];
  const int lane = threadIdx.x & (CG_WAVE - 1), wave = threadIdx.x / CG_WAVE;
  for (int t = blockIdx.x; t < To; t += gridDim.x) {
    const double wt = cg_em_wt(t, To);
    double m = -INFINITY;
    for (int b = wave; b < B; b += CG_EM_PRE_WAVES) {       // wave-uniform trip count: the shuffle below has all 64 lanes
      const float s = lane < J ? speeds[((long long)b * To + t) * J + lane] : -INFINITY;
      const float mx = cg_wave_allmax(s);
      m = fmax(m, cg_em_sn(s, mx) + wt);
    }
    red[wave][lane] = m;
    __syncthreads();
    if (wave == 0 && lane < J) {
      for (int w = 1; w < CG_EM_PRE_WAVES; ++w) m = fmax(m, red[w][lane]);
      bmax[(long long)t * J + lane] = m;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// the main pass: wave w of workgroup g takes frames g * CG_EM_WAVES + w, + gridDim.x * CG_EM_WAVES, ...
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CG_EM_THREADS) void cg_eval_metrics_kernel(CgEvalMetrics a) {
  const int lane = threadIdx.x & (CG_WAVE - 1), wave = threadIdx.x / CG_WAVE;
  const int J = a.J, To = a.To, Nb = a.Nb;
  const long long F = (long long)a.B * To;
  const bool on = lane < J;
  const double* bmax = a.ws;
  double* part = a.ws + (long long)To * J;
  for (long long f = (long long)blockIdx.x * CG_EM_WAVES + wave; f < F; f += (long long)gridDim.x * CG_EM_WAVES) {      // wave-uniform
    const int t = (int)(f % To);
    const long long b = f / To;
    const double wt = cg_em_wt(t, To);
    const bool vel = t < To - 1;
    const float* pf = a.pred + f * J * 3;
    const float* xf = a.target + f * J * 3;
    double P[3] = {0.0, 0.0, 0.0}, X[3] = {0.0, 0.0, 0.0}, mve = 0.0;
    float sp = -INFINITY;
    if (on) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { P[c] = (double)pf[lane * 3 + c]; X[c] = (double)xf[lane * 3 + c]; }
      sp = a.speeds[f * J + lane];
      if (vel) {
        double d[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = ((double)pf[(J + lane) * 3 + c] - P[c]) - ((double)xf[(J + lane) * 3 + c] - X[c]);
        mve = cg_em_norm3(d[0], d[1], d[2]);
      }
    }
    double e, en, epa;
    cg_em_frame_errors(P, X, on, J, e, en, epa);

    // the speed weights
    const float smax = cg_wave_allmax(sp);
    double wj = 0.0, wjt = 0.0;
    if (on) {
      const double sn = cg_em_sn(sp, smax);
      wj = sn * e;
      wjt = (sn + wt) / bmax[(long long)t * J + lane] * e;
    }

    // bones: lane k takes bones k, k + 64, ...
    double bsum = 0.0;
    for (int k = lane; k < Nb; k += CG_WAVE) {
      const int i = a.bones[2 * k], j = a.bones[2 * k + 1];
      double v = 0.0;
      if ((unsigned)i < (unsigned)J && (unsigned)j < (unsigned)J) {      // the operator refuses other indices; never read past the frame
        const double lp = cg_em_norm3((double)pf[3 * i] - (double)pf[3 * j], (double)pf[3 * i + 1] - (double)pf[3 * j + 1], (double)pf[3 * i + 2] - (double)pf[3 * j + 2]);
        const double lx = cg_em_norm3((double)xf[3 * i] - (double)xf[3 * j], (double)xf[3 * i + 1] - (double)xf[3 * j + 1], (double)xf[3 * i + 2] - (double)xf[3 * j + 2]);
        v = fabs(lp - lx);
      }
      if (!a.frames) {
        a.out[CG_EM_BONE][f * Nb + k] = (float)v;
        a.out[CG_EM_WBONE][f * Nb + k] = (float)(wt * v);
      }
      bsum += v;
    }

    if (a.frames) {
      double r3[CG_EM_SUMS] = {on ? e : 0.0, on ? epa : 0.0, on ? en : 0.0, mve, bsum, wj, wjt};
      cg_wave_allsum(r3);
      if (lane < CG_EM_SUMS) {
        double v = r3[0];
#pragma unroll
        for (int m = 1; m < CG_EM_SUMS; ++m) v = lane == m ? r3[m] : v;
        part[((long long)lane * a.B + b) * To + t] = v;
      }
    } else if (on) {
      const long long o = f * J + lane;
      a.out[CG_EM_MPJPE][o] = (float)e;
      a.out[CG_EM_PA][o] = (float)epa;
      a.out[CG_EM_N][o] = (float)en;
      a.out[CG_EM_W][o] = (float)(wt * e);
      a.out[CG_EM_WJ][o] = (float)wj;
      a.out[CG_EM_WJT][o] = (float)wjt;
      if (vel) a.out[CG_EM_MVE][(b * (To - 1) + t) * J + lane] = (float)mve;
    }
  }
}

// out[q][t] = mean over samples and joints (bones): one wave per (q,t); lane l adds samples l, l + 64, ... in order, then the
// lanes are added in the fixed tree of cg_wave_sum
__global__ __launch_bounds__(CG_EM_THREADS) void cg_em_frames_kernel(CgEvalMetrics a) {
  const int lane = threadIdx.x & (CG_WAVE - 1), wave = threadIdx.x / CG_WAVE;
  const int To = a.To, B = a.B;
  const double* part = a.ws + (long long)To * a.J;
  const long long U = (long long)CG_EM_METRICS * To;
  for (long long u = (long long)blockIdx.x * CG_EM_WAVES + wave; u < U; u += (long long)gridDim.x * CG_EM_WAVES) {
    const int q = (int)(u / To), t = (int)(u % To);
    if (q == CG_EM_MVE && t == To - 1) continue;      // wave-uniform
    const int m = q == CG_EM_MPJPE || q == CG_EM_W ? CG_EM_S_E : q == CG_EM_PA ? CG_EM_S_PA : q == CG_EM_N ? CG_EM_S_N : q == CG_EM_MVE ? CG_EM_S_MVE
                : q == CG_EM_BONE || q == CG_EM_WBONE ? CG_EM_S_BONE : q == CG_EM_WJ ? CG_EM_S_WJ : CG_EM_S_WJT;
    double s = 0.0;
    for (int b = lane; b < B; b += CG_WAVE) s += part[((long long)m * B + b) * To + t];
    s = cg_wave_sum(s);
    if (lane == 0) {
      const bool bone = q == CG_EM_BONE || q == CG_EM_WBONE;
      double v = s / ((double)B * (double)(bone ? a.Nb : a.J));
      if (q == CG_EM_W || q == CG_EM_WBONE) v *= cg_em_wt(t, To);
      a.out[q][t] = (float)v;
    }
  }
}

extern "C" long long cg_eval_metrics_ws_doubles(int B, int To, int J) {
  if (B < 1 || To < 2 || J < 1 || J > CG_WAVE) return 0;
  return (long long)To * J + (long long)CG_EM_SUMS * B * To;
}

extern "C" int cg_eval_metrics(const CgEvalMetrics* a, void* stream_) {
  if (!a || !a->pred || !a->target || !a->speeds || !a->bones || !a->ws) return CG_EARG;
  for (int q = 0; q < CG_EM_METRICS; ++q)
    if (!a->out[q]) return CG_EARG;
  if (a->B < 1 || a->To < 2 || a->J < 1 || a->J > CG_WAVE || a->Nb < 1) return CG_ESHAPE;
  hipStream_t stream = (hipStream_t)stream_;
  const long long F = (long long)a->B * a->To;
  hipLaunchKernelGGL(cg_em_batch_max_kernel, dim3((unsigned)min(a->To, 4096)), dim3(CG_EM_PRE_THREADS), 0, stream, a->speeds, a->ws, a->B, a->To, a->J);
  const long long groups = (F + CG_EM_WAVES - 1) / CG_EM_WAVES;
  hipLaunchKernelGGL(cg_eval_metrics_kernel, dim3((unsigned)min(groups, 16384LL)), dim3(CG_EM_THREADS), 0, stream, *a);
  if (a->frames) {
    const long long fg = ((long long)CG_EM_METRICS * a->To + CG_EM_WAVES - 1) / CG_EM_WAVES;
    hipLaunchKernelGGL(cg_em_frames_kernel, dim3((unsigned)min(fg, 4096LL)), dim3(CG_EM_THREADS), 0, stream, *a);
  }
  return cg_launch_status();
}
