// Distortion metrics of an attacked batch (environment/adversarial_attacks.py::ComputeAttackMetrics._get_metrics :187-342 of the
// reference, called as `_get_metrics(adv_inputs, inputs)` at environment/test.py:205): how far adv (B,T,J,3) moved from orig (B,T,J,3),
// per sample, per frame and per joint, without a host round trip and without the reference's (J,T,B,B,3) tensor:
//   cg_am_frame_kernel    one wavefront per (b,t) frame, one lane per joint: |adv - orig|, its n_mpjpe / pa_mpjpe variants (eval_frame.h,
//                         adv is `predicted`, orig is `target`), the squared error, h[b,t,j] = min_j' |adv[b,t,j] - orig[b,t,j']| and, for
//                         the histogram ranges, the row maxima of both joint-to-joint distance matrices
//   cg_am_cross_kernel    one wavefront per (t,j) and 64 samples of adv, the samples of orig pass through LDS in tiles of 64:
//                         min_b' |adv[b,t,j] - orig[b',t,j]| (the "spatial" Hausdorff, :214,:218) and the sums of the cosine similarity
//                         along the batch axis (:209-210)
//   cg_am_range_kernel    the B + T + J histogram ranges: maxima of the row maxima (the minimum is the diagonal's exact 0)
//   cg_am_hist_kernel     the J x J distances of every frame once more, binned into the histograms of their sample, frame index and
//                         first joint (CustomKLD / CustomJSD / CustomKolmogorovSmirnovTest :55-103, convert_to_dists :39-48) in LDS;
//                         integer atomics only
//   cg_am_finish_kernel   every remaining sum, in a fixed order, and the 33 results
// A histogram count flips on the last bit of a distance, so the binned distances carry the reference's fp32 bits (cg_am_dist32);
// everything else is widened to fp64 once and rounded to fp32 once, at the store.  No floating-point atomics: two calls give the same
// bits.  Neither adv nor orig is written.
#include "eval_frame.h"

#define CG_AM_THREADS 256
#define CG_AM_WAVES (CG_AM_THREADS / CG_WAVE)
#define CG_AM_TILE CG_WAVE      // cross pass: samples of adv per wavefront and samples of orig per LDS tile
#define CG_AM_HB 8              // histogram pass: a workgroup bins a rectangle of CG_AM_HB samples x CG_AM_HT frame indices
#define CG_AM_HT 8
#define CG_AM_HIST_THREADS 512  // eight waves, eight frames of the rectangle each
#define CG_AM_HIST_WAVES (CG_AM_HIST_THREADS / CG_WAVE)
#define CG_AM_COS_EPS 1e-6      // nn.CosineSimilarity(eps=1e-6) (:155-156): each norm is clamped from below

// the (B,T,J) maps the per-joint ("spatial") means are taken from
enum { CG_AM_M_E = 0, CG_AM_M_N, CG_AM_M_PA, CG_AM_M_SE, CG_AM_MAPS };
// per (b,t) frame: sums over the joints (the maximum for HMAX); AO / AA / OO are adv.orig, adv.adv, orig.orig of the flattened frame
enum { CG_AM_S_E = 0, CG_AM_S_N, CG_AM_S_PA, CG_AM_S_SE, CG_AM_S_H, CG_AM_S_AO, CG_AM_S_AA, CG_AM_S_OO, CG_AM_S_HMAX, CG_AM_SUMS };
// per (chunk of 64 samples, t, j): sum and maximum of the cross-batch minima, the dot products along the batch axis per coordinate
enum { CG_AM_X_HSUM = 0, CG_AM_X_AO, CG_AM_X_AA = CG_AM_X_AO + 3, CG_AM_X_OO = CG_AM_X_AA + 3, CG_AM_X_HMAX = CG_AM_X_OO + 3, CG_AM_CROSS };
// order of a family's ten results: out[3 + 10 * family + q], family 0 temporal_*, 1 spatial_*, 2 *_sample; out[0..2] the scalars
enum { CG_AM_Q_E = 0, CG_AM_Q_N, CG_AM_Q_PA, CG_AM_Q_HMEAN, CG_AM_Q_HMAX, CG_AM_Q_MSE, CG_AM_Q_COS, CG_AM_Q_KLD, CG_AM_Q_JSD, CG_AM_Q_KS };

struct CgAmWs {
  double* map;      // [CG_AM_MAPS][B*T*J]
  double* fs;       // [CG_AM_SUMS][B*T]
  double* cp;       // [CG_AM_CROSS][chunks][T*J]
  float* rowmax;    // [B*T*J] max_j of d_adv[i,j] and d_orig[i,j]
  float* fmx;       // [B*T] maximum of the frame's row maxima
};

__host__ __device__ static inline long long cg_am_chunks(int B) { return ((long long)B + CG_AM_TILE - 1) / CG_AM_TILE; }

__host__ __device__ static inline long long cg_am_ws_layout(int B, int T, int J, double* base, CgAmWs* w) {
  const long long F = (long long)B * T, N = F * J;
  long long at = 0;
  w->map = base + at; at += CG_AM_MAPS * N;
  w->fs = base + at; at += CG_AM_SUMS * F;
  w->cp = base + at; at += CG_AM_CROSS * cg_am_chunks(B) * T * J;
  w->rowmax = (float*)(base + at);
  w->fmx = w->rowmax + N;
  at += (N + F + 1) / 2;
  return at;
}

// |p - q| with the reference's fp32 bits: sqrt(((dx*dx)+(dy*dy))+(dz*dz)), every operation rounded to fp32 and none contracted.  Each
// operation is done in fp64 on fp32 operands and rounded to fp32; with 53 >= 2 * 24 + 2 bits the double rounding is harmless for
// +, -, *, and the square root.
__device__ __forceinline__ float cg_am_dist32(const float* p, const float* q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float dx = (float)((double)p[0] - (double)q[0]), dy = (float)((double)p[1] - (double)q[1]), dz = (float)((double)p[2] - (double)q[2]);
  const float sx = (float)((double)dx * (double)dx), sy = (float)((double)dy * (double)dy), sz = (float)((double)dz * (double)dz);
  const float sxy = (float)((double)sx + (double)sy);
  const float s = (float)((double)sxy + (double)sz);
  return (float)sqrt((double)s);
}

// edge k of the 65 edges from 0 to mx: `linspace(0, 1, 65)[k] * mx` as one fp32 product (tensor_linspace :9-36; k / 64 is exact)
__device__ __forceinline__ float cg_am_edge(int k, float mx) { return ((float)k * 0.015625f) * mx; }

// bin of x in [0, mx]: the largest k with edge k <= x, the last edge inclusive (torch.histogram with a tensor of edges).
// per_mx = 64 / mx places a first guess: x * per_mx is within 2^-23 of the quotient and an edge within 2^-24 of k / 64 * mx, so the
// guess is at most two bins off and two steps either way, decided by the edges themselves, reach the bin.  The result is checked
// against its two edges; a range so small that 64 / mx overflows takes the scan.
__device__ __forceinline__ int cg_am_bin(float x, float mx, float per_mx) {
  if (!(mx > 0.f)) return CG_AM_BINS - 1;
  int k = (int)fminf(fmaxf(x * per_mx, 0.f), (float)(CG_AM_BINS - 1));
  k -= (k > 0 && cg_am_edge(k, mx) > x) ? 1 : 0;
  k -= (k > 0 && cg_am_edge(k, mx) > x) ? 1 : 0;
  k += (k < CG_AM_BINS - 1 && cg_am_edge(k + 1, mx) <= x) ? 1 : 0;
  k += (k < CG_AM_BINS - 1 && cg_am_edge(k + 1, mx) <= x) ? 1 : 0;
  if ((k > 0 && cg_am_edge(k, mx) > x) || (k < CG_AM_BINS - 1 && cg_am_edge(k + 1, mx) <= x)) {
    k = 0;
#pragma nounroll
    while (k < CG_AM_BINS - 1 && cg_am_edge(k + 1, mx) <= x) ++k;
  }
  return k;
}

// ---------------------------------------------------------------------------------------------
// frame pass: wave w of workgroup g takes frames g * CG_AM_WAVES + w, + gridDim.x * CG_AM_WAVES, ...
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CG_AM_THREADS) void cg_am_frame_kernel(CgAttackMetrics a) {
  const int lane = threadIdx.x & (CG_WAVE - 1), wave = threadIdx.x / CG_WAVE;
  const int J = a.J;
  const long long F = (long long)a.B * a.T, N = F * J;
  const bool on = lane < J;
  const int li = on ? lane : 0;      // idle lanes compute on joint 0 and store nothing
  CgAmWs w;
  cg_am_ws_layout(a.B, a.T, J, a.ws, &w);
  for (long long f = (long long)blockIdx.x * CG_AM_WAVES + wave; f < F; f += (long long)gridDim.x * CG_AM_WAVES) {      // wave-uniform
    const float* pf = a.adv + f * J * 3;
    const float* xf = a.orig + f * J * 3;
    double P[3] = {0.0, 0.0, 0.0}, X[3] = {0.0, 0.0, 0.0};
    if (on) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { P[c] = (double)pf[lane * 3 + c]; X[c] = (double)xf[lane * 3 + c]; }
    }
    double e, en, epa;
    cg_em_frame_errors(P, X, on, J, e, en, epa);
    const double d0 = P[0] - X[0], d1 = P[1] - X[1], d2 = P[2] - X[2];
    const double se = d0 * d0 + d1 * d1 + d2 * d2;
    double h2 = INFINITY;
    float rm = 0.f;
    const float ownp[3] = {pf[3 * li], pf[3 * li + 1], pf[3 * li + 2]}, ownx[3] = {xf[3 * li], xf[3 * li + 1], xf[3 * li + 2]};
    for (int j = 0; j < J; ++j) {      // every lane reads joint j of the frame: one address per wave
      const double q0 = P[0] - (double)xf[3 * j], q1 = P[1] - (double)xf[3 * j + 1], q2 = P[2] - (double)xf[3 * j + 2];
      h2 = fmin(h2, q0 * q0 + q1 * q1 + q2 * q2);
      rm = fmaxf(rm, fmaxf(cg_am_dist32(ownp, pf + 3 * j), cg_am_dist32(ownx, xf + 3 * j)));
    }
    const double h = on ? sqrt(h2) : 0.0;
    if (on) {
      const long long o = f * J + lane;
      w.map[CG_AM_M_E * N + o] = e;
      w.map[CG_AM_M_N * N + o] = en;
      w.map[CG_AM_M_PA * N + o] = epa;
      w.map[CG_AM_M_SE * N + o] = se;
      w.rowmax[o] = rm;
    }
    double r[CG_AM_SUMS - 1] = {on ? e : 0.0, on ? en : 0.0, on ? epa : 0.0, se, h, P[0] * X[0] + P[1] * X[1] + P[2] * X[2],
                                P[0] * P[0] + P[1] * P[1] + P[2] * P[2], X[0] * X[0] + X[1] * X[1] + X[2] * X[2]};
    cg_wave_allsum(r);
    const double hmax = cg_wave_allmax(h);
    const float fm = cg_wave_allmax(on ? rm : 0.f);
    if (lane < CG_AM_SUMS) {
      double v = hmax;
#pragma unroll
      for (int m = 0; m < CG_AM_SUMS - 1; ++m) v = lane == m ? r[m] : v;
      w.fs[lane * F + f] = v;
    }
    if (lane == 0) w.fmx[f] = fm;
  }
}

// ---------------------------------------------------------------------------------------------
// cross pass: workgroup (t * J + j, chunk) is one wavefront; lane l owns sample chunk * 64 + l of adv
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CG_AM_TILE) void cg_am_cross_kernel(CgAttackMetrics a) {
  __shared__ double tile[CG_AM_TILE * 3];
  const int lane = threadIdx.x, B = a.B;
  const long long TJ = (long long)a.T * a.J, u = blockIdx.x, chunk = blockIdx.y, chunks = cg_am_chunks(B);
  const long long b = chunk * CG_AM_TILE + lane;
  const bool on = b < B;
  CgAmWs w;
  cg_am_ws_layout(B, a.T, a.J, a.ws, &w);
  double P[3] = {0.0, 0.0, 0.0}, X[3] = {0.0, 0.0, 0.0};
  if (on) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { P[c] = (double)a.adv[(b * TJ + u) * 3 + c]; X[c] = (double)a.orig[(b * TJ + u) * 3 + c]; }
  }
  double h2 = INFINITY;
  for (long long b0 = 0; b0 < B; b0 += CG_AM_TILE) {
    const int n = (int)min((long long)CG_AM_TILE, B - b0);
    __syncthreads();
    if (lane < n) {
#pragma unroll
      for (int c = 0; c < 3; ++c) tile[lane * 3 + c] = (double)a.orig[((b0 + lane) * TJ + u) * 3 + c];
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {      // one LDS address per wave: a broadcast
      const double q0 = P[0] - tile[3 * k], q1 = P[1] - tile[3 * k + 1], q2 = P[2] - tile[3 * k + 2];
      h2 = fmin(h2, q0 * q0 + q1 * q1 + q2 * q2);
    }
  }
  const double h = on ? sqrt(h2) : 0.0;
  double r[CG_AM_CROSS - 1] = {h, P[0] * X[0], P[1] * X[1], P[2] * X[2], P[0] * P[0], P[1] * P[1], P[2] * P[2], X[0] * X[0], X[1] * X[1], X[2] * X[2]};
  cg_wave_allsum(r);
  const double hmax = cg_wave_allmax(h);
  if (lane < CG_AM_CROSS) {
    double v = hmax;
#pragma unroll
    for (int m = 0; m < CG_AM_CROSS - 1; ++m) v = lane == m ? r[m] : v;
    w.cp[(lane * chunks + chunk) * TJ + u] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// ranges: one wavefront per group (sample b, frame index t, first joint i); a maximum does not depend on the order
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CG_AM_THREADS) void cg_am_range_kernel(CgAttackMetrics a) {
  const int lane = threadIdx.x & (CG_WAVE - 1), wave = threadIdx.x / CG_WAVE;
  const int B = a.B, T = a.T, J = a.J, G = B + T + J;
  const long long F = (long long)B * T;
  CgAmWs w;
  cg_am_ws_layout(B, T, J, a.ws, &w);
  for (int g = blockIdx.x * CG_AM_WAVES + wave; g < G; g += gridDim.x * CG_AM_WAVES) {      // wave-uniform
    float m = 0.f;
    if (g < B) {
      for (int t = lane; t < T; t += CG_WAVE) m = fmaxf(m, w.fmx[(long long)g * T + t]);
    } else if (g < B + T) {
      for (int b = lane; b < B; b += CG_WAVE) m = fmaxf(m, w.fmx[(long long)b * T + (g - B)]);
    } else {
      for (long long f = lane; f < F; f += CG_WAVE) m = fmaxf(m, w.rowmax[f * J + (g - B - T)]);
    }
    m = cg_wave_allmax(m);
    if (lane == 0) a.gmax[g] = m;
  }
}

// ---------------------------------------------------------------------------------------------
// histogram pass: LDS holds [CG_AM_HB samples | CG_AM_HT frame indices | J joints][adv, orig][64 bins]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CG_AM_HIST_THREADS) void cg_am_hist_kernel(CgAttackMetrics a) {
  __shared__ int hist[(CG_AM_HB + CG_AM_HT + CG_WAVE) * 2 * CG_AM_BINS];
  __shared__ float pose[CG_AM_HIST_WAVES][2][CG_WAVE * 3];      // the frame a wave is binning: adv, orig
  __shared__ float jmax[CG_WAVE];                               // ranges of the per-joint histograms
  const int lane = threadIdx.x & (CG_WAVE - 1), wave = threadIdx.x / CG_WAVE;
  const int B = a.B, T = a.T, J = a.J;
  const int nbt = (T + CG_AM_HT - 1) / CG_AM_HT;
  const int b0 = (int)(blockIdx.x / nbt) * CG_AM_HB, t0 = (int)(blockIdx.x % nbt) * CG_AM_HT;
  const int nb = min(CG_AM_HB, B - b0), nt = min(CG_AM_HT, T - t0);
  const int used = (CG_AM_HB + CG_AM_HT + J) * 2 * CG_AM_BINS;
  for (int i = threadIdx.x; i < used; i += CG_AM_HIST_THREADS) hist[i] = 0;
  if (threadIdx.x < J) jmax[threadIdx.x] = a.gmax[B + T + threadIdx.x];
  const int frames = nb * nt, pairs = J * J;
  for (int base = 0; base < frames; base += CG_AM_HIST_WAVES) {      // the same trip count in every wave: barriers inside
    const int fr = base + wave;
    const bool live = fr < frames;      // wave-uniform
    const int bb = fr / nt, tt = fr % nt;
    __syncthreads();      // the histograms are zero / the previous frame of this wave has been read
    if (live && lane < J) {      // the frame goes through LDS once: a joint is then an LDS read instead of a global load per pair
      const long long f = (long long)(b0 + bb) * T + (t0 + tt);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pose[wave][0][lane * 3 + c] = a.adv[(f * J + lane) * 3 + c];
        pose[wave][1][lane * 3 + c] = a.orig[(f * J + lane) * 3 + c];
      }
    }
    __syncthreads();
    if (live) {
      const float mxs = a.gmax[b0 + bb], mxt = a.gmax[B + t0 + tt], pms = (float)CG_AM_BINS / mxs, pmt = (float)CG_AM_BINS / mxt;
      int* hs = hist + bb * 2 * CG_AM_BINS;
      int* ht = hist + (CG_AM_HB + tt) * 2 * CG_AM_BINS;
      for (int p = lane; p < pairs; p += CG_WAVE) {      // the J x J pairs of the frame over the 64 lanes
        const int i = p / J, j = p - i * J;
        const float mxi = jmax[i], pmi = (float)CG_AM_BINS / mxi;
        int* hi = hist + (CG_AM_HB + CG_AM_HT + i) * 2 * CG_AM_BINS;
        const float da = cg_am_dist32(&pose[wave][0][3 * i], &pose[wave][0][3 * j]), dx = cg_am_dist32(&pose[wave][1][3 * i], &pose[wave][1][3 * j]);
        atomicAdd(&hs[cg_am_bin(da, mxs, pms)], 1);
        atomicAdd(&ht[cg_am_bin(da, mxt, pmt)], 1);
        atomicAdd(&hi[cg_am_bin(da, mxi, pmi)], 1);
        atomicAdd(&hs[CG_AM_BINS + cg_am_bin(dx, mxs, pms)], 1);
        atomicAdd(&ht[CG_AM_BINS + cg_am_bin(dx, mxt, pmt)], 1);
        atomicAdd(&hi[CG_AM_BINS + cg_am_bin(dx, mxi, pmi)], 1);
      }
    }
  }
  __syncthreads();
  int32_t* cs = a.counts;
  int32_t* ct = cs + (long long)2 * B * CG_AM_BINS;
  int32_t* ci = ct + (long long)2 * T * CG_AM_BINS;
  for (int i = threadIdx.x; i < used; i += CG_AM_HIST_THREADS) {      // a wave flushes the 64 bins of one histogram: 256 contiguous bytes
    const int v = hist[i];
    if (v == 0) continue;
    const int g = i / (2 * CG_AM_BINS), s = (i / CG_AM_BINS) & 1, k = i % CG_AM_BINS;
    if (g < CG_AM_HB) {
      if (g < nb) atomicAdd(&cs[((long long)s * B + b0 + g) * CG_AM_BINS + k], v);
    } else if (g < CG_AM_HB + CG_AM_HT) {
      if (g - CG_AM_HB < nt) atomicAdd(&ct[((long long)s * T + t0 + g - CG_AM_HB) * CG_AM_BINS + k], v);
    } else {
      atomicAdd(&ci[((long long)s * J + g - CG_AM_HB - CG_AM_HT) * CG_AM_BINS + k], v);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// finish: workgroup u < T is frame index u, then J joints, then B samples, then the three scalars
// ---------------------------------------------------------------------------------------------
#define CG_AM_NS 8
// sums over the workgroup in a fixed order (the butterfly of each wave, then the waves in turn), result in every thread
__device__ __forceinline__ void cg_am_block_reduce(double (&s)[CG_AM_NS], double& m, double* red) {
  const int lane = threadIdx.x & (CG_WAVE - 1), wave = threadIdx.x / CG_WAVE;
  cg_wave_allsum(s);
  m = cg_wave_allmax(m);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < CG_AM_NS; ++i) red[wave * (CG_AM_NS + 1) + i] = s[i];
    red[wave * (CG_AM_NS + 1) + CG_AM_NS] = m;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CG_AM_NS; ++i) {
    double v = red[i];
    for (int k = 1; k < CG_AM_WAVES; ++k) v += red[k * (CG_AM_NS + 1) + i];
    s[i] = v;
  }
  m = red[CG_AM_NS];
  for (int k = 1; k < CG_AM_WAVES; ++k) m = fmax(m, red[k * (CG_AM_NS + 1) + CG_AM_NS]);
}

// cosine similarity along the batch axis at (t,j), coordinate c: the chunks of the cross pass are added in order
__device__ __forceinline__ double cg_am_batch_cos(const double* cp, long long chunks, long long TJ, long long tj, int c) {
  double ao = 0.0, aa = 0.0, oo = 0.0;
  for (long long k = 0; k < chunks; ++k) {
    ao += cp[((CG_AM_X_AO + c) * chunks + k) * TJ + tj];
    aa += cp[((CG_AM_X_AA + c) * chunks + k) * TJ + tj];
    oo += cp[((CG_AM_X_OO + c) * chunks + k) * TJ + tj];
  }
  return ao / (fmax(sqrt(aa), CG_AM_COS_EPS) * fmax(sqrt(oo), CG_AM_COS_EPS));
}

__global__ __launch_bounds__(CG_AM_THREADS) void cg_am_finish_kernel(CgAttackMetrics a) {
  __shared__ double red[CG_AM_WAVES * (CG_AM_NS + 1)];
  const int tid = threadIdx.x, lane = threadIdx.x & (CG_WAVE - 1), wave = threadIdx.x / CG_WAVE;
  const int B = a.B, T = a.T, J = a.J;
  const long long F = (long long)B * T, N = F * J, TJ = (long long)T * J, chunks = cg_am_chunks(B);
  CgAmWs w;
  cg_am_ws_layout(B, T, J, a.ws, &w);
  const int u = blockIdx.x;
  const int fam = u < T ? 0 : u < T + J ? 1 : u < T + J + B ? 2 : 3;
  const int g = fam == 0 ? u : fam == 1 ? u - T : u - T - J;
  double s[CG_AM_NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, m = 0.0;      // every maximum is over distances >= 0
  double den = 1.0, cos_den = 1.0;      // elements per mean
  long long hist_n = 0;                 // distances per histogram
  int hist_at = 0, hist_g = 1;          // first group of the family in counts / gmax, groups of the family
  if (fam == 0) {
    for (int b = tid; b < B; b += CG_AM_THREADS) {
      const long long f = (long long)b * T + g;
#pragma unroll
      for (int q = 0; q <= CG_AM_S_H; ++q) s[q] += w.fs[q * F + f];
      m = fmax(m, w.fs[CG_AM_S_HMAX * F + f]);
    }
    for (int i = tid; i < 3 * J; i += CG_AM_THREADS) s[5] += cg_am_batch_cos(w.cp, chunks, TJ, (long long)g * J + i / 3, i % 3);
    den = (double)B * J; cos_den = 3.0 * J;
    hist_n = (long long)B * J * J; hist_at = B; hist_g = T;
  } else if (fam == 1) {
    for (long long f = tid; f < F; f += CG_AM_THREADS) {
#pragma unroll
      for (int q = 0; q < CG_AM_MAPS; ++q) s[q] += w.map[q * N + f * J + g];
    }
    for (int t = tid; t < T; t += CG_AM_THREADS)
      for (long long k = 0; k < chunks; ++k) {
        s[4] += w.cp[(CG_AM_X_HSUM * chunks + k) * TJ + (long long)t * J + g];
        m = fmax(m, w.cp[(CG_AM_X_HMAX * chunks + k) * TJ + (long long)t * J + g]);
      }
    for (int i = tid; i < 3 * T; i += CG_AM_THREADS) s[5] += cg_am_batch_cos(w.cp, chunks, TJ, (long long)(i / 3) * J + g, i % 3);
    den = (double)F; cos_den = 3.0 * T;
    hist_n = F * J; hist_at = B + T; hist_g = J;
  } else if (fam == 2) {
    for (int t = tid; t < T; t += CG_AM_THREADS) {
      const long long f = (long long)g * T + t;
#pragma unroll
      for (int q = 0; q <= CG_AM_S_OO; ++q) s[q] += w.fs[q * F + f];
      m = fmax(m, w.fs[CG_AM_S_HMAX * F + f]);
    }
    den = (double)TJ;
    hist_n = TJ * J; hist_at = 0; hist_g = B;
  } else {
    for (long long f = tid; f < F; f += CG_AM_THREADS) {
#pragma unroll
      for (int q = 0; q <= CG_AM_S_PA; ++q) s[q] += w.fs[q * F + f];
    }
  }
  cg_am_block_reduce(s, m, red);
  if (fam == 3) {
    if (tid < 3) a.out[tid][0] = (float)((tid == 0 ? s[0] : tid == 1 ? s[1] : s[2]) / (double)N);
    return;
  }
  const int ob = 3 + 10 * fam;
  if (tid == 0) {
    a.out[ob + CG_AM_Q_E][g] = (float)(s[CG_AM_S_E] / den);
    a.out[ob + CG_AM_Q_N][g] = (float)(s[CG_AM_S_N] / den);
    a.out[ob + CG_AM_Q_PA][g] = (float)(s[CG_AM_S_PA] / den);
    a.out[ob + CG_AM_Q_MSE][g] = (float)(s[CG_AM_S_SE] / (3.0 * den));
    a.out[ob + CG_AM_Q_HMEAN][g] = (float)(s[CG_AM_S_H] / den);
    a.out[ob + CG_AM_Q_HMAX][g] = (float)m;
    // the sample's similarity is over its flattened poses (:207-208), the other two are means of the batch-axis similarity
    a.out[ob + CG_AM_Q_COS][g] = (float)(fam == 2 ? s[CG_AM_S_AO] / (fmax(sqrt(s[CG_AM_S_AA]), CG_AM_COS_EPS) * fmax(sqrt(s[CG_AM_S_OO]), CG_AM_COS_EPS))
                                           : s[5] / cos_den);
  }
  if (wave == 0) {      // the group's two histograms, one bin per lane: density = count / n / width (compute_entropy :51-52, eps 1e-8)
    const int32_t* cnt = a.counts + (long long)2 * hist_at * CG_AM_BINS;
    const int ca = cnt[((long long)g) * CG_AM_BINS + lane], co = cnt[((long long)hist_g + g) * CG_AM_BINS + lane];
    const float mx = a.gmax[hist_at + g];
    const double width = (double)mx / CG_AM_BINS, eps = 1e-8;
    const double p = (double)ca / (double)hist_n / width, q = (double)co / (double)hist_n / width, mid = (p + q) / 2.0;
    double r[3] = {p * (log(p + eps) - log(q + eps)), p * (log(p + eps) - log(mid + eps)), q * (log(q + eps) - log(mid + eps))};
    cg_wave_allsum(r);
    int cum = ca - co;      // the cumulated counts are exact
    for (int off = 1; off < CG_WAVE; off <<= 1) {
      const int up = __shfl_up(cum, off, CG_WAVE);
      if (lane >= off) cum += up;
    }
    const double ks = cg_wave_allmax(fabs((double)cum) / (double)hist_n / width);
    if (lane == 0) {
      const bool flat = !(mx > 0.f);      // every joint of the group coincides: the 65 edges are all 0, the densities undefined
      a.out[ob + CG_AM_Q_KLD][g] = flat ? NAN : (float)r[0];
      a.out[ob + CG_AM_Q_JSD][g] = flat ? NAN : (float)((r[1] + r[2]) / 2.0);
      a.out[ob + CG_AM_Q_KS][g] = flat ? NAN : (float)ks;
    }
  }
}

extern "C" long long cg_attack_metrics_ws_doubles(int B, int T, int J) {
  if (B < 1 || T < 1 || J < 2 || J > CG_WAVE) return 0;
  CgAmWs w;
  return cg_am_ws_layout(B, T, J, nullptr, &w);
}

extern "C" int cg_attack_metrics(const CgAttackMetrics* a, void* stream_) {
  if (!a || !a->adv || !a->orig || !a->counts || !a->gmax || !a->ws) return CG_EARG;
  for (int q = 0; q < CG_AM_OUT; ++q)
    if (!a->out[q]) return CG_EARG;
  const int B = a->B, T = a->T, J = a->J;
  if (B < 1 || T < 1 || J < 2 || J > CG_WAVE) return CG_ESHAPE;
  if ((long long)T * J > 0x7fffffffLL || cg_am_chunks(B) > 65535) return CG_ESHAPE;      // grid of the cross pass
  hipStream_t stream = (hipStream_t)stream_;
  const long long F = (long long)B * T, G = (long long)B + T + J;
  const int st = cg_zero_fill(a->counts, 2 * G * CG_AM_BINS * (long long)sizeof(int32_t), stream);
  if (st != CG_OK) return st;
  const long long fg = (F + CG_AM_WAVES - 1) / CG_AM_WAVES;
  hipLaunchKernelGGL(cg_am_frame_kernel, dim3((unsigned)min(fg, 16384LL)), dim3(CG_AM_THREADS), 0, stream, *a);
  hipLaunchKernelGGL(cg_am_cross_kernel, dim3((unsigned)(T * J), (unsigned)cg_am_chunks(B)), dim3(CG_AM_TILE), 0, stream, *a);
  hipLaunchKernelGGL(cg_am_range_kernel, dim3((unsigned)min((G + CG_AM_WAVES - 1) / CG_AM_WAVES, 4096LL)), dim3(CG_AM_THREADS), 0, stream, *a);
  const long long hg = (((long long)B + CG_AM_HB - 1) / CG_AM_HB) * ((T + CG_AM_HT - 1) / CG_AM_HT);
  hipLaunchKernelGGL(cg_am_hist_kernel, dim3((unsigned)hg), dim3(CG_AM_HIST_THREADS), 0, stream, *a);
  hipLaunchKernelGGL(cg_am_finish_kernel, dim3((unsigned)(G + 1)), dim3(CG_AM_THREADS), 0, stream, *a);
  return cg_launch_status();
}
