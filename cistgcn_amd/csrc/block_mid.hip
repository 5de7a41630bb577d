// Middle of a DSTD_GC block (reference: conv_s / conv_t slots 5-7 with the (1,V) convolution behind them, CISTGCN.py:331-352, and the
// towers' BatchNorm -> Dropout -> 1x1 map, time_compress / joint_compress slots 4-6, CISTGCN.py:138-163): per item
//   x (B,C,L) -> BatchNorm2d -> Dropout [-> PReLU] = h,   then   z[b,o] = sum_{c,l} W[o,c,l] h[b,c,l]   (full: the gates)
//                                                          or     y[b,o,l] = sum_c W[o,c] h[b,c,l]       (pointwise: the towers).
// As separate operators this was the channel sums, two row kernels and two split-K contractions forward and four operator calls (about
// eleven kernels) backward, each 8-40 us of launch latency and split-K bookkeeping on tensors of 0.2-1.6 MB.  The recipe of gate_head.hip:
// cut only at the batch statistics.  Forward is ONE launch (the statistics of x come from the producing collapse kernel), backward two.
// A workgroup owns a slice of `sb` samples of one item (blockIdx.y = item), holds their h in LDS and
//   full:      reads W (O, C*L: up to 180 KB, too large for LDS) from L2 once per slice, a lane = a k column, four output rows at a time;
//   pointwise: keeps W (<= 64 x 64) in LDS.
// Backward launch 1 rebuilds h, forms dh = W^T dy and g = dh * keep * PReLU', and leaves per-slice partials of the BatchNorm-backward
// sums (f64) and of dW; launch 2 sums them in a fixed order in every workgroup, applies the BatchNorm backward and folds dW.  No float
// atomics, nothing that has to be zero on entry: the gradients are the same from run to run.
#include "cg_common.h"
#include "cg_phase.h"
#include "block_mid.h"

HIP_DYNAMIC_SHARED(unsigned char, cg_dyn_lds)

#define CG_MID_THREADS 1024                   // sixteen waves: the sixteen groups of four output rows of O = 64 in one pass
#define CG_MID_KSTEPS 4                       // column steps of a wave whose W loads are in flight together (16 loads per lane)
#define CG_MID_OSTEPS 8                       // rows of W in flight per lane in the full backward
#define CG_MID_WAVES (CG_MID_THREADS / CG_WAVE)
#define CG_MID_SB 8                        // samples per slice at most (the accumulator tile of the full product)
#define CG_MID_FULL_FLOATS 8192            // h image of a slice, full items
#define CG_MID_PW_FLOATS 4096              // h (and dy) image of a slice, pointwise items

static inline int cg_mid_pad4(int n) { return (n + 3) & ~3; }
static inline int cg_mid_sb(int kind, int C, int L, int O) {
  const int per = kind == 0 ? C * L : (C > O ? C : O) * L;
  int sb = (kind == 0 ? CG_MID_FULL_FLOATS : CG_MID_PW_FLOATS) / per;
  return sb < 1 ? 1 : (sb > CG_MID_SB ? CG_MID_SB : sb);
}

// BatchNorm constants of channel c: {mean, rstd, gamma * rstd, beta}.  Forward, train: from the producer's replicated f64 sums (the owner
// records save / running statistics, cg_bn_record); eval: running statistics; backward: the saved pair.
__device__ __forceinline__ void cg_mid_aff(const CgMidItem& it, int c, double cnt, int train, bool backward, bool owner, float* k) {
  const CgTailBN& bn = it.bn;
  const int C = it.C;
  float mean, rstd;
  if (backward) { mean = bn.save[c]; rstd = bn.save[C + c]; }
  else if (train) {
    double s1, s2, m, var;
    cg_bn_sums(bn.stats, it.stats_ld, c, s1, s2);
    cg_bn_moments(s1, s2, cnt, m, var);
    mean = (float)m;
    rstd = cg_bn_rstd(var, bn.eps);
    if (owner) cg_bn_record(bn, c, C, mean, rstd, var, cnt);
  } else {
    mean = bn.running_mean[c];
    rstd = cg_bn_rstd_eval(bn.running_var[c], bn.eps);
    if (owner) cg_bn_save(bn, c, C, mean, rstd);
  }
  k[0] = mean; k[1] = rstd; k[2] = bn.gamma[c] * rstd; k[3] = bn.beta[c];
}

// pre-activation behind BatchNorm and Dropout of element r of sample b (cg_norm_act's expression and its dropout index)
__device__ __forceinline__ float cg_mid_u(const CgBlockMid& t, const CgMidItem& it, const float (*sAff)[4], unsigned long long seed, bool drop,
                                          int b, int r, int K, float& keep, float& xv) {
  const int c = r / it.L;
  xv = it.x[(long long)b * it.x_ld + r];
  keep = drop ? cg_drop_scale(t.drop_p, seed, it.salt, (unsigned long long)b * K + r) : 1.f;
  return ((xv - sAff[c][0]) * sAff[c][2] + sAff[c][3]) * keep;
}

// h of the slice's samples into sH [sb][K] (rows behind the batch: zero)
__device__ __forceinline__ void cg_mid_stage_h(const CgBlockMid& t, const CgMidItem& it, const float (*sAff)[4], float* sH, int b0, int nb, bool tap) {
  const int K = it.C * it.L;
  const bool drop = t.train && t.drop_p > 0.f;
  const unsigned long long seed = drop ? *t.seed : 0ull;
  for (int e = threadIdx.x; e < it.sb_ * K; e += CG_MID_THREADS) {
    const int b = e / K, r = e - b * K;
    float h = 0.f;
    if (b < nb) {
      float keep, xv;
      const float u = cg_mid_u(t, it, sAff, seed, drop, b0 + b, r, K, keep, xv);
      h = it.alpha ? (u > 0.f ? u : it.alpha[0] * u) : u;
      if (tap && it.tap) it.tap[(long long)(b0 + b) * K + r] = h;
    }
    sH[e] = h;
  }
}

// (the products below are written as fmaf: one rounding per term on the matrix-free paths, on the GPU and on the CPU test shim alike)
// ======================================================================================================================
// forward: grid (slices, items)
__global__ __launch_bounds__(CG_MID_THREADS) void cg_block_mid_fwd_kernel(CgBlockMid t) {
  const CgMidItem& it = t.it[blockIdx.y];
  if ((int)blockIdx.x >= it.ns_) return;
  const int C = it.C, L = it.L, O = it.O, K = C * L, sb = it.sb_;
  const int tid = threadIdx.x, lane = tid & (CG_WAVE - 1), wave = tid / CG_WAVE;
  const int b0 = (int)blockIdx.x * sb, nb = min(sb, t.B - b0);
  __shared__ float sAff[CG_MID_MAXD][4];
  __shared__ double sRed[CG_MID_WAVES][4 * CG_MID_SB][4];
  float* sH = reinterpret_cast<float*>(cg_dyn_lds);                   // [sb][K]
  float* sW = sH + ((sb * K + 3) & ~3);                               // pointwise: [C][OP] W transposed, columns O .. OP-1 zero
  const int OP = (O + 3) & ~3;
  if (tid < C) cg_mid_aff(it, tid, (double)t.B * L, t.train, false, blockIdx.x == 0, sAff[tid]);
  if (it.kind == 1)
    for (int e = tid; e < C * OP; e += CG_MID_THREADS) { const int c = e / OP, o = e - c * OP; sW[e] = o < O ? it.W[o * C + c] : 0.f; }
  __syncthreads();
  cg_mid_stage_h(t, it, sAff, sH, b0, nb, true);
  __syncthreads();
  if (it.kind == 1) {
    const int OG = OP >> 2, total = nb * OG * L;
    for (int idx = tid; idx < total; idx += CG_MID_THREADS) {
      const int l = idx % L, r = idx / L, og = r % OG, b = r / OG;
      const float* h = sH + b * K + l;
      const float* w = sW + 4 * og;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < C; ++c) {
        const float hv = h[c * L];
        const float4 wv = *reinterpret_cast<const float4*>(w + c * OP);
        acc[0] = fmaf(wv.x, hv, acc[0]); acc[1] = fmaf(wv.y, hv, acc[1]); acc[2] = fmaf(wv.z, hv, acc[2]); acc[3] = fmaf(wv.w, hv, acc[3]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * og + j < O) it.y[((long long)(b0 + b) * O + 4 * og + j) * L + l] = acc[j];
    }
    return;
  }
  // full: a wave takes four output rows at a time, a lane the columns k = lane, lane + 64, ...; W straight from L2 into registers
  const int OG = (O + 3) >> 2, iters = (OG + CG_MID_WAVES - 1) / CG_MID_WAVES;
  for (int i = 0; i < iters; ++i) {
    const int og = i * CG_MID_WAVES + wave;
    float acc[4][CG_MID_SB];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < CG_MID_SB; ++b) acc[j][b] = 0.f;
    if (og < OG) {
      const float* w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = it.W + (long long)min(4 * og + j, O - 1) * K;
      for (int k0 = lane; k0 < K; k0 += CG_MID_KSTEPS * CG_WAVE) {
        // all loads of the chunk first: the loop is bound by the latency of L2, not by its bandwidth
        float wv[CG_MID_KSTEPS][4];
#pragma unroll
        for (int s = 0; s < CG_MID_KSTEPS; ++s)
#pragma unroll
          for (int j = 0; j < 4; ++j) wv[s][j] = k0 + s * CG_WAVE < K ? w[j][k0 + s * CG_WAVE] : 0.f;
#pragma unroll
        for (int s = 0; s < CG_MID_KSTEPS; ++s) {
          const int k = k0 + s * CG_WAVE;
          if (k < K) {
#pragma unroll
            for (int b = 0; b < CG_MID_SB; ++b)
              if (b < sb) {
                const float hv = sH[b * K + k];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j][b] = fmaf(wv[s][j], hv, acc[j][b]);
              }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < CG_MID_SB; ++b) {
        const double v = cg_row16_sum((double)acc[j][b]);      // the lanes' partial sums are folded in f64: the order of the fold does not show
        if ((lane & 15) == 0) sRed[wave][j * CG_MID_SB + b][lane >> 4] = v;
      }
    __syncthreads();
    if (tid < CG_MID_WAVES * 4 * CG_MID_SB) {
      const int w2 = tid / (4 * CG_MID_SB), q = tid - w2 * (4 * CG_MID_SB), j = q / CG_MID_SB, b = q - j * CG_MID_SB;
      const int o = 4 * (i * CG_MID_WAVES + w2) + j;
      if (o < O && b < nb) it.y[(long long)(b0 + b) * O + o] = (float)((sRed[w2][q][0] + sRed[w2][q][1]) + (sRed[w2][q][2] + sRed[w2][q][3]));
    }
    __syncthreads();
  }
}

// ======================================================================================================================
// backward, launch 1: g (gradient in front of the BatchNorm) and the per-slice partials of its sums and of dW
__global__ __launch_bounds__(CG_MID_THREADS) void cg_block_mid_bwd1_kernel(CgBlockMid t) {
  const CgMidItem& it = t.it[blockIdx.y];
  if ((int)blockIdx.x >= it.ns_) return;
  const int C = it.C, L = it.L, O = it.O, K = C * L, sb = it.sb_;
  const int tid = threadIdx.x, lane = tid & (CG_WAVE - 1), wave = tid / CG_WAVE;
  const int slice = (int)blockIdx.x, b0 = slice * sb, nb = min(sb, t.B - b0);
  __shared__ float sAff[CG_MID_MAXD][4];
  __shared__ double sRedD[CG_MID_WAVES];
  const int HK = (sb * K + 3) & ~3;
  float* sH = reinterpret_cast<float*>(cg_dyn_lds);                   // [sb][K] h
  float* sG = sH + HK;                                                // [sb][K] dh, then g
  float* sDy = sG + HK;                                               // full: [O][8] dy transposed; pointwise: [sb][O][L]
  const int CP = (C + 3) & ~3;
  float* sW = sDy + (it.kind == 0 ? O * CG_MID_SB : ((sb * O * L + 3) & ~3));   // pointwise: [O][CP] as it lies in memory, columns C .. CP-1 zero
  if (tid < C) cg_mid_aff(it, tid, 0.0, t.train, true, false, sAff[tid]);
  if (it.kind == 0) {
    for (int e = tid; e < O * CG_MID_SB; e += CG_MID_THREADS) {
      const int o = e / CG_MID_SB, b = e - o * CG_MID_SB;
      sDy[e] = b < nb ? it.dy[(long long)(b0 + b) * O + o] : 0.f;
    }
  } else {
    for (int e = tid; e < O * CP; e += CG_MID_THREADS) { const int o = e / CP, c = e - o * CP; sW[e] = c < C ? it.W[o * C + c] : 0.f; }
    for (int e = tid; e < nb * O * L; e += CG_MID_THREADS) sDy[e] = it.dy[(long long)b0 * O * L + e];
  }
  __syncthreads();
  cg_mid_stage_h(t, it, sAff, sH, b0, nb, false);
  __syncthreads();
  if (it.kind == 0) {
    // a thread = a column k: dh[b][k] = sum_o W[o][k] dy[b][o] and this slice's dW[o][k] = sum_b dy[b][o] h[b][k] from one read of W
    float* wp = it.wpart + (long long)slice * O * K;
    for (int k = tid; k < K; k += CG_MID_THREADS) {
      float hv[CG_MID_SB], dh[CG_MID_SB];
#pragma unroll
      for (int b = 0; b < CG_MID_SB; ++b) { hv[b] = b < sb ? sH[b * K + k] : 0.f; dh[b] = 0.f; }
      for (int o0 = 0; o0 < O; o0 += CG_MID_OSTEPS) {
        float wv[CG_MID_OSTEPS];                         // the loads of several rows in flight together (latency of L2)
#pragma unroll
        for (int s = 0; s < CG_MID_OSTEPS; ++s) wv[s] = o0 + s < O ? it.W[(long long)(o0 + s) * K + k] : 0.f;
#pragma unroll
        for (int s = 0; s < CG_MID_OSTEPS; ++s) {
          const int o = o0 + s;
          if (o < O) {
            const float4 d0 = *reinterpret_cast<const float4*>(sDy + o * CG_MID_SB), d1 = *reinterpret_cast<const float4*>(sDy + o * CG_MID_SB + 4);
            const float d[CG_MID_SB] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
            float a = 0.f;
#pragma unroll
            for (int b = 0; b < CG_MID_SB; ++b) { dh[b] = fmaf(wv[s], d[b], dh[b]); a = fmaf(d[b], hv[b], a); }
            wp[(long long)o * K + k] = a;
          }
        }
      }
#pragma unroll
      for (int b = 0; b < CG_MID_SB; ++b) if (b < sb) sG[b * K + k] = dh[b];
    }
  } else {
    // this slice's dW[o][c] = sum_{b,l} dy[b][o][l] h[b][c][l]: a thread = four rows o of one column c
    float* wp = it.wpart + (long long)slice * O * C;
    const int OG = (O + 3) >> 2;
    for (int e = tid; e < OG * C; e += CG_MID_THREADS) {
      const int og = e / C, c = e - og * C;
      int oo[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) oo[j] = min(4 * og + j, O - 1);
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      for (int b = 0; b < nb; ++b) {                  // a sample's row on its own, then the samples: two short sums instead of one long one
        const float* h = sH + b * K + c * L;
        const float* d = sDy + b * O * L;
        float ab[4] = {0.f, 0.f, 0.f, 0.f};
        for (int l = 0; l < L; ++l) {
          const float hv = h[l];
#pragma unroll
          for (int j = 0; j < 4; ++j) ab[j] = fmaf(d[oo[j] * L + l], hv, ab[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += ab[j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) if (4 * og + j < O) wp[(4 * og + j) * C + c] = a[j];
    }
    // dh[b][c][l] = sum_o W[o][c] dy[b][o][l]: a thread = four channels of one position
    const int CG = CP >> 2, total = nb * CG * L;
    for (int idx = tid; idx < total; idx += CG_MID_THREADS) {
      const int l = idx % L, r = idx / L, cg = r % CG, b = r / CG;
      const float* d = sDy + b * O * L + l;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int o = 0; o < O; ++o) {
        const float dv = d[o * L];
        const float4 wv = *reinterpret_cast<const float4*>(sW + o * CP + 4 * cg);
        acc[0] = fmaf(wv.x, dv, acc[0]); acc[1] = fmaf(wv.y, dv, acc[1]); acc[2] = fmaf(wv.z, dv, acc[2]); acc[3] = fmaf(wv.w, dv, acc[3]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) if (4 * cg + j < C) sG[b * K + (4 * cg + j) * L + l] = acc[j];
    }
  }
  __syncthreads();
  // through Dropout and PReLU: g = dh * PReLU'(u) * keep, the slope sum
  const bool drop = t.train && t.drop_p > 0.f;
  const unsigned long long seed = drop ? *t.seed : 0ull;
  const float alpha = it.alpha ? it.alpha[0] : 1.f;
  double SA = 0.0;
  for (int e = tid; e < nb * K; e += CG_MID_THREADS) {
    const int b = e / K, r = e - b * K;
    float keep, xv;
    const float u = cg_mid_u(t, it, sAff, seed, drop, b0 + b, r, K, keep, xv);
    const float dh = sG[e];
    const bool neg = it.alpha && !(u > 0.f);
    if (neg) SA += (double)dh * (double)u;
    const float g = (neg ? alpha * dh : dh) * keep;
    sG[e] = g;
    it.g[(long long)(b0 + b) * K + r] = g;
  }
  __syncthreads();
  // per-slice sums of g and g * xhat per channel: a wave = a channel, f64, fixed order
  double* part = it.part + (long long)slice * (2 * C + 1);
  for (int c = wave; c < C; c += CG_MID_WAVES) {
    double s1 = 0.0, s2 = 0.0;
    const float mean = sAff[c][0], rstd = sAff[c][1];
    for (int i = lane; i < nb * L; i += CG_WAVE) {
      const int b = i / L, l = i - b * L;
      const double v = (double)sG[b * K + c * L + l];
      s1 += v;
      s2 += v * (double)((it.x[(long long)(b0 + b) * it.x_ld + c * L + l] - mean) * rstd);
    }
    s1 = cg_wave_sum(s1); s2 = cg_wave_sum(s2);
    if (lane == 0) { part[c] = s1; part[C + c] = s2; }
  }
  SA = cg_block_sum(SA, sRedD);
  if (tid == 0) part[2 * C] = SA;
}

// backward, launch 2: every workgroup sums the slices' statistics itself (fixed order), BatchNorm backward of its samples, its share of dW
__global__ __launch_bounds__(CG_MID_THREADS) void cg_block_mid_bwd2_kernel(CgBlockMid t) {
  const CgMidItem& it = t.it[blockIdx.y];
  if ((int)blockIdx.x >= it.ns_) return;
  const int C = it.C, L = it.L, O = it.O, K = C * L, sb = it.sb_, ns = it.ns_, nv = 2 * C + 1;
  const int tid = threadIdx.x, lane = tid & (CG_WAVE - 1), wave = tid / CG_WAVE;
  const int slice = (int)blockIdx.x, b0 = slice * sb, nb = min(sb, t.B - b0);
  __shared__ float sAff[CG_MID_MAXD][4];
  __shared__ double sP[CG_MID_WAVES][2 * CG_MID_MAXD + 1];
  __shared__ float sM[CG_MID_MAXD][2];
  if (tid < C) cg_mid_aff(it, tid, 0.0, t.train, true, false, sAff[tid]);
  for (int v = lane; v < nv; v += CG_WAVE) {
    double s = 0.0;
    for (int sl = wave; sl < ns; sl += CG_MID_WAVES) s += it.part[(long long)sl * nv + v];
    sP[wave][v] = s;
  }
  __syncthreads();
  if (tid < C) {
    double S1 = 0.0, S2 = 0.0;
    for (int w = 0; w < CG_MID_WAVES; ++w) { S1 += sP[w][tid]; S2 += sP[w][C + tid]; }
    const double cnt = (double)t.B * L;
    sM[tid][0] = t.train ? (float)(S1 / cnt) : 0.f; sM[tid][1] = t.train ? (float)(S2 / cnt) : 0.f;
    if (slice == 0) { it.dgamma[tid] = (float)S2; it.dbeta[tid] = (float)S1; }
  }
  if (tid == 0 && slice == 0 && it.dalpha) {
    double SA = 0.0;
    for (int w = 0; w < CG_MID_WAVES; ++w) SA += sP[w][2 * C];
    it.dalpha[0] = (float)SA;
  }
  __syncthreads();
  for (int e = tid; e < nb * K; e += CG_MID_THREADS) {
    const int b = e / K, r = e - b * K, c = r / L;
    const long long idx = (long long)(b0 + b) * K + r;
    const float xv = it.x[(long long)(b0 + b) * it.x_ld + r];
    it.dx[idx] = sAff[c][2] * (it.g[idx] - sM[c][0] - (xv - sAff[c][0]) * sAff[c][1] * sM[c][1]);
  }
  // dW: this workgroup's share of the elements, summed over the slices in their order
  const long long NW = (long long)O * (it.kind == 0 ? K : C), chunk = (NW + ns - 1) / ns;
  const long long e1 = min(NW, (slice + 1) * chunk);
  for (long long e = slice * chunk + tid; e < e1; e += CG_MID_THREADS) {
    double a = 0.0;                                   // up to hundreds of slices: folded in f64
    for (int sl = 0; sl < ns; ++sl) a += (double)it.wpart[sl * NW + e];
    it.dW[e] = (float)a;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
static size_t cg_mid_lds_fwd(int kind, int C, int L, int O) {
  const int sb = cg_mid_sb(kind, C, L, O);
  return ((size_t)cg_mid_pad4(sb * C * L) + (kind == 1 ? (size_t)C * cg_mid_pad4(O) : 0)) * sizeof(float);
}
static size_t cg_mid_lds_bwd(int kind, int C, int L, int O) {
  const int sb = cg_mid_sb(kind, C, L, O);
  size_t f = (size_t)2 * cg_mid_pad4(sb * C * L);
  f += kind == 0 ? (size_t)O * CG_MID_SB : (size_t)cg_mid_pad4(sb * O * L) + (size_t)O * cg_mid_pad4(C);
  return f * sizeof(float);
}

extern "C" int cg_block_mid_supported(int B, int kind, int C, int L, int O) {
  if (B <= 0 || kind < 0 || kind > 1 || C <= 0 || L <= 0 || O <= 0 || C > CG_MID_MAXD || L > CG_MID_MAXD || O > CG_MID_MAXD) return 0;
  const int sb = cg_mid_sb(kind, C, L, O);
  const long long ns = ((long long)B + sb - 1) / sb;
  return (ns <= 65535 && ns * O * C * (kind == 0 ? L : 1) < (1ll << 31)) ? 1 : 0;
}

// out[0] samples per slice, [1] slices, [2] / [3] dynamic LDS bytes forward / backward launch 1, [4] `part` doubles, [5] `wpart` floats,
// [6] passes of the full product over the groups of four output rows, [7] passes of the backward over the columns k (full items)
extern "C" int cg_block_mid_geometry(int B, int kind, int C, int L, int O, int* out) {
  if (!out || !cg_block_mid_supported(B, kind, C, L, O)) return CG_ESHAPE;
  const int sb = cg_mid_sb(kind, C, L, O), ns = (B + sb - 1) / sb;
  out[0] = sb; out[1] = ns;
  out[2] = (int)cg_mid_lds_fwd(kind, C, L, O); out[3] = (int)cg_mid_lds_bwd(kind, C, L, O);
  out[4] = ns * (2 * C + 1);
  out[5] = ns * O * C * (kind == 0 ? L : 1);
  out[6] = kind == 0 ? (((O + 3) >> 2) + CG_MID_WAVES - 1) / CG_MID_WAVES : 0;
  out[7] = kind == 0 ? (C * L + CG_MID_THREADS - 1) / CG_MID_THREADS : 0;
  return CG_OK;
}

static int cg_mid_prepare(const CgBlockMid* t, bool bwd, CgBlockMid& a, int& slices, size_t& lds) {
  if (!t || t->n < 1 || t->n > CG_MID_MAXN || t->B <= 0) return CG_EARG;
  if (t->drop_p < 0.f || t->drop_p >= 1.f) return CG_EARG;
  if (t->train && t->drop_p > 0.f && !t->seed) return CG_EARG;
  a = *t;
  slices = 0; lds = 0;
  for (int i = 0; i < t->n; ++i) {
    CgMidItem& p = a.it[i];
    if (!cg_block_mid_supported(t->B, p.kind, p.C, p.L, p.O)) return CG_ESHAPE;
    if (t->train && (long long)t->B * p.L < 2) return CG_ESHAPE;
    if (!p.x || p.x_ld < (long long)p.C * p.L || !p.W || !p.bn.gamma || !p.bn.beta || !p.bn.save) return CG_EARG;
    if (!bwd && (!p.y || (t->train ? (!p.bn.stats || p.stats_ld < p.C) : (!p.bn.running_mean || !p.bn.running_var)))) return CG_EARG;
    if (bwd && (!p.dy || !p.dx || !p.dW || !p.dgamma || !p.dbeta || (p.alpha && !p.dalpha) || !p.g || !p.part || !p.wpart)) return CG_EARG;
    p.sb_ = cg_mid_sb(p.kind, p.C, p.L, p.O);
    p.ns_ = (t->B + p.sb_ - 1) / p.sb_;
    if (p.ns_ > slices) slices = p.ns_;
    const size_t l = bwd ? cg_mid_lds_bwd(p.kind, p.C, p.L, p.O) : cg_mid_lds_fwd(p.kind, p.C, p.L, p.O);
    if (l > lds) lds = l;
  }
  return CG_OK;
}

// include/cistgcn_hip.h : cg_block_mid_fwd (one launch) / cg_block_mid_bwd (two)
extern "C" int cg_block_mid_fwd(const CgBlockMid* t, void* stream_) {
  CgBlockMid a;
  int slices; size_t lds;
  int st = cg_mid_prepare(t, false, a, slices, lds);
  if (st != CG_OK) return st;
  if (lds > CG_LDS_DEFAULT && cg_lds_limit((const void*)cg_block_mid_fwd_kernel, lds) != hipSuccess) return CG_ESHAPE;
  hipLaunchKernelGGL(cg_block_mid_fwd_kernel, dim3((unsigned)slices, (unsigned)a.n), dim3(CG_MID_THREADS), lds, (hipStream_t)stream_, a);
  return cg_launch_status();
}

extern "C" int cg_block_mid_bwd(const CgBlockMid* t, void* stream_) {
  CgBlockMid a;
  int slices; size_t lds;
  int st = cg_mid_prepare(t, true, a, slices, lds);
  if (st != CG_OK) return st;
  if (lds > CG_LDS_DEFAULT && cg_lds_limit((const void*)cg_block_mid_bwd1_kernel, lds) != hipSuccess) return CG_ESHAPE;
  const dim3 grid((unsigned)slices, (unsigned)a.n), block(CG_MID_THREADS);
  hipLaunchKernelGGL(cg_block_mid_bwd1_kernel, grid, block, lds, (hipStream_t)stream_, a);
  st = cg_launch_status();
  if (st != CG_OK) return st;
  hipLaunchKernelGGL(cg_block_mid_bwd2_kernel, grid, block, 0, (hipStream_t)stream_, a);
  return cg_launch_status();
}
