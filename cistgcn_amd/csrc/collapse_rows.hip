// Collapsing convolution over the frame axis (reference: nn.Conv2d(C, O, (T, 1)) of the gate paths, CISTGCN.py:331-336, and of
// Map2Adj.time_compress, :138-150): y[b,o,v] = sum_{c,t} W[o,c,t] x[b,c,t,v].  Per sample this is Y_b (O x V) = W (O x K) X_b (K x V)
// with K = C*T and X_b = x[b] as it lies in memory; the tensors are 36-72 MB, the outputs a few hundred KB.  The generic
// contraction needed split-K with atomics and strided gathers for it (0.3 TB/s); here
//   forward   one 512-thread workgroup per sample: eight waves split K, feed the matrix cores straight from global memory
//             (W rows as float4 along k, x rows as 16-lane pieces along v), partial tiles are added in LDS
//   backward  a workgroup owns 64 rows k of W for a slice of the samples: dx[b,k,v] = sum_o W[o,k] dy[b,o,v] is written as one
//             contiguous 64 x V piece per sample, dW[o,k] += sum_v dy[b,o,v] x[b,k,v] stays in registers over the slice
#include "cg_common.h"
#include "cg_phase.h"

HIP_DYNAMIC_SHARED(unsigned char, cg_dyn_lds)

#define CG_ROWS_FWD_THREADS 512
#define CG_ROWS_BWD_THREADS 256
#define CG_ROWS_KB 64            // rows of W per backward workgroup

struct CgRowsGeom { int K, OT, slices, per, kranges, rpc; };      // rpc: rows k per channel (T on the frame axis, V on the joint axis)
struct CgRowsArgs { CgRowsConv t; CgRowsGeom g; };

// ======================================================================================================================
// forward
// ======================================================================================================================
// OT: 16-row tiles of the O outputs (compile time: the accumulators are registers).  The operands come straight from global memory, a
// wave walks ~K / 128 groups of 16 rows k: with one group per iteration every iteration waited out a full memory latency in front of its
// 16-32 MFMAs (one workgroup per CU: nothing else to run meanwhile; 34 us for 36 MB).  Now four groups of a wave are in flight: the loads
// of group g + 4 are issued right behind the MFMAs of group g.  No load sits behind a branch: indices outside the tensor are clamped to
// a neighbouring element (rows o >= O and columns v >= V land in results that are never stored), only rows k >= K are zeroed.
template <int OT>
__global__ __launch_bounds__(CG_ROWS_FWD_THREADS) void cg_rows_fwd_kernel(CgRowsArgs a, unsigned magicT) {
  const CgRowsConv& t = a.t; const CgRowsGeom& g = a.g;
  const int b = blockIdx.x, K = g.K, V = t.V, O = t.O;
  constexpr int nw = CG_ROWS_FWD_THREADS / 64, DEPTH = 4;
  float* sY = reinterpret_cast<float*>(cg_dyn_lds);              // [nw][16 * OT][33] partial tiles of the eight waves (no LDS atomics: 1 000 cycles each)
  float* sTab = sY + nw * 16 * OT * 33;                           // [C][4] input transform: mean, gamma * rstd, beta, -
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, slot = lane >> 4;
  const bool tr = t.in_on != 0;
  const float in_alpha = tr ? t.in_alpha[0] : 1.f;
  float* const tapb = (tr && t.in_tap) ? t.in_tap + (long long)b * K * V : nullptr;
  if (tr) {
    for (int c = tid; c < t.C; c += CG_ROWS_FWD_THREADS) {
      const CgAff af = cg_tail_aff(t.in_bn, c, t.C, (double)t.B * t.T * V, t.in_train, false, blockIdx.x == 0);
      sTab[4 * c] = af.mean; sTab[4 * c + 1] = af.gamma * af.rstd; sTab[4 * c + 2] = af.beta; sTab[4 * c + 3] = 0.f;
    }
    __syncthreads();
  }
  const float* xb = t.x + (long long)b * K * V;
  cg_f32x4 acc[OT][2];
#pragma unroll
  for (int i = 0; i < OT; ++i) { acc[i][0] = cg_f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][1] = acc[i][0]; }
  // groups of 16 consecutive k: lane (l15, slot) takes k = k0 + 4 slot + s in MFMA step s (both operands agree, a sum does not
  // care about the order)
  const int ngroups = (K + 15) >> 4;
  const int vA = min(l15, V - 1), vB = min(16 + l15, V - 1);
  const float* wrow[OT];
#pragma unroll
  for (int i = 0; i < OT; ++i) wrow[i] = t.W + (long long)min(16 * i + l15, O - 1) * K;
  struct Frag { float4 w[OT]; float x0[4], x1[4]; float mask; int kc; };      // mask: 0 for rows k >= K (applied in front of the MFMAs: arithmetic on a
                                                                                // loaded value right behind its load would wait for it there)
  auto load = [&](int gi, Frag& f) {
    const int k = 16 * gi + 4 * slot;
    const bool kin = k < K;                                 // K % 4 == 0: a lane's four rows are inside or outside together
    const int kc = kin ? k : K - 4;
    f.mask = kin ? 1.f : 0.f; f.kc = kc;
#pragma unroll
    for (int i = 0; i < OT; ++i) f.w[i] = *reinterpret_cast<const float4*>(wrow[i] + kc);
    const float* xr = xb + (long long)kc * V;
#pragma unroll
    for (int s = 0; s < 4; ++s) { f.x0[s] = xr[s * V + vA]; f.x1[s] = xr[s * V + vB]; }
  };
  auto mma = [&](Frag& f) {
    if (tr) {                                               // PReLU(BatchNorm(x)) of the four rows k = (c, t) of this lane, constants of channel c from LDS
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int c = (int)cg_div((unsigned)(f.kc + s), magicT);
        const float4 k4 = *reinterpret_cast<const float4*>(sTab + 4 * c);
        f.x0[s] = cg_prelu((f.x0[s] - k4.x) * k4.y + k4.z, in_alpha);
        f.x1[s] = cg_prelu((f.x1[s] - k4.x) * k4.y + k4.z, in_alpha);
        if (tapb && f.mask != 0.f) {                        // every element of x[b] is held by exactly one lane (clamped lanes repeat a neighbour's value)
          tapb[(long long)(f.kc + s) * V + vA] = f.x0[s];
          tapb[(long long)(f.kc + s) * V + vB] = f.x1[s];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < OT; ++i) {
      const float w4[4] = {f.w[i].x * f.mask, f.w[i].y * f.mask, f.w[i].z * f.mask, f.w[i].w * f.mask};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[s], f.x0[s], acc[i][0], 0, 0, 0);
        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[s], f.x1[s], acc[i][1], 0, 0, 0);
      }
    }
  };
  Frag f[DEPTH];
#pragma unroll
  for (int j = 0; j < DEPTH; ++j)
    if (wave + j * nw < ngroups) load(wave + j * nw, f[j]);
  for (int gi = wave; gi < ngroups; gi += DEPTH * nw) {
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      const int gj = gi + j * nw;
      if (gj < ngroups) {
        mma(f[j]);
        if (gj + DEPTH * nw < ngroups) load(gj + DEPTH * nw, f[j]);
      }
    }
  }
  float* mine = sY + wave * 16 * OT * 33;
#pragma unroll
  for (int i = 0; i < OT; ++i) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = 16 * i + 4 * slot + q;
      mine[o * 33 + l15] = acc[i][0][q];
      mine[o * 33 + 16 + l15] = acc[i][1][q];
    }
  }
  __syncthreads();
  for (int e = tid; e < O * V; e += CG_ROWS_FWD_THREADS) {
    const int o = e / V, v = e - o * V;
    float y = 0.f;
#pragma unroll
    for (int w = 0; w < nw; ++w) y += sY[(w * 16 * OT + o) * 33 + v];
    t.y[(long long)b * O * V + e] = y;
    sY[o * 33 + v] = y;                                    // this thread's own element of slot 0: the channel sums below read it
  }
  if (t.stats) {                                       // f64 channel sums for the BatchNorm behind the convolution
    __syncthreads();
    for (int o = tid; o < O; o += CG_ROWS_FWD_THREADS) {
      double s1 = 0.0, s2 = 0.0;
      for (int v = 0; v < V; ++v) { const double y = (double)sY[o * 33 + v]; s1 += y; s2 += y * y; }
      double* rep = t.stats + ((long long)(b % CG_STAT_REPLICAS) * O + o) * 2;
      atomicAdd(&rep[0], s1); atomicAdd(&rep[1], s2);
    }
  }
}

// ======================================================================================================================
// backward: workgroup = (64 rows k of W, slice of the samples)
// ======================================================================================================================
// The dW tile of a backward workgroup ([16 OT][64 rows k], wave w holds the columns 16 w ..) leaves through the LDS that held W: rows along k
// as 16-byte stores into this slice's partial (float atomics into shared replicas left in one burst at the end of the launch, needed the
// replicas zeroed and made dW vary from run to run).
template <int N>
__device__ __forceinline__ void cg_rows_put_dw(float* sT, const cg_f32x4 (&wacc)[N], int OT, float* part, int O, int K, int k0, int tid, int wave, int l15, int slot) {
  constexpr int WS = CG_ROWS_KB + 4;
  __syncthreads();                                                // every wave has read its last W
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (i < OT) {
#pragma unroll
      for (int q = 0; q < 4; ++q) sT[(16 * i + 4 * slot + q) * WS + 16 * wave + l15] = wacc[i][q];
    }
  }
  __syncthreads();
  for (int e = tid; e < 16 * OT * (CG_ROWS_KB / 4); e += CG_ROWS_BWD_THREADS) {
    const int o = e >> 4, kk = 4 * (e & 15);
    if (o < O && k0 + kk < K) *reinterpret_cast<float4*>(part + (long long)o * K + k0 + kk) = *reinterpret_cast<const float4*>(sT + o * WS + kk);      // K % 4 == 0
  }
}

// VW consecutive floats (VW * 4 bytes aligned) global <-> registers, no condition: the callers clamp the address.  Not cg_ldv / cg_stv of
// cg_common.h: through their float4 form cg_rows_bwd_kernel<4, false> takes 120 VGPRs instead of 116 (profiles/device_helpers_isa.txt).
template <int VW>
__device__ __forceinline__ void cg_rows_ldv(const float* __restrict__ p, float* v) {
  if constexpr (VW == 4) {
    const cg_f32x4 q = *reinterpret_cast<const cg_f32x4*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
    v[0] = p[0];
  }
}
template <int VW>
__device__ __forceinline__ void cg_rows_stv(float* __restrict__ p, const float* v) {
  if constexpr (VW == 4) *reinterpret_cast<cg_f32x4*>(p) = cg_f32x4{v[0], v[1], v[2], v[3]};
  else p[0] = v[0];
}

// ---- channel sums of the producer's BatchNorm / PReLU backward (CgRowsConv.sums / red) -----------------------------------------
// The collapsing backward holds, per element of x, the raw value and dh = (W^T dy): everything the reduction pass of the producer's
// BatchNorm / PReLU backward would read back from memory (cg_norm_act_bwd_reduce_many: 2 x 36 MB per map at B = 256).  With the
// template switch SUMS a lane adds up, for ITS row k (one channel), s1 = sum gh, s2 = sum gh xhat, sa = sum_{u <= 0} dh u with
// gh = dh PReLU'(u), xhat = (x - mean) rstd: f32 over the few values of one sample (or of one frame tile), f64 from there on.
// Positions outside the tensor (rows k >= K, columns v >= V, frames t >= T) need no mask: the zero padding of W and dy makes dh exactly
// 0 there, x is a finite stand-in (zeros, an old dx tile = 0, or the clamped duplicate of a neighbour), so every term is 0.
// u is formed by the very expression of the operand, `cg_rows_u`.
__device__ __forceinline__ float cg_rows_u(float x, float tm, float ts, float tb) { return (x - tm) * ts + tb; }
__device__ __forceinline__ void cg_rows_sum_term(float x, float dh, float tm, float ts, float tb, float trs, float ta, float& p1, float& p2, float& pa) {
  const float u = cg_rows_u(x, tm, ts, tb);
  const float gh = u > 0.f ? dh : ta * dh;
  p1 += gh; p2 += gh * ((x - tm) * trs);
  if (!(u > 0.f)) pa += dh * u;
}
// doubles of CgRowsConv.sums: per slice [2][Kp] row sums (s1, s2; Kp = 64 kranges) and [kranges] slope sums of the workgroups
__host__ __device__ __forceinline__ long long cg_rows_sums_stride(int kranges) { return (2ll * CG_ROWS_KB + 1) * kranges; }
// A workgroup's sums leave through LDS (free by now): the four slots of a row are added in a fixed order, the 64 rows' slope sums too.
__device__ __forceinline__ void cg_rows_put_sums(double* sS, double s1, double s2, double sa, double* sums, int kranges, int sl, int kr, int tid) {
  __syncthreads();                                                // every wave is done with W, dy and its rows
  sS[tid] = s1; sS[CG_ROWS_BWD_THREADS + tid] = s2; sS[2 * CG_ROWS_BWD_THREADS + tid] = sa;
  __syncthreads();
  double* dst = sums + (long long)sl * cg_rows_sums_stride(kranges);
  if (tid < CG_ROWS_KB) {                                         // row tid of the range: wave tid / 16, lanes l15 + 16 slot
    const int i = 64 * (tid >> 4) + (tid & 15);
    double r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double* q = sS + CG_ROWS_BWD_THREADS * j + i;
      r[j] = (q[0] + q[16]) + (q[32] + q[48]);
    }
    dst[kr * CG_ROWS_KB + tid] = r[0];
    dst[(long long)kranges * CG_ROWS_KB + kr * CG_ROWS_KB + tid] = r[1];
    sS[3 * CG_ROWS_BWD_THREADS + tid] = r[2];
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < CG_ROWS_KB; ++i) s += sS[3 * CG_ROWS_BWD_THREADS + i];
    dst[2ll * kranges * CG_ROWS_KB + kr] = s;
  }
}

// (128 rows x 512 threads per workgroup: 57 us instead of 44.)
// (Round 4 tried this kernel with compile-time OT, dy of the next sample through registers and clamped instead of conditional loads:
// 90 us instead of 100 on the 64-output gate convolutions, but 152 us instead of 47 on the 32-output tower convolutions; not understood,
// not shipped.)
// Pieces: the 64 x V piece of x[b] (and of dx[b]) of a workgroup is one contiguous run, and so is the 16 x V piece of each wave: 16 V floats,
// 16-byte aligned for any V.  A wave moves its piece as runs of VW floats (VW = 4 where dy[b] and the tensors are 16-byte aligned, else 1):
// x global -> registers -> LDS rows [16][CG_ROWS_XS], where the lanes read their MFMA operand (row l15, four v per slot); the dx tile goes
// accumulators -> the same LDS rows -> registers -> global.  The rows belong to the wave alone (wave barriers order them); the table `xo`
// says where the floats of a lane's runs lie in them.  (Before: 16 four-byte loads and 8 four-byte stores per lane and sample, each load
// instruction across all eleven cache lines of the piece.)
// Staging is split: the loads of dy[b + 1] and x[b + 1] are issued in front of the matrix work of sample b and stored to LDS behind it
// (dy[b + 1] used to be waited for and stored in front of the MFMAs of sample b: one exposed memory latency per sample).
#define CG_ROWS_XS 36            // floats per LDS row of a piece: V <= 32 and four that are never read (column XS - 1 takes the floats of no one)
template <int VW, bool SUMS>
__global__ __launch_bounds__(CG_ROWS_BWD_THREADS) void cg_rows_bwd_kernel(CgRowsArgs a) {
  const CgRowsConv& t = a.t; const CgRowsGeom& g = a.g;
  const int K = g.K, V = t.V, O = t.O, OV = O * V;
  const int kr = blockIdx.x, sl = blockIdx.y, k0 = kr * CG_ROWS_KB;
  const int b0 = sl * g.per, b1 = min(t.B, b0 + g.per);
  if (b0 >= t.B) return;
  constexpr int WS = CG_ROWS_KB + 4, DS = 36, XS = CG_ROWS_XS, NG = 8 / VW;
  float* sW = reinterpret_cast<float*>(cg_dyn_lds);              // [16 * OT][KB + 4]  W[o][k0 ..]
  float* sDY = sW + 16 * g.OT * WS;                               // [2][16 * OT][36]   dy of the current / next sample, v padded with zeros
  float* sX = sDY + 2 * 16 * g.OT * DS;                           // [4 waves][16][XS]  a wave's piece of x[b + 1], then of dx[b]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, slot = lane >> 4;
  // eight loads of a thread in flight (a load - store loop waits out one memory latency per element: 9 to 17 of them in this prologue)
  for (int e0 = tid; e0 < 16 * g.OT * WS; e0 += 8 * CG_ROWS_BWD_THREADS) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = e0 + CG_ROWS_BWD_THREADS * j, o = e / WS, kk = e - o * WS;
      const bool in = o < O && kk < CG_ROWS_KB && k0 + kk < K;
      v[j] = t.W[in ? (long long)o * K + k0 + kk : (long long)k0];       // W[0][k0] stands in for the padding (k0 < K); zeroed at the store
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = e0 + CG_ROWS_BWD_THREADS * j, o = e / WS, kk = e - o * WS;
      if (e < 16 * g.OT * WS) sW[e] = (o < O && kk < CG_ROWS_KB && k0 + kk < K) ? v[j] : 0.f;
    }
  }
  for (int e = tid; e < 2 * 16 * g.OT * DS + (CG_ROWS_BWD_THREADS / 64) * 16 * XS; e += CG_ROWS_BWD_THREADS) sDY[e] = 0.f;      // sDY and sX
  __syncthreads();
  // a wave owns the 16 rows k = k0 + 16 wave + .. of the range: dW tiles [o][k] in registers over the slice
  const int kw = k0 + 16 * wave;                                 // first row of this wave
  const int nx = max(0, min(16, K - kw)) * V;                    // floats of this wave's piece (K % 4 == 0: a multiple of 4)
  float* sXw = sX + wave * 16 * XS;
  // run r of this lane: the floats VW (lane + 64 r) .. of the wave's piece; outside the piece the first run of the workgroup stands in
  // for the load (k0 < K), LDS column XS - 1 for the store, and nothing is written to dx
  int xg[NG], xo[8]; bool xok[NG];
#pragma unroll
  for (int r = 0; r < NG; ++r) {
    const int f = VW * (lane + 64 * r);
    xok[r] = f < nx;
    xg[r] = xok[r] ? kw * V + f : k0 * V;
#pragma unroll
    for (int i = 0; i < VW; ++i) { const int e = f + i, row = e / V; xo[VW * r + i] = xok[r] ? row * XS + (e - row * V) : XS - 1; }
  }
  // the same for dy[b] (O * V floats, all 256 threads): run r of this thread -> [o][DS] rows of sDY
  int dyg[NG], dyo[8];
#pragma unroll
  for (int r = 0; r < NG; ++r) {
    const int f = VW * (tid + CG_ROWS_BWD_THREADS * r);
    dyg[r] = f < OV ? f : 0;
#pragma unroll
    for (int i = 0; i < VW; ++i) { const int e = f + i, o = e / V; dyo[VW * r + i] = f < OV ? o * DS + (e - o * V) : DS - 1; }
  }
  float dr[8], xr[8];
  auto stage_load = [&](int b) {
    const float* dyb = t.dy + (long long)b * OV;
    const float* xb = t.x + (long long)b * K * V;
#pragma unroll
    for (int r = 0; r < NG; ++r) cg_rows_ldv<VW>(dyb + dyg[r], dr + VW * r);
#pragma unroll
    for (int r = 0; r < NG; ++r) cg_rows_ldv<VW>(xb + xg[r], xr + VW * r);
  };
  auto stage_write = [&](int buf) {
    float* dst = sDY + buf * 16 * g.OT * DS;
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[dyo[j]] = dr[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) sXw[xo[j]] = xr[j];
  };
  stage_load(b0);
  stage_write(0);
  cg_f32x4 wacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) wacc[i] = cg_f32x4{0.f, 0.f, 0.f, 0.f};
  // optional input transform (see CgRowsConv.in_on): this lane's row k = (c, t) has ONE channel c; the values outside the tensor meet dy = 0
  const int krow = kw + l15;
  const bool tr = t.in_on != 0;
  float tm = 0.f, ts = 1.f, tb = 0.f, ta = 1.f, trs = 1.f;
  if (tr) {
    const CgAff af = cg_tail_aff(t.in_bn, min(krow, K - 1) / t.T, t.C, 0.0, t.in_train, true, false);
    tm = af.mean; ts = af.gamma * af.rstd; tb = af.beta; ta = t.in_alpha[0]; trs = af.rstd;
  }
  double s1 = 0.0, s2 = 0.0, sa = 0.0;                             // SUMS: this lane's share of row krow over the slice
  for (int b = b0; b < b1; ++b) {
    const int buf = (b - b0) & 1;
    const bool more = b + 1 < b1;
    __syncthreads();                                              // dy[b] is in sDY[buf], x[b] in the waves' rows; the other dy buffer is free
    // this lane's share of x[b][kw + l15][:]: four consecutive v per slot (v = 4 slot + s) and the second half (16 + ..); rows outside the
    // tensor and columns v >= V hold zeros (or what a dx tile left there: W^T dy of zeros), they meet dy = 0 or rows of dW that are not stored
    const cg_f32x4 xa4 = *reinterpret_cast<const cg_f32x4*>(sXw + l15 * XS + 4 * slot);
    const cg_f32x4 xc4 = *reinterpret_cast<const cg_f32x4*>(sXw + l15 * XS + 16 + 4 * slot);
    float xa[4] = {xa4[0], xa4[1], xa4[2], xa4[3]}, xc[4] = {xc4[0], xc4[1], xc4[2], xc4[3]};
    if (tr) {
#pragma unroll
      for (int s = 0; s < 4; ++s) { xa[s] = cg_prelu(cg_rows_u(xa[s], tm, ts, tb), ta); xc[s] = cg_prelu(cg_rows_u(xc[s], tm, ts, tb), ta); }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                              // every lane holds its operand: the rows are free for the dx tile
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (more) stage_load(b + 1);                                  // in flight over the matrix work below
    const float* dyb = sDY + buf * 16 * g.OT * DS;
    float* dxb = t.dx + (long long)b * K * V;
    // dx[k][v] = sum_o W[o][k] dy[o][v]: rows k of this wave, both halves of v
    cg_f32x4 c0 = cg_f32x4{0.f, 0.f, 0.f, 0.f}, c1 = c0;
    for (int oc = 0; oc < 16 * g.OT; oc += 16) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int o = oc + 4 * slot + s;
        const float w = sW[o * WS + 16 * wave + l15];              // A[i = k][kk = o]
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w, dyb[o * DS + l15], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w, dyb[o * DS + 16 + l15], c1, 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sXw[(4 * slot + q) * XS + l15] = c0[q];
      sXw[(4 * slot + q) * XS + 16 + l15] = c1[q];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    {
      float dv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) dv[j] = sXw[xo[j]];
#pragma unroll
      for (int r = 0; r < NG; ++r)
        if (xok[r]) cg_rows_stv<VW>(dxb + xg[r], dv + VW * r);
    }
    if constexpr (SUMS) {
      // one more read of the rows, in the operand pattern: dh next to the raw x this lane still holds (xa4 / xc4).  No mask: rows
      // k >= K and columns v >= V of the tile are W^T dy of zeros
      const cg_f32x4 ha4 = *reinterpret_cast<const cg_f32x4*>(sXw + l15 * XS + 4 * slot);
      const cg_f32x4 hc4 = *reinterpret_cast<const cg_f32x4*>(sXw + l15 * XS + 16 + 4 * slot);
      float p1 = 0.f, p2 = 0.f, pa = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        cg_rows_sum_term(xa4[s], ha4[s], tm, ts, tb, trs, ta, p1, p2, pa);
        cg_rows_sum_term(xc4[s], hc4[s], tm, ts, tb, trs, ta, p1, p2, pa);
      }
      s1 += (double)p1; s2 += (double)p2; sa += (double)pa;
    }
    // dW[o][k] += sum_v dy[o][v] x[k][v]: A[i = o][kk = v] from LDS (float4 along v), B[kk = v][j = k] = this lane's x values
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < g.OT) {
        const float4 d0 = *reinterpret_cast<const float4*>(dyb + (16 * i + l15) * DS + 4 * slot);
        const float4 d1 = *reinterpret_cast<const float4*>(dyb + (16 * i + l15) * DS + 16 + 4 * slot);
        const float e0[4] = {d0.x, d0.y, d0.z, d0.w}, e1[4] = {d1.x, d1.y, d1.z, d1.w};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          wacc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(e0[s], xa[s], wacc[i], 0, 0, 0);
          wacc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(e1[s], xc[s], wacc[i], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                              // the dx tile has left the rows
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (more) stage_write(buf ^ 1);
  }
  if constexpr (SUMS) cg_rows_put_sums(reinterpret_cast<double*>(cg_dyn_lds), s1, s2, sa, t.sums, g.kranges, sl, kr, tid);
  cg_rows_put_dw<4>(sW, wacc, g.OT, t.ws + (long long)sl * O * K, O, K, k0, tid, wave, l15, slot);
}

// dW[e] = sum over the slices' partials.  A workgroup takes 64 consecutive elements, its four waves every fourth slice; the order of the
// sum is fixed, so dW is the same from run to run.
// SUMS: the launch also folds the row sums of the backward kernel (CgRowsConv.sums) into `red`, dgamma, dbeta, dalpha - channel c by
// workgroup c (mod the grid), the slope by the last workgroup; 256 threads take the (slice, row) entries in a fixed assignment, then a tree.
__device__ __forceinline__ void cg_rows_fold_tree(double (*sR)[CG_ROWS_BWD_THREADS], int tid) {
  __syncthreads();
  for (int w = CG_ROWS_BWD_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) { sR[0][tid] += sR[0][tid + w]; sR[1][tid] += sR[1][tid + w]; }
    __syncthreads();
  }
}
template <bool SUMS>
__global__ __launch_bounds__(CG_ROWS_BWD_THREADS) void cg_rows_fold_kernel(CgRowsArgs a) {
  const CgRowsConv& t = a.t;
  if constexpr (SUMS) {
    __shared__ double sR[2][CG_ROWS_BWD_THREADS];
    const int tid = threadIdx.x, C = t.C, rpc = a.g.rpc, kranges = a.g.kranges;
    const long long Kp = (long long)kranges * CG_ROWS_KB, stride = cg_rows_sums_stride(kranges);
    for (int c = blockIdx.x; c < C; c += gridDim.x) {
      double a1 = 0.0, a2 = 0.0;
      for (int e = tid; e < a.g.slices * rpc; e += CG_ROWS_BWD_THREADS) {
        const int r = e / rpc;
        const double* q = t.sums + r * stride + (long long)c * rpc + (e - r * rpc);
        a1 += q[0]; a2 += q[Kp];
      }
      sR[0][tid] = a1; sR[1][tid] = a2;
      cg_rows_fold_tree(sR, tid);
      if (tid == 0) {
        t.red[2 * c] = sR[0][0]; t.red[2 * c + 1] = sR[1][0];
        if (t.dbeta) t.dbeta[c] = (float)sR[0][0];
        if (t.dgamma) t.dgamma[c] = (float)sR[1][0];
      }
      __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1) {
      double a1 = 0.0;
      for (int e = tid; e < a.g.slices * kranges; e += CG_ROWS_BWD_THREADS) {
        const int r = e / kranges;
        a1 += t.sums[r * stride + 2 * Kp + (e - r * kranges)];
      }
      sR[0][tid] = a1; sR[1][tid] = 0.0;
      cg_rows_fold_tree(sR, tid);
      if (tid < CG_ALPHA_SLOTS) t.red[2 * C + tid] = tid == 0 ? sR[0][0] : 0.0;      // the total in the first slot: cg_alpha_sum adds all of them
      if (tid == 0 && t.dalpha) t.dalpha[0] = (float)sR[0][0];
    }
  }
  __shared__ float part[CG_ROWS_BWD_THREADS / 64][64];
  const long long n = (long long)t.O * a.g.K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long e = (long long)blockIdx.x * 64 + lane, ec = e < n ? e : n - 1;
  float s = 0.f;
#pragma unroll 4
  for (int r = wave; r < a.g.slices; r += CG_ROWS_BWD_THREADS / 64) s += t.ws[r * n + ec];
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && e < n) t.dW[e] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// ======================================================================================================================
// The same for the JOINT axis (reference: nn.Conv2d(C, O, (1, V)) of Map2Adj.joint_compress, CISTGCN.py:152-163):
//   y[b,o,t] = sum_{c,v} W[o,c,v] x[b,c,t,v]        per sample  Y_b (O x T) = W (O x K) X_b (K x T),  K = C * V
// x[b] lies in memory as [c][t][v]: row k = (c, v) of X_b is a column of stride V.  A lane's four consecutive k of an MFMA step are
// four consecutive v of one frame (a 16-byte run; a step that crosses from channel c to c + 1 splits), the 16 lanes of a row take 16
// frames.  Round 3 ran this through the generic contraction (split-K with atomics: 92 / 154 us per block next to the gate items).
//   forward   one 512-thread workgroup per sample, eight waves split K, operands straight from global memory, DEPTH groups in flight
//   backward  a workgroup owns 64 rows k for a slice of the samples (dx[b,k,t] from W^T dy, dW[o,k] in registers over the slice)
// T <= 64 (NT tiles of 16 frames), O <= 64, C * V % 4 == 0.
// ======================================================================================================================
template <int OT, int NT>
__global__ __launch_bounds__(CG_ROWS_FWD_THREADS) void cg_cols_fwd_kernel(CgRowsArgs a, unsigned magicV) {
  const CgRowsConv& t = a.t; const CgRowsGeom& g = a.g;
  const int b = blockIdx.x, K = g.K, V = t.V, T = t.T, O = t.O, TV = T * V;
  constexpr int nw = CG_ROWS_FWD_THREADS / 64, DEPTH = 3, YS = 16 * NT + 1;
  float* sY = reinterpret_cast<float*>(cg_dyn_lds);              // [nw][16 * OT][YS] partial tiles of the eight waves
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, slot = lane >> 4;
  const float* xb = t.x + (long long)b * K * T;
  cg_f32x4 acc[OT][NT];
#pragma unroll
  for (int i = 0; i < OT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = cg_f32x4{0.f, 0.f, 0.f, 0.f};
  const int ngroups = (K + 15) >> 4;
  const float* wrow[OT];
#pragma unroll
  for (int i = 0; i < OT; ++i) wrow[i] = t.W + (long long)min(16 * i + l15, O - 1) * K;
  int toff[NT];                                                   // frame of this lane in tile j (clamped: columns t >= T are never stored)
#pragma unroll
  for (int j = 0; j < NT; ++j) toff[j] = min(16 * j + l15, T - 1) * V;
  float* sTab = sY + nw * 16 * OT * YS;                           // [C][4] input transform: mean, gamma * rstd, beta, -
  const bool tr = t.in_on != 0;
  const float in_alpha = tr ? t.in_alpha[0] : 1.f;
  float* const tapb = (tr && t.in_tap) ? t.in_tap + (long long)b * K * T : nullptr;
  if (tr) {
    for (int c = tid; c < t.C; c += CG_ROWS_FWD_THREADS) {
      const CgAff af = cg_tail_aff(t.in_bn, c, t.C, (double)t.B * T * V, t.in_train, false, blockIdx.x == 0);
      sTab[4 * c] = af.mean; sTab[4 * c + 1] = af.gamma * af.rstd; sTab[4 * c + 2] = af.beta; sTab[4 * c + 3] = 0.f;
    }
    __syncthreads();
  }
  struct Frag { float4 w[OT]; float x[NT][4]; float mask; int kc; };
  auto load = [&](int gi, Frag& f) {
    const int k = 16 * gi + 4 * slot;
    const bool kin = k < K;                                       // K % 4 == 0
    const int kc = kin ? k : K - 4;
    f.mask = kin ? 1.f : 0.f; f.kc = kc;
#pragma unroll
    for (int i = 0; i < OT; ++i) f.w[i] = *reinterpret_cast<const float4*>(wrow[i] + kc);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kk = kc + s, c = (int)cg_div((unsigned)kk, magicV), v = kk - c * V;
      const float* xr = xb + c * TV + v;
#pragma unroll
      for (int j = 0; j < NT; ++j) f.x[j][s] = xr[toff[j]];
    }
  };
  auto mma = [&](Frag& f) {
    if (tr) {                                               // PReLU(BatchNorm(x)) of the rows k = (c, v) of this lane
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int c = (int)cg_div((unsigned)(f.kc + s), magicV);
        const float4 k4 = *reinterpret_cast<const float4*>(sTab + 4 * c);
#pragma unroll
        for (int j = 0; j < NT; ++j) f.x[j][s] = cg_prelu((f.x[j][s] - k4.x) * k4.y + k4.z, in_alpha);
        if (tapb && f.mask != 0.f) {
          const int v = f.kc + s - c * V;
#pragma unroll
          for (int j = 0; j < NT; ++j) tapb[c * TV + toff[j] + v] = f.x[j][s];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < OT; ++i) {
      const float w4[4] = {f.w[i].x * f.mask, f.w[i].y * f.mask, f.w[i].z * f.mask, f.w[i].w * f.mask};
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[s], f.x[j][s], acc[i][j], 0, 0, 0);
    }
  };
  Frag f[DEPTH];
#pragma unroll
  for (int j = 0; j < DEPTH; ++j)
    if (wave + j * nw < ngroups) load(wave + j * nw, f[j]);
  for (int gi = wave; gi < ngroups; gi += DEPTH * nw) {
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      const int gj = gi + j * nw;
      if (gj < ngroups) {
        mma(f[j]);
        if (gj + DEPTH * nw < ngroups) load(gj + DEPTH * nw, f[j]);
      }
    }
  }
  float* mine = sY + wave * 16 * OT * YS;
#pragma unroll
  for (int i = 0; i < OT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) mine[(16 * i + 4 * slot + q) * YS + 16 * j + l15] = acc[i][j][q];
  __syncthreads();
  for (int e = tid; e < O * T; e += CG_ROWS_FWD_THREADS) {
    const int o = e / T, tt = e - o * T;
    float y = 0.f;
#pragma unroll
    for (int w = 0; w < nw; ++w) y += sY[(w * 16 * OT + o) * YS + tt];
    t.y[(long long)b * O * T + e] = y;
    sY[o * YS + tt] = y;                                   // this thread's own element of slot 0: the channel sums below read it
  }
  if (t.stats) {
    __syncthreads();
    for (int o = tid; o < O; o += CG_ROWS_FWD_THREADS) {
      double s1 = 0.0, s2 = 0.0;
      for (int tt = 0; tt < T; ++tt) { const double y = (double)sY[o * YS + tt]; s1 += y; s2 += y * y; }
      double* rep = t.stats + ((long long)(b % CG_STAT_REPLICAS) * O + o) * 2;
      atomicAdd(&rep[0], s1); atomicAdd(&rep[1], s2);
    }
  }
}

// SUMS (see cg_rows_sum_term): the lane's x operand is row l15 with four consecutive frames per slot, its dx results are the rows 4 slot + q
// at frame l15 - the tile is turned through 16 wave-private LDS rows of 16 NT frames, so that dh meets the raw x in the operand layout,
// where a lane has one channel.
template <int OT, int NT, bool SUMS>
__global__ __launch_bounds__(CG_ROWS_BWD_THREADS, (SUMS && OT <= 2) ? 2 : 1) void cg_cols_bwd_kernel(CgRowsArgs a, unsigned magicV) {
  const CgRowsConv& t = a.t; const CgRowsGeom& g = a.g;
  const int K = g.K, V = t.V, T = t.T, O = t.O, TV = T * V;
  const int kr = blockIdx.x, sl = blockIdx.y, k0 = kr * CG_ROWS_KB;
  const int b0 = sl * g.per, b1 = min(t.B, b0 + g.per);
  if (b0 >= t.B) return;
  constexpr int WS = CG_ROWS_KB + 4, DS = 16 * NT + 4;
  float* sW = reinterpret_cast<float*>(cg_dyn_lds);              // [16 * OT][KB + 4]  W[o][k0 ..]
  float* sDY = sW + 16 * OT * WS;                                 // [2][16 * OT][DS]   dy of the current / next sample, frames padded with zeros
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, slot = lane >> 4;
  for (int e0 = tid; e0 < 16 * OT * WS; e0 += 8 * CG_ROWS_BWD_THREADS) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = e0 + CG_ROWS_BWD_THREADS * j, o = e / WS, kk = e - o * WS;
      const bool in = o < O && kk < CG_ROWS_KB && k0 + kk < K;
      v[j] = t.W[in ? (long long)o * K + k0 + kk : (long long)k0];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = e0 + CG_ROWS_BWD_THREADS * j, o = e / WS, kk = e - o * WS;
      if (e < 16 * OT * WS) sW[e] = (o < O && kk < CG_ROWS_KB && k0 + kk < K) ? v[j] : 0.f;
    }
  }
  for (int e = tid; e < 2 * 16 * OT * DS; e += CG_ROWS_BWD_THREADS) sDY[e] = 0.f;
  __syncthreads();
  // dy[b] (O * T <= 256 * OT * NT floats) global -> registers -> [o][DS] rows of sDY, split: the loads of sample b + 1 are issued in front of the
  // matrix work of sample b and stored behind it.  Element j of this thread; outside dy the first element stands in for the load and
  // column DS - 1 of row 0, which nobody reads, for the store.
  int dyo[OT * NT];
#pragma unroll
  for (int j = 0; j < OT * NT; ++j) {
    const int e = tid + CG_ROWS_BWD_THREADS * j, o = e / T;
    dyo[j] = e < O * T ? o * DS + (e - o * T) : DS - 1;
  }
  float dr[OT * NT];
  auto dy_load = [&](int b) {
    const float* src = t.dy + (long long)b * O * T;
#pragma unroll
    for (int j = 0; j < OT * NT; ++j) { const int e = tid + CG_ROWS_BWD_THREADS * j; dr[j] = src[e < O * T ? e : 0]; }
  };
  auto dy_write = [&](int buf) {
    float* dst = sDY + buf * 16 * OT * DS;
#pragma unroll
    for (int j = 0; j < OT * NT; ++j) dst[dyo[j]] = dr[j];
  };
  dy_load(b0);
  dy_write(0);
  // a wave owns the 16 rows k = k0 + 16 wave + .. of the range: dW tiles [o][k] in registers over the slice
  cg_f32x4 wacc[OT];
#pragma unroll
  for (int i = 0; i < OT; ++i) wacc[i] = cg_f32x4{0.f, 0.f, 0.f, 0.f};
  const int kw = k0 + 16 * wave;
  // row k = (c, v) of this lane as the B operand of the dW product (x[b][c][t][v], t = 16 tt + 4 slot + s), clamped: rows k >= K are never stored
  const int kl = min(kw + l15, K - 1), cl = (int)cg_div((unsigned)kl, magicV);
  const int xoff = cl * TV + (kl - cl * V);
  int tx[NT][4];
#pragma unroll
  for (int tt = 0; tt < NT; ++tt)
#pragma unroll
    for (int s = 0; s < 4; ++s) tx[tt][s] = min(16 * tt + 4 * slot + s, T - 1) * V;      // frames >= T meet dy = 0
  // rows k = kw + 4 slot + q of this lane's dx results
  int doff[4]; bool dok[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = kw + 4 * slot + q, kc = min(k, K - 1), c = (int)cg_div((unsigned)kc, magicV);
    doff[q] = c * TV + (kc - c * V); dok[q] = k < K;
  }
  auto load_x = [&](int b, float xv[NT][4]) {
    const float* xr = t.x + (long long)b * K * T + xoff;
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
      for (int s = 0; s < 4; ++s) xv[tt][s] = xr[tx[tt][s]];
  };
  const bool tr = t.in_on != 0;                                   // optional input transform: this lane's row k = (c, v) has one channel
  float tm = 0.f, ts = 1.f, tb = 0.f, ta = 1.f, trs = 1.f;
  if (tr) {
    const CgAff af = cg_tail_aff(t.in_bn, cl, t.C, 0.0, t.in_train, true, false);
    tm = af.mean; ts = af.gamma * af.rstd; tb = af.beta; ta = t.in_alpha[0]; trs = af.rstd;
  }
  auto act = [&](float xv[NT][4]) {
    if (tr) {
#pragma unroll
      for (int tt = 0; tt < NT; ++tt)
#pragma unroll
        for (int s = 0; s < 4; ++s) xv[tt][s] = cg_prelu(cg_rows_u(xv[tt][s], tm, ts, tb), ta);
    }
  };
  double s1 = 0.0, s2 = 0.0, sa = 0.0;                             // SUMS: this lane's share of row kl over the slice
  // x[b] is taken over from the registers it was loaded into at the top of its own iteration, in front of the loads of sample b + 1: the one
  // place where a load is waited for (the first sample's operand used to be loaded straight into `xa`; the compiler then could not tell
  // those loads from the ones in flight and waited out the loads of sample b + 1 in front of the dW products of sample b)
  float xa[NT][4], xn[NT][4], xraw[SUMS ? NT : 1][4];
  load_x(b0, xn);
  for (int b = b0; b < b1; ++b) {
    const int buf = (b - b0) & 1;
    __syncthreads();                                              // dy[b] is in sDY[buf]; the other buffer is free
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        xa[tt][s] = xn[tt][s];
        if constexpr (SUMS) xraw[tt][s] = xn[tt][s];              // the raw value: xhat and the branch cannot be had from the activated one
      }
    act(xa);
    if (b + 1 < b1) { dy_load(b + 1); load_x(b + 1, xn); }
    const float* dyb = sDY + buf * 16 * OT * DS;
    float* dxb = t.dx + (long long)b * K * T;
    // dx[k][t] = sum_o W[o][k] dy[o][t]: rows k of this wave, NT tiles of frames
    cg_f32x4 c[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) c[j] = cg_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int oc = 0; oc < 16 * OT; oc += 16) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int o = oc + 4 * slot + s;
        const float w = sW[o * WS + 16 * wave + l15];              // A[i = k][kk = o]
#pragma unroll
        for (int j = 0; j < NT; ++j) c[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, dyb[o * DS + 16 * j + l15], c[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int tt = 16 * j + l15;
      if (tt < T) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (dok[q]) dxb[doff[q] + tt * V] = c[j][q];
      }
    }
    if constexpr (SUMS) {
      // No mask: rows k >= K meet zero rows of W, frames t >= T zero columns of dy - dh is 0 where this lane's x is the clamped
      // duplicate of row K - 1 or of frame T - 1.
      float* sTw = sDY + 2 * 16 * OT * DS + wave * 16 * DS;        // [4 waves][16][DS] behind the dy buffers: a wave's dx tile, rows k x frames
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) sTw[(4 * slot + q) * DS + 16 * j + l15] = c[j][q];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const cg_f32x4 h4 = *reinterpret_cast<const cg_f32x4*>(sTw + l15 * DS + 16 * tt + 4 * slot);
        float p1 = 0.f, p2 = 0.f, pa = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) cg_rows_sum_term(xraw[tt][s], h4[s], tm, ts, tb, trs, ta, p1, p2, pa);
        s1 += (double)p1; s2 += (double)p2; sa += (double)pa;
      }
    }
    // dW[o][k] += sum_t dy[o][t] x[k][t]: A[i = o][kk = t] from LDS (float4 along t), B[kk = t][j = k] = this lane's x values
#pragma unroll
    for (int i = 0; i < OT; ++i) {
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const float4 d4 = *reinterpret_cast<const float4*>(dyb + (16 * i + l15) * DS + 16 * tt + 4 * slot);
        const float e4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int s = 0; s < 4; ++s) wacc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(e4[s], xa[tt][s], wacc[i], 0, 0, 0);
      }
    }
    if (b + 1 < b1) dy_write(buf ^ 1);
  }
  if constexpr (SUMS) cg_rows_put_sums(reinterpret_cast<double*>(cg_dyn_lds), s1, s2, sa, t.sums, g.kranges, sl, kr, tid);
  cg_rows_put_dw<OT>(sW, wacc, OT, t.ws + (long long)sl * O * K, O, K, k0, tid, wave, l15, slot);
}

// ---- host side ---------------------------------------------------------------------------------------------------
static int cg_rows_geometry(const CgRowsConv* t, CgRowsGeom* g) {
  if (!t || !t->x || !t->W) return CG_EARG;
  if (t->B <= 0 || t->C <= 0 || t->T <= 0 || t->V <= 0 || t->V > 32 || t->O <= 0 || t->O > 64) return CG_ESHAPE;
  const long long K = (long long)t->C * t->T;
  if (K > (1 << 20) || (K & 3) || K * t->T >= (1ll << 32)) return CG_ESHAPE;      // K * T: the channel of row k = (c, t) is cg_div(k, T)
  g->K = (int)K; g->OT = (t->O + 15) / 16;
  g->kranges = (g->K + CG_ROWS_KB - 1) / CG_ROWS_KB;
  int slices = 768 / g->kranges;                        // ~768 backward workgroups (1024-1536: 53 us against 46 us on the tower tensors, round 4)
  slices = slices < 1 ? 1 : (slices > t->B ? t->B : slices);
  g->per = (t->B + slices - 1) / slices;
  g->slices = (t->B + g->per - 1) / g->per;
  g->rpc = t->T;
  return CG_OK;
}

// one dW partial per sample slice, for the most slices the geometry can choose at this K (any B)
static long long cg_rows_ws(long long K, int O) {
  const long long kranges = (K + CG_ROWS_KB - 1) / CG_ROWS_KB, slices = 768 / kranges;
  return (slices < 1 ? 1 : slices) * O * K;
}
extern "C" long long cg_collapse_rows_ws_floats(int C, int T, int O) { return cg_rows_ws((long long)C * T, O); }
// include/cistgcn_hip.h : floats of CgRowsConv.sums (f64 partials of the most slices the geometry can choose at K = C * rows, any B)
extern "C" long long cg_collapse_sums_ws_floats(int C, int rows) {
  const long long K = (long long)C * rows, kranges = (K + CG_ROWS_KB - 1) / CG_ROWS_KB, slices = 768 / kranges;
  return 2 * (slices < 1 ? 1 : slices) * cg_rows_sums_stride((int)kranges);
}
// the optional sums of the backward: 1 asked for, 0 not, < 0 a bad combination
static int cg_rows_want_sums(const CgRowsConv* t) {
  if (!t->sums && !t->red) return (t->dgamma || t->dbeta || t->dalpha) ? CG_EARG : 0;
  return (t->sums && t->red && t->in_on) ? 1 : CG_EARG;
}

static int cg_rows_fold(const CgRowsArgs& a, int sums, hipStream_t stream) {
  const dim3 grid((unsigned)(((long long)a.t.O * a.g.K + 63) / 64)), block(CG_ROWS_BWD_THREADS);
  if (sums) hipLaunchKernelGGL(cg_rows_fold_kernel<true>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(cg_rows_fold_kernel<false>, grid, block, 0, stream, a);
  return cg_launch_status();
}

// include/cistgcn_hip.h : cg_collapse_rows_fwd / cg_collapse_rows_bwd
extern "C" int cg_collapse_rows_fwd(const CgRowsConv* t, void* stream_) {
  CgRowsArgs a;
  int st = cg_rows_geometry(t, &a.g);
  if (st != CG_OK) return st;
  if (!t->y) return CG_EARG;
  a.t = *t;
  if (t->in_on && (!t->in_alpha || !t->in_bn.gamma || !t->in_bn.beta || !t->in_bn.save || (t->in_train ? !t->in_bn.stats : !t->in_bn.running_mean))) return CG_EARG;
  const size_t lds = ((size_t)(CG_ROWS_FWD_THREADS / 64) * 16 * a.g.OT * 33 + (size_t)4 * t->C) * sizeof(float);
  const dim3 grid((unsigned)t->B), block(CG_ROWS_FWD_THREADS);
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned magicT = cg_div_magic(t->T);
#define CG_ROWS_FWD_LAUNCH(N)                                                                   \
  {                                                                                            \
    hipError_t e = cg_lds_limit((const void*)cg_rows_fwd_kernel<N>, lds);                       \
    if (e != hipSuccess) return (int)e;                                                        \
    hipLaunchKernelGGL((cg_rows_fwd_kernel<N>), grid, block, lds, stream, a, magicT);            \
  }
  switch (a.g.OT) {
    case 1: CG_ROWS_FWD_LAUNCH(1) break;
    case 2: CG_ROWS_FWD_LAUNCH(2) break;
    case 3: CG_ROWS_FWD_LAUNCH(3) break;
    default: CG_ROWS_FWD_LAUNCH(4) break;
  }
#undef CG_ROWS_FWD_LAUNCH
  return cg_launch_status();
}

extern "C" int cg_collapse_rows_bwd(const CgRowsConv* t, void* stream_) {
  CgRowsArgs a;
  int st = cg_rows_geometry(t, &a.g);
  if (st != CG_OK) return st;
  if (!t->dy || !t->dx || !t->dW || !t->ws) return CG_EARG;
  if (t->in_on && (!t->in_alpha || !t->in_bn.gamma || !t->in_bn.beta || !t->in_bn.save)) return CG_EARG;
  const int sums = cg_rows_want_sums(t);
  if (sums < 0) return sums;
  a.t = *t;
  const size_t lds = ((size_t)16 * a.g.OT * (CG_ROWS_KB + 4) + (size_t)2 * 16 * a.g.OT * 36 + (size_t)(CG_ROWS_BWD_THREADS / 64) * 16 * CG_ROWS_XS) * sizeof(float);
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)a.g.kranges, (unsigned)a.g.slices), block(CG_ROWS_BWD_THREADS);
  // 16-byte runs where every sample's dy, x and dx piece is 16-byte aligned (the pieces of x and dx are whole multiples of four floats)
  const bool wide = ((long long)t->O * t->V) % 4 == 0 && (((uintptr_t)t->dy | (uintptr_t)t->x | (uintptr_t)t->dx) & 15) == 0;
  if (sums) {
    if (wide) hipLaunchKernelGGL((cg_rows_bwd_kernel<4, true>), grid, block, lds, stream, a);
    else hipLaunchKernelGGL((cg_rows_bwd_kernel<1, true>), grid, block, lds, stream, a);
  } else {
    if (wide) hipLaunchKernelGGL((cg_rows_bwd_kernel<4, false>), grid, block, lds, stream, a);
    else hipLaunchKernelGGL((cg_rows_bwd_kernel<1, false>), grid, block, lds, stream, a);
  }
  st = cg_launch_status();
  if (st != CG_OK) return st;
  return cg_rows_fold(a, sums, stream);
}

// ---- joint axis ----
static int cg_cols_geometry(const CgRowsConv* t, CgRowsGeom* g) {
  if (!t || !t->x || !t->W) return CG_EARG;
  if (t->B <= 0 || t->C <= 0 || t->T <= 0 || t->V <= 0 || t->T > 64 || t->O <= 0 || t->O > 64) return CG_ESHAPE;
  const long long K = (long long)t->C * t->V;
  if (K > (1 << 20) || (K & 3) || K * t->T >= (1ll << 31) || K * t->V >= (1ll << 32)) return CG_ESHAPE;      // K * V: cg_div(k, V)
  g->K = (int)K; g->OT = (t->O + 15) / 16;
  g->kranges = (g->K + CG_ROWS_KB - 1) / CG_ROWS_KB;
  int slices = 768 / g->kranges;
  slices = slices < 1 ? 1 : (slices > t->B ? t->B : slices);
  g->per = (t->B + slices - 1) / slices;
  g->slices = (t->B + g->per - 1) / g->per;
  g->rpc = t->V;
  return CG_OK;
}
static int cg_cols_nt(int T) { return T <= 16 ? 1 : T <= 32 ? 2 : 4; }

extern "C" int cg_collapse_cols_supported(int C, int T, int V, int O) { return T >= 1 && T <= 64 && O >= 1 && O <= 64 && (((long long)C * V) & 3) == 0 ? 1 : 0; }
extern "C" long long cg_collapse_cols_ws_floats(int C, int V, int O) { return cg_rows_ws((long long)C * V, O); }

// include/cistgcn_hip.h : host-only, the backward grid of cg_collapse_rows_bwd (cols == 0) / cg_collapse_cols_bwd (no launch)
extern "C" int cg_collapse_geometry(int B, int C, int T, int V, int O, int cols, int* out) {
  if (!out) return CG_EARG;
  static const float dummy = 0.f;               // the geometry refuses null operands; it never reads them
  CgRowsConv t = {};
  t.B = B; t.C = C; t.T = T; t.V = V; t.O = O; t.x = &dummy; t.W = &dummy;
  CgRowsGeom g;
  const int st = cols ? cg_cols_geometry(&t, &g) : cg_rows_geometry(&t, &g);
  if (st != CG_OK) return st;
  out[0] = g.kranges; out[1] = g.slices; out[2] = g.per;
  return CG_OK;
}

#define CG_COLS_DISPATCH(OT_, NT_, LAUNCH)                         \
  switch (4 * ((OT_) - 1) + ((NT_) == 1 ? 0 : (NT_) == 2 ? 1 : 2)) { \
    case 0: LAUNCH(1, 1) break; case 1: LAUNCH(1, 2) break; case 2: LAUNCH(1, 4) break;       \
    case 4: LAUNCH(2, 1) break; case 5: LAUNCH(2, 2) break; case 6: LAUNCH(2, 4) break;       \
    case 8: LAUNCH(3, 1) break; case 9: LAUNCH(3, 2) break; case 10: LAUNCH(3, 4) break;      \
    case 12: LAUNCH(4, 1) break; case 13: LAUNCH(4, 2) break; default: LAUNCH(4, 4) break;    \
  }

// include/cistgcn_hip.h : cg_collapse_cols_fwd / cg_collapse_cols_bwd
extern "C" int cg_collapse_cols_fwd(const CgRowsConv* t, void* stream_) {
  CgRowsArgs a;
  int st = cg_cols_geometry(t, &a.g);
  if (st != CG_OK) return st;
  if (!t->y) return CG_EARG;
  a.t = *t;
  const int nt = cg_cols_nt(t->T);
  if (t->in_on && (!t->in_alpha || !t->in_bn.gamma || !t->in_bn.beta || !t->in_bn.save || (t->in_train ? !t->in_bn.stats : !t->in_bn.running_mean))) return CG_EARG;
  const size_t lds = ((size_t)(CG_ROWS_FWD_THREADS / 64) * 16 * a.g.OT * (16 * nt + 1) + (size_t)4 * t->C + 4) * sizeof(float);
  const dim3 grid((unsigned)t->B), block(CG_ROWS_FWD_THREADS);
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned magic = cg_div_magic(t->V);
#define CG_COLS_FWD_LAUNCH(N, M)                                                                \
  {                                                                                            \
    hipError_t e = cg_lds_limit((const void*)cg_cols_fwd_kernel<N, M>, lds);                    \
    if (e != hipSuccess) return (int)e;                                                        \
    hipLaunchKernelGGL((cg_cols_fwd_kernel<N, M>), grid, block, lds, stream, a, magic);          \
  }
  CG_COLS_DISPATCH(a.g.OT, nt, CG_COLS_FWD_LAUNCH)
#undef CG_COLS_FWD_LAUNCH
  return cg_launch_status();
}

extern "C" int cg_collapse_cols_bwd(const CgRowsConv* t, void* stream_) {
  CgRowsArgs a;
  int st = cg_cols_geometry(t, &a.g);
  if (st != CG_OK) return st;
  if (!t->dy || !t->dx || !t->dW || !t->ws) return CG_EARG;
  if (t->in_on && (!t->in_alpha || !t->in_bn.gamma || !t->in_bn.beta || !t->in_bn.save)) return CG_EARG;
  const int sums = cg_rows_want_sums(t);
  if (sums < 0) return sums;
  a.t = *t;
  const int nt = cg_cols_nt(t->T);
  const size_t lds = ((size_t)16 * a.g.OT * (CG_ROWS_KB + 4) + (size_t)2 * 16 * a.g.OT * (16 * nt + 4) +
                      (sums ? (size_t)(CG_ROWS_BWD_THREADS / 64) * 16 * (16 * nt + 4) : 0)) * sizeof(float);
  const dim3 grid((unsigned)a.g.kranges, (unsigned)a.g.slices), block(CG_ROWS_BWD_THREADS);
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned magic = cg_div_magic(t->V);
#define CG_COLS_BWD_LAUNCH_S(N, M, S)                                                           \
  {                                                                                            \
    hipError_t e = cg_lds_limit((const void*)cg_cols_bwd_kernel<N, M, S>, lds);                 \
    if (e != hipSuccess) return (int)e;                                                        \
    hipLaunchKernelGGL((cg_cols_bwd_kernel<N, M, S>), grid, block, lds, stream, a, magic);       \
  }
#define CG_COLS_BWD_LAUNCH(N, M) CG_COLS_BWD_LAUNCH_S(N, M, false)
#define CG_COLS_BWD_LAUNCH_SUMS(N, M) CG_COLS_BWD_LAUNCH_S(N, M, true)
  if (sums) { CG_COLS_DISPATCH(a.g.OT, nt, CG_COLS_BWD_LAUNCH_SUMS) }
  else { CG_COLS_DISPATCH(a.g.OT, nt, CG_COLS_BWD_LAUNCH) }
#undef CG_COLS_BWD_LAUNCH_SUMS
#undef CG_COLS_BWD_LAUNCH
#undef CG_COLS_BWD_LAUNCH_S
  st = cg_launch_status();
  if (st != CG_OK) return st;
  return cg_rows_fold(a, sums, stream);
}
