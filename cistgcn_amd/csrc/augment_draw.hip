// The random draws of the augmentations on the device: what environment/input_pipeline.py::DeviceAugmentation.draw /
// RobustnessTest.draw do on the host with np.random, sample by sample, here from the device-resident seed word of the dropout
// with the counter-based generator of cg_common.h (cg_drop_bits).  (include/cistgcn_hip.h: cg_draw_augmentation gives the generator -
// salts, counters, the fp32 uniform -, the two table layouts and the return codes.)  The seed is read, never written: a captured
// step advances it with cg_seed_bump and then draws, so every replay augments differently without a host round trip.
//   cg_draw_kernel   one thread per (sample, step) fills that step's entries of the table; one thread per element fills the noise
//                    draws.  The step list arrives by value with the launch.  Grid-stride, no LDS, no barriers, no atomics.
#include "cg_common.h"
#include "cg_rotvec.h"

#define CG_DRAW_NPAR 24                         // a row of cg_augment_sequences (CG_AUG_NPAR of input_pipeline.hip)
#define CG_DRAW_KINDS (CG_PERTURB_INVERT + 1)

// the validated host step list, passed by value
struct CgDrawPlan {
  CgDrawStep st[CG_PERTURB_MAX_STEPS];
  unsigned char fills[CG_PERTURB_MAX_STEPS];    // CG_DRAW_TABLE24: this step fills the columns of its kind (the last step of the kind)
  int absent;                                   // CG_DRAW_TABLE24: bit k set = no step of kind k, its columns keep the identity
};

// u in [0, 1): the top 24 bits of the hash, exact in fp32
__device__ __forceinline__ float cg_draw_u(unsigned long long seed, unsigned int salt, unsigned long long counter) {
  return (float)(unsigned int)(cg_drop_bits(seed, salt, counter) >> 40) * 5.9604644775390625e-8f;      // 2^-24
}

// lo + (hi - lo) * u in f64 on the fp32 bounds, rounded once
__device__ __forceinline__ float cg_draw_amount(float lo, float hi, float u) {
#pragma clang fp contract(off)
  return (float)((double)lo + ((double)hi - (double)lo) * (double)u);
}

// the columns of `kind` in a row of cg_augment_sequences when the step does not apply (or does not exist)
__device__ __forceinline__ void cg_draw_identity(float* r, int kind) {
  if (kind == CG_PERTURB_FLIP) { r[0] = 0.f; r[1] = 0.f; r[2] = 0.f; }
  else if (kind == CG_PERTURB_ROTATION) { for (int k = 3; k < 13; ++k) r[k] = 0.f; }
  else if (kind == CG_PERTURB_SCALE) { r[13] = 1.f; r[14] = 1.f; r[15] = 1.f; }
  else if (kind == CG_PERTURB_TRANSLATION) { r[16] = 0.f; r[17] = 0.f; r[18] = 0.f; }
  else if (kind == CG_PERTURB_NOISE) r[19] = 0.f;
  else r[20] = 0.f;
}

__global__ __launch_bounds__(CG_DRAW_THREADS) void cg_draw_kernel(const CgDrawPlan plan, const unsigned long long* __restrict__ seed_word,
                                                                  unsigned int stream_id, int n_steps, int layout, long long n_tab,
                                                                  long long n_noise_el, float* __restrict__ table,
                                                                  float* __restrict__ noise_tab) {
  const unsigned long long seed = *seed_word;
  const int per = max(n_steps, 1);                          // threads per sample: TABLE24 writes a row for an empty list too
  const long long total = n_tab + n_noise_el, stride = (long long)gridDim.x * CG_DRAW_THREADS;
  for (long long t = (long long)blockIdx.x * CG_DRAW_THREADS + threadIdx.x; t < total; t += stride) {
    if (t >= n_tab) {                                       // noise element e = ((b * n_noise + slot) * J + j) * 3 + axis
      const long long e = t - n_tab;
      noise_tab[e] = 2.f * cg_draw_u(seed, CG_DRAW_SALT + 0x10000u + stream_id, (unsigned long long)e) - 1.f;
      continue;
    }
    const long long b = t / per;
    const int i = (int)(t - b * per);
    float* r = layout == CG_DRAW_TABLE24 ? table + b * CG_DRAW_NPAR : table + t * 4;
    if (layout == CG_DRAW_TABLE24 && i == 0) {
      for (int k = 0; k < CG_DRAW_KINDS; ++k)
        if ((plan.absent >> k) & 1) cg_draw_identity(r, k);
      r[21] = 0.f; r[22] = 0.f; r[23] = 0.f;
    }
    if (i >= n_steps) continue;
    const CgDrawStep& s = plan.st[i];
    const unsigned long long c0 = ((unsigned long long)b * (unsigned long long)n_steps + (unsigned long long)i) * 4ull;
    const unsigned int salt = CG_DRAW_SALT + stream_id;
    const float u0 = cg_draw_u(seed, salt, c0);
    float row[4] = {0.f, 0.f, 0.f, 0.f};                    // [apply?, v0, v1, v2], the row of cg_perturb_sequences
    if (s.kind == CG_PERTURB_FLIP) {
      row[1] = (s.lo[0] != 0.f && u0 > s.prob_threshold) ? 1.f : 0.f;
      row[2] = (s.lo[1] != 0.f && cg_draw_u(seed, salt, c0 + 1) > s.prob_threshold) ? 1.f : 0.f;
      row[3] = (s.lo[2] != 0.f && cg_draw_u(seed, salt, c0 + 2) > s.prob_threshold) ? 1.f : 0.f;
      row[0] = (row[1] != 0.f || row[2] != 0.f || row[3] != 0.f) ? 1.f : 0.f;
    } else if (u0 > s.prob_threshold) {
      row[0] = 1.f;
      if (s.kind == CG_PERTURB_NOISE) row[1] = s.lo[0];
      else if (s.kind != CG_PERTURB_INVERT)
        for (int a = 0; a < 3; ++a) row[1 + a] = cg_draw_amount(s.lo[a], s.hi[a], cg_draw_u(seed, salt, c0 + 1 + a));
    }
    if (layout == CG_DRAW_STEPS4) {
      r[0] = row[0]; r[1] = row[1]; r[2] = row[2]; r[3] = row[3];
      continue;
    }
    if (!plan.fills[i]) continue;                           // a later step of the same kind fills these columns
    if (s.kind == CG_PERTURB_FLIP) { r[0] = row[1]; r[1] = row[2]; r[2] = row[3]; }
    else if (row[0] == 0.f) cg_draw_identity(r, s.kind);
    else if (s.kind == CG_PERTURB_ROTATION) {
      float R[9];
      cg_rotvec_matrix(row[1], row[2], row[3], R);
      r[3] = 1.f;
      for (int k = 0; k < 9; ++k) r[4 + k] = R[k];
    }
    else if (s.kind == CG_PERTURB_SCALE) { r[13] = row[1]; r[14] = row[2]; r[15] = row[3]; }
    else if (s.kind == CG_PERTURB_TRANSLATION) { r[16] = row[1]; r[17] = row[2]; r[18] = row[3]; }
    else if (s.kind == CG_PERTURB_NOISE) r[19] = row[1];
    else r[20] = 1.f;
  }
}

// include/cistgcn_hip.h : cg_draw_augmentation
extern "C" int cg_draw_augmentation(const CgDrawStep* steps, int n_steps, const unsigned long long* seed, int stream_id, int B, int J,
                                    int layout, float* table, float* noise_tab, void* stream_) {
  if (!seed) return CG_EARG;
  if (B < 1 || n_steps < 0 || n_steps > CG_PERTURB_MAX_STEPS || stream_id < 0 || stream_id > 0xFFFF) return CG_ESHAPE;
  if (layout != CG_DRAW_TABLE24 && layout != CG_DRAW_STEPS4) return CG_ESHAPE;
  if (n_steps > 0 && !steps) return CG_EARG;
  CgDrawPlan plan = {};
  int n_noise = 0, last[CG_DRAW_KINDS];
  for (int k = 0; k < CG_DRAW_KINDS; ++k) last[k] = -1;
  for (int i = 0; i < n_steps; ++i) {
    const int kind = steps[i].kind;
    if (kind < CG_PERTURB_ROTATION || kind > CG_PERTURB_INVERT) return CG_ESHAPE;
    if (kind == CG_PERTURB_NOISE) {
      if (J < 1 || !noise_tab) return CG_ESHAPE;
      ++n_noise;
    }
    plan.st[i] = steps[i];
    last[kind] = i;
  }
  for (int k = 0; k < CG_DRAW_KINDS; ++k) {
    if (last[k] >= 0) plan.fills[last[k]] = 1;
    else plan.absent |= 1 << k;
  }
  const long long n_tab = layout == CG_DRAW_TABLE24 ? (long long)B * max(n_steps, 1) : (long long)B * n_steps;
  const long long n_noise_el = (long long)B * n_noise * (n_noise ? J : 0) * 3;
  if (n_tab > 0 && !table) return CG_EARG;
  const long long total = n_tab + n_noise_el;
  if (total == 0) return CG_OK;                             // CG_DRAW_STEPS4 of an empty list
  const unsigned blocks = (unsigned)min((total + CG_DRAW_THREADS - 1) / CG_DRAW_THREADS, (long long)CG_DRAW_MAX_BLOCKS);
  hipLaunchKernelGGL(cg_draw_kernel, dim3(blocks), dim3(CG_DRAW_THREADS), 0, (hipStream_t)stream_, plan, seed, (unsigned int)stream_id,
                     n_steps, layout, n_tab, n_noise_el, table, noise_tab);
  return cg_launch_status();
}
