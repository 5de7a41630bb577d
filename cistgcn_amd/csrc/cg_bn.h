// BatchNorm channel constants, once: every fused kernel that applies a BatchNorm in its prologue or epilogue (rowops.hip, dstd_tail.hip,
// map2adj_tail.hip, block_input.hip, collapse_rows.hip, gate_head.hip, block_mid.hip, context_heads.hip) builds them from the pieces below.
// The sites differ in where their sums come from (replicated f64 sums of a producer, the workgroup's own batch sums, the moments of a
// one-channel input), so each keeps its own result struct; the rules of nn.BatchNorm - biased variance for the normalisation, unbiased into
// running_var, one count per forward - are written here and nowhere else.
#pragma once
#include "cg_common.h"        // CgTailBN (cistgcn_hip.h): one BatchNorm of a chain

// sums of channel c over the replicas of a [CG_STAT_REPLICAS][ld][2] buffer (cg_common.h), in replica order
__device__ __forceinline__ void cg_bn_sums(const double* stats, long long ld, int c, double& s1, double& s2) {
  s1 = 0.0; s2 = 0.0;
  for (int r = 0; r < CG_STAT_REPLICAS; ++r) { s1 += stats[((long long)r * ld + c) * 2]; s2 += stats[((long long)r * ld + c) * 2 + 1]; }
}
// mean and biased variance from {sum, sum of squares} over cnt elements; E[x^2] - E[x]^2 in f64 can round below zero
__device__ __forceinline__ void cg_bn_moments(double s1, double s2, double cnt, double& mean, double& var) {
  mean = s1 / cnt;
  var = s2 / cnt - mean * mean;
  if (var < 0.0) var = 0.0;
}
__device__ __forceinline__ float cg_bn_rstd(double var, float eps) { return (float)(1.0 / sqrt(var + (double)eps)); }           // batch statistics
__device__ __forceinline__ float cg_bn_rstd_eval(float running_var, float eps) { return 1.0f / sqrtf(running_var + eps); }    // running statistics

// Bookkeeping of channel c by the ONE thread that owns it.
// cg_bn_track: the running statistics of a train-mode forward exactly like nn.BatchNorm, when the module tracks them (`running_mean` not
// null) - the unbiased variance of the cnt elements into running_var, num_batches_tracked once per forward.
__device__ __forceinline__ void cg_bn_track(float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, int c,
                                            float mean, double var, double cnt) {
  if (running_mean) {
    const double unb = cnt > 1.0 ? var * cnt / (cnt - 1.0) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
    if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;
  }
}
// cg_bn_save (eval mode): the pair the backward reads; cg_bn_record (train mode): that pair and the running statistics
__device__ __forceinline__ void cg_bn_save(const CgTailBN& bn, int c, int C, float mean, float rstd) { bn.save[c] = mean; bn.save[C + c] = rstd; }
__device__ __forceinline__ void cg_bn_record(const CgTailBN& bn, int c, int C, float mean, float rstd, double var, double cnt) {
  cg_bn_save(bn, c, C, mean, rstd);
  cg_bn_track(bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, c, mean, var, cnt);
}

// ---- the common case: sums from a producer's replicas, stride C ------------------------------------------------------
struct CgAff { float mean, rstd, gamma, beta; };

// train: batch statistics from the replicated f64 sums (recorded by the block that owns channel bookkeeping); eval: running
// statistics.  backward: the saved pair.
static __device__ __forceinline__ CgAff cg_tail_aff(const CgTailBN& bn, int c, int C, double cnt, int train, bool backward, bool owner) {
  CgAff a;
  a.gamma = bn.gamma[c]; a.beta = bn.beta[c];
  if (backward) { a.mean = bn.save[c]; a.rstd = bn.save[C + c]; return a; }
  if (train) {
    double s1, s2, mean, var;
    cg_bn_sums(bn.stats, C, c, s1, s2);
    cg_bn_moments(s1, s2, cnt, mean, var);
    a.mean = (float)mean;
    a.rstd = cg_bn_rstd(var, bn.eps);
    if (owner) cg_bn_record(bn, c, C, a.mean, a.rstd, var, cnt);
  } else {
    a.mean = bn.running_mean[c];
    a.rstd = cg_bn_rstd_eval(bn.running_var[c], bn.eps);
    if (owner) cg_bn_save(bn, c, C, a.mean, a.rstd);
  }
  return a;
}

static __device__ __forceinline__ float cg_bn(const CgAff& a, float v) { return (v - a.mean) * (a.gamma * a.rstd) + a.beta; }
static __device__ __forceinline__ float cg_prelu(float u, float alpha) { return u > 0.f ? u : alpha * u; }
