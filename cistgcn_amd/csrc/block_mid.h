// Argument block of the block mid-section kernels (block_mid.hip); mirrored by include/cistgcn_hip.h and cistgcn_amd/_lib.py.
#pragma once
#include "cg_bn.h"            // CgTailBN

// Middle of a DSTD_GC block, between the collapsing convolutions and the fused tails (gate_head.hip, map2adj_tail.hip).  Up to six items,
// each  x (B,C,L) -> BatchNorm2d over C -> Dropout [-> PReLU] -> a bias-free map:
//   kind 0 (full, the gate paths conv_s|t[5..7] + map input):   z[b,o]   = sum_{c,l} W[o,c,l] h[b,c,l]        (B,O)
//   kind 1 (pointwise, the towers' *_compress[4..6]):           y[b,o,l] = sum_c W[o,c] h[b,c,l]              (B,O,L)
#define CG_MID_MAXN 6
#define CG_MID_MAXD 64        // C, L, O <= 64
struct CgMidItem {
  int kind, C, L, O;
  int sb_, ns_;                                 // samples per slice, slices: filled in by the launcher (cg_block_mid_geometry)
  const float* x; long long x_ld;               // (B,C,L), sample stride in floats (rows of C*L floats are dense)
  CgTailBN bn; long long stats_ld;              // bn.stats: [CG_STAT_REPLICAS][stats_ld][2] f64 sums of x, this item's channels from c = 0 (train)
  const float* alpha;                           // optional single PReLU slope
  const float* W;                               // (O, C*L) | (O, C)
  unsigned int salt; int pad;
  float* y;                                     // (B,O) | (B,O,L)
  float* tap;                                   // optional (B,C,L): h (branch records)
  // backward
  const float* dy;                              // like y
  float* dx;                                    // (B,C,L) dense
  float* dW; float* dgamma; float* dbeta; float* dalpha;
  float* g;                                     // (B,C,L) scratch: the gradient in front of the BatchNorm
  double* part;                                 // [ns][2C+1] scratch, all written by launch 1 (see cg_block_mid_geometry)
  float* wpart;                                 // [ns][O*C*L | O*C] scratch, all written by launch 1
};
struct CgBlockMid {
  int B, train, n, pad;
  float drop_p; int pad2; const unsigned long long* seed;
  CgMidItem it[CG_MID_MAXN];
};
