// Internal limits of the block mid-section kernels (block_mid.hip); argument blocks CgMidItem / CgBlockMid and CG_MID_MAXN:
// include/cistgcn_hip.h.
#pragma once
#include "cg_bn.h"

// Middle of a DSTD_GC block, between the collapsing convolutions and the fused tails (gate_head.hip, map2adj_tail.hip).  Up to CG_MID_MAXN
// items, each  x (B,C,L) -> BatchNorm2d over C -> Dropout [-> PReLU] -> a bias-free map:
//   kind 0 (full, the gate paths conv_s|t[5..7] + map input):   z[b,o]   = sum_{c,l} W[o,c,l] h[b,c,l]        (B,O)
//   kind 1 (pointwise, the towers' *_compress[4..6]):           y[b,o,l] = sum_c W[o,c] h[b,c,l]              (B,O,L)
#define CG_MID_MAXD 64        // C, L, O <= 64
