// Map2Adj tail kernels (map2adj_tail.hip); argument block CgAdjTail: include/cistgcn_hip.h.
#pragma once
#include "cg_bn.h"

#define CG_ADJ_MAXW 4        // weight-gradient register tiles per wave: (Kc/16)^2 / 4 waves, Kc <= 64

// One tower pair's tail: rank-1 seed of s (B,V,T) and q (B,T,V) -> expansor (conv Kc x Kc, BatchNorm, Dropout, PReLU, conv Kc x Kc).
// domain 0 (space): slab axis Kc = V, maps J x J = T x T;   domain 1 (time): Kc = T, J = V.
// launch geometry of one tower (internal): padded slab count, LDS strides, tile width (KcM * PT = 4096), chunking, magic divisors
struct CgAdjGeom { int KcM, WS, JS, Pn, PT, PS, NP, lgq, ntiles, nch; unsigned magicJ, magicKc, magicPad; int tpw; };
struct CgAdjTailPair { int n, nch_max; CgAdjGeom g[2]; CgAdjTail t[2]; };
