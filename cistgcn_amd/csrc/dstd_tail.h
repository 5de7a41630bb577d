// Internal limits of the DSTD_GC tail kernels (dstd_tail.hip); argument block CgDstdTail: include/cistgcn_hip.h.
#pragma once
#include "cg_bn.h"

#define CG_TAIL_MAXW 8       // dWc register tiles per wave: (C/16) * (2C/16) / 4 waves, C <= 64
#define CG_TAIL_ROWSUMS 6    // f64 row sums per (b, c) of CgDstdTail.rows_c
#define CG_TAIL_FMOM 4       // f64 moments per channel and replica of CgDstdTail.fmom
