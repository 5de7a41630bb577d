// Forward kinematics and the window gather of the device-resident motion bank: what utils/data_utils.py::load_data_h36m (:843-942)
// and ::load_data_amass (:738-839) of the reference do between a file of joint angles and the (n, seq_len, J, 3) array a loader
// indexes.  (include/cistgcn_hip.h: CgForwardKinematics / CgGatherWindows give the two conventions, the quirk of the chain convention,
// the clamps and the return codes.)
//   cg_fk_kernel<CONV>         one lane per joint; a wavefront holds two frames while J and J_out <= 32, else one.  Every lane builds its
//                              joint's local rotation, then the tree is walked level by level: the lanes of the current level read their
//                              parent's rotation and position (12 values) from LDS and store their own.  The tree (parent, level of every
//                              joint) arrives by value with the launch, `rest` and `select` are read once per workgroup.  The loop over
//                              the levels and the grid-stride loop over the frame groups have workgroup-uniform trip counts, so every
//                              barrier is reached by all threads.  No dynamic register indexing (nothing goes to scratch), no atomics.
//   cg_gather_windows_kernel   one workgroup per window: copy, joint selection, normalisation; a window whose first frame is upside
//                              down gets its y mirrored about the window's own mean (f64, fixed order).  cg_gather_windows_at_kernel
//                              is the same with the window ids read at a device-resident cursor into a permutation, which
//                              cg_cursor_advance moves: a captured step walks an epoch without the host naming a batch.
// The composition runs in f64 on the fp32 inputs and is rounded once per coordinate: the chains are up to ~10 joints deep in the loaders'
// trees (63 at the limit) and fp32 products would carry the rounding of every level (the reference's own fp32 output is 1.5e-4 .. 5e-4
// off at coordinates of 1100 .. 2600, recorded per case in tests/golden/aug_kinematics.npz).
#include "cg_common.h"

#include <math.h>

#define CG_FK_WAVES (CG_FK_THREADS / CG_WAVE)

struct CgFkTree { signed char parent[CG_FK_MAX_JOINTS]; unsigned char level[CG_FK_MAX_JOINTS]; };      // validated on the host, passed by value

// local rotation of a joint, row-major in R[9]
template <int CONV>
__device__ __forceinline__ void cg_fk_local(double x, double y, double z, double* R) {
  const double th = sqrt(x * x + y * y + z * z);
  if (CONV == CG_FK_SMPL && !(th > 0.0)) {                  // the reference's result for r = 0 (its noise only keeps 0 / 0 away)
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  const double sn = sin(th), cs = cos(th), c1 = 1.0 - cs;
  if (CONV == CG_FK_EXPMAP_CHAIN) {
    // I + sin K + (1 - cos) K^2 with K = skew(r / (theta + 1e-7)); theta = 0: K = 0 and R = I exactly
    const double d = th + 1e-7, kx = x / d, ky = y / d, kz = z / d;
    const double K[3][3] = {{0.0, -kz, ky}, {kz, 0.0, -kx}, {-ky, kx, 0.0}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double kk = 0.0;
#pragma unroll
        for (int m = 0; m < 3; ++m) kk += K[i][m] * K[m][j];
        R[3 * i + j] = ((i == j ? 1.0 : 0.0) + sn * K[i][j]) + c1 * kk;
      }
  } else {
    // cos I + (1 - cos) k k^T + sin skew(k), k = r / theta
    const double k[3] = {x / th, y / th, z / th};
    const double S[3][3] = {{0.0, -k[2], k[1]}, {k[2], 0.0, -k[0]}, {-k[1], k[0], 0.0}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[3 * i + j] = ((i == j ? cs : 0.0) + c1 * (k[i] * k[j])) + sn * S[i][j];
  }
}

template <int CONV>
__global__ __launch_bounds__(CG_FK_THREADS) void cg_fk_kernel(CgForwardKinematics a, CgFkTree tree, int max_level, int fpw, long long groups) {
  __shared__ double G[12][CG_FK_THREADS];                   // per lane: global rotation (9, row-major) and position (3) of its joint
  __shared__ float rest[CG_FK_MAX_JOINTS][3];
  __shared__ int sel[CG_FK_MAX_JOINTS];
  const int tid = threadIdx.x, lane = tid & (CG_WAVE - 1);
  const int J = a.J, J_out = a.J_out;
  const int width = CG_WAVE / fpw;                          // lanes per frame: 64 or 32
  const int j = lane & (width - 1);                         // this lane's joint (and output slot)
  const int slot = (tid >> 6) * fpw + lane / width;         // frame of the group this lane works on, 0 .. CG_FK_WAVES * fpw - 1
  const int base = tid - j;                                 // lane of joint 0 of the same frame
  for (int i = tid; i < J * 3; i += CG_FK_THREADS) rest[i / 3][i % 3] = a.rest[i];
  for (int i = tid; i < J_out; i += CG_FK_THREADS) sel[i] = a.select ? min(max(a.select[i], 0), J - 1) : i;
  __syncthreads();
  const bool joint = j < J;
  const int par = joint ? tree.parent[j] : -1, lvl = joint ? tree.level[j] : 0;
  const long long ld = CONV == CG_FK_EXPMAP_CHAIN ? 3 + 3 * (long long)J : 3 * (long long)a.J_pose;
  const int off = CONV == CG_FK_EXPMAP_CHAIN ? 3 : 0;
  const int fpg = CG_FK_WAVES * fpw;                        // frames per group
  for (long long g = blockIdx.x; g < groups; g += gridDim.x) {        // uniform in the workgroup
    const long long n = g * fpg + slot;
    const bool live = joint && n < a.N;
    double R[9], p[3];
    if (live) {
      const float* r = a.angles + n * ld + off + 3 * j;
      cg_fk_local<CONV>((double)r[0], (double)r[1], (double)r[2], R);
#pragma unroll
      for (int c = 0; c < 3; ++c) p[c] = (double)rest[j][c];
#pragma unroll
      for (int k = 0; k < 9; ++k) G[k][tid] = R[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) G[9 + c][tid] = p[c];
    }
    __syncthreads();
    for (int l = 1; l <= max_level; ++l) {                  // max_level is the same for every thread
      // chain convention: a joint below joint 0 (par == 0) composes nothing, but its children compose with its local rotation
      const bool mine = live && lvl == l && (CONV == CG_FK_SMPL ? par >= 0 : par > 0);
      if (mine) {
        const int pt = base + par;
        double P[9], q[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) P[k] = G[k][pt];
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = G[9 + c][pt];
        double Rn[9], pn[3];
        if (CONV == CG_FK_EXPMAP_CHAIN) {
          // R_i = R_local R_parent;  p_i = rest_i R_parent + p_parent (row vector)
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) Rn[3 * i + c] = (R[3 * i] * P[c] + R[3 * i + 1] * P[3 + c]) + R[3 * i + 2] * P[6 + c];
#pragma unroll
          for (int c = 0; c < 3; ++c) pn[c] = ((p[0] * P[c] + p[1] * P[3 + c]) + p[2] * P[6 + c]) + q[c];
        } else {
          // G_i = G_parent [R_i | rest_i - rest_parent]:  R_i = R_parent R_local;  t_i = R_parent (rest_i - rest_parent) + t_parent
          double d[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) d[c] = (double)rest[j][c] - (double)rest[par][c];
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) Rn[3 * i + c] = (P[3 * i] * R[c] + P[3 * i + 1] * R[3 + c]) + P[3 * i + 2] * R[6 + c];
#pragma unroll
          for (int i = 0; i < 3; ++i) pn[i] = ((P[3 * i] * d[0] + P[3 * i + 1] * d[1]) + P[3 * i + 2] * d[2]) + q[i];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) G[k][tid] = Rn[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) G[9 + c][tid] = pn[c];
      }
      __syncthreads();
    }
    if (j < J_out && n < a.N) {                             // lane j writes output joint j: the wave's stores cover one contiguous range
      const int src = base + sel[j];
      float* o = a.out + (n * J_out + j) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (float)(G[9 + c][src] * (double)a.scale);
    }
    __syncthreads();                                        // the next group overwrites G
  }
}

// include/cistgcn_hip.h : cg_forward_kinematics
extern "C" int cg_forward_kinematics(const CgForwardKinematics* a, void* stream_) {
  if (!a || !a->angles || !a->parent || !a->rest || !a->out) return CG_EARG;
  const int J = a->J, J_out = a->J_out;
  if (J < 1 || J > CG_FK_MAX_JOINTS || J_out < 1 || J_out > CG_FK_MAX_JOINTS || a->N < 0) return CG_ESHAPE;
  if (a->convention != CG_FK_EXPMAP_CHAIN && a->convention != CG_FK_SMPL) return CG_ESHAPE;
  if (a->convention == CG_FK_SMPL && a->J_pose < J) return CG_ESHAPE;
  if (!a->select && J_out != J) return CG_ESHAPE;
  CgFkTree tree = {};
  int max_level = 0;
  if (a->parent[0] != -1) return CG_ESHAPE;
  tree.parent[0] = -1;
  for (int i = 1; i < J; ++i) {
    const int p = a->parent[i];
    if (p < -1 || p >= i) return CG_ESHAPE;
    tree.parent[i] = (signed char)p;
    tree.level[i] = p < 0 ? 0 : (unsigned char)(tree.level[p] + 1);
    max_level = max(max_level, (int)tree.level[i]);
  }
  if (a->N == 0) return CG_OK;
  const int fpw = (J <= 32 && J_out <= 32) ? 2 : 1;
  const long long fpg = (long long)CG_FK_WAVES * fpw, groups = (a->N + fpg - 1) / fpg;
  const unsigned blocks = (unsigned)min(groups, (long long)CG_FK_MAX_BLOCKS);
  hipStream_t stream = (hipStream_t)stream_;
  if (a->convention == CG_FK_EXPMAP_CHAIN)
    hipLaunchKernelGGL(cg_fk_kernel<CG_FK_EXPMAP_CHAIN>, dim3(blocks), dim3(CG_FK_THREADS), 0, stream, *a, tree, max_level, fpw, groups);
  else
    hipLaunchKernelGGL(cg_fk_kernel<CG_FK_SMPL>, dim3(blocks), dim3(CG_FK_THREADS), 0, stream, *a, tree, max_level, fpw, groups);
  return cg_launch_status();
}

// ---- window gather ---------------------------------------------------------------------------------------------------------------
#define CG_GATHER_THREADS 256

__device__ __forceinline__ float cg_gather_norm(float v, bool on, float mean, float std) {
#pragma clang fp contract(off)
  return on ? (v - mean) / std : v;
}

// window `item` (clamped into [0, W)) -> raw[b]; called by every thread of the workgroup (barriers inside)
__device__ __forceinline__ void cg_gather_window(const CgGatherWindows& a, int b, int item) {
  __shared__ double red[16];
  __shared__ double centre;
  const int tid = threadIdx.x;
  const int L = a.L, J = a.J, Js = a.J_src;
  const int w = min(max(item, 0), a.W - 1);
  const long long s = min(max((long long)a.starts[w], 0LL), a.F - L);          // F >= L (launcher)
  const float* src = a.frames + s * Js * 3;
  float* dst = a.raw + (long long)b * L * J * 3;
  const bool norm = !(a.mean == 0.f && a.std == 1.f);
  auto joint = [&](int jj) { return a.select ? min(max(a.select[jj], 0), Js - 1) : jj; };
  // upside down?  every thread reads the same two values of the first frame
  bool flip = false;
  if (a.up_hi >= 0) {
    const float hi = cg_gather_norm(src[joint(a.up_hi) * 3 + 1], norm, a.mean, a.std);
    const float lo = cg_gather_norm(src[joint(a.up_lo) * 3 + 1], norm, a.mean, a.std);
    flip = hi - lo < 0.f;
  }
  float c = 0.f;
  if (flip) {                                               // uniform in the workgroup
    // mean of the L * J normalised y values: thread t adds points t, t + 256, ... in order, cg_block_sum adds the threads in a fixed tree
    double acc = 0.0;
    for (int p = tid; p < L * J; p += CG_GATHER_THREADS) {
      const int t = p / J, jj = p - t * J;
      acc += (double)cg_gather_norm(src[((long long)t * Js + joint(jj)) * 3 + 1], norm, a.mean, a.std);
    }
    acc = cg_block_sum(acc, red);
    if (tid == 0) centre = acc / (double)(L * J);
    __syncthreads();
    c = (float)centre;
  }
  const int n = L * J * 3;
  for (int e = tid; e < n; e += CG_GATHER_THREADS) {
    const int p = e / 3, ax = e - 3 * p, t = p / J, jj = p - t * J;
    const float v = cg_gather_norm(src[((long long)t * Js + joint(jj)) * 3 + ax], norm, a.mean, a.std);
    dst[e] = (flip && ax == 1) ? c - v : v;
  }
}

__global__ __launch_bounds__(CG_GATHER_THREADS) void cg_gather_windows_kernel(CgGatherWindows a) {
  cg_gather_window(a, blockIdx.x, a.items[blockIdx.x]);
}

// the window ids at a device-resident cursor: order[min(*cursor + b, W - 1)] - a cursor past W - B repeats the last entry of `order`
__global__ __launch_bounds__(CG_GATHER_THREADS) void cg_gather_windows_at_kernel(CgGatherWindows a, const int32_t* __restrict__ order,
                                                                                 const int32_t* __restrict__ cursor) {
  const long long at = (long long)max(*cursor, 0) + blockIdx.x;
  cg_gather_window(a, blockIdx.x, order[min(at, (long long)a.W - 1)]);
}

// the checks cg_gather_windows and cg_gather_windows_at share (everything but the source of the window ids)
static int cg_gather_check(const CgGatherWindows* a) {
  if (!a || !a->frames || !a->starts || !a->raw) return CG_EARG;
  if (a->B < 1 || a->L < 1 || a->J < 1 || a->J_src < 1 || a->W < 1 || a->F < a->L || a->std == 0.f) return CG_ESHAPE;
  if ((long long)a->L * a->J * 3 > 0x7fffffffLL) return CG_ESHAPE;
  if (!a->select && a->J != a->J_src) return CG_ESHAPE;
  const bool off = a->up_hi == -1 && a->up_lo == -1;
  const bool on = a->up_hi >= 0 && a->up_hi < a->J && a->up_lo >= 0 && a->up_lo < a->J;
  if (!off && !on) return CG_ESHAPE;
  return CG_OK;
}

// include/cistgcn_hip.h : cg_gather_windows
extern "C" int cg_gather_windows(const CgGatherWindows* a, void* stream_) {
  if (a && !a->items) return CG_EARG;
  const int bad = cg_gather_check(a);
  if (bad) return bad;
  hipLaunchKernelGGL(cg_gather_windows_kernel, dim3((unsigned)a->B), dim3(CG_GATHER_THREADS), 0, (hipStream_t)stream_, *a);
  return cg_launch_status();
}

// include/cistgcn_hip.h : cg_gather_windows_at
extern "C" int cg_gather_windows_at(const CgGatherWindows* a, const int32_t* order, const int32_t* cursor, void* stream_) {
  if (!order || !cursor) return CG_EARG;
  const int bad = cg_gather_check(a);
  if (bad) return bad;
  hipLaunchKernelGGL(cg_gather_windows_at_kernel, dim3((unsigned)a->B), dim3(CG_GATHER_THREADS), 0, (hipStream_t)stream_, *a, order, cursor);
  return cg_launch_status();
}

// include/cistgcn_hip.h : cg_cursor_advance
__global__ void cg_cursor_advance_kernel(int32_t* cursor, int by) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *cursor = *cursor + by;
}

extern "C" int cg_cursor_advance(int32_t* cursor, int by, void* stream_) {
  if (!cursor) return CG_EARG;
  hipLaunchKernelGGL(cg_cursor_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, cursor, by);
  return cg_launch_status();
}
