// On-device input pipeline: the training augmentations of the reference
// (environment/custom_transforms.py: RandomFlip :243-298, RandomRotation :10-84, RandomScale :87-161, RandomNoise :350-400,
// RandomTranslation :164-240, RandomPoseInvers :301-347, composed in the order of loaders/loader.py:42-130) and the per-item tensors of
// loaders/h36m_motion_3d.py:94-108 (sample / target split, velocities, cumulative target velocities and speeds), for a
// whole batch in one launch: one workgroup per sequence, the sequence lives in LDS between the steps.
// The random draws are made on the host in the reference's order (environment/input_pipeline.py) and arrive as one
// parameter row per sequence; everything that depends on the data (centroids, per-axis extent) is computed here.
#include "cg_common.h"
#include "cg_rotvec.h"

#define CG_AUG_NPAR 24      // flip x,y,z | rot_on | R[3][3] (row vector times matrix) | scale x,y,z | translation rate x,y,z | noise | invert | pad

HIP_DYNAMIC_SHARED(unsigned char, cg_dyn_lds)

// mean over all points of the sequence, per axis (f64 accumulation, result valid in every thread)
__device__ __forceinline__ void cg_aug_centroid(const float* s, int n_pts, double* red, float c[3]) {
  double a[3] = {0.0, 0.0, 0.0};
  for (int p = threadIdx.x; p < n_pts; p += blockDim.x) { a[0] += s[3 * p]; a[1] += s[3 * p + 1]; a[2] += s[3 * p + 2]; }
  __shared__ double out[3];
  for (int k = 0; k < 3; ++k) {
    const double t = cg_block_sum(a[k], red);
    if (threadIdx.x == 0) out[k] = t / (double)n_pts;
  }
  __syncthreads();
  c[0] = (float)out[0]; c[1] = (float)out[1]; c[2] = (float)out[2];
  __syncthreads();
}

// per-axis extent (max - min over the whole sequence) of the current data -> ext[0..2] (LDS), valid in every thread on return;
// wave shuffles, one slot per wave in `red`: 4 waves x 6 values fit the 16 doubles
__device__ __forceinline__ void cg_aug_extent(const float* s, int n_pts, double* red, float* ext) {
  const int tid = threadIdx.x, nt = blockDim.x;
  float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f}, mx[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
  for (int p = tid; p < n_pts; p += nt)
    for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], s[3 * p + a]); mx[a] = fmaxf(mx[a], s[3 * p + a]); }
  float* part = reinterpret_cast<float*>(red);
  for (int a = 0; a < 3; ++a)
    for (int off = 32; off > 0; off >>= 1) { mn[a] = fminf(mn[a], __shfl_xor(mn[a], off, 64)); mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off, 64)); }
  const int wave = tid >> 6;
  if ((tid & 63) == 0) for (int a = 0; a < 3; ++a) { part[wave * 6 + a] = mn[a]; part[wave * 6 + 3 + a] = mx[a]; }
  __syncthreads();
  if (tid < 3) {
    float lo = part[tid], hi = part[3 + tid];
    for (int w = 1; w < (nt >> 6); ++w) { lo = fminf(lo, part[w * 6 + tid]); hi = fmaxf(hi, part[w * 6 + 3 + tid]); }
    ext[tid] = hi - lo;
  }
  __syncthreads();
}

// The outputs of H36m_Motion3D.__getitem__ (h36m_motion_3d.py:94-108) of sequence b, shared by both kernels of this file:
// at(e) is element e of the finished (L, J, 3) sequence (the LDS copy seen through the joint permutation of RandomPoseInvers where
// that applies to the frame of e)
template <typename At>
__device__ __forceinline__ void cg_aug_emit(At at, int b, int L, int J, int input_n, float* __restrict__ sample, float* __restrict__ target,
                                            float* __restrict__ target_vel, float* __restrict__ target_gvel, float* __restrict__ processed,
                                            float* __restrict__ sample_vel) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int n = L * J * 3, n_in = input_n * J * 3, n_out = (L - input_n) * J * 3;
  if (processed) for (int e = tid; e < n; e += nt) processed[(long long)b * n + e] = at(e);
  for (int e = tid; e < n_in; e += nt) sample[(long long)b * n_in + e] = at(e);
  for (int e = tid; e < n_out; e += nt) target[(long long)b * n_out + e] = at(n_in + e);
  if (sample_vel)                                          // "sample_vel": velocities[:input_n] (h36m_motion_3d.py:101)
    for (int e = tid; e < n_in; e += nt) sample_vel[(long long)b * n_in + e] = at(e + 3 * J) - at(e);
  // velocities[t] = s[t+1] - s[t]; target_vel = cumsum_t velocities[input_n-1:], target_gvel = cumsum_t |velocities[input_n-1:]|
  const int To = L - input_n;
  for (int j = tid; j < J; j += nt) {
    float acc[3] = {0.f, 0.f, 0.f}, gacc = 0.f;
    for (int k = 0; k < To; ++k) {
      const int t = input_n - 1 + k;
      float v[3];
      for (int a = 0; a < 3; ++a) { v[a] = at(((t + 1) * J + j) * 3 + a) - at((t * J + j) * 3 + a); acc[a] += v[a]; }
      gacc += sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      float* tv = target_vel + (((long long)b * To + k) * J + j) * 3;
      tv[0] = acc[0]; tv[1] = acc[1]; tv[2] = acc[2];
      target_gvel[((long long)b * To + k) * J + j] = gacc;
    }
  }
}

__global__ void cg_augment_sequences_kernel(const float* __restrict__ raw, const float* __restrict__ params, float* __restrict__ sample,
                                            float* __restrict__ target, float* __restrict__ target_vel, float* __restrict__ target_gvel,
                                            float* __restrict__ processed, float* __restrict__ sample_vel,
                                            const float* __restrict__ noise_tab, const int* __restrict__ perm, int L, int J, int input_n) {
  float* s = reinterpret_cast<float*>(cg_dyn_lds);
  __shared__ double red[16];
  __shared__ float ext[6];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n_pts = L * J, n = 3 * n_pts;
  const float* par = params + (long long)b * CG_AUG_NPAR;
  const float* src = raw + (long long)b * n;
  for (int e = tid; e < n; e += nt) s[e] = src[e];
  __syncthreads();
  float c[3];
  // RandomFlip: mirror about the centroid of the incoming sequence (one centroid for all axes)
  if (par[0] != 0.f || par[1] != 0.f || par[2] != 0.f) {
    cg_aug_centroid(s, n_pts, red, c);
    for (int e = tid; e < n; e += nt) {
      const int a = e % 3;
      if (par[a] != 0.f) s[e] = c[a] - (s[e] - c[a]);
    }
    __syncthreads();
  }
  // RandomRotation: (p - centroid) R + centroid, R from the rotation vector (host)
  if (par[3] != 0.f) {
    cg_aug_centroid(s, n_pts, red, c);
    for (int p = tid; p < n_pts; p += nt) {
      const float x = s[3 * p] - c[0], y = s[3 * p + 1] - c[1], z = s[3 * p + 2] - c[2];
      s[3 * p] = (x * par[4] + y * par[7] + z * par[10]) + c[0];
      s[3 * p + 1] = (x * par[5] + y * par[8] + z * par[11]) + c[1];
      s[3 * p + 2] = (x * par[6] + y * par[9] + z * par[12]) + c[2];
    }
    __syncthreads();
  }
  // RandomScale (about the origin, as the reference)
  for (int e = tid; e < n; e += nt) s[e] *= par[13 + e % 3];
  __syncthreads();
  // RandomNoise (custom_transforms.py:368-396, whole sequence, constant amplitude): data += noise * u[joint][axis] * extent[axis],
  // u ~ U(-1, 1) drawn per (joint, axis) on the host
  if (par[19] != 0.f && noise_tab) {
    cg_aug_extent(s, n_pts, red, ext);
    const float* u = noise_tab + (long long)b * J * 3;
    for (int e = tid; e < n; e += nt) { const int a = e % 3, j = (e / 3) % J; s[e] += par[19] * u[3 * j + a] * ext[a]; }
    __syncthreads();
  }
  // RandomTranslation: rate x per-axis extent of the (scaled) sequence
  if (par[16] != 0.f || par[17] != 0.f || par[18] != 0.f) {
    cg_aug_extent(s, n_pts, red, ext);
    for (int e = tid; e < n; e += nt) { const int a = e % 3; s[e] += par[16 + a] * ext[a]; }
    __syncthreads();
  }
  // RandomPoseInvers (custom_transforms.py:323-344, whole sequence): left and right joints trade places.  The pair swaps of the
  // reference compose to a joint permutation (host): output joint j shows joint perm[j]; applied while the results are written
  const bool inv = par[20] != 0.f && perm;
  auto at = [&](int e) {                                  // element e of the (L, J, 3) result
    if (!inv) return s[e];
    const int a = e % 3, p = e / 3, j = p % J;
    return s[(p - j + perm[j]) * 3 + a];
  };
  cg_aug_emit(at, b, L, J, input_n, sample, target, target_vel, target_gvel, processed, sample_vel);
}

// include/cistgcn_hip.h : cg_augment_sequences
extern "C" int cg_augment_sequences(const float* raw, const float* params, float* sample, float* target, float* target_vel,
                                    float* target_gvel, float* processed, float* sample_vel, const float* noise_tab, const int* perm,
                                    int B, int L, int J, int input_n, void* stream_) {
  if (!raw || !params || !sample || !target || !target_vel || !target_gvel) return CG_EARG;
  if (B <= 0 || L <= 1 || J <= 0 || input_n <= 0 || input_n >= L) return CG_ESHAPE;
  const size_t lds = (size_t)L * J * 3 * sizeof(float);
  if (lds > 150 * 1024) return CG_ESHAPE;
  if (lds > 48 * 1024) {
    hipError_t e = cg_lds_limit((const void*)cg_augment_sequences_kernel, lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(cg_augment_sequences_kernel, dim3((unsigned)B), dim3(256), lds, (hipStream_t)stream_, raw, params, sample, target,
                     target_vel, target_gvel, processed, sample_vel, noise_tab, perm, L, J, input_n);
  return cg_launch_status();
}

// ---- robustness-test transforms: the same transform classes with `seq_idx`, `continuous` and `keep` ---------------------------------
// (custom_transforms.py: RandomRotation :50-78, RandomScale :127-153, RandomTranslation :202-231, RandomFlip :262-294, RandomPoseInvers
// :321-344, RandomNoise :370-392; built from the `robustness_test:` section by loaders/loader.py:75-127).  The order is no longer fixed:
// the kernel walks a step list.  Every step has a frame window [s0, s1) and a per-frame weight f(t) (cistgcn_hip.h), and takes its
// centroid / extent from the whole sequence as the step before left it.
#define CG_PERTURB_ROT_FRAMES 64               // rotation matrices are built for this many frames at a time (LDS)

struct CgPerturbSteps { int v[CG_PERTURB_MAX_STEPS][6]; };       // the validated host step table, passed by value

// f(t): 0 before the window; inside it 1, or the ramp (t - s0) / (n - 1) of torch.linspace(0, v, n) / v (0 when n == 1); behind it the
// last value of the window (keep) or 0
__device__ __forceinline__ float cg_perturb_weight(int t, int s0, int s1, int cont, int keep) {
  if (t < s0) return 0.f;
  if (t >= s1) { if (!keep) return 0.f; t = s1 - 1; }
  if (!cont) return 1.f;
  const int n = s1 - s0;
  return n > 1 ? (float)(t - s0) / (float)(n - 1) : 0.f;
}

// (rotation matrix of a rotation vector in degrees: cg_rotvec_matrix, cg_rotvec.h)

__global__ void cg_perturb_sequences_kernel(const float* __restrict__ raw, const CgPerturbSteps steps, const float* __restrict__ params,
                                            const float* __restrict__ noise_tab, const int* __restrict__ perm, float* __restrict__ sample,
                                            float* __restrict__ target, float* __restrict__ target_vel, float* __restrict__ target_gvel,
                                            float* __restrict__ processed, float* __restrict__ sample_vel, int L, int J, int input_n,
                                            int n_steps, int n_noise) {
  float* s = reinterpret_cast<float*>(cg_dyn_lds);
  __shared__ double red[16];
  __shared__ float ext[6];
  __shared__ float rot[CG_PERTURB_ROT_FRAMES][9];
  __shared__ float rot_w[CG_PERTURB_ROT_FRAMES];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n_pts = L * J, n = 3 * n_pts;
  const float* src = raw + (long long)b * n;
  for (int e = tid; e < n; e += nt) s[e] = src[e];
  __syncthreads();
  int inv_lo = 0, inv_hi = 0;                               // points [inv_lo, inv_hi) are read through the joint permutation
  for (int i = 0; i < n_steps; ++i) {
    const float* par = params + ((long long)b * n_steps + i) * 4;          // the same for every thread of the workgroup
    if (par[0] == 0.f) continue;
    const int kind = steps.v[i][0], s0 = steps.v[i][1], s1 = steps.v[i][2], cont = steps.v[i][3], keep = steps.v[i][4];
    const int hi = keep ? L : s1;                           // frames outside [s0, hi) have weight 0: they are not touched
    const int p_lo = s0 * J, p_hi = hi * J;
    const float v[3] = {par[1], par[2], par[3]};
    float c[3];
    if (kind == CG_PERTURB_FLIP) {
      // mirror the frames of the window (and behind it: keep) about the centroid of the step's input, one centroid for all axes
      cg_aug_centroid(s, n_pts, red, c);
      for (int p = p_lo + tid; p < p_hi; p += nt)
        for (int a = 0; a < 3; ++a)
          if (v[a] != 0.f) s[3 * p + a] = c[a] - (s[3 * p + a] - c[a]);
      __syncthreads();
    } else if (kind == CG_PERTURB_ROTATION) {
      // (p - centroid) R(t) + centroid, R(t) the matrix of the rotation vector f(t) * v degrees
      cg_aug_centroid(s, n_pts, red, c);
      for (int t0 = s0; t0 < hi; t0 += CG_PERTURB_ROT_FRAMES) {
        const int nf = min(CG_PERTURB_ROT_FRAMES, hi - t0);
        if (tid < nf) {
          const float f = cg_perturb_weight(t0 + tid, s0, s1, cont, keep);
          rot_w[tid] = f;
          if (f != 0.f) cg_rotvec_matrix(f * v[0], f * v[1], f * v[2], rot[tid]);
        }
        __syncthreads();
        for (int q = tid; q < nf * J; q += nt) {
          const int lt = q / J, p = t0 * J + q;
          if (rot_w[lt] == 0.f) continue;                   // weight 0 is the exact identity
          const float* R = rot[lt];
          const float x = s[3 * p] - c[0], y = s[3 * p + 1] - c[1], z = s[3 * p + 2] - c[2];
          s[3 * p] = (x * R[0] + y * R[3] + z * R[6]) + c[0];
          s[3 * p + 1] = (x * R[1] + y * R[4] + z * R[7]) + c[1];
          s[3 * p + 2] = (x * R[2] + y * R[5] + z * R[8]) + c[2];
        }
        __syncthreads();
      }
    } else if (kind == CG_PERTURB_SCALE) {
      // about the origin: 1 + f(t) * (factor - 1), the factor itself where f(t) == 1
      for (int p = p_lo + tid; p < p_hi; p += nt) {
        const float f = cont ? cg_perturb_weight(p / J, s0, s1, cont, keep) : 1.f;
        for (int a = 0; a < 3; ++a) s[3 * p + a] *= (f == 1.f ? v[a] : 1.f + f * (v[a] - 1.f));
      }
      __syncthreads();
    } else if (kind == CG_PERTURB_NOISE) {
      // data += f(t) * amplitude * u[joint][axis] * extent[axis], u ~ U(-1, 1) drawn per (joint, axis) on the host
      cg_aug_extent(s, n_pts, red, ext);
      const float* u = noise_tab + ((long long)b * n_noise + steps.v[i][5]) * J * 3;
      for (int p = p_lo + tid; p < p_hi; p += nt) {
        const int t = p / J, j = p - t * J;
        const float wa = cg_perturb_weight(t, s0, s1, cont, keep) * v[0];
        for (int a = 0; a < 3; ++a) s[3 * p + a] += wa * u[3 * j + a] * ext[a];
      }
      __syncthreads();
    } else if (kind == CG_PERTURB_TRANSLATION) {
      // data += f(t) * rate * per-axis extent of the step's input
      cg_aug_extent(s, n_pts, red, ext);
      for (int p = p_lo + tid; p < p_hi; p += nt) {
        const float f = cont ? cg_perturb_weight(p / J, s0, s1, cont, keep) : 1.f;
        for (int a = 0; a < 3; ++a) s[3 * p + a] += (f * v[a]) * ext[a];
      }
      __syncthreads();
    } else {
      // CG_PERTURB_INVERT, the last step of a list (launcher): left and right joints trade places in these frames while the results
      // are written; output joint j shows joint perm[j]
      inv_lo = p_lo;
      inv_hi = p_hi;
    }
  }
  auto at = [&](int e) {                                  // element e of the (L, J, 3) result
    const int p = e / 3;
    if (p < inv_lo || p >= inv_hi) return s[e];
    const int a = e - 3 * p, j = p % J;
    return s[(p - j + perm[j]) * 3 + a];
  };
  cg_aug_emit(at, b, L, J, input_n, sample, target, target_vel, target_gvel, processed, sample_vel);
}

// include/cistgcn_hip.h : cg_perturb_sequences
extern "C" int cg_perturb_sequences(const float* raw, const int* steps, const float* params, const float* noise_tab, const int* perm,
                                    float* sample, float* target, float* target_vel, float* target_gvel, float* processed,
                                    float* sample_vel, int B, int L, int J, int input_n, int n_steps, int n_noise, void* stream_) {
  if (!raw || !sample || !target || !target_vel || !target_gvel) return CG_EARG;
  if (B <= 0 || L <= 1 || J <= 0 || input_n <= 0 || input_n >= L) return CG_ESHAPE;
  if (n_steps < 0 || n_steps > CG_PERTURB_MAX_STEPS || n_noise < 0) return CG_ESHAPE;
  if (n_steps > 0 && (!steps || !params)) return CG_EARG;
  CgPerturbSteps st = {};
  for (int i = 0; i < n_steps; ++i) {
    const int* row = steps + 6 * i;
    if (row[0] < CG_PERTURB_ROTATION || row[0] > CG_PERTURB_INVERT) return CG_ESHAPE;
    if (!(0 <= row[1] && row[1] < row[2] && row[2] <= L)) return CG_ESHAPE;
    if (row[0] == CG_PERTURB_NOISE) {
      if (!noise_tab) return CG_EARG;
      if (row[5] < 0 || row[5] >= n_noise) return CG_ESHAPE;
    }
    if (row[0] == CG_PERTURB_INVERT) {
      if (!perm) return CG_EARG;
      if (i != n_steps - 1) return CG_ESHAPE;
    }
    for (int k = 0; k < 6; ++k) st.v[i][k] = row[k];
    st.v[i][3] = row[3] != 0;
    st.v[i][4] = row[4] != 0;
  }
  const size_t lds = (size_t)L * J * 3 * sizeof(float);
  if (lds > 150 * 1024) return CG_ESHAPE;
  if (lds > 48 * 1024) {
    hipError_t e = cg_lds_limit((const void*)cg_perturb_sequences_kernel, lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(cg_perturb_sequences_kernel, dim3((unsigned)B), dim3(256), lds, (hipStream_t)stream_, raw, st, params, noise_tab, perm,
                     sample, target, target_vel, target_gvel, processed, sample_vel, L, J, input_n, n_steps, n_noise);
  return cg_launch_status();
}
