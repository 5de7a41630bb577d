// Rotation matrix of a rotation vector in degrees, shared by the robustness-test kernel (input_pipeline.hip, per frame) and the device
// draws (augment_draw.hip, per sample).
#pragma once
#include "cg_common.h"

#include <math.h>

// scipy's Rotation.from_rotvec(., degrees=True).as_matrix() (custom_transforms.py:69): Rodrigues' formula
// in f64, operation by operation what environment/input_pipeline.py::_rotvec_matrix does on the host for cg_augment_sequences (no
// contraction into FMAs), rounded to f32 at the end; row-major, used as p' = p R.
__device__ __forceinline__ void cg_rotvec_matrix(float dx, float dy, float dz, float* R) {
#pragma clang fp contract(off)
  const double rad = 3.14159265358979323846 / 180.0;
  const double v[3] = {(double)dx * rad, (double)dy * rad, (double)dz * rad};
  const double th = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (!(th > 0.0)) {
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.f : 0.f;
    return;
  }
  const double k[3] = {v[0] / th, v[1] / th, v[2] / th};
  const double K[3][3] = {{0.0, -k[2], k[1]}, {k[2], 0.0, -k[0]}, {-k[1], k[0], 0.0}};
  const double sn = sin(th), c1 = 1.0 - cos(th);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double kk = 0.0;
      for (int m = 0; m < 3; ++m) kk += K[i][m] * K[m][j];
      R[3 * i + j] = (float)(((i == j ? 1.0 : 0.0) + sn * K[i][j]) + c1 * kk);
    }
}
