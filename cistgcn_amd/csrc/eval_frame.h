// Per-frame pose errors shared by the evaluation metrics (eval_metrics.hip) and the attack distortion metrics (attack_metrics.hip):
// one wavefront per frame, one lane per joint; the sums over the joints of a frame are wave reductions in fp64.
#pragma once
#include "cg_common.h"

#include <math.h>

// ---------------------------------------------------------------------------------------------
// 3x3 Procrustes rotation.  H = U diag(s) V^T; the reference forms R = V' U^T with the last ROW of V scaled by sigma = sign det(V U^T)
// (losses.py:106-119), i.e. R = diag(1,1,sigma) V U^T, and V U^T is the transposed polar factor of H: it does not depend on the signs
// or the order a particular SVD gives its vectors.  V and s^2 come from cyclic Jacobi rotations of H^T H in fp64, u_i = H v_i / s_i for
// the two larger singular values and u_3 = +-(u_1 x u_2), on the side of H v_3 (so a flat pose, s_3 = 0, still has a rotation).
// Every lane of the wave runs this on the same numbers.
// ---------------------------------------------------------------------------------------------
#define CG_EM_ROTATE(p, q, r)                                                              \
  if (A[p][q] != 0.0) {                                                                    \
    const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);                            \
    const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0)); \
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;                                \
    const double apq = A[p][q], arp = A[r][p], arq = A[r][q];                              \
    A[p][p] -= tt * apq;                                                                   \
    A[q][q] += tt * apq;                                                                   \
    A[p][q] = A[q][p] = 0.0;                                                               \
    A[r][p] = A[p][r] = c * arp - s * arq;                                                 \
    A[r][q] = A[q][r] = s * arp + c * arq;                                                 \
    for (int k = 0; k < 3; ++k) {                                                          \
      const double vp = V[k][p], vq = V[k][q];                                             \
      V[k][p] = c * vp - s * vq;                                                           \
      V[k][q] = s * vp + c * vq;                                                           \
    }                                                                                      \
  }

#define CG_EM_SWAP_COLS(i, j)                                                              \
  {                                                                                        \
    const double l = lam[i]; lam[i] = lam[j]; lam[j] = l;                                  \
    for (int k = 0; k < 3; ++k) { const double v = V[k][i]; V[k][i] = V[k][j]; V[k][j] = v; } \
  }

#define CG_EM_RANK1_TOL 1e-14      // on the eigenvalues of H^T H: a singular value below 1e-7 of the largest is rounding

// R0 = V U^T and the singular values of H (sv[2] the smallest)
__device__ __forceinline__ void cg_em_polar(const double (&H)[3][3], double (&R0)[3][3], double (&sv)[3]) {
  double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[i][j] = H[0][i] * H[0][j] + H[1][i] * H[1][j] + H[2][i] * H[2][j];
  for (int sweep = 0; sweep < 8; ++sweep) {       // quadratic convergence: 3x3 is at fp64 rounding after 5 sweeps
    CG_EM_ROTATE(0, 1, 2)
    CG_EM_ROTATE(0, 2, 1)
    CG_EM_ROTATE(1, 2, 0)
  }
  double lam[3] = {A[0][0], A[1][1], A[2][2]};
  if (lam[0] < lam[2]) CG_EM_SWAP_COLS(0, 2)
  if (lam[1] < lam[2]) CG_EM_SWAP_COLS(1, 2)
  double U[3][3];      // U[c][m]: component c of u_m
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    sv[m] = sqrt(fmax(lam[m], 0.0));
#pragma unroll
    for (int c = 0; c < 3; ++c) U[c][m] = H[c][0] * V[0][m] + H[c][1] * V[1][m] + H[c][2] * V[2][m];      // H v_m, scaled below
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { U[c][0] /= sv[0]; U[c][1] /= sv[1]; }
  // H of rank 1 (a frame of two joints, or all joints on one line): only one u_i is given by H.  The second is any unit vector
  // orthogonal to it and u_3 is taken on the side that makes V U^T a proper rotation (sigma = 1); the aligned pose does not depend on
  // the choice, and an SVD's own completion is as arbitrary.
  const double lbig = fmax(lam[0], lam[1]);
  const bool rank1 = lbig > 0.0 && fmin(lam[0], lam[1]) <= CG_EM_RANK1_TOL * lbig;
  if (rank1) {
    const bool first = lam[0] >= lam[1];      // the column that carries the direction
    const double u0 = first ? U[0][0] : U[0][1], u1 = first ? U[1][0] : U[1][1], u2 = first ? U[2][0] : U[2][1];
    const int k = fabs(u0) <= fabs(u1) && fabs(u0) <= fabs(u2) ? 0 : (fabs(u1) <= fabs(u2) ? 1 : 2);      // the axis furthest from u
    const double uk = k == 0 ? u0 : k == 1 ? u1 : u2;
    double w0 = (k == 0 ? 1.0 : 0.0) - uk * u0, w1 = (k == 1 ? 1.0 : 0.0) - uk * u1, w2 = (k == 2 ? 1.0 : 0.0) - uk * u2;
    const double wn = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    w0 /= wn; w1 /= wn; w2 /= wn;
    if (first) { U[0][1] = w0; U[1][1] = w1; U[2][1] = w2; sv[1] = 0.0; }
    else { U[0][0] = w0; U[1][0] = w1; U[2][0] = w2; sv[0] = 0.0; }
  }
  const double x0 = U[1][0] * U[2][1] - U[2][0] * U[1][1], x1 = U[2][0] * U[0][1] - U[0][0] * U[2][1], x2 = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  const double detV = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                      V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
  const double side = (rank1 ? detV : x0 * U[0][2] + x1 * U[1][2] + x2 * U[2][2]) < 0.0 ? -1.0 : 1.0;
  U[0][2] = side * x0; U[1][2] = side * x1; U[2][2] = side * x2;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R0[r][c] = V[r][0] * U[c][0] + V[r][1] * U[c][1] + V[r][2] * U[c][2];
}

__device__ __forceinline__ double cg_em_norm3(double a, double b, double c) { return sqrt(a * a + b * b + c * c); }

// The three errors of one joint of a frame (P the predicted joint, X the target; lanes with `on` false hold zeros):
//   e   = |P - X|                                                   losses.mpjpe (losses/losses.py:50-61)
//   en  = |c P - X|, c = mean_j(X.P) / mean_j(P.P)                  losses.n_mpjpe (:147-160)
//   epa = |a P R + t - X| after the Procrustes fit of the frame     losses.pa_mpjpe (:79-144), with the replacement of :94 and the NaN rule
// Every lane of the wave must call it.
__device__ __forceinline__ void cg_em_frame_errors(const double (&P)[3], const double (&X)[3], bool on, int J, double& e, double& en, double& epa) {
  e = cg_em_norm3(P[0] - X[0], P[1] - X[1], P[2] - X[2]);

  // sums over the joints, first round: centroids and the two means of n_mpjpe (lanes past J hold zeros)
  double r1[8] = {X[0], X[1], X[2], P[0], P[1], P[2], X[0] * P[0] + X[1] * P[1] + X[2] * P[2], P[0] * P[0] + P[1] * P[1] + P[2] * P[2]};
  cg_wave_allsum(r1);
  const double scale = (r1[6] / J) / (r1[7] / J);
  en = cg_em_norm3(scale * P[0] - X[0], scale * P[1] - X[1], scale * P[2] - X[2]);

  // second round: the centred poses, the reference's replacement of small target coordinates, norms and X0^T Y0
  double muX[3], muY[3], X0[3], Y0[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    muX[c] = r1[c] / J;
    muY[c] = r1[3 + c] / J;
    X0[c] = on ? X[c] - muX[c] : 0.0;
    Y0[c] = on ? P[c] - muY[c] : 0.0;
    if (on && X0[c] * X0[c] < 1e-6) X0[c] = 1e-3;      // losses.py:94, kept as it is
  }
  double r2[11];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) r2[3 * i + j] = X0[i] * Y0[j];
  r2[9] = X0[0] * X0[0] + X0[1] * X0[1] + X0[2] * X0[2];
  r2[10] = Y0[0] * Y0[0] + Y0[1] * Y0[1] + Y0[2] * Y0[2];
  cg_wave_allsum(r2);
  const double normX = fmax(sqrt(r2[9]), 1e-3), normY = sqrt(r2[10]);
  double H[3][3], R[3][3], sv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) H[i][j] = r2[3 * i + j] / (normX * normY);      // 0 / 0 = NaN when every predicted joint coincides
  cg_em_polar(H, R, sv);
  const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                     R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
  const double sigma = det > 0.0 ? 1.0 : (det < 0.0 ? -1.0 : det);      // torch.sign: 0 stays 0, NaN stays NaN
  double al = (sv[0] + sv[1] + sigma * sv[2]) * normX / normY, tr[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) R[2][c] *= sigma;
#pragma unroll
  for (int c = 0; c < 3; ++c) tr[c] = muX[c] - al * (muY[0] * R[0][c] + muY[1] * R[1][c] + muY[2] * R[2][c]);
  // losses.py:130-132, element by element: NaN in the scale -> 1, in the rotation -> 0, in the translation -> 0
  if (al != al) al = 1.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (tr[c] != tr[c]) tr[c] = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (R[r][c] != R[r][c]) R[r][c] = 0.0;
  }
  double dpa[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) dpa[c] = al * (P[0] * R[0][c] + P[1] * R[1][c] + P[2] * R[2][c]) + tr[c] - X[c];
  epa = cg_em_norm3(dpa[0], dpa[1], dpa[2]);
}
