// newmat's symmetric 3x3 eigensolver restated on the device, shared by ann.hip (k_ann_normals) and query.hip (the k-NN and
// fixed-radius normals, the adaptive-k normals of both): the PCA step of calculateNormal (normals.cc:518-558) after the
// covariance.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

namespace tdtk {

// newmat's EigenValues on a symmetric 3x3 (evalue.cpp:24-156, 283-284; sort.cpp:190-222): tred2, tql2, ascending
// sort.  z holds the matrix (lower triangle used) on entry and the eigenvectors (columns) on exit.
static __device__ __forceinline__ double nm_sign(double x, double y) { return (y >= 0) ? x : -x; }

static __device__ void eigen3_newmat(double z[3][3], double D[3])
{
  double E[3];
  const double tol = DBL_MIN / DBL_EPSILON;
  // tred2, n = 3
#pragma unroll
  for (int i = 2; i > 0; i--) {
    double f = z[i][i - 1], g = 0.0;
#pragma unroll
    for (int k = 0; k < i - 1; k++) g += z[i][k] * z[i][k];
    double h = g + f * f;
    if (g <= tol) { E[i] = f; h = 0.0; }
    else {
      g = nm_sign(-__dsqrt_rn(h), f); E[i] = g; h -= f * g;
      z[i][i - 1] = f - g; f = 0.0;
#pragma unroll
      for (int j = 0; j < i; j++) {
        z[j][i] = z[i][j] / h; g = 0.0;
#pragma unroll
        for (int k = 0; k < j; k++) g += z[j][k] * z[i][k];
#pragma unroll
        for (int k = j; k < i; k++) g += z[k][j] * z[i][k];
        E[j] = g / h; f += g * z[j][i];
      }
      const double hh = f / (h + h);
#pragma unroll
      for (int j = 0; j < i; j++) {
        f = z[i][j]; g = E[j] - hh * f; E[j] = g;
#pragma unroll
        for (int k = 0; k <= j; k++) z[j][k] -= (f * E[k] + g * z[i][k]);
      }
    }
    D[i] = h;
  }
  D[0] = 0.0; E[0] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    if (D[i] != 0.0) {
#pragma unroll
      for (int j = 0; j < i; j++) {
        double g = 0.0;
#pragma unroll
        for (int k = 0; k < i; k++) g += z[i][k] * z[k][j];
#pragma unroll
        for (int k = 0; k < i; k++) z[k][j] -= g * z[k][i];
      }
    }
#pragma unroll
    for (int j = 0; j < i; j++) { z[i][j] = 0.0; z[j][i] = 0.0; }
    D[i] = z[i][i]; z[i][i] = 1.0;
  }
  // tql2, n = 3
  const double eps = DBL_EPSILON;
  E[0] = E[1]; E[1] = E[2];
  double b = 0.0, f = 0.0;
  E[2] = 0.0;
#pragma unroll
  for (int l = 0; l < 3; l++) {
    double h = eps * (fabs(D[l]) + fabs(E[l]));
    if (b < h) b = h;
    int m = 3;
#pragma unroll
    for (int mm = 2; mm >= 0; mm--)
      if (mm >= l && fabs(E[mm]) <= b) m = mm;     // first m >= l with |E[m]| <= b (E[2] == 0 ends it)
    for (int j = 0; j < 30; j++) {
      if (m == l) break;
      double g = D[l];
      const double dl1 = (l == 0) ? D[1] : D[2];   // l < m <= 2 here
      double p = (dl1 - g) / (2.0 * E[l]), r = __dsqrt_rn(p * p + 1.0);
      D[l] = E[l] / (p < 0.0 ? p - r : p + r);
      const double hh = g - D[l];
      f += hh;
#pragma unroll
      for (int i = 1; i < 3; i++) if (i > l) D[i] -= hh;
      p = (m == 1) ? D[1] : D[2];
      double c = 1.0, s = 0.0;
#pragma unroll
      for (int i = 1; i >= 0; i--) {
        if (i <= m - 1 && i >= l) {
          const double ei = E[i], di = D[i];
          g = c * ei; h = c * p;
          if (fabs(p) >= fabs(ei)) {
            c = ei / p; r = __dsqrt_rn(c * c + 1.0);
            E[i + 1] = s * p * r; s = c / r; c = 1.0 / r;
          } else {
            c = p / ei; r = __dsqrt_rn(c * c + 1.0);
            E[i + 1] = s * ei * r; s = 1.0 / r; c /= r;
          }
          p = c * di - s * g; D[i + 1] = h + s * (c * g + s * di);
#pragma unroll
          for (int k = 0; k < 3; k++) {
            h = z[k][i + 1];
            z[k][i + 1] = s * z[k][i] + c * h;
            z[k][i] = c * z[k][i] - s * h;
          }
        }
      }
      E[l] = s * p; D[l] = c * p;
      if (fabs(E[l]) <= b) break;
    }
    D[l] += f;     // (30 sweeps without convergence throw in the reference; unreachable for a 3x3)
  }
  // SortSV ascending: selection sort, columns follow
#pragma unroll
  for (int i = 0; i < 3; i++) {
    int k = i;
    double p = D[i];
#pragma unroll
    for (int j = i + 1; j < 3; j++) if (D[j] < p) { k = j; p = D[j]; }
    if (k != i) {
#pragma unroll
      for (int kk = 1; kk < 3; kk++)
        if (kk == k) {
          D[kk] = D[i]; D[i] = p;
#pragma unroll
          for (int j = 0; j < 3; j++) { const double t = z[j][i]; z[j][i] = z[j][kk]; z[j][kk] = t; }
        }
    }
  }
}

// calculateNormal's tail (normals.cc:518-558) with the orientation of its callers (normals.cc:64-105, 369-516), in two
// parts.  The adaptive estimators (normals.cc:116-213, 563-682) read the eigenvalues between them.
//
// first part: z holds the covariance (lower triangle, c <= r, summed in list order) on entry, the eigenvectors (columns,
// ascending eigenvalues D) on exit
static __device__ __forceinline__ void cov_eigen(double z[3][3], double D[3])
{
  z[0][1] = z[1][0]; z[0][2] = z[2][0]; z[1][2] = z[2][1];
  eigen3_newmat(z, D);
}

// second part: the eigenvector of the smallest eigenvalue (nx, ny, nz = column 0), flipped so that n . (q - rPos) >= 0,
// normalised -- newmat's "v / norm" is v * (1 / norm)
static __device__ __forceinline__ void orient_normal(const double nx, const double ny, const double nz, const double qx,
                                                     const double qy, const double qz, const double rx, const double ry,
                                                     const double rz, double* out)
{
  double nv[3] = {nx, ny, nz};
  double pv[3] = {qx - rx, qy - ry, qz - rz};
  const double pl = 1.0 / __dsqrt_rn((pv[0] * pv[0] + pv[1] * pv[1]) + pv[2] * pv[2]);
  pv[0] *= pl; pv[1] *= pl; pv[2] *= pl;
  const double angle = (nv[0] * pv[0] + nv[1] * pv[1]) + nv[2] * pv[2];
  if (angle < 0) { nv[0] *= -1.0; nv[1] *= -1.0; nv[2] *= -1.0; }
  const double nl = 1.0 / __dsqrt_rn((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
  out[0] = nv[0] * nl;
  out[1] = nv[1] * nl;
  out[2] = nv[2] * nl;
}

// both parts: k_ann_normals and the fixed-k query.hip normals
static __device__ __forceinline__ void normal_from_cov(double z[3][3], const double qx, const double qy, const double qz,
                                                       const double rx, const double ry, const double rz, double* out)
{
  double D[3];
  cov_eigen(z, D);
  orient_normal(z[0][0], z[1][0], z[2][0], qx, qy, qz, rx, ry, rz, out);
}

// the stopping rule of the adaptive estimators (normals.cc:189, 653), D ascending.  Kept in the reference's sense: with
// e3 == 0 the quotient is NaN or inf and the test is false
static __device__ __forceinline__ bool adaptive_k_accepts(const double D[3])
{
  const double e1 = D[0], e2 = D[1], e3 = D[2];
  return (e1 > 0.25 * e2) && (fabs(1.0 - e2 / e3) < 0.25);
}

}  // namespace tdtk
