// kl_cov.h -- the KL covariance between two positions, for every user: the
// basis kernels (kl_fit.hip, kl_fit_wide.hip: piercepoint against
// piercepoint) and the pixel / point bases (kl_eval.hip, kl_points.hip:
// piercepoint against (x, y, 0)).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace sf {

// -(|a - b|^2 / r0^2)^(beta/2) / 2 in numpy's evaluation order
// ((dx^2 + dy^2) + dz^2; sum(square(PIERCEPOINTS - (x, y, 0)), axis=1) for a
// pixel), no contraction.  One expression on purpose: a point at a grid
// position carries the bits of the grid's entry, and C of the wide basis is C
// of the narrow one.
__device__ inline double kl_cov(double ax, double ay, double az, double bx,
                                double by, double bz, double r0sq, double half_beta) {
#pragma clang fp contract(off)
  const double dx = ax - bx;
  const double dy = ay - by;
  const double dz = az - bz;
  const double d2 = (dx * dx + dy * dy) + dz * dz;
  return -pow(d2 / r0sq, half_beta) / 2.0;
}

// C[i][j] of the basis: a, b = [3] piercepoints
__device__ inline double kl_cov(const double* a, const double* b, double r0sq,
                                double half_beta) {
  return kl_cov(a[0], a[1], a[2], b[0], b[1], b[2], r0sq, half_beta);
}

}  // namespace sf
