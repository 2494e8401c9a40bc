// kl_fit_exact.h -- one _fit_screen (stationscreen.py:433-594) with the
// reference's exact pinv semantics, for a wavefront (kl_fit_general_kernel)
// and for a workgroup (kl_fit_wide_kernel): the subset basis by Jacobi, the
// normal equations by Cholesky or the truncated eigen-solve, the screen by
// C pinv(C) mat-vecs.
//
// Templates over the Team (kl_fit_steps.h) and a matrix-access struct X that
// says where things live (FitLds of kl_fit.hip: everything in LDS; WideFit of
// kl_fit_wide.hip: C / U / eig in global memory, V / M1 / M2 in LDS or a
// workspace):
//   csym(r, q)     C[r][q] = C[q][r] for the lane that holds r (C is symmetric
//                  bit for bit: kl_cov squares the differences), read the way
//                  X's memory likes
//   u(p, k), eigv(p)   the shared sorted basis and its eigenvalues
//   V, M1, M2, ld  the team's matrices; lam, idx, perm its subset state;
//   vec(k)         its k-th broadcast vector (six)
//   jacobi(), cholesky(), decomposed()   its solvers and its statistics
//   kFused         whether the pinv / C mat-vec sums are fused multiply-adds
#pragma once

#include "kl_fit_steps.h"

namespace sf {

struct Subset {
  int n;        // number of unflagged directions
  bool full;    // n == D: use the shared basis (quirk Q1)
  double wmin;  // smallest unflagged weight
};

// acc + a * b of the pinv / C mat-vecs.  The wavefront kernel has always
// fused them (its mat-vecs were compiled under the default contraction), the
// workgroup kernel never has; each keeps its bits.
template <bool FUSED>
__device__ __forceinline__ double mac(double a, double b, double acc) {
#pragma clang fp contract(off)
  if constexpr (FUSED) return fma(a, b, acc);
  return acc + a * b;
}

// Basis of the unflagged subset (stationscreen.py:493-499): idx, and for a
// flagged slot the eigen-decomposition of C_sub = C[idx][:, idx] in V /
// perm / lam (its columns split between the shares).  um: the team's vote on
// unfl, st: what follows from it.
template <class Team, class X>
__device__ void setup_subset(const Team& tm, const X& L, int D, const Subset& st,
                             const typename Team::Mask& um, bool unfl) {
  const int t = tm.lane();
  const int i = tm.row();
  const int ld = L.ld, n = st.n;
  if (t < D && unfl) L.idx[tm.rank(um)] = t;
  tm.sync();
  if (st.full || n == 0) return;  // shared U / eig (already sorted)
  if (i < n)
    for (int q = tm.share(); q < n; q += tm.shares())
      L.M1[i * ld + q] = L.csym(L.idx[i], L.idx[q]);
  tm.sync();
  L.jacobi(L.M1, L.V, n, ld);
  eig_order(tm, L.M1, n, ld, L.perm);
  if (t < n) {
    const int m = L.perm[t];
    L.lam[t] = L.M1[m * ld + m];
  }
  L.decomposed();
  tm.sync();
}

// column `rank` of the (sorted) U of the subset, or of the shared basis; row p
template <class X>
__device__ __forceinline__ double ucol(const X& L, bool full, int p, int rank) {
  return full ? L.u(p, rank) : L.V[p * L.ld + L.perm[rank]];
}

// y = pinv(C_sub) x (or pinv(C): full, n = D) for x held one element per
// lane (lanes < n), through the eigen-decomposition:
// y = sum_{|lam|>atol} u_r (u_r^T x) / lam_r.
template <class Team, class X>
__device__ double apply_pinv(const Team& tm, const X& L, bool full, int n,
                             double x, double* vtmp) {
#pragma clang fp contract(off)
  const int p = tm.lane();
  if (p < n) vtmp[p] = x;
  tm.sync();
  double t = 0.0;
  if (p < n) {
    for (int q = 0; q < n; ++q) t = mac<X::kFused>(ucol(L, full, q, p), vtmp[q], t);
    const double lam = full ? L.eigv(p) : L.lam[p];
    t = (fabs(lam) > kPinvAtol) ? t / lam : 0.0;
  }
  tm.sync();
  if (p < n) vtmp[p] = t;
  tm.sync();
  double y = 0.0;
  if (p < n)
    for (int r = 0; r < n; ++r) y = mac<X::kFused>(ucol(L, full, p, r), vtmp[r], y);
  tm.sync();
  return y;
}

// y_p = sum_q C[idx p][idx q] x_q  (lanes < n)
template <class Team, class X>
__device__ double apply_csub(const Team& tm, const X& L, int n, double x,
                             double* vtmp) {
#pragma clang fp contract(off)
  const int p = tm.lane();
  if (p < n) vtmp[p] = x;
  tm.sync();
  double y = 0.0;
  if (p < n) {
    const int r = L.idx[p];
    for (int q = 0; q < n; ++q) y = mac<X::kFused>(L.csym(r, L.idx[q]), vtmp[q], y);
  }
  tm.sync();
  return y;
}

// One _fit_screen call at order K.  Per direction (lane of row d, in every
// share): phi_d, w_d in, white_d, resid_d out.
template <class Team, class X>
__device__ void fit_screen(const Team& tm, const X& L, const Subset& st, int D,
                           int K, int screen_type,
                           const typename Team::Mask& um, double phi_d,
                           double w_d, double& white_d, double& resid_d) {
#pragma clang fp contract(off)
  using M = FitMath<false>;
  const int lp = tm.lane();
  const int i = tm.row();
  const int ld = L.ld, n = st.n;
  double* v0 = L.vec(0);
  double* v1 = L.vec(1);
  double* v2 = L.vec(2);
  double* v3 = L.vec(3);
  double* v4 = L.vec(4);
  double* v5 = L.vec(5);
  // the unflagged directions onto lanes p < n
  if (lp < D) {
    v4[lp] = screen_type == SF_SCREEN_AMPLITUDE ? M::lg10(phi_d) : phi_d;
    v5[lp] = w_d;
  }
  tm.sync();
  double phi_p = 0.0, w_p = 0.0;
  if (lp < n) {
    phi_p = v4[L.idx[lp]];
    w_p = v5[L.idx[lp]];
  }
  double rc, rs;
  if (screen_type == SF_SCREEN_PHASE) {
    double sn, cn;
    M::sin_cos(phi_p, &sn, &cn);
    rc = w_p * cn;  // W cos(phi)
    rs = w_p * sn;  // W sin(phi)
  } else {
    rc = w_p * phi_p;
    rs = 0.0;
  }
  if (lp < n) {
    v0[lp] = rc;
    v1[lp] = rs;
    v2[lp] = w_p;
  }
  tm.sync();
  double tie_lam[2] = {0.0, 0.0};
  if (n == 2)
    for (int k = 0; k < 2; ++k) tie_lam[k] = st.full ? L.eigv(k) : L.lam[k];
  const Tie2 tie(n, K, v0, v1, v2, tie_lam);
  // rr1 = U_k^T W r (lane k < K);  G = U_k^T W U_k (row k, the columns split
  // between the shares)
  double g1 = 0.0, g2 = 0.0;
  if (i < K) {
    if (tm.share() == 0) {
      for (int p = 0; p < n; ++p) {
        const double u = ucol(L, st.full, p, i);
        g1 += u * v0[p];
        g2 += u * v1[p];
      }
    }
    for (int j = tm.share(); j < K; j += tm.shares()) {
      double s = 0.0;
      for (int p = 0; p < n; ++p)
        s += ucol(L, st.full, p, i) * (v2[p] * ucol(L, st.full, p, j));
      L.M2[i * ld + j] = s;
    }
  }
  tm.sync();
  // inv_u = pinv(G, atol=1e-3) applied to rr1.  lambda_min(G) >= min w over
  // the unflagged rows (U_k has orthonormal columns over exactly those rows),
  // so for wmin above the cutoff pinv == inverse: Cholesky.  Otherwise the
  // eigen path reproduces the truncation.
  double a1 = g1, a2 = g2;
  if (K > 0) {
    if (st.wmin > kPinvAtol * (1.0 + 1e-9)) {
      L.cholesky(L.M2, K, ld, a1, a2);
    } else {
      truncated_eig_solve(tm, L, L.M2, L.M1, K, ld, v0, v1, v2, v3, a1, a2);
      tm.sync();
    }
  }
  // h = U_k a  (lane p < n)
  if (lp < K) {
    v0[lp] = a1;
    v1[lp] = a2;
  }
  tm.sync();
  double h1 = 0.0, h2 = 0.0;
  if (lp < n)
    for (int k = 0; k < K; ++k) {
      const double u = ucol(L, st.full, lp, k);
      h1 += u * v0[k];
      h2 += u * v1[k];
    }
  tm.sync();
  double screen;
  if (tie.on) {
    screen = tie.template screen<M>(screen_type, lp);
  } else if (screen_type == SF_SCREEN_PHASE) {
    const double re = apply_pinv(tm, L, st.full, n, h1, v3);
    const double im = apply_pinv(tm, L, st.full, n, h2, v3);
    const double cre = apply_csub(tm, L, n, re, v3);
    const double cim = apply_csub(tm, L, n, im, v3);
    screen = M::arctan2(cim, cre);
  } else {
    const double tf = apply_pinv(tm, L, st.full, n, h1, v3);
    screen = apply_csub(tm, L, n, tf, v3);
  }
  const double white = apply_pinv(tm, L, st.full, n, screen, v3);
  double wh, rd;
  if (st.full) {
    const double cw = apply_csub(tm, L, n, white, v3);  // idx = identity
    wh = white;
    rd = phi_d - model_value(screen_type, cw);
  } else {
    // flagged directions: the screen from the unflagged white coefficients,
    // then re-whitened with the full pinv (stationscreen.py:565-582)
    if (lp < n) {
      v0[lp] = screen;
      v1[lp] = white;
    }
    tm.sync();
    double screen_all = 0.0;
    if (lp < D) {
      if (w_d > 0.0) {
        screen_all = v0[tm.rank(um)];
      } else {
        for (int p = 0; p < n; ++p) screen_all += L.csym(lp, L.idx[p]) * v1[p];
      }
    }
    tm.sync();
    wh = apply_pinv(tm, L, true, D, screen_all, v3);
    rd = phi_d - model_value(screen_type, screen_all);
  }
  if constexpr (Team::shares() == 1) {
    white_d = wh;
    resid_d = rd;
  } else {
    // every share holds the direction's result
    if (lp < D) {
      v4[lp] = wh;
      v5[lp] = rd;
    }
    tm.sync();
    white_d = i < D ? v4[i] : 0.0;
    resid_d = i < D ? v5[i] : 0.0;
    tm.sync();
  }
}

}  // namespace sf
