// kl_fit_steps.h -- the per-slot steps of the KL fit, once: what the three
// slot loops (kl_fit_general_kernel, kl_fit_pass_kernel, kl_fit_wide_kernel)
// restate of stationscreen.py's _process_station (:597-782), _flag_outliers
// (:303-350) and _circ_chi2 (:353-387).  Every sum keeps one order, so a
// kernel that calls a step computes the bits every other caller computes.
//
// Two small policies parameterise the steps:
//   Math  FitMath<NI>: the fp64 transcendentals, inlined or called;
//   Team  the lanes that hold one slot: Group<SPW> (sf_wave.h) for a wave or
//         half-wave, WideTeam (kl_fit_wide.h) for the 256-thread workgroup.
//         lane(), row() / share() / shares() (the column split; row = lane,
//         0 and 1 on a wave), sync(), sum() of N terms at once, max(),
//         ballot() and rank().
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "screenfit.h"
#include "sf_wave.h"

namespace sf {

constexpr double kPinvAtol = 1e-3;   // pinv(rcond=1e-3), scipy>=1.7 semantics
constexpr int kJacobiMaxSweeps = 40;

// row stride of an n x n fp64 matrix: odd, so that lane i reading row i hits
// distinct LDS bank pairs
__host__ __device__ inline int odd_ld(int n) { return n | 1; }

// The fp64 transcendentals of a slot step, inlined or called (NI).  Inlined
// into the two-slots-per-wave pass, their polynomial constants were hoisted
// out of the slot loop into ~100 VGPRs (235-256 VGPRs: 2 waves per SIMD for
// a latency-bound kernel); called, that pass fits 128 VGPRs at 4 waves per
// SIMD (config-4 fit 34 -> 28 ms, gain fits faster still).  The one-slot
// pass (D > 32) calls them too, with C read from L2 so that its LDS admits
// the same 4 waves per SIMD (calls alone, LDS-capped at 3, were slower).
// The SLOW class, the general and the wide kernel keep them inlined.  Same
// functions either way, same bits.
inline __device__ __noinline__ void nl_sincos(double x, double* s, double* c) { sincos(x, s, c); }
inline __device__ __noinline__ double nl_atan2(double y, double x) { return atan2(y, x); }
inline __device__ __noinline__ double nl_log10(double x) { return log10(x); }
inline __device__ __noinline__ double nl_pow(double x, double y) { return pow(x, y); }
inline __device__ __noinline__ double nl_log(double x) { return log(x); }
inline __device__ __noinline__ double nl_fmod(double x, double y) { return fmod(x, y); }

template <bool NI>
struct FitMath {
  static __device__ __forceinline__ void sin_cos(double x, double* s, double* c) {
    if constexpr (NI) nl_sincos(x, s, c); else sincos(x, s, c);
  }
  static __device__ __forceinline__ double arctan2(double y, double x) {
    if constexpr (NI) return nl_atan2(y, x); else return atan2(y, x);
  }
  static __device__ __forceinline__ double lg10(double x) {
    if constexpr (NI) return nl_log10(x); else return log10(x);
  }
  static __device__ __forceinline__ double power(double x, double y) {
    if constexpr (NI) return nl_pow(x, y); else return pow(x, y);
  }
  static __device__ __forceinline__ double ln(double x) {
    if constexpr (NI) return nl_log(x); else return log(x);
  }
  static __device__ __forceinline__ double mod(double x, double y) {
    if constexpr (NI) return nl_fmod(x, y); else return fmod(x, y);
  }
};

// value of direction d of slot s (station a of A) after referencing: minus
// the external reference phases, or minus station `sub` of the same time and
// frequency
__device__ __forceinline__ double phase_ref(const double* phase,
                                            const double* refph, int sub,
                                            int64_t s, int a, int A, int D,
                                            int d) {
  double v = phase[s * D + d];
  if (refph) v -= refph[(s / A) * D + d];
  else if (sub >= 0) v -= phase[(s + (sub - a)) * D + d];
  return v;
}

// Where slot s = (t * F + f) * A + a sits: its station, frequency and
// (station, freq) block, and whether no pass fits it -- the reference
// station's slots and the skipped blocks (stationscreen.py:818-825)
struct SlotGeom {
  int a, f, blk;
  __device__ __forceinline__ SlotGeom(int64_t s, int F, int A)
      : a((int)(s % A)), f((int)((s / A) % F)), blk(f * A + a) {}
  __device__ __forceinline__ bool skipped(const uint8_t* skip, int ref_skip) const {
    return a == ref_skip || skip[blk];
  }
};

// amplitude screens are log10 values (stationscreen.py:535-548, 576-588)
template <class Math = FitMath<false>>
__device__ __forceinline__ double model_value(int screen_type, double x) {
  return screen_type == SF_SCREEN_AMPLITUDE ? Math::power(10.0, x) : x;
}

// residual as the outlier test / chi^2 see it (stationscreen.py:660-668,
// 733-746): phase & tec use the residual, amplitude the log10 ratio
template <class Math = FitMath<false>>
__device__ __forceinline__ double screen_diff(int screen_type, double val,
                                              double resid) {
  if (screen_type == SF_SCREEN_AMPLITUDE)
    return Math::lg10(val) - Math::lg10(fabs(val - resid));
  return resid;
}

// The order walk of adjust_order (stationscreen.py:700-782): up to four
// fits of one slot, each followed by one step from the reduced chi^2 of its
// residual.
struct OrderWalk {
  bool hit_upper = false, hit_lower = false, hit_upper2 = false,
       hit_lower2 = false;
  double sign = 1.0, prev_redchi2 = 0.0;

  // the walk met a bound twice: the fit just made is the last
  __device__ __forceinline__ bool done() const { return hit_lower2 || hit_upper2; }

  // Step `oi` from redchi2: moves `order` within [station_order, n_unfl - 1];
  // returns true where the walk stops (the order did not move).
  template <class Math>
  __device__ __forceinline__ bool step(int oi, double redchi2, int n_unfl,
                                       double station_order, double& order) {
#pragma clang fp contract(off)
    if (oi > 0) {
      if (redchi2 > 1.0 && prev_redchi2 < redchi2) sign = -sign;
      if (redchi2 < 1.0 && prev_redchi2 > redchi2) sign = -sign;
    }
    prev_redchi2 = redchi2;
    const double order_factor = Math::power((double)n_unfl - order, 0.2);
    double target = order - sign * order_factor * (1.0 - redchi2);
    target = fmax(station_order, target);
    target = fmin(rint(target), (double)(n_unfl - 1));
    if (target <= 0.0) target = fmin(station_order, (double)(n_unfl - 1));
    if (target == order) return true;
    if (target == n_unfl - 1) {
      if (hit_upper) hit_upper2 = true;
      hit_upper = true;
    }
    if (target == station_order) {
      if (hit_lower) hit_lower2 = true;
      hit_lower = true;
    }
    order = target;
    return false;
  }
};

// Reduced chi^2 of a slot's residual at `order`.  live: this lane holds a
// direction; unfl: with a positive weight.
template <class Math, class Team>
__device__ __forceinline__ double slot_redchi2(const Team& tm, int screen_type,
                                               bool live, bool unfl,
                                               double phi_d, double w_d,
                                               double resid_d, int n_unfl,
                                               double order) {
#pragma clang fp contract(off)
  if (screen_type == SF_SCREEN_PHASE) {
    // _circ_chi2: squares of sin / cos (quirk Q7)
    double sn = 0.0, cn = 0.0;
    if (unfl) Math::sin_cos(resid_d, &sn, &cn);
    const double ww = unfl ? w_d : 0.0;
    double r[3] = {ww, sn * sn * ww, cn * cn * ww};
    tm.sum(r);
    const double m1 = r[1] / r[0];
    const double m2 = r[2] / r[0];
    return (1.0 - hypot(m1, m2)) * r[0] / (n_unfl - order);
  }
  // np.sum(square(diff) * w) over all directions
  double r[1] = {0.0};
  if (live) {
    const double sd = screen_diff<Math>(screen_type, phi_d, resid_d);
    r[0] = (sd * sd) * w_d;
  }
  tm.sum(r);
  return r[0] / (n_unfl - order);
}

// _flag_outliers on one phase slot (stationscreen.py:303-350): circular std
// across directions of the wrapped residual; an outlier's weight becomes 0.
// Returns whether THIS lane was flagged (the callers that keep a mask vote
// on it; the slot must have an unflagged direction).
template <class Math, class Team>
__device__ __forceinline__ bool flag_circular_outliers(const Team& tm, bool live,
                                                       double nsigma,
                                                       double resid_d,
                                                       double& w_d) {
#pragma clang fp contract(off)
  double r = Math::mod(resid_d, 2.0 * M_PI);
  if (r < -M_PI) r += 2.0 * M_PI;
  if (r > M_PI) r -= 2.0 * M_PI;
  const bool inc = live && (w_d != 0.0) && !isnan(r);
  double sn = 0.0, cn = 0.0;
  if (inc) Math::sin_cos(r, &sn, &cn);
  double t[3] = {inc ? 1.0 : 0.0, sn, cn};
  tm.sum(t);
  const double ms = t[1] / t[0];
  const double mc = t[2] / t[0];
  const double stdv = sqrt(-2.0 * Math::ln(hypot(ms, mc)));
  const bool outl = live && (fabs(r) > nsigma * stdv);
  if (outl) w_d = 0.0;
  return outl;
}

// Two unflagged directions (order clipped to n - 1 = 1): their C is
// [[0, b], [b, 0]], singular values |b| twice, and the reference's
// svd(C)[0] (LAPACK gesdd, stationscreen.py:427) is [[0, 1], [1, 0]] --
// unit vectors, not eigenvectors -- whose first column e_2 it keeps
// (:490-534): inv_u = pinv([w_2]) (0 below the 1e-3 cutoff), the fit
// C pinv(C) e_2 inv_u w_2 x_2 = (0, t), and the screen (0, atan2(t_im,
// t_re)) -- 0 = atan2(+0, +0) where the BLAS products leave +0
// (tests/golden/make_golden_ties.py pins it; LAPACK builds whose SVD
// leaves rounding residue there give atan2 of that residue instead).
// Taken from rc = W cos / W x, rs = W sin and w of the gathered directions
// before those vectors are overwritten.
// Only while the pair's eigenvalues (lam: those of the slot's basis, +-b)
// pass the pinv cutoff: at |b| <= 1e-3 (a pair closer than ~2.4
// piercepoint units at r_0 = 100, or a large r_0) the reference's pinv(C) is 0, and the slot goes
// the ordinary way, whose `keep` tests leave the screen and the coefficients
// at +0 and the residual at the values (tests/golden/make_golden_near.py).
struct Tie2 {
  bool on;
  double t_re = 0.0, t_im = 0.0;
  __device__ __forceinline__ Tie2(int n, int K, const double* rc,
                                  const double* rs, const double* w,
                                  const double* lam)
      : on(n == 2 && K == 1 && fabs(lam[0]) > kPinvAtol &&
           fabs(lam[1]) > kPinvAtol) {
#pragma clang fp contract(off)
    // w_2 at or below the cutoff: inv_u = 0 and t stays (+0, +0) -- not
    // 0 * rc, whose zero takes the sign of cos(phi_2) and would make
    // atan2(0, -0) = pi where the reference's screen is 0 (near_tie4.npz)
    if (on && w[1] > kPinvAtol) {
      const double iw = 1.0 / w[1];
      t_re = iw * rc[1];
      t_im = iw * rs[1];
    }
  }
  template <class Math>
  __device__ __forceinline__ double screen(int screen_type, int l) const {
    return l != 1 ? 0.0
           : screen_type == SF_SCREEN_PHASE ? Math::arctan2(t_im, t_re) : t_re;
  }
};

// a = pinv(G, atol=1e-3) b for two right-hand sides (b1, b2 on lanes < K in,
// a1, a2 out) where a weight below the cutoff can truncate: G = Z diag(mu)
// Z^T by the Jacobi of `L` (G in place, Z into M), then
// sum_{|mu| > 1e-3} z z^T b / mu (scipy >= 1.7).  v0..v3: vectors of the team.
template <class Team, class X>
__device__ __forceinline__ void truncated_eig_solve(const Team& tm, const X& L,
                                                    double* G, double* M, int K,
                                                    int ld, double* v0,
                                                    double* v1, double* v2,
                                                    double* v3, double& a1,
                                                    double& a2) {
#pragma clang fp contract(off)
  const int l = tm.lane();
  L.jacobi(G, M, K, ld);
  if (l < K) {
    v0[l] = a1;
    v1[l] = a2;
  }
  tm.sync();
  double t1 = 0.0, t2 = 0.0;
  if (l < K) {
    for (int q = 0; q < K; ++q) {
      t1 += M[q * ld + l] * v0[q];
      t2 += M[q * ld + l] * v1[q];
    }
    const double mu = G[l * ld + l];
    if (fabs(mu) > kPinvAtol) {
      t1 /= mu;
      t2 /= mu;
    } else {
      t1 = t2 = 0.0;
    }
  }
  tm.sync();
  if (l < K) {
    v2[l] = t1;
    v3[l] = t2;
  }
  tm.sync();
  a1 = a2 = 0.0;
  if (l < K)
    for (int m = 0; m < K; ++m) {
      a1 += M[l * ld + m] * v2[m];
      a2 += M[l * ld + m] * v3[m];
    }
}

}  // namespace sf
