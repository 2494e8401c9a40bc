// kl_fit_wide.hip -- the KL basis and the per-slot KL fit with 61..128
// directions (gfx950, float64): sf_set_basis_wide and sf_kl_fit on a
// wide-basis context.
//
// The same restatement of stationscreen.run as kl_fit.hip
// (_process_station / _fit_screen / _flag_outliers / _circ_chi2,
// stationscreen.py:597-782, 433-594, 303-350, 353-387), with one WORKGROUP of
// 256 threads per slot instead of one wavefront: thread t handles direction
// t & 127, the two 128-thread shares split the column pairs of the Jacobi
// rounds and the columns of the normal matrix (kl_fit_wide.h).
//   * kl_basis_wide_kernel    <- _calculate_svd for D <= 128 (one workgroup,
//                                matrices in a global workspace)
//   * kl_wide_init_kernel     <- per-slot state before pass 0
//   * kl_fit_wide_kernel      <- one outlier iteration `it` for all slots;
//                                state in coef / resid / w_out / order_out
//   * kl_wide_block_flag_kernel <- tec / amplitude flags from the
//                                (station, freq) block sigma (quirk Q6)
// A slot with every direction unflagged uses the global basis (quirk Q1); a
// slot with flagged directions decomposes its own C_sub (no mask cache above
// 60 directions).  The shared C and U are read from global memory (L2); the
// per-workgroup matrices V / M1 / M2 sit in LDS as far as 160 KiB reach, the
// rest in a workspace sized by the (capped, persistent) grid.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kl_cov.h"
#include "kl_fit_wide.h"
#include "sf_internal.h"

namespace sf {

// ---------------------------------------------------------------------------
// basis: one workgroup; a and v ([D][ld] each) in the global workspace `ws`
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWideThreads) void kl_basis_wide_kernel(
    const double* __restrict__ pp, int D, double r0, double beta,
    double* __restrict__ c_out, double* __restrict__ pinv_out,
    double* __restrict__ u_out, double* __restrict__ eig_out, double* ws) {
#pragma clang fp contract(off)
  __shared__ WideSmall S;
  const int ld = wide_ld(D);
  double* a = ws;
  double* v = ws + (size_t)D * ld;
  const int i = wide_row();
  const int w = wide_share();
  const double r0sq = r0 * r0, hb = beta / 2.0;
  if (i < D) {
    for (int j = w; j < D; j += kWideShares) {
      const double c = kl_cov(pp + 3 * i, pp + 3 * j, r0sq, hb);
      a[i * ld + j] = c;
      c_out[i * D + j] = c;
    }
  }
  __syncthreads();
  wide_jacobi(a, v, S, D, ld, kWideMaxSweeps);
  wide_eig_order(a, D, ld, S.perm);
  if ((int)threadIdx.x < D) {
    const int m = S.perm[threadIdx.x];
    const double lam = a[m * ld + m];
    eig_out[threadIdx.x] = lam;
    S.lam[threadIdx.x] = lam;
  }
  __syncthreads();
  if (i < D) {
    for (int r = w; r < D; r += kWideShares) u_out[i * D + r] = v[i * ld + S.perm[r]];
    for (int j = w; j < D; j += kWideShares) {
      double s = 0.0;
      for (int r = 0; r < D; ++r) {
        const int m = S.perm[r];
        const double lam = S.lam[r];
        if (fabs(lam) > kWideAtol) s += v[i * ld + m] * (v[j * ld + m] / lam);
      }
      pinv_out[i * D + j] = s;
    }
  }
}

// ---------------------------------------------------------------------------
// per-slot fit
// ---------------------------------------------------------------------------
__device__ __forceinline__ double wide_phase_ref(const double* phase,
                                                 const double* refph, int sub,
                                                 int64_t s, int a, int A, int D,
                                                 int d) {
  double v = phase[s * D + d];
  if (refph) v -= refph[(s / A) * D + d];
  else if (sub >= 0) v -= phase[(s + (sub - a)) * D + d];
  return v;
}

// amplitude screens are log10 values (stationscreen.py:535-548, 576-588)
__device__ __forceinline__ double wide_model_value(int screen_type, double x) {
  return screen_type == SF_SCREEN_AMPLITUDE ? pow(10.0, x) : x;
}

// residual as the outlier test / chi^2 see it (stationscreen.py:660-668,
// 733-746): phase & tec the residual, amplitude the log10 ratio
__device__ __forceinline__ double wide_screen_diff(int screen_type, double val,
                                                   double resid) {
  if (screen_type == SF_SCREEN_AMPLITUDE)
    return log10(val) - log10(fabs(val - resid));
  return resid;
}

struct WideFit {
  WideSmall* S;
  const double* gC;    // [D][D] global
  const double* gU;    // [D][D] global, columns sorted
  const double* gEig;  // [D]
  double* V;           // [D][ld] eigenvectors of C_sub (unsorted columns)
  double* M1;          // [D][ld] scratch
  double* M2;          // [D][ld] normal matrix / scratch
  int D, ld;
  int n;        // unflagged directions
  bool full;    // n == D: the shared basis (quirk Q1)
  double wmin;  // smallest unflagged weight
};

// Basis of the unflagged subset (stationscreen.py:493-499): idx, and for a
// flagged slot the eigen-decomposition of C_sub in V / perm / lam.
__device__ void wide_setup_subset(WideFit& L, const WideMask& um, bool unfl,
                                  int* counters) {
  WideSmall& S = *L.S;
  const int t = threadIdx.x;
  const int i = wide_row();
  const int w = wide_share();
  const int D = L.D, ld = L.ld, n = L.n;
  if (t < D && unfl) S.idx[wide_rank(um, t)] = t;
  __syncthreads();
  if (L.full || n == 0) return;
  // C_sub = C[idx][:, idx] (C is symmetric: read along the row of idx[q])
  if (i < n)
    for (int q = w; q < n; q += kWideShares)
      L.M1[i * ld + q] = L.gC[(size_t)S.idx[q] * D + S.idx[i]];
  __syncthreads();
  wide_jacobi(L.M1, L.V, S, n, ld, kWideMaxSweeps);
  wide_eig_order(L.M1, n, ld, S.perm);
  if (t < n) {
    const int m = S.perm[t];
    S.lam[t] = L.M1[m * ld + m];
  }
  if (t == 0) atomicAdd(counters, 1);
  __syncthreads();
}

// column `rank` of the (sorted) U of the current subset, row p
__device__ __forceinline__ double wide_ucol(const WideFit& L, int p, int rank) {
  return L.full ? L.gU[(size_t)p * L.D + rank] : L.V[p * L.ld + L.S->perm[rank]];
}

// y = pinv(C_sub) x for x on threads < n, through the eigen-decomposition
__device__ double wide_apply_pinv(const WideFit& L, bool full, int n, double x,
                                  double* vtmp) {
#pragma clang fp contract(off)
  const int p = threadIdx.x;
  WideFit B = L;
  B.full = full;
  if (p < n) vtmp[p] = x;
  __syncthreads();
  double t = 0.0;
  if (p < n) {
    for (int q = 0; q < n; ++q) t += wide_ucol(B, q, p) * vtmp[q];
    const double lam = full ? L.gEig[p] : L.S->lam[p];
    t = (fabs(lam) > kWideAtol) ? t / lam : 0.0;
  }
  __syncthreads();
  if (p < n) vtmp[p] = t;
  __syncthreads();
  double y = 0.0;
  if (p < n)
    for (int r = 0; r < n; ++r) y += wide_ucol(B, p, r) * vtmp[r];
  __syncthreads();
  return y;
}

// y_p = sum_q C[idx p][idx q] x_q  (threads < n)
__device__ double wide_apply_csub(const WideFit& L, int n, double x, double* vtmp) {
#pragma clang fp contract(off)
  const int p = threadIdx.x;
  const int* idx = L.S->idx;
  if (p < n) vtmp[p] = x;
  __syncthreads();
  double y = 0.0;
  if (p < n) {
    const int r = idx[p];
    for (int q = 0; q < n; ++q) y += L.gC[(size_t)idx[q] * L.D + r] * vtmp[q];
  }
  __syncthreads();
  return y;
}

// One _fit_screen call (stationscreen.py:433-594) at order K: fit_screen of
// kl_fit.hip on a workgroup, plus the log10 / 10^x of amplitude screens.
// Per direction thread d = t & 127 (both shares): phi_d, w_d in, white_d,
// resid_d out.
__device__ void wide_fit_screen(const WideFit& L, int K, int screen_type,
                                const WideMask& um, double phi_d, double w_d,
                                double& white_d, double& resid_d) {
#pragma clang fp contract(off)
  WideSmall& S = *L.S;
  const int lp = threadIdx.x;
  const int w = wide_share();
  const int i = wide_row();
  const int D = L.D, ld = L.ld, n = L.n;
  double* v0 = S.vec[0];
  double* v1 = S.vec[1];
  double* v2 = S.vec[2];
  double* v3 = S.vec[3];
  double* v4 = S.vec[4];
  double* v5 = S.vec[5];
  // the unflagged directions onto threads p < n
  if (lp < D) {
    v4[lp] = screen_type == SF_SCREEN_AMPLITUDE ? log10(phi_d) : phi_d;
    v5[lp] = w_d;
  }
  __syncthreads();
  double phi_p = 0.0, w_p = 0.0;
  if (lp < n) {
    phi_p = v4[S.idx[lp]];
    w_p = v5[S.idx[lp]];
  }
  double rc, rs;
  if (screen_type == SF_SCREEN_PHASE) {
    double sn, cn;
    sincos(phi_p, &sn, &cn);
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
  __syncthreads();
  // two unflagged directions: the reference's U_k = e_2 (fit_once in
  // kl_fit_fast.hip has the derivation)
  const bool tie2 = n == 2 && K == 1;
  double t_re = 0.0, t_im = 0.0;
  if (tie2) {
    const double w2 = v2[1];
    const double iw = w2 > kWideAtol ? 1.0 / w2 : 0.0;
    t_re = iw * v0[1];
    t_im = iw * v1[1];
  }
  // rr1 = U_k^T W r (thread k < K);  G = U_k^T W U_k (row k, the columns
  // split between the shares)
  double g1 = 0.0, g2 = 0.0;
  if (i < K) {
    if (w == 0) {
      for (int p = 0; p < n; ++p) {
        const double u = wide_ucol(L, p, i);
        g1 += u * v0[p];
        g2 += u * v1[p];
      }
    }
    for (int j = w; j < K; j += kWideShares) {
      double s = 0.0;
      for (int p = 0; p < n; ++p)
        s += wide_ucol(L, p, i) * (v2[p] * wide_ucol(L, p, j));
      L.M2[i * ld + j] = s;
    }
  }
  __syncthreads();
  // inv_u = pinv(G, atol=1e-3) rr1: Cholesky when lambda_min(G) >= wmin is
  // above the cutoff, else the truncated eigen-solve (see kl_fit.hip)
  double a1 = g1, a2 = g2;
  if (K > 0) {
    if (L.wmin > kWideAtol * (1.0 + 1e-9)) {
      wide_cholesky_solve2(L.M2, K, ld, a1, a2, S.red);
    } else {
      wide_jacobi(L.M2, L.M1, S, K, ld, kWideMaxSweeps);
      if (lp < K) {
        v0[lp] = g1;
        v1[lp] = g2;
      }
      __syncthreads();
      double t1 = 0.0, t2 = 0.0;
      if (lp < K) {
        for (int q = 0; q < K; ++q) {
          t1 += L.M1[q * ld + lp] * v0[q];
          t2 += L.M1[q * ld + lp] * v1[q];
        }
        const double mu = L.M2[lp * ld + lp];
        if (fabs(mu) > kWideAtol) {
          t1 /= mu;
          t2 /= mu;
        } else {
          t1 = t2 = 0.0;
        }
      }
      __syncthreads();
      if (lp < K) {
        v2[lp] = t1;
        v3[lp] = t2;
      }
      __syncthreads();
      a1 = a2 = 0.0;
      if (lp < K)
        for (int m = 0; m < K; ++m) {
          a1 += L.M1[lp * ld + m] * v2[m];
          a2 += L.M1[lp * ld + m] * v3[m];
        }
      __syncthreads();
    }
  }
  // h = U_k a  (thread p < n)
  if (lp < K) {
    v0[lp] = a1;
    v1[lp] = a2;
  }
  __syncthreads();
  double h1 = 0.0, h2 = 0.0;
  if (lp < n)
    for (int k = 0; k < K; ++k) {
      const double u = wide_ucol(L, lp, k);
      h1 += u * v0[k];
      h2 += u * v1[k];
    }
  __syncthreads();
  double screen;
  if (tie2) {
    screen = lp != 1 ? 0.0
             : screen_type == SF_SCREEN_PHASE ? atan2(t_im, t_re) : t_re;
  } else if (screen_type == SF_SCREEN_PHASE) {
    const double re = wide_apply_pinv(L, L.full, n, h1, v3);
    const double im = wide_apply_pinv(L, L.full, n, h2, v3);
    const double cre = wide_apply_csub(L, n, re, v3);
    const double cim = wide_apply_csub(L, n, im, v3);
    screen = atan2(cim, cre);
  } else {
    const double tf = wide_apply_pinv(L, L.full, n, h1, v3);
    screen = wide_apply_csub(L, n, tf, v3);
  }
  const double white = wide_apply_pinv(L, L.full, n, screen, v3);
  double wh, rd;
  if (L.full) {
    const double cw = wide_apply_csub(L, n, white, v3);  // idx = identity
    wh = white;
    rd = phi_d - wide_model_value(screen_type, cw);
  } else {
    // flagged directions: the screen from the unflagged white coefficients,
    // then re-whitened with the full pinv (stationscreen.py:565-582)
    if (lp < n) {
      v0[lp] = screen;
      v1[lp] = white;
    }
    __syncthreads();
    double screen_all = 0.0;
    if (lp < D) {
      if (w_d > 0.0) {
        screen_all = v0[wide_rank(um, lp)];
      } else {
        for (int p = 0; p < n; ++p)
          screen_all += L.gC[(size_t)S.idx[p] * D + lp] * v1[p];
      }
    }
    __syncthreads();
    wh = wide_apply_pinv(L, true, D, screen_all, v3);
    rd = phi_d - wide_model_value(screen_type, screen_all);
  }
  // both shares hold the direction's result
  if (lp < D) {
    v4[lp] = wh;
    v5[lp] = rd;
  }
  __syncthreads();
  white_d = i < D ? v4[i] : 0.0;
  resid_d = i < D ? v5[i] : 0.0;
  __syncthreads();
}

// (station, freq) block skip for D <= 128 (kl_skip_kernel of kl_fit.hip has
// one 64-lane wave per block): all phases NaN after referencing, or all
// weights zero (stationscreen.py:821-825).  One 128-thread workgroup per block.
__global__ __launch_bounds__(kWideRows) void kl_wide_skip_kernel(
    const double* __restrict__ phase, const float* __restrict__ weight, int T,
    int F, int A, int D, int ref, const double* __restrict__ refph,
    uint8_t* __restrict__ skip) {
  const int blk = blockIdx.x;  // f * A + a
  const int f = blk / A, a = blk % A;
  const int d = threadIdx.x;
  int any_val = 0, any_w = 0;
  if (d < D) {
    for (int t = 0; t < T; ++t) {
      const int64_t s = (int64_t)(t * F + f) * A + a;
      const double ph = wide_phase_ref(phase, refph, ref, s, a, A, D, d);
      any_val |= !isnan(ph);
      any_w |= weight[s * D + d] != 0.0f;
    }
  }
  const int av = __syncthreads_or(any_val);
  const int aw = __syncthreads_or(any_w);
  if (d == 0) skip[blk] = (!av || !aw) ? 1 : 0;
}

// state of every slot before pass 0: weights, orders; zero outputs of the
// skipped blocks (the passes write every other slot)
__global__ __launch_bounds__(256) void kl_wide_init_kernel(
    const float* __restrict__ weight, int64_t S, int F, int A, int D,
    const int* __restrict__ st_order, const uint8_t* __restrict__ skip,
    int ref_skip, double* __restrict__ coef, double* __restrict__ resid,
    float* __restrict__ w_out, int32_t* __restrict__ order_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S * D) return;
  const int64_t s = e / D;
  const int d = (int)(e % D);
  const int a = (int)(s % A);
  const int f = (int)((s / A) % F);
  const bool skipped = a == ref_skip || skip[f * A + a];
  w_out[e] = weight[e];
  if (skipped) {
    coef[e] = 0.0;
    resid[e] = 0.0;
  }
  if (d == 0) order_out[s] = skipped ? 0 : st_order[a];
}

// tec / amplitude: |diff| > nsigma sigma(block) -> weight 0
__global__ __launch_bounds__(256) void kl_wide_block_flag_kernel(
    int64_t S, int F, int A, int D, const double* __restrict__ phase,
    const double* __restrict__ refph, int ref_sub,
    const uint8_t* __restrict__ skip, int ref_skip, int screen_type,
    double nsigma, const double* __restrict__ sigma,
    const double* __restrict__ resid, float* __restrict__ w_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S * D) return;
  const int64_t s = e / D;
  const int d = (int)(e % D);
  const int a = (int)(s % A);
  const int f = (int)((s / A) % F);
  if (a == ref_skip || skip[f * A + a]) return;
  const double sig = sigma[f * A + a];
  const double v = wide_phase_ref(phase, refph, ref_sub, s, a, A, D, d);
  const double sd = wide_screen_diff(screen_type, v, resid[e]);
  if (fabs(sd) > nsigma * sig && w_out[e] != 0.0f) w_out[e] = 0.0f;
}

// One outlier iteration `it` of every slot: one workgroup per slot, walking
// the slots with the grid's stride.  nl of the matrices V, M1, M2 sit in the
// dynamic LDS, the others in this workgroup's slice of `ws`.
__global__ __launch_bounds__(kWideThreads) void kl_fit_wide_kernel(
    int it, int niter, int64_t nslots, int F, int A, int D, int nl,
    const double* __restrict__ phase, const double* __restrict__ refph,
    int ref_sub, int ref_skip, const double* __restrict__ g_c,
    const double* __restrict__ g_u, const double* __restrict__ g_eig,
    const int* __restrict__ st_order, const uint8_t* __restrict__ skip,
    int screen_type, double nsigma, int adjust_order, double* ws,
    int* __restrict__ counters, double* __restrict__ coef,
    double* __restrict__ resid, float* __restrict__ w_out,
    int32_t* __restrict__ order_out) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char wide_smem[];
  WideSmall& S = *reinterpret_cast<WideSmall*>(wide_smem);
  const int ld = wide_ld(D);
  const size_t mat = (size_t)D * ld;
  double* lmat = reinterpret_cast<double*>(wide_smem + sizeof(WideSmall));
  double* gmat = ws + (size_t)blockIdx.x * (size_t)(3 - nl) * mat;
  double* mats[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    mats[k] = k < nl ? lmat + k * mat : gmat + (size_t)(k - nl) * mat;
  WideFit L;
  L.S = &S;
  L.gC = g_c;
  L.gU = g_u;
  L.gEig = g_eig;
  L.V = mats[0];
  L.M1 = mats[1];
  L.M2 = mats[2];
  L.D = D;
  L.ld = ld;
  const int d = wide_row();
  const bool live = d < D;

  for (int64_t s = blockIdx.x; s < nslots; s += gridDim.x) {
    const int a = (int)(s % A);
    const int f = (int)((s / A) % F);
    if (a == ref_skip || skip[f * A + a]) continue;  // workgroup-uniform
    const int64_t base = s * D;
    double phi_d = 0.0, w_d = 0.0, white_d = 0.0, resid_d = 0.0;
    if (live) {
      phi_d = wide_phase_ref(phase, refph, ref_sub, s, a, A, D, d);
      w_d = (double)w_out[base + d];
      // pass 0 starts from zero (kl_wide_init_kernel leaves them unwritten)
      white_d = it == 0 ? 0.0 : coef[base + d];
      resid_d = it == 0 ? 0.0 : resid[base + d];
    }
    double order = (double)order_out[s];
    const double station_order = (double)st_order[a];
    // every thread has read the slot's state before any thread writes it
    __syncthreads();
    const bool unfl = live && w_d > 0.0;
    const WideMask um = wide_ballot(unfl, S.bal);
    const int n_unfl = um.n;
    L.n = n_unfl;
    L.full = n_unfl == D;
    L.wmin = -wide_max(unfl ? -w_d : -INFINITY, S.red);
    bool decomposed = false;  // workgroup-uniform

    if (n_unfl > 0) {
      if (order > n_unfl - 1) order = n_unfl - 1;
      if (it == 0) {
        wide_setup_subset(L, um, unfl, counters);
        decomposed = true;
        wide_fit_screen(L, (int)order, screen_type, um, phi_d, w_d, white_d,
                        resid_d);
      } else if (adjust_order) {
        bool hit_upper = false, hit_lower = false, hit_upper2 = false,
             hit_lower2 = false;
        double sign = 1.0, prev_redchi2 = 0.0;
        for (int oi = 0; oi < 4; ++oi) {
          // oi == 0: the weights always compare equal (quirk Q2) -> no fit
          if (oi > 0) {
            if (!decomposed) {
              wide_setup_subset(L, um, unfl, counters);
              decomposed = true;
            }
            wide_fit_screen(L, (int)order, screen_type, um, phi_d, w_d,
                            white_d, resid_d);
          }
          if (hit_lower2 || hit_upper2) break;
          double redchi2;
          if (screen_type == SF_SCREEN_PHASE) {
            // _circ_chi2: squares of sin / cos (quirk Q7)
            double sn = 0.0, cn = 0.0;
            if (unfl) sincos(resid_d, &sn, &cn);
            const double ww = unfl ? w_d : 0.0;
            double r3[3] = {ww, sn * sn * ww, cn * cn * ww};
            wide_sum(r3, S.red);
            const double m1 = r3[1] / r3[0];
            const double m2 = r3[2] / r3[0];
            redchi2 = (1.0 - hypot(m1, m2)) * r3[0] / (n_unfl - order);
          } else {
            // np.sum(square(diff) * w) over all directions
            double r1[1] = {0.0};
            if (live) {
              const double sd = wide_screen_diff(screen_type, phi_d, resid_d);
              r1[0] = (sd * sd) * w_d;
            }
            wide_sum(r1, S.red);
            redchi2 = r1[0] / (n_unfl - order);
          }
          if (oi > 0) {
            if (redchi2 > 1.0 && prev_redchi2 < redchi2) sign = -sign;
            if (redchi2 < 1.0 && prev_redchi2 > redchi2) sign = -sign;
          }
          prev_redchi2 = redchi2;
          const double order_factor = pow((double)n_unfl - order, 0.2);
          double target = order - sign * order_factor * (1.0 - redchi2);
          target = fmax(station_order, target);
          target = fmin(rint(target), (double)(n_unfl - 1));
          if (target <= 0.0) target = fmin(station_order, (double)(n_unfl - 1));
          if (target == order) break;
          if (target == n_unfl - 1) {
            if (hit_upper) hit_upper2 = true;
            hit_upper = true;
          }
          if (target == station_order) {
            if (hit_lower) hit_lower2 = true;
            hit_lower = true;
          }
          order = target;
        }
      }
    }
    // phase: outlier flags for the next pass, per slot (circular sigma
    // across directions, stationscreen.py:303-350); tec / amplitude: one
    // sigma per station block -> kl_block_sigma / kl_wide_block_flag kernels
    if (it + 1 < niter && screen_type == SF_SCREEN_PHASE && n_unfl > 0) {
      double r = fmod(resid_d, 2.0 * M_PI);
      if (r < -M_PI) r += 2.0 * M_PI;
      if (r > M_PI) r -= 2.0 * M_PI;
      const bool inc = live && (w_d != 0.0) && !isnan(r);
      double sn = 0.0, cn = 0.0;
      if (inc) sincos(r, &sn, &cn);
      double r3[3] = {inc ? 1.0 : 0.0, sn, cn};
      wide_sum(r3, S.red);
      const double ms = r3[1] / r3[0];
      const double mc = r3[2] / r3[0];
      const double stdv = sqrt(-2.0 * log(hypot(ms, mc)));
      if (live && (fabs(r) > nsigma * stdv)) w_d = 0.0;
    }
    if (live && threadIdx.x < kWideRows) {
      coef[base + d] = white_d;
      resid[base + d] = resid_d;
      w_out[base + d] = (float)w_d;
    }
    if (threadIdx.x == 0) order_out[s] = (int32_t)order;
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
namespace {
constexpr size_t kWideLds = 160 * 1024;  // LDS of one gfx950 CU

// matrices of the fit workgroup that fit the LDS beside WideSmall
int wide_lds_mats(int D) {
  const size_t mat = (size_t)D * wide_ld(D) * sizeof(double);
  const size_t n = (kWideLds - sizeof(WideSmall)) / mat;
  return n > 3 ? 3 : (int)n;
}
}  // namespace

size_t wide_basis_ws_doubles(int D) { return (size_t)2 * D * wide_ld(D); }

int launch_basis_wide(sf_ctx* ctx) {
  const int D = ctx->D;
  SF_TRY_RC(grow(&ctx->d_wide_ws, ctx->wide_ws_cap, wide_basis_ws_doubles(D)));
  hipLaunchKernelGGL(kl_basis_wide_kernel, dim3(1), dim3(kWideThreads), 0,
                     ctx->stream, ctx->d_pp, D, ctx->r0, ctx->beta, ctx->d_c,
                     ctx->d_pinv, ctx->d_u, ctx->d_eig, ctx->d_wide_ws);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

int launch_fit_wide(sf_ctx* ctx, const double* phase, const float* weight,
                    int T, int F, int A, const sf_fit_params* p, double* coef,
                    double* resid, float* w_out, int32_t* order_out) {
  const int D = ctx->D;
  const int64_t S = (int64_t)T * F * A;
  const RefSpec r = ref_spec(p, A);
  hipLaunchKernelGGL(kl_wide_skip_kernel, dim3(F * A), dim3(kWideRows), 0,
                     ctx->stream, phase, weight, T, F, A, D, r.sub, r.refph,
                     ctx->d_skip);
  SF_HIP(hipGetLastError());
  // scratch for outputs the caller does not want (they carry pass state)
  if (!resid) {
    SF_TRY_RC(grow(&ctx->d_scratch, ctx->scratch_cap, (size_t)S * D));
    resid = ctx->d_scratch;
  }
  if (!w_out) {
    SF_TRY_RC(grow(&ctx->d_wide_w, ctx->wide_w_cap, (size_t)S * D));
    w_out = ctx->d_wide_w;
  }
  if (!order_out) {
    SF_TRY_RC(grow(&ctx->d_wide_o, ctx->wide_o_cap, (size_t)S));
    order_out = ctx->d_wide_o;
  }
  if (ctx->sigma_cap < (size_t)F * A || !ctx->d_sigma) {
    size_t c = 0;
    if (ctx->d_sigma) (void)hipFree(ctx->d_sigma);
    ctx->d_sigma = nullptr;
    ctx->sigma_cap = 0;
    SF_TRY_RC(grow(&ctx->d_sigma, c, (size_t)F * A));
    ctx->sigma_cap = (size_t)F * A;
  }
  if (!ctx->d_counters) {
    size_t c = 0;
    SF_TRY_RC(grow(&ctx->d_counters, c, 8));
  }
  SF_HIP(hipMemsetAsync(ctx->d_counters, 0, 8 * sizeof(int), ctx->stream));

  // persistent grid: one workgroup per CU (the kernel's registers and, from
  // D = 61, its LDS leave room for no second one), never more than slots;
  // the workspace is sized by it
  const int nl = wide_lds_mats(D);
  const size_t mat = (size_t)D * wide_ld(D);
  const size_t shm = sizeof(WideSmall) + (size_t)nl * mat * sizeof(double);
  int n_cu = 0;
  SF_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount,
                               ctx->device));
  int64_t grid = n_cu > 0 ? n_cu : 1;
  if (grid > S) grid = S;
  const size_t ws = (size_t)grid * (size_t)(3 - nl) * mat;
  if (ws > 0) SF_TRY_RC(grow(&ctx->d_wide_ws, ctx->wide_ws_cap, ws));
  if (shm > 64 * 1024)
    SF_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&kl_fit_wide_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));

  {
    const int64_t n = S * D;
    hipLaunchKernelGGL(kl_wide_init_kernel, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, ctx->stream, weight, S, F, A, D,
                       ctx->d_st_order, ctx->d_skip, r.skip, coef, resid, w_out,
                       order_out);
    SF_HIP(hipGetLastError());
  }
  const bool block_flags = p->screen_type != SF_SCREEN_PHASE;
  for (int it = 0; it < p->niter; ++it) {
    hipLaunchKernelGGL(kl_fit_wide_kernel, dim3((unsigned)grid),
                       dim3(kWideThreads), shm, ctx->stream, it, p->niter, S, F,
                       A, D, nl, phase, r.refph, r.sub, r.skip, ctx->d_c,
                       ctx->d_u, ctx->d_eig, ctx->d_st_order, ctx->d_skip,
                       p->screen_type, p->nsigma, p->adjust_order,
                       ctx->d_wide_ws, ctx->d_counters, coef, resid, w_out,
                       order_out);
    SF_HIP(hipGetLastError());
    if (block_flags && it + 1 < p->niter) {
      SF_TRY_RC(launch_block_sigma(ctx, T, F, A, phase, r, p->screen_type,
                                   resid, w_out));
      const int64_t n = S * D;
      hipLaunchKernelGGL(kl_wide_block_flag_kernel,
                         dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                         ctx->stream, S, F, A, D, phase, r.refph, r.sub,
                         ctx->d_skip, r.skip, p->screen_type, p->nsigma,
                         ctx->d_sigma, resid, w_out);
      SF_HIP(hipGetLastError());
    }
  }
  // as the <= 60 path: the call returns with the fit complete (the scratch
  // outputs and the statistics belong to this call)
  SF_HIP(hipStreamSynchronize(ctx->stream));
  return SF_OK;
}

}  // namespace sf
