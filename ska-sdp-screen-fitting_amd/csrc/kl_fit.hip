// kl_fit.hip -- shared KL basis and the batched per-slot KL least-squares fit
// (gfx950, float64).
//
// Restates on the GPU (not a translation -- one wavefront per slot, one lane
// per direction, LDS-resident basis) the reference operator
// stationscreen.run (stationscreen.py:858-1161):
//   * kl_basis_kernel   <- _calculate_svd (stationscreen.py:390-430)
//   * kl_skip_kernel    <- the (station, freq) block skip of
//                          _process_single_freq (stationscreen.py:817-825)
//   * kl_fit_general_kernel <- _process_station (stationscreen.py:597-782)
//                          for one slot per wavefront, every outlier iteration
//                          in one launch: the slot loop here, its steps
//                          (_flag_outliers, _circ_chi2, the order walk) in
//                          kl_fit_steps.h, _fit_screen (:433-594) with the
//                          exact pinv in kl_fit_exact.h.
// Every phase slot is independent (see oracle/kl.py for the argument), so a
// slot is the unit of parallelism.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kl_cov.h"
#include "kl_fit_exact.h"
#include "sf_internal.h"

namespace sf {

// ---------------------------------------------------------------------------
// basis: one wavefront. C, eigen-decomposition by Jacobi, U sorted by
// descending |lambda| (= svd(C)[0] up to column signs), pinv with absolute
// cutoff.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void kl_basis_kernel(
    const double* __restrict__ pp, int D, double r0, double beta,
    double* __restrict__ c_out, double* __restrict__ pinv_out,
    double* __restrict__ u_out, double* __restrict__ eig_out) {
  extern __shared__ double smem[];
  const int ld = odd_ld(D);
  double* a = smem;
  double* v = a + D * ld;
  double2* cs = reinterpret_cast<double2*>(v + D * ld);
  int2* pr = reinterpret_cast<int2*>(cs + 64);      // 64 int2 + 64 int
  int* perm = reinterpret_cast<int*>(pr + 96);
  const int i = lane();
  const double r0sq = r0 * r0, hb = beta / 2.0;
  if (i < D) {
    for (int j = 0; j < D; ++j) {
      const double c = kl_cov(pp + 3 * i, pp + 3 * j, r0sq, hb);
      a[i * ld + j] = c;
      c_out[i * D + j] = c;
    }
  }
  lds_sync();
  wave_jacobi(a, v, cs, pr, D, ld, kJacobiMaxSweeps);
  eig_order(Group<1>{}, a, D, ld, perm);
  if (i < D) {
    for (int r = 0; r < D; ++r) u_out[i * D + r] = v[i * ld + perm[r]];
    const int pr = perm[i];
    eig_out[i] = a[pr * ld + pr];
    for (int j = 0; j < D; ++j) {
      double s = 0.0;
      for (int r = 0; r < D; ++r) {
        const int m = perm[r];
        const double lam = a[m * ld + m];
        if (fabs(lam) > kPinvAtol) s += v[i * ld + m] * (v[j * ld + m] / lam);
      }
      pinv_out[i * D + j] = s;
    }
  }
}

// ---------------------------------------------------------------------------
// (station, freq) block skip: all phases NaN after referencing, or all
// weights zero (stationscreen.py:821-825).  One wavefront per block.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void kl_skip_kernel(
    const double* __restrict__ phase, const float* __restrict__ weight, int T,
    int F, int A, int D, int ref, const double* __restrict__ refph,
    uint8_t* __restrict__ skip) {
  const int blk = blockIdx.x;  // f * A + a
  const int f = blk / A, a = blk % A;
  const int d = lane();
  bool any_val = false, any_w = false;
  for (int t = 0; t < T; ++t) {
    if (d < D) {
      // phase_ref (kl_fit_steps.h) with the block's (t, f) in hand: no
      // division by A per element
      const int64_t base = ((int64_t)(t * F + f) * A) * D;
      double ph = phase[base + (int64_t)a * D + d];
      if (refph) ph -= refph[(int64_t)(t * F + f) * D + d];
      else if (ref >= 0) ph -= phase[base + (int64_t)ref * D + d];
      any_val |= !isnan(ph);
      any_w |= weight[base + (int64_t)a * D + d] != 0.0f;
    }
    // a block is kept as soon as it has one finite phase and one non-zero
    // weight: stop there (every 8 times, a wave-uniform test)
    if ((t & 7) == 7 && __any(any_val) && __any(any_w)) break;
  }
  const bool av = __any(any_val), aw = __any(any_w);
  if (d == 0) skip[blk] = (!av || !aw) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// per-slot fit
// ---------------------------------------------------------------------------
// Where the matrices of one wavefront's exact fit live (the X of
// kl_fit_exact.h): everything in LDS, rows of stride ld.
struct FitLds {
  static constexpr bool kFused = true;
  // shared by the workgroup
  double* C;     // [D][ld]
  double* U;     // [D][ld], columns sorted
  double* eig;   // [64]
  // per wave
  double* V;     // [D][ld] eigenvectors of C_sub (unsorted columns)
  double* M1;    // [D][ld] scratch
  double* M2;    // [D][ld] normal matrix / scratch
  double* lam;   // [64] eigenvalues of C_sub by rank
  double* vecs;  // [6][64] broadcast vectors
  int* idx;      // [64] subset -> direction
  int* perm;     // [64] rank -> column of V
  double2* cs;   // [64] Jacobi rotations
  int2* pr;      // [64] + 64 int: Jacobi round pairs / partners
  int ld;
  __device__ double csym(int r, int q) const { return C[r * ld + q]; }
  __device__ double u(int p, int k) const { return U[p * ld + k]; }
  __device__ double eigv(int p) const { return eig[p]; }
  __device__ double* vec(int k) const { return vecs + 64 * k; }
  __device__ void jacobi(double* a, double* v, int n, int ld_) const {
    wave_jacobi(a, v, cs, pr, n, ld_, kJacobiMaxSweeps);
  }
  __device__ void cholesky(double* g, int k, int ld_, double& b1, double& b2) const {
    wave_cholesky_solve2(g, k, ld_, b1, b2);
  }
  __device__ void decomposed() const {}
};

__host__ __device__ inline size_t fit_shared_bytes(int D) {
  return (size_t)(2 * D * odd_ld(D) + 64) * sizeof(double);
}
__host__ __device__ inline size_t fit_wave_bytes(int D) {
  return (size_t)(3 * D * odd_ld(D) + 64 + 6 * 64) * sizeof(double) +
         (size_t)(64 + 64) * sizeof(int) + 64 * sizeof(double2) +
         96 * sizeof(int2);
}

__global__ __launch_bounds__(256) void kl_fit_general_kernel(
    const double* __restrict__ phase, const float* __restrict__ weight,
    int T, int F, int A, int D, const int* __restrict__ st_order,
    const uint8_t* __restrict__ skip, const double* __restrict__ refph,
    const double* __restrict__ g_c,
    const double* __restrict__ g_u, const double* __restrict__ g_eig,
    int screen_type, int niter, double nsigma, int adjust_order, int ref,
    int ref_skip, double* __restrict__ coef, double* __restrict__ resid_out,
    float* __restrict__ w_out, int32_t* __restrict__ order_out) {
#pragma clang fp contract(off)
  extern __shared__ double smem[];
  const int ld = odd_ld(D);
  const int nwaves = blockDim.x / 64;
  const int wv = threadIdx.x / 64;
  const int d = lane();
  using M = FitMath<false>;  // the transcendentals inlined
  const Group<1> tm;
  FitLds L;
  L.C = smem;
  L.U = L.C + D * ld;
  L.eig = L.U + D * ld;
  char* wbase = reinterpret_cast<char*>(L.eig + 64) + (size_t)wv * fit_wave_bytes(D);
  L.V = reinterpret_cast<double*>(wbase);
  L.M1 = L.V + D * ld;
  L.M2 = L.M1 + D * ld;
  L.lam = L.M2 + D * ld;
  L.vecs = L.lam + 64;
  L.idx = reinterpret_cast<int*>(L.vecs + 6 * 64);
  L.perm = L.idx + 64;
  L.cs = reinterpret_cast<double2*>(L.perm + 64);
  L.pr = reinterpret_cast<int2*>(L.cs + 64);
  L.ld = ld;
  // shared basis -> LDS
  for (int e = threadIdx.x; e < D * D; e += blockDim.x) {
    const int r = e / D, c = e % D;
    L.C[r * ld + c] = g_c[e];
    L.U[r * ld + c] = g_u[e];
  }
  for (int e = threadIdx.x; e < D; e += blockDim.x) L.eig[e] = g_eig[e];
  __syncthreads();

  const int64_t S = (int64_t)T * F * A;
  for (int64_t s = (int64_t)blockIdx.x * nwaves + wv; s < S;
       s += (int64_t)gridDim.x * nwaves) {
    const SlotGeom g(s, F, A);
    const int a = g.a;
    const int64_t base = s * D;
    double phi_d = 0.0;
    float w_f = 0.0f;
    if (d < D) {
      phi_d = phase_ref(phase, refph, ref, s, a, A, D, d);
      w_f = weight[base + d];
    }
    if (g.skipped(skip, ref_skip)) {
      if (d < D) {
        coef[base + d] = 0.0;
        if (resid_out) resid_out[base + d] = 0.0;
        if (w_out) w_out[base + d] = w_f;
      }
      if (d == 0 && order_out) order_out[s] = 0;
      continue;
    }
    double w_d = (double)w_f;
    double order = (double)st_order[a];
    const double station_order = order;
    double white_d = 0.0, resid_d = 0.0;
    const bool live = d < D;
    Subset st{-1, false, 0.0};
    bool mask_valid = false;
    for (int it = 0; it < niter; ++it) {
      if (it > 0 && screen_type == SF_SCREEN_PHASE && tm.any(live && w_d > 0.0)) {
        if (tm.any(flag_circular_outliers<M>(tm, live, nsigma, resid_d, w_d)))
          mask_valid = false;
      }
      const int norderiter = (adjust_order && it > 0) ? 4 : 1;
      const bool unfl = live && w_d > 0.0;
      const uint64_t um = tm.ballot(unfl);
      const int n_unfl = __popcll(um);
      if (n_unfl == 0) continue;
      if (order > n_unfl - 1) order = n_unfl - 1;
      OrderWalk walk;
      for (int oi = 0; oi < norderiter; ++oi) {
        bool skip_fit = false;
        if (it > 0) {
          // quirk Q2: the weights always compare equal to "previous"
          if (!adjust_order) break;
          if (oi == 0) skip_fit = true;
        }
        if (!skip_fit) {
          if (!mask_valid) {
            st.n = n_unfl;
            st.full = n_unfl == D;
            st.wmin = -tm.max(unfl ? -w_d : -INFINITY);
            setup_subset(tm, L, D, st, um, unfl);
            mask_valid = true;
          }
          fit_screen(tm, L, st, D, (int)order, screen_type, um, phi_d, w_d,
                     white_d, resid_d);
        }
        if (walk.done()) break;
        if (adjust_order && it > 0) {
          // phase only: launch_fit rejects tec with niter > 1 on this path
          const double redchi2 = slot_redchi2<M>(tm, screen_type, live, unfl, phi_d,
                                                 w_d, resid_d, n_unfl, order);
          if (walk.step<M>(oi, redchi2, n_unfl, station_order, order)) break;
        }
      }
    }
    if (d < D) {
      coef[base + d] = white_d;
      if (resid_out) resid_out[base + d] = resid_d;
      if (w_out) w_out[base + d] = (float)w_d;
    }
    if (d == 0 && order_out) order_out[s] = (int32_t)order;
  }
}

int launch_basis(sf_ctx* ctx) {
  const int D = ctx->D;
  const int ld = odd_ld(D);
  const size_t shm = (size_t)2 * D * ld * sizeof(double) + 64 * sizeof(double2) +
                     96 * sizeof(int2) + 64 * sizeof(int);
  hipLaunchKernelGGL(kl_basis_kernel, dim3(1), dim3(64), shm, ctx->stream,
                     ctx->d_pp, D, ctx->r0, ctx->beta, ctx->d_c, ctx->d_pinv,
                     ctx->d_u, ctx->d_eig);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

// Referencing / ref-station skip parameters of one sf_kl_fit call
// (stationscreen.py:994-997, :818), including the operator-precedence quirk
// Q15 (tec is always referenced: with ref_ant == -1 to the last station of
// the whole soltab, whose values a station shard passes as ref_phase; NULL =
// the call's own last station).
RefSpec ref_spec(const sf_fit_params* p, int A) {
  RefSpec r;
  const int ref = (p->ref_ant == -1) ? -1 : p->ref_ant - p->ant_offset;
  if (p->screen_type == SF_SCREEN_AMPLITUDE) return r;  // never referenced
  if (p->screen_type == SF_SCREEN_PHASE) {
    if (p->ref_ant != -1) {
      if (p->ref_phase) r.refph = p->ref_phase; else r.sub = ref;
    }
  } else {
    if (p->ref_phase) r.refph = p->ref_phase;
    else if (p->ref_ant == -1) r.sub = A - 1;
    else r.sub = ref;
  }
  if (ref >= 0 && ref < A) r.skip = ref;
  return r;
}

int launch_skip(sf_ctx* ctx, const double* phase, const float* weight, int T,
                int F, int A, const RefSpec& r) {
  hipLaunchKernelGGL(kl_skip_kernel, dim3(F * A), dim3(64), 0, ctx->stream,
                     phase, weight, T, F, A, ctx->D, r.sub, r.refph, ctx->d_skip);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

int launch_fit_general(sf_ctx* ctx, const double* phase, const float* weight,
                       int T, int F, int A, const sf_fit_params* p,
                       const RefSpec& r, double* coef, double* resid,
                       float* w_out, int32_t* order_out) {
  const int D = ctx->D;
  const size_t shared = fit_shared_bytes(D);
  const size_t wave = fit_wave_bytes(D);
  int nw = 4;
  while (nw > 1 && shared + nw * wave > 80 * 1024) --nw;
  const size_t shm = shared + nw * wave;
  int64_t blocks = ((int64_t)T * F * A + nw - 1) / nw;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  SF_TRY(allow_lds(kl_fit_general_kernel, shm));
  hipLaunchKernelGGL(kl_fit_general_kernel, dim3((unsigned)blocks),
                     dim3(64 * nw), shm, ctx->stream, phase, weight, T, F, A, D,
                     ctx->d_st_order, ctx->d_skip, r.refph, ctx->d_c, ctx->d_u, ctx->d_eig, p->screen_type, p->niter,
                     p->nsigma, p->adjust_order, r.sub, r.skip, coef, resid,
                     w_out, order_out);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

}  // namespace sf
