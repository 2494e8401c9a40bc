// kl_fit_wide.hip -- the KL basis and the per-slot KL fit with 61..128
// directions (gfx950, float64): sf_set_basis_wide and sf_kl_fit on a
// wide-basis context.
//
// The slot steps of kl_fit_steps.h and the exact-pinv _fit_screen of
// kl_fit_exact.h (_process_station / _fit_screen / _flag_outliers /
// _circ_chi2, stationscreen.py:597-782, 433-594, 303-350, 353-387) on one
// WORKGROUP of 256 threads per slot (WideTeam, kl_fit_wide.h): thread t
// handles direction t & 127, the two 128-thread shares split the column pairs
// of the Jacobi rounds and the columns of the normal matrix.
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
#include "kl_fit_exact.h"
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
  const int ld = odd_ld(D);
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
  wide_jacobi(a, v, S, D, ld, kJacobiMaxSweeps);
  eig_order(WideTeam{S.red, S.bal}, a, D, ld, S.perm);
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
        if (fabs(lam) > kPinvAtol) s += v[i * ld + m] * (v[j * ld + m] / lam);
      }
      pinv_out[i * D + j] = s;
    }
  }
}

// ---------------------------------------------------------------------------
// per-slot fit
// ---------------------------------------------------------------------------
// Where the matrices of one workgroup's exact fit live (the X of
// kl_fit_exact.h): the shared C / U / eig in global memory (L2), V / M1 / M2
// in LDS or the workspace, the vectors and the subset state in WideSmall.
struct WideFit {
  static constexpr bool kFused = false;
  WideSmall* S;
  const double* gC;    // [D][D] global
  const double* gU;    // [D][D] global, columns sorted
  const double* gEig;  // [D]
  double* V;           // [D][ld] eigenvectors of C_sub (unsorted columns)
  double* M1;          // [D][ld] scratch
  double* M2;          // [D][ld] normal matrix / scratch
  double* lam;         // S->lam, idx, perm: the subset state
  int* idx;
  int* perm;
  int* counters;       // [0]: subset decompositions run
  int D, ld;
  // C is symmetric: thread r reads along the row of q (coalesced)
  __device__ double csym(int r, int q) const { return gC[(size_t)q * D + r]; }
  __device__ double u(int p, int k) const { return gU[(size_t)p * D + k]; }
  __device__ double eigv(int p) const { return gEig[p]; }
  __device__ double* vec(int k) const { return S->vec[k]; }
  __device__ void jacobi(double* a, double* v, int n, int ld_) const {
    wide_jacobi(a, v, *S, n, ld_, kJacobiMaxSweeps);
  }
  __device__ void cholesky(double* g, int k, int ld_, double& b1, double& b2) const {
    wide_cholesky_solve2(g, k, ld_, b1, b2, S->red);
  }
  __device__ void decomposed() const {
    if (threadIdx.x == 0) atomicAdd(counters, 1);
  }
};

// (station, freq) block skip for D <= 128 (kl_skip_kernel has one 64-lane
// wave per block): all phases NaN after referencing, or all
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
      const double ph = phase_ref(phase, refph, ref, s, a, A, D, d);
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
  const double v = phase_ref(phase, refph, ref_sub, s, a, A, D, d);
  const double sd = screen_diff(screen_type, v, resid[e]);
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
  const int ld = odd_ld(D);
  const size_t mat = (size_t)D * ld;
  double* lmat = reinterpret_cast<double*>(wide_smem + sizeof(WideSmall));
  double* gmat = ws + (size_t)blockIdx.x * (size_t)(3 - nl) * mat;
  double* mats[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    mats[k] = k < nl ? lmat + k * mat : gmat + (size_t)(k - nl) * mat;
  using M = FitMath<false>;  // the transcendentals inlined
  const WideTeam tm{S.red, S.bal};
  WideFit L;
  L.S = &S;
  L.gC = g_c;
  L.gU = g_u;
  L.gEig = g_eig;
  L.V = mats[0];
  L.M1 = mats[1];
  L.M2 = mats[2];
  L.lam = S.lam;
  L.idx = S.idx;
  L.perm = S.perm;
  L.counters = counters;
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
      phi_d = phase_ref(phase, refph, ref_sub, s, a, A, D, d);
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
    const WideMask um = tm.ballot(unfl);
    const int n_unfl = um.n;
    const Subset st{n_unfl, n_unfl == D, -tm.max(unfl ? -w_d : -INFINITY)};
    bool decomposed = false;  // workgroup-uniform

    if (n_unfl > 0) {
      if (order > n_unfl - 1) order = n_unfl - 1;
      if (it == 0) {
        setup_subset(tm, L, D, st, um, unfl);
        decomposed = true;
        fit_screen(tm, L, st, D, (int)order, screen_type, um, phi_d, w_d, white_d,
                   resid_d);
      } else if (adjust_order) {
        OrderWalk walk;
        for (int oi = 0; oi < 4; ++oi) {
          // oi == 0: the weights always compare equal (quirk Q2) -> no fit
          if (oi > 0) {
            if (!decomposed) {
              setup_subset(tm, L, D, st, um, unfl);
              decomposed = true;
            }
            fit_screen(tm, L, st, D, (int)order, screen_type, um, phi_d, w_d,
                       white_d, resid_d);
          }
          if (walk.done()) break;
          const double redchi2 = slot_redchi2<M>(tm, screen_type, live, unfl, phi_d,
                                                 w_d, resid_d, n_unfl, order);
          if (walk.step<M>(oi, redchi2, n_unfl, station_order, order)) break;
        }
      }
    }
    // phase: outlier flags for the next pass, per slot (circular sigma
    // across directions, stationscreen.py:303-350); tec / amplitude: one
    // sigma per station block -> kl_block_sigma / kl_wide_block_flag kernels
    if (it + 1 < niter && screen_type == SF_SCREEN_PHASE && n_unfl > 0)
      flag_circular_outliers<M>(tm, live, nsigma, resid_d, w_d);
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
  const size_t mat = (size_t)D * odd_ld(D) * sizeof(double);
  const size_t n = (kWideLds - sizeof(WideSmall)) / mat;
  return n > 3 ? 3 : (int)n;
}
}  // namespace

size_t wide_basis_ws_doubles(int D) { return (size_t)2 * D * odd_ld(D); }

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
  SF_TRY_RC(fit_buffers(ctx, S, F, A, &resid, &w_out, &order_out));
  SF_HIP(hipMemsetAsync(ctx->d_counters, 0, 8 * sizeof(int), ctx->stream));

  // persistent grid: one workgroup per CU (the kernel's registers and, from
  // D = 61, its LDS leave room for no second one), never more than slots;
  // the workspace is sized by it
  const int nl = wide_lds_mats(D);
  const size_t mat = (size_t)D * odd_ld(D);
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
