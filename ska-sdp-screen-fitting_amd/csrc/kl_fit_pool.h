// kl_fit_pool.h -- the mask-keyed pool of subset bases of the <= 60 direction
// fit (kl_fit_fast.hip, which alone includes this): the open-addressing
// table of 64-bit unflagged-direction masks, the numbering of a pass's new
// masks, their decomposition -- by deletions from the global basis or an
// ancestor (kl_subset_secular_kernel), else by Jacobi (kl_subset_eig_kernel)
// -- and the host step between two passes, number_and_decompose.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "kl_fit_masks.h"
#include "kl_fit_steps.h"
#include "sf_internal.h"

namespace sf {

// The slot of `key` in the table, or -1 (read-only: the table does not
// change while the subset bases are decomposed).
__device__ int table_find(const unsigned long long* keys, int cap,
                          unsigned long long key) {
  int h = (int)(mix64(key) & (unsigned long long)(cap - 1));
  for (int probe = 0; probe < cap; ++probe) {
    const unsigned long long k = keys[h];
    if (k == key) return h;
    if (k == kEmptyKey) return -1;
    h = (h + 1) & (cap - 1);
  }
  return -1;
}

// number the newly inserted masks (one thread per table entry)
__global__ __launch_bounds__(256) void kl_assign_kernel(
    const unsigned long long* __restrict__ keys, int cap, int* __restrict__ ids,
    unsigned long long* __restrict__ pool_mask, int pool_cap,
    int* __restrict__ counters, int D) {
  int lvl = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; wave_in_table(i, cap);
       i += gridDim.x * blockDim.x) {
    const unsigned long long k = i < cap ? keys[i] : kEmptyKey;
    const int id = number_fresh(k != kEmptyKey && ids[i] < 0, counters + kCntIds);
    if (id < 0) continue;
    ids[i] = id;
    if (id < pool_cap) pool_mask[id] = k;
    lvl = max(lvl, D - __popcll(k));
  }
  // the most flagged directions among the new masks (the deletion levels):
  // one atomic per wavefront
  for (int o = 32; o > 0; o >>= 1) lvl = max(lvl, __shfl_xor(lvl, o));
  if (lane() == 0 && lvl > 0) atomicMax(counters + kCntMaxLevel, lvl);
}

// subset bases of this pass's masks, numbered [kCntPassStart, kCntIds):
//    C_sub = C[idx][:, idx] -> Jacobi -> U_sub sorted by |lambda| desc.
//    A pool mask leaves at least one direction out (the full mask is the
//    global basis, kl_classify_kernel), so the LDS matrices are sized for
//    D - 1 rows: at D = 50 a wave's 40,720 bytes let 4 waves share a CU's
//    160 KiB (43,104 bytes, sized for D, let 3).
__host__ __device__ inline int subset_ld(int D) { return odd_ld(D > 1 ? D - 1 : 1); }
__host__ __device__ inline int subset_rows(int D) { return D > 1 ? D - 1 : 1; }
// NW: waves per mask of the subset Jacobi (wg_jacobi); the library runs 3
// (kEigWavesDefault), SF_OPT_FIT_EIG_WAVES picks 1..4 -- the same bits at
// every count (tests/test_gpu_parity.py::test_subset_jacobi_wave_count_*)
constexpr int kEigWavesDefault = 3;
template <int NW>
__global__ __launch_bounds__(64 * NW) void kl_subset_eig_kernel(
    const double* __restrict__ g_c, int D,
    const unsigned long long* __restrict__ pool_mask, int pool_cap,
    int* __restrict__ counters, double* __restrict__ pool,
    const uint8_t* __restrict__ done) {
  extern __shared__ double smem[];
  const int ld = subset_ld(D);
  double* a = smem;
  double* v = a + subset_rows(D) * ld;
  double2* cs = reinterpret_cast<double2*>(v + subset_rows(D) * ld);
  int2* pr = reinterpret_cast<int2*>(cs + 64);  // 64 int2 + 64 int
  int* perm = reinterpret_cast<int*>(pr + 96);
  int* idx = perm + 64;
  const int first = counters[kCntPassStart];
  const int last = min(counters[kCntIds], pool_cap);
  const int l = lane();
  const bool w0 = threadIdx.x < 64;  // NW waves per mask
  for (int id = first + blockIdx.x; id < last; id += gridDim.x) {
    // masks the deletion kernel already decomposed (status 0)
    if (done && done[id] == 0) continue;
    const unsigned long long m = pool_mask[id];
    const bool in = (l < D) && ((m >> l) & 1ull);
    const int n = __popcll(m);
    if (n >= D) {  // cannot happen (full masks never enter the pool): flag it
      if (threadIdx.x == 0) atomicOr(counters + kCntError, kErrFullMaskInPool);
      continue;
    }
    if (w0 && in) idx[Group<1>::rank(m)] = l;
    __syncthreads();
    if (w0 && l < n) {
      const int r = idx[l];
      for (int q = 0; q < n; ++q) a[l * ld + q] = g_c[r * D + idx[q]];
    }
    __syncthreads();
    wg_jacobi<NW>(a, v, cs, pr, n, ld, kJacobiMaxSweeps);
    __syncthreads();
    if (w0) eig_order(Group<1>{}, a, n, ld, perm);
    double* e = pool + (size_t)id * (D * D + D);
    if (w0 && l < n) {
      for (int r = 0; r < n; ++r) e[l * D + r] = v[l * ld + perm[r]];
      const int pr = perm[l];
      e[D * D + l] = a[pr * ld + pr];
    }
    __syncthreads();
  }
}

// (U, lam) <- the m eigenpairs of a source -- eigenvectors in the columns of
// src (row stride `stride`), eigenvalues eig -- in ascending eigenvalue order;
// perm: LDS scratch.  One wavefront.
__device__ __forceinline__ void load_ascending(const double* src, const double* eig,
                                               int stride, int m, double* U, int ld,
                                               double* lam, int* perm) {
#pragma clang fp contract(off)
  const int l = lane();
  if (l < m) perm[order_rank<AscendingValue>(m, l, [&](int k) { return eig[k]; })] = l;
  lds_sync();
  if (l < m) lam[l] = eig[perm[l]];
  for (int e = l; e < m * m; e += 64) {
    const int p = e / m, c = e % m;
    U[p * ld + c] = src[p * stride + perm[c]];
  }
}

// subset bases by deletions: the eigenpairs of the principal
//     submatrix C_sub = C[idx][:, idx] follow from those of C = U diag(lam)
//     U^T one deleted direction j at a time.  With z = row j of U, the
//     eigenvalues mu of the matrix without row / column j are the roots of
//         f(mu) = sum_i z_i^2 / (lam_i - mu) = 0
//     (det(C_j - mu) / det(C - mu) = [(C - mu)^-1]_jj), one between each
//     pair of consecutive poles, and its eigenvectors are U w with w_i ~
//     z_i / (lam_i - mu) (row j of U w is f(mu) = 0).  Each root is found
//     relative to its nearer pole (tau = mu - pole, Newton on tau rest(tau) -
//     z_pole^2 inside a bisection bracket), and the z_i are recomputed from
//     the roots by Loewner's formula before the vectors are formed
//     (Gu & Eisenstat: the vectors then come out orthogonal to rounding).
//     A direction whose z_i is negligible keeps its eigenpair (deflation).
//     One wavefront per mask, k deletions for k flagged directions (in
//     descending direction order, so the row of direction f is f), lane =
//     root / row; O(k n^2) per lane against the Jacobi's ~8 sweeps of n - 1
//     rounds.  Cases it does not take -- two poles closer than 1e-12 of the
//     spectrum, a root that does not converge -- are left to the Jacobi
//     kernel (status 1).  Eigenvalues to ~1e-15 of |lam|max and
//     eigenvectors to the conditioning LAPACK's have (~1e-11 for
//     close pairs), tests/test_gpu_parity.py::test_subset_secular_*.
//
//     Ancestors (level > 0): the launch takes the masks with `level` flagged
//     directions, launches run level 1, 2, ... in order, and a mask starts
//     from its nearest decomposed ancestor -- the mask with its lowest
//     flagged directions unflagged, whose deletions are the first ones of
//     its own (found in the mask table; decomposed by an earlier pass, or by
//     this call's lower levels without falling back) -- so a mask whose
//     parent is in the pool costs one deletion instead of one per flagged
//     direction.  level 0: every new mask from the global basis.  Either
//     way a mask's basis is bit for bit the chain's from the global basis:
//     an ancestor is taken only if the chain built it (status 0; status is
//     kept for every pool entry of the call, the host sets 1 before a pass's
//     launches, so an entry the Jacobi built is never a start).
__global__ __launch_bounds__(64) void kl_subset_secular_kernel(
    const double* __restrict__ g_u, const double* __restrict__ g_eig, int D,
    const unsigned long long* __restrict__ pool_mask, int pool_cap,
    int* __restrict__ counters, double* __restrict__ pool,
    uint8_t* __restrict__ status, const unsigned long long* __restrict__ keys,
    const int* __restrict__ ids, int table_cap, int level) {
#pragma clang fp contract(off)
  extern __shared__ double smem[];
  const int ld = odd_ld(D);
  double* U = smem;            // [D][ld] current eigenvectors (row = direction)
  double* W = U + D * ld;      // [D][ld] w (row = non-deflated pole, col = root), then U w
  double* lam = W + D * ld;    // [64] current eigenvalues, ascending
  double* lz = lam + 64;       // [64] the non-deflated ones
  double* zh = lz + 64;        // [64] their z (then Loewner's)
  double* tau = zh + 64;       // [64] root - its pole
  double* nlam = tau + 64;     // [64] next eigenvalues (unsorted)
  int* ndi = reinterpret_cast<int*>(nlam + 64);  // [64] non-deflated pole -> column
  int* orig = ndi + 64;        // [64] root -> its pole (index into lz)
  int* src = orig + 64;        // [64] next slot -> root r, or -1 - deflated column
  int* perm = src + 64;        // [64] an order
  const int l = lane();
  const int first = counters[kCntPassStart];
  const int last = min(counters[kCntIds], pool_cap);
  constexpr double kEps = 2.220446049250313e-16;
  for (int id = first + blockIdx.x; id < last; id += gridDim.x) {
    const unsigned long long msk = pool_mask[id];
    const int n = __popcll(msk);
    if (level > 0 && D - n != level) continue;  // another launch's
    if (n >= D) {
      if (l == 0) status[id] = 1;
      continue;
    }
    // ---- the nearest decomposed ancestor (wave-uniform search)
    const unsigned long long full = full_mask(D);
    unsigned long long anc = full;
    int aid = -1;
    if (level > 0) {
      unsigned long long a = msk;
      for (;;) {
        const unsigned long long fl = full & ~a;
        a |= fl & (~fl + 1ull);  // unflag the lowest flagged direction
        if (a == full) break;
        const int h = table_find(keys, table_cap, a);
        const int pid = h >= 0 ? ids[h] : -1;
        // chain-built ancestors only (status 0, kept across the passes of
        // the call): an entry the Jacobi decomposed is not the chain's bits
        if (pid >= 0 && pid < pool_cap && status[pid] == 0) {
          anc = a;
          aid = pid;
          break;
        }
      }
    }
    // ---- the start: the global basis, or the ancestor's pool entry (rows =
    //      its directions ascending, columns by |mu| descending)
    int m = __popcll(anc);
    if (aid < 0) {
      load_ascending(g_u, g_eig, D, m, U, ld, lam, perm);
    } else {
      const double* ea = pool + (size_t)aid * (D * D + D);
      load_ascending(ea, ea + D * D, D, m, U, ld, lam, perm);
    }
    lds_sync();
    bool ok = true;
    for (int f = D - 1; f >= 0 && ok; --f) {
      if ((msk >> f) & 1ull) continue;  // unflagged: stays
      if (!((anc >> f) & 1ull)) continue;  // deleted in the ancestor
      const int j = f;                  // its row (every deleted row so far is > f)
      // ---- z, deflation of negligible components
      const double z = l < m ? U[j * ld + l] : 0.0;
      const double zmax = wave_max(fabs(z));
      const double lmax = wave_max(l < m ? fabs(lam[l]) : 0.0);
      const bool nd = l < m && fabs(z) > 1e-14 * zmax;
      const unsigned long long ndm = __ballot(nd);
      const int nn = __popcll(ndm);
      const int kk = Group<1>::rank(ndm);
      if (nd) {
        ndi[kk] = l;
        lz[kk] = lam[l];
        zh[kk] = z;
      }
      lds_sync();
      // two non-deflated poles too close to separate a root between them
      const bool close = l + 1 < nn && lz[l + 1] - lz[l] <= 1e-12 * lmax;
      if (__ballot(close) != 0ull) {
        ok = false;
        break;
      }
      // ---- roots: lane r < nn - 1 between poles r and r + 1, as
      //      tau = mu - (nearer pole); Newton on tau rest(tau) - z_pole^2
      //      (the nearer pole's term divided out) inside a bisection bracket
      double t = 0.0;
      int o = 0;
      bool conv = true;
      if (l + 1 < nn) {
        const double lo = lz[l], hi = lz[l + 1];
        const double mid = lo + 0.5 * (hi - lo);
        double fm = 0.0;  // only its sign is used
#pragma unroll 4
        for (int k = 0; k < nn; ++k) {
          const double zk = zh[k];
          const double x = lz[k] - mid;
          double q = __builtin_amdgcn_rcp(x);
          q = q * (2.0 - x * q);
          fm += zk * zk * q;
        }
        double a, b;
        if (fm >= 0.0) {
          o = l;
          a = 0.0;
          b = mid - lo;
        } else {
          o = l + 1;
          a = mid - hi;
          b = 0.0;
        }
        const double lo_ = lz[o];
        const double zo = zh[o];
        const double zo2 = zo * zo;
        t = 0.5 * (a + b);
        conv = false;
        for (int it = 0; it < 64; ++it) {
          double rest = 0.0, drest = 0.0;
#pragma unroll 4
          for (int k = 0; k < nn; ++k) {
            const double zk = zh[k];
            const double x = (lz[k] - lo_) - t;
            // 1 / x: the hardware reciprocal and one Newton step (to ~1 ulp)
            double q = __builtin_amdgcn_rcp(x);
            q = q * (2.0 - x * q);
            q = k == o ? 0.0 : q;
            const double zq = zk * zk * q;
            rest += zq;
            drest += zq * q;
          }
          const double fv = rest - zo2 / t;  // increasing in t
          if (fv == 0.0) {
            conv = true;
            break;
          }
          if (fv < 0.0) a = t; else b = t;
          double tn = t - (t * rest - zo2) / (rest + t * drest);
          if (fabs(tn - t) <= 4.0 * kEps * fabs(t)) {
            t = tn;
            conv = true;
            break;
          }
          if (!(tn > a && tn < b)) tn = 0.5 * (a + b);
          t = tn;
          if (!(b - a > 4.0 * kEps * fmax(fabs(a), fabs(b)))) {
            conv = true;
            break;
          }
        }
        tau[l] = t;
        orig[l] = o;
      }
      if (__ballot(!conv) != 0ull) {
        ok = false;
        break;
      }
      lds_sync();
      // ---- Loewner: z_k^2 = prod_r (mu_r - lam_k) / prod_{k' != k} (lam_k' - lam_k),
      //      root r paired with pole r (r < k) or r + 1 (r >= k)
      double zn = 0.0;
      if (l < nn) {
        const double lk = lz[l];
        double pr = 1.0;
#pragma unroll 4
        for (int r = 0; r + 1 < nn; ++r) {
          const int kp = r < l ? r : r + 1;
          pr *= ((lz[orig[r]] - lk) + tau[r]) / (lz[kp] - lk);
        }
        zn = sqrt(fabs(pr));
        if (zh[l] < 0.0) zn = -zn;
      }
      lds_sync();
      if (l < nn) zh[l] = zn;
      lds_sync();
      // ---- w columns (lane r = root), normalised
      if (l + 1 < nn) {
        const double ol = lz[o];
        double nrm = 0.0;
#pragma unroll 4
        for (int k = 0; k < nn; ++k) {
          const double w = zh[k] / ((lz[k] - ol) - t);
          W[k * ld + l] = w;
          nrm += w * w;
        }
        const double inv = 1.0 / sqrt(nrm);
        for (int k = 0; k < nn; ++k) W[k * ld + l] *= inv;
      }
      // next eigenvalues: the roots (slots 0 .. nn - 2), then the deflated
      // poles (slots nn - 1 ..)
      const int dk = l - kk;  // deflated lanes below this one
      if (l + 1 < nn) {
        nlam[l] = lz[o] + t;
        src[l] = l;
      }
      if (l < m && !nd) {
        nlam[nn - 1 + dk] = lam[l];
        src[nn - 1 + dk] = -1 - l;
      }
      lds_sync();
      // ---- U w into W's root columns (column r is read whole by every
      //      lane before any lane writes it), deflated columns copied
      if (l < m) {
        // four root columns at a time: each U element read once per four
        // products; no deflation (the common case) reads U's columns directly
        const bool dense = nn == m;
        int r = 0;
        for (; r + 4 < nn; r += 4) {
          double y0 = 0.0, y1 = 0.0, y2 = 0.0, y3 = 0.0;
#pragma unroll 2
          for (int k = 0; k < nn; ++k) {
            const double u = U[l * ld + (dense ? k : ndi[k])];
            const double* wk = W + k * ld + r;
            y0 += u * wk[0];
            y1 += u * wk[1];
            y2 += u * wk[2];
            y3 += u * wk[3];
          }
          lds_sync();
          W[l * ld + r] = y0;
          W[l * ld + r + 1] = y1;
          W[l * ld + r + 2] = y2;
          W[l * ld + r + 3] = y3;
        }
        for (; r + 1 < nn; ++r) {
          double y = 0.0;
          for (int k = 0; k < nn; ++k) y += U[l * ld + (dense ? k : ndi[k])] * W[k * ld + r];
          lds_sync();
          W[l * ld + r] = y;
        }
        for (int c = 0; c < m - nn; ++c) {
          const int sc = src[nn - 1 + c];
          W[l * ld + nn - 1 + c] = U[l * ld + (-1 - sc)];
        }
      }
      // ascending order of the m - 1 next eigenvalues
      const int m1 = m - 1;
      if (l < m1) {
        const double v = nlam[l];
        int r2 = 0;
#pragma unroll 4
        for (int k = 0; k < m1; ++k) {
          r2 += ranks_before<AscendingValue>(nlam[k], k, v, l);
        }
        perm[r2] = l;
      }
      lds_sync();
      // ---- next U: rows without j, columns ascending
      if (l < m && l != j) {
        const int pn = l < j ? l : l - 1;
        for (int c = 0; c < m1; ++c) U[pn * ld + c] = W[l * ld + perm[c]];
      }
      lds_sync();
      if (l < m1) lam[l] = nlam[perm[l]];
      // column norms without row j (lane = column, rows summed in order;
      // ~1 to rounding: row j of U w is f(mu) = 0), then each row rescaled
      if (l < m1) {
        double nr = 0.0;
#pragma unroll 4
        for (int r = 0; r < m1; ++r) {
          const double y = U[r * ld + l];
          nr += y * y;
        }
        tau[l] = sqrt(nr);
      }
      lds_sync();
      if (l < m1)
        for (int c = 0; c < m1; ++c) U[l * ld + c] = U[l * ld + c] / tau[c];
      lds_sync();
      m = m1;
    }
    if (!ok) {
      if (l == 0) status[id] = 1;
      continue;
    }
    // ---- pool entry: columns by |mu| descending (eig_order's rule)
    if (l < m) perm[order_rank<DescendingAbs>(m, l, [&](int k) { return lam[k]; })] = l;
    lds_sync();
    double* e = pool + (size_t)id * (D * D + D);
    if (l < m) {
      for (int r = 0; r < m; ++r) e[l * D + r] = U[l * ld + perm[r]];
      e[D * D + l] = lam[perm[l]];
    }
    if (l == 0) status[id] = 0;
    lds_sync();
  }
}

// The pool holds `need` entries or more: d_pool_mask.size() of them, 1024
// doubled as often as it takes, the earlier entries kept.
static int ensure_pool(sf_ctx* ctx, size_t need) {
  const size_t entry = (size_t)ctx->D * ctx->D + ctx->D;
  if (ctx->pool_D != ctx->D) {
    ctx->d_pool.reset();
    ctx->d_pool_mask.reset();
    ctx->pool_D = ctx->D;
  }
  size_t cap = ctx->d_pool_mask.size() ? ctx->d_pool_mask.size() : 1024;
  while (cap < need) cap *= 2;
  SF_TRY(ctx->d_pool.reserve_keep(cap * entry, kFitAlloc));
  return ctx->d_pool_mask.reserve_keep(cap, kFitAlloc);
}

// pool_mask[id] for ids assigned beyond a previous pool capacity
__global__ __launch_bounds__(256) void kl_fill_mask_kernel(
    const unsigned long long* __restrict__ keys, const int* __restrict__ ids,
    int cap, unsigned long long* __restrict__ pool_mask, int lo) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  if (keys[i] != kEmptyKey && ids[i] >= lo) pool_mask[ids[i]] = keys[i];
}

// new masks of a pass from which SF_OPT_FIT_SUBSET_DELETION = 1 starts
// deletions from ancestors (below it: one launch from the global basis)
constexpr int kAncestorMinMasks = 8192;

// number new masks, make sure the pool holds them, decompose them
static int number_and_decompose(sf_ctx* ctx, int* n_slow, int* n_nonuniform) {
  SF_HIP(hipMemcpyAsync(ctx->d_counters + kCntPassStart, ctx->d_counters + kCntIds,
                        sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
  SF_HIP(hipMemsetAsync(ctx->d_counters + kCntMaxLevel, 0, sizeof(int), ctx->stream));
  const int cap = (int)ctx->d_keys.size();
  const int old_cap = (int)ctx->d_pool_mask.size();
  hipLaunchKernelGGL(kl_assign_kernel, dim3(std::min((cap + 255) / 256, 8192)), dim3(256), 0,
                     ctx->stream, ctx->d_keys, cap, ctx->d_ids,
                     ctx->d_pool_mask, old_cap, ctx->d_counters, ctx->D);
  SF_HIP(hipGetLastError());
  int cnt[kCntMaxLevel + 1];
  SF_HIP(hipMemcpyAsync(cnt, ctx->d_counters, sizeof(cnt), hipMemcpyDeviceToHost,
                        ctx->stream));
  SF_HIP(hipStreamSynchronize(ctx->stream));
  *n_slow = cnt[kCntSlow];
  *n_nonuniform = cnt[kCntNonUniform];
  if (cnt[kCntIds] > old_cap) {
    SF_TRY(ensure_pool(ctx, (size_t)cnt[kCntIds]));
    hipLaunchKernelGGL(kl_fill_mask_kernel, dim3((cap + 255) / 256), dim3(256),
                       0, ctx->stream, ctx->d_keys, ctx->d_ids, cap,
                       ctx->d_pool_mask, old_cap);
    SF_HIP(hipGetLastError());
  }
  const int n_new = cnt[kCntIds] - cnt[kCntPassStart];
  const uint8_t* done = nullptr;
  if (n_new > 0 && ctx->fit_subset_deletion && ctx->D <= 64) {
    // subset bases by deletions first (kl_subset_secular_kernel); the
    // Jacobi below takes the masks it left (status 1)
    // (the status of every pool entry of the call is kept: a later pass's
    // masks take an earlier pass's entries as ancestors only if the chain
    // built them; the stream was synchronised above, so the copy is safe)
    SF_TRY(ctx->d_pool_status.reserve_keep(ctx->d_pool_mask.size(),
                                           kFitAlloc));
    SF_HIP(hipMemsetAsync(ctx->d_pool_status + cnt[kCntPassStart], 1, (size_t)n_new, ctx->stream));
    const int D = ctx->D;
    const int ldd = odd_ld(D);
    const size_t shm = (size_t)2 * D * ldd * sizeof(double) + 6 * 64 * sizeof(double) +
                       4 * 64 * sizeof(int);
    SF_TRY(allow_lds(kl_subset_secular_kernel, shm));
    const int blocks = n_new < 16384 ? n_new : 16384;
    // levels 1 .. (most flagged directions), each mask from its nearest
    // decomposed ancestor (option 3, and option 1 -- the default -- when the
    // pass has kAncestorMinMasks new masks or more), or one launch, every
    // mask from the global basis (option 2, and option 1 below that count):
    // the same bits either way.  The level launches are serial, one per
    // level; they pay off where the deletions they save are many (config 5:
    // ~113 k masks, 229 -> 192 ms per fit) and cost where the masks are few
    // and deep (the gain step's amplitude fit: block flags, up to D - 1
    // flagged directions per mask, ~31 level launches per step: 10.4 ->
    // 18.7 ms per step)
    const bool anc = ctx->fit_subset_deletion == 3 ||
                     (ctx->fit_subset_deletion == 1 && n_new >= kAncestorMinMasks);
    const int levels = anc ? cnt[kCntMaxLevel] : 0;
    for (int lv = levels > 0 ? 1 : 0; lv <= levels; ++lv) {
      hipLaunchKernelGGL(kl_subset_secular_kernel, dim3(blocks), dim3(64), shm, ctx->stream,
                         ctx->d_u, ctx->d_eig, D, ctx->d_pool_mask, (int)ctx->d_pool_mask.size(),
                         ctx->d_counters, ctx->d_pool, ctx->d_pool_status, ctx->d_keys,
                         ctx->d_ids, cap, lv);
      SF_HIP(hipGetLastError());
    }
    done = ctx->d_pool_status;
  }
  if (n_new > 0) {
    const int D = ctx->D;
    const size_t shm = (size_t)2 * subset_rows(D) * subset_ld(D) * sizeof(double) +
                       64 * sizeof(double2) + 96 * sizeof(int2) +
                       128 * sizeof(int);
    const int blocks = n_new < 8192 ? n_new : 8192;
    // 1..4 waves per mask (sf_set_option admits no other count)
    const int nw = ctx->fit_eig_waves > 0 ? ctx->fit_eig_waves : kEigWavesDefault;
    decltype(&kl_subset_eig_kernel<1>) const eig[4] = {
        kl_subset_eig_kernel<1>, kl_subset_eig_kernel<2>, kl_subset_eig_kernel<3>,
        kl_subset_eig_kernel<4>};
    SF_TRY(allow_lds(eig[nw - 1], shm));
    hipLaunchKernelGGL(eig[nw - 1], dim3(blocks), dim3(64 * nw), shm, ctx->stream,
                       ctx->d_c, D, ctx->d_pool_mask, (int)ctx->d_pool_mask.size(),
                       ctx->d_counters, ctx->d_pool, done);
    SF_HIP(hipGetLastError());
  }
  return SF_OK;
}

}  // namespace sf
