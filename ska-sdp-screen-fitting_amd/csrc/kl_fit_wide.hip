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
//   * kl_wide_keys / _insert / _assign / _slot_id / _subset kernels: the
//                                mask cache (below)
// A slot with every direction unflagged uses the global basis (quirk Q1); a
// slot with flagged directions needs the eigen-decomposition of its C_sub.
// The mask cache (SF_OPT_FIT_WIDE_CACHE) decomposes every distinct flag mask
// of the call's input once, before pass 0: the 128-bit masks go into an
// open-addressing table, each distinct one gets a pool entry (V, lam, perm as
// setup_subset leaves them) built by kl_wide_subset_kernel with the calls
// setup_subset makes, and the fit workgroup of a slot that finds its mask in
// the pool copies the entry instead of running the Jacobi.  Masks that
// outlier flags create in later passes are looked up, never inserted: a miss
// decomposes in the slot's own workgroup, and only where the pass fits the
// slot at all.  With the cache off, or for a mask without an entry, the slot
// decomposes its own C_sub.  The shared C and U are read from global memory
// (L2); the per-workgroup matrices V / M1 / M2 sit in LDS as far as 160 KiB
// reach, the rest in a workspace sized by the (capped, persistent) grid.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "kl_cov.h"
#include "kl_fit_exact.h"
#include "kl_fit_masks.h"
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
  int* counters;       // d_counters: kCntWideDecomp counts the decompositions
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
    if (threadIdx.x == 0) atomicAdd(counters + kCntWideDecomp, 1);
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
  const SlotGeom g(s, F, A);
  const bool skipped = g.skipped(skip, ref_skip);
  w_out[e] = weight[e];
  if (skipped) {
    coef[e] = 0.0;
    resid[e] = 0.0;
  }
  if (d == 0) order_out[s] = skipped ? 0 : st_order[g.a];
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
  const SlotGeom g(s, F, A);
  if (g.skipped(skip, ref_skip)) return;
  const double sig = sigma[g.blk];
  const double v = phase_ref(phase, refph, ref_sub, s, g.a, A, D, d);
  const double sd = screen_diff(screen_type, v, resid[e]);
  if (fabs(sd) > nsigma * sig && w_out[e] != 0.0f) w_out[e] = 0.0f;
}

// ---------------------------------------------------------------------------
// mask cache: 128-bit keys, a table of claimants, a pool of subset bases
// ---------------------------------------------------------------------------
// A pool entry: V [D][ld] (rows and columns < n used), lam [D], perm [D] ints
// in the space of D doubles.
__host__ __device__ inline size_t wide_entry_doubles(int D) {
  return (size_t)D * odd_ld(D) + 2 * (size_t)D;
}

// What the fit kernel reads of the cache (n == 0: off).  Nothing of it
// changes while a fit pass runs.
struct WidePool {
  const unsigned long long* tab;   // [cap] claimant slot + 1, 0 = empty
  const unsigned long long* keys;  // [S][2] initial mask of every slot
  const int* tab_id;               // [cap] pool id of a claimed entry
  const int* slot_id;              // [S] pool id of the slot's initial mask, -1: none
  const double* pool;              // [n] entries
  int cap;                         // power of two
  int n;
};

__device__ __forceinline__ int wide_hash(unsigned long long lo,
                                         unsigned long long hi, int cap) {
  return (int)(mix64(mix64(lo ^ 0x9e3779b97f4a7c15ull) + hi) &
               (unsigned long long)(cap - 1));
}

// the unflagged-direction mask of every slot (bit d of (lo, hi) = weight of
// direction d positive, as the fit kernel votes it); (0, 0) for the slots no
// pass fits.  One wavefront per slot.
__global__ __launch_bounds__(256) void kl_wide_keys_kernel(
    const float* __restrict__ weight, int64_t S, int F, int A, int D,
    const uint8_t* __restrict__ skip, int ref_skip,
    unsigned long long* __restrict__ keys) {
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= S) return;  // wave-uniform
  const int l = lane();
  const float* w = weight + s * D;
  const unsigned long long lo = __ballot(l < D && w[l] > 0.0f);
  const unsigned long long hi = __ballot(l + 64 < D && w[l + 64] > 0.0f);
  const bool skipped = SlotGeom(s, F, A).skipped(skip, ref_skip);
  if (l == 0) {
    keys[2 * s] = skipped ? 0ull : lo;
    keys[2 * s + 1] = skipped ? 0ull : hi;
  }
}

// Insert the masks with 0 < n < D (one thread per slot); slot_pos[s] = the
// table entry of the slot's mask, or -1.  An entry is claimed by one CAS of
// the slot's index + 1, and the key of a claimed entry is the claimant's row
// of `keys`, complete since the previous kernel: equality is decided on both
// words, and no thread ever waits for another.
__global__ __launch_bounds__(256) void kl_wide_insert_kernel(
    const unsigned long long* __restrict__ keys, int64_t S, int D,
    unsigned long long* __restrict__ tab, int cap, int* __restrict__ slot_pos) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const unsigned long long lo = keys[2 * s], hi = keys[2 * s + 1];
  const int n = __popcll(lo) + __popcll(hi);
  int pos = -1;
  if (n > 0 && n < D) {
    int h = wide_hash(lo, hi, cap);
    for (int probe = 0; probe < cap; ++probe) {
      // a plain load first: most slots find their mask's entry taken
      unsigned long long e = tab[h];
      if (e == 0ull) e = atomicCAS(tab + h, 0ull, (unsigned long long)(s + 1));
      if (e == 0ull) {  // claimed here
        pos = h;
        break;
      }
      const int64_t c = (int64_t)(e - 1ull);
      if (keys[2 * c] == lo && keys[2 * c + 1] == hi) {
        pos = h;
        break;
      }
      h = (h + 1) & (cap - 1);
    }
  }
  slot_pos[s] = pos;
}

// number the claimed entries (number_fresh, as kl_assign_kernel) and copy
// their claimants' keys to pool_mask (ids below mask_cap)
__global__ __launch_bounds__(256) void kl_wide_assign_kernel(
    const unsigned long long* __restrict__ tab, int cap,
    const unsigned long long* __restrict__ keys, int* __restrict__ tab_id,
    unsigned long long* __restrict__ pool_mask, int mask_cap,
    int* __restrict__ count) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; wave_in_table(i, cap);
       i += gridDim.x * blockDim.x) {
    const unsigned long long e = i < cap ? tab[i] : 0ull;
    const int id = number_fresh(e != 0ull, count);
    if (id < 0) continue;
    tab_id[i] = id;
    if (id < mask_cap) {
      pool_mask[2 * (size_t)id] = keys[2 * (e - 1ull)];
      pool_mask[2 * (size_t)id + 1] = keys[2 * (e - 1ull) + 1];
    }
  }
}

// per slot: table entry -> pool id (-1: no entry for the slot's mask)
__global__ __launch_bounds__(256) void kl_wide_slot_id_kernel(
    int64_t S, const int* __restrict__ tab_id, int n_entries,
    int* __restrict__ slot) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int pos = slot[s];
  int id = -1;
  if (pos >= 0) {
    id = tab_id[pos];
    if (id >= n_entries) id = -1;
  }
  slot[s] = id;
}

// pool id of the mask (lo, hi), or -1 (find, no insert).  Called by the whole
// workgroup with the same mask: every thread reads the same addresses.
__device__ inline int wide_pool_find(const WidePool& P, unsigned long long lo,
                                     unsigned long long hi) {
  int h = wide_hash(lo, hi, P.cap);
  for (int probe = 0; probe < P.cap; ++probe) {
    const unsigned long long e = P.tab[h];
    if (e == 0ull) return -1;
    const unsigned long long* k = P.keys + 2 * (e - 1ull);
    if (k[0] == lo && k[1] == hi) {
      const int id = P.tab_id[h];
      return id < P.n ? id : -1;
    }
    h = (h + 1) & (P.cap - 1);
  }
  return -1;
}

// setup_subset from pool entry `ent`: idx as setup_subset builds it, lam and
// perm from the entry, and its V (rows < n whole: the columns from n on are
// never read) copied into the workgroup's own V, which sits in LDS for every
// D <= 128: the fit reads each element many times, and the structured
// workload of tools/fit_wide.py ran 8 % (D = 80) and 6.5 % (D = 128) slower
// with V read in place from L2.
__device__ inline void wide_pool_subset(const WideTeam& tm, const WideFit& L,
                                        const double* ent, int D, int n,
                                        const WideMask& um, bool unfl) {
  const int t = tm.lane();
  const double* lam = ent + (size_t)D * L.ld;
  const int* perm = reinterpret_cast<const int*>(lam + D);
  if (t < D && unfl) L.idx[tm.rank(um)] = t;
  if (t < n) {
    L.lam[t] = lam[t];
    L.perm[t] = perm[t];
  }
  for (int k = t; k < n * L.ld; k += kWideThreads) L.V[k] = ent[k];
  tm.sync();
}

// The subset bases of pool entries [0, n_entries): one workgroup per entry on
// a persistent grid.  setup_subset itself on the entry's mask -- the gather
// of C_sub, wide_jacobi, eig_order on the same values in the same order as in
// the fit workgroup, so the entry holds that workgroup's bits.  The Jacobi's
// `a` (M1) sits in LDS; V beside it where both fit 160 KiB (v_lds), else the
// Jacobi works on the entry's own V in global memory.
__global__ __launch_bounds__(kWideThreads) void kl_wide_subset_kernel(
    int n_entries, int D, int v_lds, const double* __restrict__ g_c,
    const unsigned long long* __restrict__ pool_mask, double* pool,
    int* __restrict__ counters) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char wide_smem[];
  WideSmall& S = *reinterpret_cast<WideSmall*>(wide_smem);
  const int ld = odd_ld(D);
  const size_t mat = (size_t)D * ld;
  double* lmat = reinterpret_cast<double*>(wide_smem + sizeof(WideSmall));
  const WideTeam tm{S.red, S.bal};
  WideFit L;
  L.S = &S;
  L.gC = g_c;
  L.gU = nullptr;
  L.gEig = nullptr;
  L.M1 = lmat;
  L.M2 = nullptr;
  L.lam = S.lam;
  L.idx = S.idx;
  L.perm = S.perm;
  L.counters = counters;
  L.D = D;
  L.ld = ld;
  const int t = threadIdx.x;
  const int d = wide_row();
  for (int e = blockIdx.x; e < n_entries; e += gridDim.x) {
    double* ent = pool + (size_t)e * wide_entry_doubles(D);
    L.V = v_lds ? lmat + mat : ent;
    WideMask um;
    um.lo = pool_mask[2 * (size_t)e];
    um.hi = pool_mask[2 * (size_t)e + 1];
    um.n = __popcll(um.lo) + __popcll(um.hi);
    const int n = um.n;
    const bool unfl = d < D && (((d < 64 ? um.lo >> d : um.hi >> (d - 64)) & 1ull) != 0ull);
    setup_subset(tm, L, D, Subset{n, false, 0.0}, um, unfl);
    if (v_lds)
      for (int k = t; k < n * ld; k += kWideThreads)
        if (k % ld < n) ent[k] = L.V[k];
    double* lam = ent + mat;
    int* perm = reinterpret_cast<int*>(lam + D);
    if (t < n) {
      lam[t] = S.lam[t];
      perm[t] = S.perm[t];
    }
    // the next entry's setup overwrites what was just read
    __syncthreads();
  }
}

// One outlier iteration `it` of every slot: one workgroup per slot, walking
// the slots with the grid's stride.  nl of the matrices V, M1, M2 sit in the
// dynamic LDS, the others in this workgroup's slice of `ws`.  P: the mask
// cache (P.n == 0: every flagged slot decomposes its own subset).
__global__ __launch_bounds__(kWideThreads) void kl_fit_wide_kernel(
    int it, int niter, int64_t nslots, int F, int A, int D, int nl,
    const double* __restrict__ phase, const double* __restrict__ refph,
    int ref_sub, int ref_skip, const double* __restrict__ g_c,
    const double* __restrict__ g_u, const double* __restrict__ g_eig,
    const int* __restrict__ st_order, const uint8_t* __restrict__ skip,
    int screen_type, double nsigma, int adjust_order, double* ws,
    const WidePool P, int* __restrict__ counters, double* __restrict__ coef,
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
  const size_t entry = wide_entry_doubles(D);

  for (int64_t s = blockIdx.x; s < nslots; s += gridDim.x) {
    const SlotGeom g(s, F, A);
    const int a = g.a;
    if (g.skipped(skip, ref_skip)) continue;  // workgroup-uniform
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
    // The slot's subset basis: its mask's pool entry -- pass 0: the id the
    // assign kernels left for the slot; later passes: the mask after the
    // outlier flags, looked up -- else decomposed here.  The id is read at
    // one address (the lookup: from one mask) by the whole workgroup, so the
    // branch is workgroup-uniform.
    auto subset_basis = [&]() {
      int id = -1;
      if (P.n > 0 && !st.full)
        id = __builtin_amdgcn_readfirstlane(
            it == 0 ? P.slot_id[s] : wide_pool_find(P, um.lo, um.hi));
      if (id >= 0) {
        wide_pool_subset(tm, L, P.pool + (size_t)id * entry, D, n_unfl, um, unfl);
      } else {
        setup_subset(tm, L, D, st, um, unfl);
      }
    };

    if (n_unfl > 0) {
      if (order > n_unfl - 1) order = n_unfl - 1;
      if (it == 0) {
        subset_basis();
        decomposed = true;
        fit_screen(tm, L, st, D, (int)order, screen_type, um, phi_d, w_d, white_d,
                   resid_d);
      } else if (adjust_order) {
        OrderWalk walk;
        for (int oi = 0; oi < 4; ++oi) {
          // oi == 0: the weights always compare equal (quirk Q2) -> no fit
          if (oi > 0) {
            if (!decomposed) {
              subset_basis();
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

// The mask cache of one fit, built before pass 0: the slots' masks, the
// table, the numbering (read back, as the <= 60 path reads its new-mask
// count), the pool sized min(distinct masks, SF_OPT_FIT_WIDE_POOL_MAX,
// SF_OPT_FIT_WIDE_POOL_MB / entry bytes) and its subset bases.  Masks
// numbered beyond the pool get no entry.  P->n = 0 when nothing is cached.
int build_wide_pool(sf_ctx* ctx, const float* weight, int64_t S, int F, int A,
                    int ref_skip, int n_cu, WidePool* P) {
  const int D = ctx->D;
  const size_t entry = wide_entry_doubles(D);
  const size_t mb = ctx->wide_pool_mb > 0 ? (size_t)ctx->wide_pool_mb : 2048;
  size_t max_entries = (mb << 20) / (entry * sizeof(double));
  if (ctx->wide_pool_max > 0 && max_entries > (size_t)ctx->wide_pool_max)
    max_entries = (size_t)ctx->wide_pool_max;
  if (max_entries > (size_t)S) max_entries = (size_t)S;
  if (max_entries == 0) return SF_OK;
  SF_TRY(reserve_pair(ctx->d_wkeys, (size_t)2 * S, ctx->d_wslot, (size_t)S, kFitAlloc));
  // at most one insert per slot: the table stays half empty
  const size_t tcap = next_pow2((size_t)2 * S, 64);
  SF_TRY(reserve_pair(ctx->d_wtab, tcap, ctx->d_wtab_id, tcap, kFitAlloc));
  SF_TRY(ctx->d_wpool_mask.reserve(2 * max_entries, kFitAlloc));
  const int cap = (int)ctx->d_wtab.size();
  SF_HIP(hipMemsetAsync(ctx->d_wtab, 0, cap * sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(kl_wide_keys_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256),
                     0, ctx->stream, weight, S, F, A, D, ctx->d_skip, ref_skip,
                     ctx->d_wkeys);
  SF_HIP(hipGetLastError());
  hipLaunchKernelGGL(kl_wide_insert_kernel, dim3((unsigned)((S + 255) / 256)),
                     dim3(256), 0, ctx->stream, ctx->d_wkeys, S, D, ctx->d_wtab,
                     cap, ctx->d_wslot);
  SF_HIP(hipGetLastError());
  int* count = ctx->d_counters + kCntWideMasks;
  hipLaunchKernelGGL(kl_wide_assign_kernel,
                     dim3((unsigned)((cap + 255) / 256 < 8192 ? (cap + 255) / 256 : 8192)),
                     dim3(256), 0, ctx->stream, ctx->d_wtab, cap, ctx->d_wkeys,
                     ctx->d_wtab_id, ctx->d_wpool_mask, (int)max_entries, count);
  SF_HIP(hipGetLastError());
  int n_masks = 0;
  SF_HIP(hipMemcpyAsync(&n_masks, count, sizeof(int), hipMemcpyDeviceToHost,
                        ctx->stream));
  SF_HIP(hipStreamSynchronize(ctx->stream));
  const int n = (size_t)n_masks < max_entries ? n_masks : (int)max_entries;
  if (n == 0) return SF_OK;
  SF_TRY(ctx->d_wpool.reserve((size_t)n * entry, kFitAlloc));
  hipLaunchKernelGGL(kl_wide_slot_id_kernel, dim3((unsigned)((S + 255) / 256)),
                     dim3(256), 0, ctx->stream, S, ctx->d_wtab_id, n, ctx->d_wslot);
  SF_HIP(hipGetLastError());
  // M1 always fits the LDS (D <= 128); V beside it up to D = 97
  const int v_lds = wide_lds_mats(D) >= 2;
  const size_t shm = sizeof(WideSmall) +
                     (size_t)(v_lds ? 2 : 1) * D * odd_ld(D) * sizeof(double);
  SF_TRY(allow_lds(kl_wide_subset_kernel, shm));
  const int grid = n_cu > 0 && n_cu < n ? n_cu : n;
  hipLaunchKernelGGL(kl_wide_subset_kernel, dim3((unsigned)grid),
                     dim3(kWideThreads), shm, ctx->stream, n, D, v_lds, ctx->d_c,
                     ctx->d_wpool_mask, ctx->d_wpool, ctx->d_counters);
  SF_HIP(hipGetLastError());
  P->tab = ctx->d_wtab;
  P->keys = ctx->d_wkeys;
  P->tab_id = ctx->d_wtab_id;
  P->slot_id = ctx->d_wslot;
  P->pool = ctx->d_wpool;
  P->cap = cap;
  P->n = n;
  ctx->wide_pool_n = n;
  return SF_OK;
}
}  // namespace

// sf_get_fit_pool_wide: entries [0, k) with perm applied, in sf_get_fit_pool's
// layout ([D][D] block, leading n x n used, then D eigenvalue slots); the
// rest of an entry is zero.  The caller has synchronised.
int read_fit_pool_wide(sf_ctx* ctx, uint64_t* masks, double* entries, int k) {
  const int D = ctx->D, ld = odd_ld(D);
  const size_t entry = wide_entry_doubles(D), out = (size_t)D * D + D;
  SF_HIP(hipMemcpy(masks, ctx->d_wpool_mask, (size_t)k * 2 * sizeof(uint64_t),
                   hipMemcpyDeviceToHost));
  const int chunk = 64;  // entries per copy: <= 8.6 MiB of host staging
  std::vector<double> buf((size_t)chunk * entry);
  for (int e0 = 0; e0 < k; e0 += chunk) {
    const int ne = k - e0 < chunk ? k - e0 : chunk;
    SF_HIP(hipMemcpy(buf.data(), ctx->d_wpool + (size_t)e0 * entry,
                     (size_t)ne * entry * sizeof(double), hipMemcpyDeviceToHost));
    for (int e = 0; e < ne; ++e) {
      const double* v = buf.data() + (size_t)e * entry;
      const double* lam = v + (size_t)D * ld;
      const int* perm = reinterpret_cast<const int*>(lam + D);
      double* o = entries + (size_t)(e0 + e) * out;
      const uint64_t* m = masks + 2 * (size_t)(e0 + e);
      const int n = __builtin_popcountll(m[0]) + __builtin_popcountll(m[1]);
      for (size_t i = 0; i < out; ++i) o[i] = 0.0;
      for (int i = 0; i < n; ++i)
        for (int r = 0; r < n; ++r) o[(size_t)i * D + r] = v[(size_t)i * ld + perm[r]];
      for (int r = 0; r < n; ++r) o[(size_t)D * D + r] = lam[r];
    }
  }
  return SF_OK;
}

size_t wide_basis_ws_doubles(int D) { return (size_t)2 * D * odd_ld(D); }

int launch_basis_wide(sf_ctx* ctx) {
  const int D = ctx->D;
  SF_TRY(ctx->d_wide_ws.reserve(wide_basis_ws_doubles(D), kFitAlloc));
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
  SF_TRY(fit_buffers(ctx, S, F, A, &resid, &w_out, &order_out));
  SF_HIP(hipMemsetAsync(ctx->d_counters, 0, kFitCounters * sizeof(int), ctx->stream));

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
  SF_TRY(ctx->d_wide_ws.reserve(ws, kFitAlloc));
  SF_TRY(allow_lds(kl_fit_wide_kernel, shm));

  WidePool pool = {};
  ctx->wide_pool_n = 0;
  if (ctx->wide_cache)
    SF_TRY(build_wide_pool(ctx, weight, S, F, A, r.skip, n_cu, &pool));

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
                       ctx->d_wide_ws, pool, ctx->d_counters, coef, resid,
                       w_out, order_out);
    SF_HIP(hipGetLastError());
    if (block_flags && it + 1 < p->niter) {
      SF_TRY(launch_block_sigma(ctx, T, F, A, phase, r, p->screen_type,
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
