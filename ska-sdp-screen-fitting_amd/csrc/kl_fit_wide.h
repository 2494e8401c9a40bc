// kl_fit_wide.h -- workgroup-level (256-thread) float64 building blocks of the
// KL fit with 61..128 directions: reductions and votes over up to 128 rows
// (WideTeam: the Team of kl_fit_steps.h), the cyclic Jacobi eigen-solver on
// the rotation of sf_wave.h, and a Cholesky solver.
//
// Layout convention: thread t of the workgroup owns row i = t & 127 and
// belongs to column share w = t >> 7 (two shares).  Per-row values are held
// by both shares alike; every reduction, vote and broadcast goes through LDS
// in a fixed order and reads the rows of share 0 (waves 0 and 1) only, so
// every decision taken from one is workgroup-uniform and does not depend on
// how the waves were scheduled.  Every function here is called by the WHOLE
// workgroup (they contain __syncthreads()).  Matrices have row stride `ld`
// (odd) and may live in LDS or in global memory (generic pointers).
#pragma once

#include <hip/hip_runtime.h>

#include "sf_wave.h"

namespace sf {

constexpr int kWideRows = 128;    // rows (directions): one thread each
constexpr int kWideShares = 2;    // column shares of the Jacobi rounds
constexpr int kWideThreads = kWideRows * kWideShares;
constexpr int kWideCH = 8;        // column pairs per Jacobi chunk

// Vectors and Jacobi scratch of one workgroup (LDS).
struct WideSmall {
  double vec[6][kWideRows];  // broadcast vectors
  double lam[kWideRows];     // eigenvalues of C_sub by rank
  double2 cs[kWideRows];     // Jacobi rotation of each row / column
  double red[8];             // reductions, broadcasts
  unsigned long long bal[2]; // votes of waves 0 and 1
  int2 pr[kWideRows / 2];    // Jacobi round pairs
  int part[kWideRows];       // Jacobi partner of each row
  int idx[kWideRows];        // subset position -> direction
  int perm[kWideRows];       // rank -> column of V
};

__device__ __forceinline__ int wide_row() { return threadIdx.x & (kWideRows - 1); }
__device__ __forceinline__ int wide_share() { return threadIdx.x >> 7; }

// Sums of N per-row terms over the 128 rows (0 on rows that do not take
// part): butterfly inside waves 0 and 1, then red[0] + red[1].
template <int N>
__device__ inline void wide_sum(double (&x)[N], double* red) {
  static_assert(2 * N <= 8, "red holds 8 doubles");
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double s = wave_sum(x[k]);
    if (wv < 2 && lane() == 0) red[2 * k + wv] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = red[2 * k] + red[2 * k + 1];
  __syncthreads();
}

__device__ inline double wide_max(double x, double* red) {
  const int wv = threadIdx.x >> 6;
  const double s = wave_max(x);
  if (wv < 2 && lane() == 0) red[wv] = s;
  __syncthreads();
  const double r = fmax(red[0], red[1]);
  __syncthreads();
  return r;
}

// Vote over the 128 rows: bit i of (lo, hi) = row i, n = set bits.
struct WideMask {
  unsigned long long lo, hi;
  int n;
};
__device__ inline WideMask wide_ballot(bool x, unsigned long long* bal) {
  const unsigned long long b = __ballot(x);
  const int wv = threadIdx.x >> 6;
  if (wv < 2 && lane() == 0) bal[wv] = b;
  __syncthreads();
  WideMask m;
  m.lo = bal[0];
  m.hi = bal[1];
  m.n = __popcll(m.lo) + __popcll(m.hi);
  __syncthreads();
  return m;
}
// number of set bits of m below row i (0 <= i < 128)
__device__ __forceinline__ int wide_rank(const WideMask& m, int i) {
  if (i < 64) return __popcll(m.lo & ((1ull << i) - 1ull));
  return __popcll(m.lo) + __popcll(m.hi & ((1ull << (i - 64)) - 1ull));
}

// The Team of the slot steps (kl_fit_steps.h) on the workgroup: lane = thread
// (threads < n hold the gathered rows), row / share as above, one barrier
// pair per sum / max / ballot.
struct WideTeam {
  using Mask = WideMask;
  double* red;              // WideSmall::red
  unsigned long long* bal;  // WideSmall::bal
  __device__ static int lane() { return threadIdx.x; }
  __device__ static int row() { return wide_row(); }
  __device__ static int share() { return wide_share(); }
  __device__ static constexpr int shares() { return kWideShares; }
  __device__ static void sync() { __syncthreads(); }
  template <int N>
  __device__ void sum(double (&x)[N]) const { wide_sum(x, red); }
  __device__ double max(double x) const { return wide_max(x, red); }
  __device__ Mask ballot(bool x) const { return wide_ballot(x, bal); }
  // set bits of m below this thread's row (threads < 128)
  __device__ static int rank(const Mask& m) { return wide_rank(m, threadIdx.x); }
};

// wg_jacobi for n <= 128 on 256 threads: the same round-robin pairing, the
// same rotations (jacobi_pair) and the same `off > 1e-26 (off + dia)` test,
// followed by one polishing sweep (below).  Thread t owns row t & 127 and
// updates the column pairs of share t >> 7.  A row's partner row may belong
// to another wave, so a workgroup barrier separates a chunk's reads from its
// writes (the chunks of a round touch disjoint columns: one barrier per chunk
// is enough), and every thread runs the same number of chunks whatever its
// share holds.  n >= 1.
// The chunk update is spelled out here, not through jacobi_update_read /
// _write: the same arithmetic through the helpers was scheduled differently
// (3 more s_waitcnt in this function) and the D = 80 fit ran 1.4 % slower,
// beyond the parent's spread.
__device__ inline int wide_jacobi(double* a, double* v, WideSmall& S, int n,
                                  int ld, int max_sweeps) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  const int i = wide_row();
  const int w = wide_share();
  const bool own = i < n;
  const int m = n + (n & 1);
  const int npairs = m / 2;
  const int share = (npairs + kWideShares - 1) / kWideShares;
  const int kb = min(w * share, npairs);
  const int ke = min(kb + share, npairs);
  const int nchunks = (share + kWideCH - 1) / kWideCH;
  for (int j = w; j < n; j += kWideShares)
    if (own) v[i * ld + j] = (i == j) ? 1.0 : 0.0;
  __syncthreads();
  int sweep = 0;
  bool polished = false;  // workgroup-uniform
  for (; sweep < max_sweeps; ++sweep) {
    double od[2] = {0.0, 0.0};  // off-diagonal, diagonal mass
    if (own) {
      for (int j = 0; j < n; ++j) {
        const double x = a[i * ld + j];
        if (j == i) od[1] += x * x; else od[0] += x * x;
      }
    }
    wide_sum(od, S.red);
    // converged at wg_jacobi's test, ||offdiag||_F <= 1e-13 ||A||_F -- and
    // then ONE more sweep.  The test is relative to the whole spectrum: at
    // D > 60 |lambda|max ~ 1e4 leaves off-diagonal elements of ~1e-9, and
    // eigenvalue gaps of 3e-3 occur (D = 65: the pair's vectors were 8.7e-9
    // off, the basis check allows 1e-9).  The sweep after the test squares
    // that (quadratic convergence) down to the rounding floor.
    if (!(od[0] > 1e-26 * (od[0] + od[1]))) {
      if (polished) break;
      polished = true;
    }
    for (int r = 0; r < m - 1; ++r) {
      if (t < npairs) jacobi_pair(a, ld, t, r, m, n, S.cs, S.pr, S.part);
      __syncthreads();
      const double2 ri = own ? S.cs[i] : make_double2(1.0, 0.0);
      const int pir = own ? S.part[i] : 0;
      // threads that own no row read (and discard) row 0: every address
      // stays inside the n x ld matrices the caller sized
      const int row = own ? i : 0;
      for (int ch = 0; ch < nchunks; ++ch) {
        const int k0 = kb + ch * kWideCH;
        const bool act = k0 < ke;
        double na[kWideCH], nb[kWideCH], nv[kWideCH], nw[kWideCH];
        int jj[kWideCH], qq[kWideCH];
        if (act) {
#pragma unroll
          for (int u = 0; u < kWideCH; ++u) {
            const int k = min(k0 + u, ke - 1);
            const int2 jq = S.pr[k];
            const int j = jq.x, pj = jq.y;
            jj[u] = j;
            qq[u] = pj;
            const double2 rj = S.cs[j];
            const double2 rq = S.cs[pj];
            const double aij = a[row * ld + j];
            const double aiq = a[row * ld + pj];
            const double apj = a[pir * ld + j];
            const double apq = a[pir * ld + pj];
            const double vij = v[row * ld + j];
            const double viq = v[row * ld + pj];
            // row rotation then column rotation, summed symmetrically
            const double r_j = ri.x * aij + ri.y * apj;
            const double r_q = ri.x * aiq + ri.y * apq;
            na[u] = rj.x * r_j + rj.y * r_q;
            nb[u] = rq.x * r_q + rq.y * r_j;
            nv[u] = rj.x * vij + rj.y * viq;
            nw[u] = rq.x * viq + rq.y * vij;
          }
        }
        __syncthreads();
        if (act && own) {
#pragma unroll
          for (int u = 0; u < kWideCH; ++u) {
            a[i * ld + jj[u]] = na[u];
            v[i * ld + jj[u]] = nv[u];
            if (qq[u] != jj[u]) {
              a[i * ld + qq[u]] = nb[u];
              v[i * ld + qq[u]] = nw[u];
            }
          }
        }
      }
      __syncthreads();
    }
  }
  return sweep;
}

// In-place Cholesky G = L L^T of the SPD k x k matrix g (lower triangle
// used), then G x = b for two right-hand sides held one element per thread
// (threads < k).  `bc` is LDS scratch of 2 doubles.
__device__ inline void wide_cholesky_solve2(double* g, int k, int ld,
                                            double& b1, double& b2, double* bc) {
#pragma clang fp contract(off)
  const int i = threadIdx.x;
  for (int c = 0; c < k; ++c) {
    const double piv = sqrt(g[c * ld + c]);
    __syncthreads();
    double lic = 0.0;
    if (i > c && i < k) {
      lic = g[i * ld + c] / piv;
      g[i * ld + c] = lic;
    }
    if (i == c) g[c * ld + c] = piv;
    __syncthreads();
    if (i > c && i < k) {
      for (int j = c + 1; j <= i; ++j) g[i * ld + j] -= lic * g[j * ld + c];
    }
    __syncthreads();
  }
  // forward: L y = b
  for (int c = 0; c < k; ++c) {
    if (i == c) {
      const double lcc = g[c * ld + c];
      b1 = b1 / lcc;
      b2 = b2 / lcc;
      bc[0] = b1;
      bc[1] = b2;
    }
    __syncthreads();
    if (i > c && i < k) {
      const double lic = g[i * ld + c];
      b1 -= lic * bc[0];
      b2 -= lic * bc[1];
    }
    __syncthreads();
  }
  // backward: L^T x = y
  for (int c = k - 1; c >= 0; --c) {
    if (i == c) {
      const double lcc = g[c * ld + c];
      b1 = b1 / lcc;
      b2 = b2 / lcc;
      bc[0] = b1;
      bc[1] = b2;
    }
    __syncthreads();
    if (i < c) {
      const double lci = g[c * ld + i];
      b1 -= lci * bc[0];
      b2 -= lci * bc[1];
    }
    __syncthreads();
  }
}

}  // namespace sf
