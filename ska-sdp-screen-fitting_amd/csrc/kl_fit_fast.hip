// kl_fit_fast.hip -- the production KL fit pipeline (gfx950, float64).
//
// Same result as kl_fit_general_kernel (and the reference operator
// stationscreen.run, stationscreen.py:597-782 / 433-594), restructured for
// throughput:
//
//  1. flagged-direction subsets are decomposed ONCE PER UNIQUE FLAG MASK
//     (the reference recomputes _calculate_svd for every slot with a flagged
//     direction, stationscreen.py:495-499): a device hash table maps each
//     64-bit unflagged-mask to an entry of a pool of subset bases (U_sub
//     sorted by |lambda|, lambda), filled by a wavefront Jacobi kernel;
//  2. the least-squares solve runs in the eigenbasis of C.  With
//     C = U Lambda U^T, pinv(C) U_k = U_k Lambda_k^+ and C pinv(C) U_k =
//     U_k (Lambda_k Lambda_k^+), so
//        C re = U_k m(a_c),  a_c = (U_k^T W U_k)^+ U_k^T W cos(phi)
//        white = U Lambda^+ U^T screen,  C white = U (Lambda Lambda^+) U^T screen
//     (m = mask of |lambda| > 1e-3).  No C / pinv(C) mat-vecs remain, and for
//     uniform unflagged weights (the common 0/1 case) U_k^T W U_k = w I;
//  3. slots with a weight in (0, 1.001e-3] -- where the 1e-3 pinv cutoff on
//     U_k^T W U_k can truncate -- are routed to kl_fit_general_kernel, which
//     keeps the reference's exact pinv semantics through a Jacobi solve.
//
// The outlier-flagging iterations become passes over all slots; between
// passes the new masks are inserted, numbered and decomposed.  The steps of a
// slot that every fit kernel takes alike (referencing, chi^2, the order walk,
// the outlier test, the two-direction rule, the truncated eigen-solve) are
// in kl_fit_steps.h, the mask table, the pool of subset bases and the step
// between two passes (number_and_decompose) in kl_fit_pool.h; here, top to
// bottom: classify, fit_once, the pass kernel, the block sigma and flag
// kernels, launch_fit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "kl_fit_lane.h"
#include "kl_fit_pool.h"
#include "kl_fit_steps.h"
#include "sf_internal.h"

namespace sf {

constexpr size_t kLdsBytes = 160 * 1024;   // LDS of one gfx950 CU
constexpr double kTinyW = kPinvAtol * 1.001;  // slow-path threshold on weights

// ---------------------------------------------------------------------------
// 1. classify slots, initialise the per-slot state, insert initial masks.
//    A slot is a group of GW = pow2 >= D lanes (64 / GW slots per wavefront),
//    lane d of the group handles direction d, so every load and store of the
//    [S][D] arrays is contiguous across the wave.
// ---------------------------------------------------------------------------
template <int GW>
__global__ __launch_bounds__(256) void kl_classify_kernel(
    const float* __restrict__ weight, int64_t S, int F, int A, int D,
    const int* __restrict__ st_order, const uint8_t* __restrict__ skip,
    int ref_skip, unsigned long long* __restrict__ keys, int cap,
    int* __restrict__ pos, uint8_t* __restrict__ cls,
    int* __restrict__ counters,
    double* __restrict__ coef, double* __restrict__ resid,
    float* __restrict__ w_out, int32_t* __restrict__ order_out, int lane_fit) {
  constexpr int kPerWave = 64 / GW;
  const int l = lane();
  const int g = l / GW;   // slot group within the wave
  const int d = l % GW;   // direction
  const int64_t s = ((int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64) *
                        kPerWave + g;
  const bool live = s < S && d < D;
  float x = 0.0f;
  if (live) {
    x = weight[s * D + d];
    w_out[s * D + d] = x;
  }
  // the group's unflagged-direction bits and tiny-weight vote
  const unsigned long long bm = __ballot(live && x > 0.0f);
  const unsigned long long bt = __ballot(live && x > 0.0f && (double)x <= kTinyW);
  const unsigned long long gmask = (GW == 64) ? ~0ull : ((1ull << GW) - 1ull);
  const unsigned long long mask = (bm >> (g * GW)) & gmask;
  const bool tiny = ((bt >> (g * GW)) & gmask) != 0ull;
  // unequal positive weights in the slot (U_k^T W U_k != w I): compared with
  // the group's first unflagged weight; zeroing weights (outlier flags) keeps
  // a uniform slot uniform, so one count per fit decides the pass kernel
  const float w_first = __shfl(x, g * GW + (mask ? __builtin_ctzll(mask) : 0));
  const unsigned long long bn = __ballot(live && x > 0.0f && x != w_first);
  const bool nonuniform = ((bn >> (g * GW)) & gmask) != 0ull;
  if (s >= S) return;
  const SlotGeom sg(s, F, A);
  const bool skipped = sg.skipped(skip, ref_skip);
  // zero outputs only where no pass writes them: skipped blocks (class 1);
  // the passes write every other slot (pass 0 starts from zero coefficients
  // and residuals without reading them)
  if (live && skipped) {
    coef[s * D + d] = 0.0;
    resid[s * D + d] = 0.0;
  }
  if (d != 0) return;
  if (skipped) {
    cls[s] = kClassSkipped;
    order_out[s] = 0;
    pos[s] = -2;
    return;
  }
  order_out[s] = st_order[sg.a];
  if (tiny) atomicAdd(counters + kCntSlow, 1);
  else if (nonuniform) atomicAdd(counters + kCntNonUniform, 1);
  // lane_fit (kl_fit_lane.h): no flagged direction and one weight -> a lane
  // of kl_fit_lane_kernel, which also lists the fast-class slots
  const bool to_lane = lane_fit && !tiny && !nonuniform && mask == full_mask(D);
  cls[s] = tiny ? kClassSlow : to_lane ? kClassLane : kClassFast;
  if (mask == full_mask(D)) pos[s] = -1;
  else if (mask == 0ull) pos[s] = -2;
  else pos[s] = table_insert(keys, cap, mask);
}

// ---------------------------------------------------------------------------
// 2. one fit pass (iteration `it` of _process_station) over the slots of one
//    class; one wavefront per slot.  SLOW (class 2: a weight in (0, 1.001e-3])
//    solves U_k^T W U_k by a Jacobi eigen-decomposition with the 1e-3 pinv
//    cutoff; the fast class uses w I (uniform weights) or Cholesky.
// ---------------------------------------------------------------------------
struct FastLds {
  const double* U;    // [D][ld] full basis, columns sorted
  const double* C;    // [D][cld]: LDS, or global for the one-slot pass
  int cld;            // row stride of C
  const double* lam;  // [64]
  double* Vs;         // per wave: subset basis [D][ld]
  double* lams;       // per wave [64]
  double* G;          // per wave [D][ld]
  double* M;          // per wave [D][ld] (SLOW: eigenvectors of G)
  double* vec;        // per wave [6][64]
  double2* cs;        // per wave [64]   (SLOW: Jacobi scratch)
  int2* pr;           // per wave [96]   (SLOW: Jacobi scratch)
  __device__ void jacobi(double* a, double* v, int n, int ld) const {
    wave_jacobi(a, v, cs, pr, n, ld, kJacobiMaxSweeps);
  }
};

// U (and C, except in the one-slot pass, which reads C from L2: at D = 50
// that halves the workgroup's shared LDS so 4 waves per SIMD fit) + lambda
__host__ __device__ inline size_t fast_shared_bytes(int D, bool c_global) {
  return (size_t)((c_global ? 1 : 2) * D * odd_ld(D) + 64) * sizeof(double);
}
__host__ __device__ inline size_t fast_wave_bytes(int D, bool slow, bool lean = false) {
  if (lean) return (size_t)6 * 64 * sizeof(double);  // the vectors only
  return (size_t)((slow ? 3 : 2) * D * odd_ld(D) + 64 + 6 * 64) * sizeof(double) +
         (slow ? 64 * sizeof(double2) + 96 * sizeof(int2) : 0);
}

struct Basis {
  int n;
  bool full;
  int ld;             // row stride of U
  const double* U;    // LDS (full basis, or a copied subset) or the global pool
  const double* lam;
};

// One _fit_screen (stationscreen.py:433-594) in the eigenbasis.  Lanes p < n
// carry the unflagged directions (phi_p, w_p); returns, per DIRECTION lane d,
// white_d and resid_d.
template <bool SLOW, int SPW, bool LEAN>
__device__ void fit_once(const FastLds& L, const Basis& B, int D, int ld,
                         int K, int screen_type, bool uniform, double wu,
                         double phi_p, double w_p, double phi_d, double w_d,
                         double& white_d, double& resid_d) {
#pragma clang fp contract(off)
  using G = Group<SPW>;
  using M = FitMath<!SLOW>;
  // mat-vec loops: four terms' loads in flight, the sums still in order (the
  // same bits); the lean layout only (the general one would spill)
  constexpr int kMatVecUnroll = LEAN ? 4 : 1;
  const int l = G::lane();
  const int n = B.n;
  double* v0 = L.vec;
  double* v1 = L.vec + 64;
  double* v2 = L.vec + 128;
  double* v3 = L.vec + 192;
  double rc = 0.0, rs = 0.0;
  if (l < n) {
    if (screen_type == SF_SCREEN_PHASE) {
      double sn, cn;
      M::sin_cos(phi_p, &sn, &cn);
      rc = w_p * cn;
      rs = w_p * sn;
    } else if (screen_type == SF_SCREEN_AMPLITUDE) {
      rc = w_p * M::lg10(phi_p);
    } else {
      rc = w_p * phi_p;
    }
    v0[l] = rc;
    v1[l] = rs;
    v2[l] = w_p;
  }
  lds_sync();
  // two unflagged directions whose tie passes the cutoff: U_k = e_2
  const Tie2 tie(n, K, v0, v1, v2, B.lam);
  double a1 = 0.0, a2 = 0.0;
  if (l < K) {
#pragma unroll kMatVecUnroll
    for (int p = 0; p < n; ++p) {
      const double u = B.U[p * B.ld + l];
      a1 += u * v0[p];
      a2 += u * v1[p];
    }
  }
  if (K > 0) {
    if (!SLOW && (LEAN || uniform)) {
      // U_k^T (w I) U_k = w I  (U_k orthonormal over the unflagged rows)
      a1 /= wu;
      a2 /= wu;
    } else {
      if (l < K) {
        for (int j = 0; j < K; ++j) {
          double s = 0.0;
          for (int p = 0; p < n; ++p)
            s += B.U[p * B.ld + l] * (v2[p] * B.U[p * B.ld + j]);
          L.G[l * ld + j] = s;
        }
      }
      lds_sync();
      if (!SLOW) {
        wave_cholesky_solve2<SPW>(L.G, K, ld, a1, a2);
      } else {
        truncated_eig_solve(G{}, L, L.G, L.M, K, ld, v0, v1, v2, v3, a1, a2);
      }
    }
  }
  lds_sync();
  // C re = U_k m(a): keep the components whose eigenvalue survives the cutoff
  if (l < K) {
    const bool keep = fabs(B.lam[l]) > kPinvAtol;
    v0[l] = keep ? a1 : 0.0;
    v1[l] = keep ? a2 : 0.0;
  }
  lds_sync();
  double screen = 0.0;
  if (l < n) {
    double cre = 0.0, cim = 0.0;
#pragma unroll kMatVecUnroll
    for (int k = 0; k < K; ++k) {
      const double u = B.U[l * B.ld + k];
      cre += u * v0[k];
      cim += u * v1[k];
    }
    screen = (screen_type == SF_SCREEN_PHASE) ? M::arctan2(cim, cre) : cre;
    if (tie.on) screen = tie.template screen<M>(screen_type, l);
  }
  lds_sync();
  if (l < n) v2[l] = screen;
  lds_sync();
  // s_hat = U^T screen; white = U Lambda^+ s_hat; C white = U (Lambda Lambda^+) s_hat
  if (l < n) {
    double sh = 0.0;
#pragma unroll kMatVecUnroll
    for (int p = 0; p < n; ++p) sh += B.U[p * B.ld + l] * v2[p];
    const double lm = B.lam[l];
    const bool keep = fabs(lm) > kPinvAtol;
    v0[l] = keep ? sh / lm : 0.0;
    v1[l] = keep ? sh : 0.0;
  }
  lds_sync();
  double white = 0.0, cw = 0.0;
  if (l < n) {
#pragma unroll kMatVecUnroll
    for (int r = 0; r < n; ++r) {
      const double u = B.U[l * B.ld + r];
      white += u * v0[r];
      cw += u * v1[r];
    }
  }
  lds_sync();
  if (B.full) {
    white_d = white;
    resid_d = phi_d - model_value<M>(screen_type, cw);
    return;
  }
  // flagged directions (stationscreen.py:565-582): screen from the subset's
  // white coefficients, then re-whitened with the full pinv(C)
  if (l < n) {
    v0[l] = screen;
    v1[l] = white;
  }
  lds_sync();
  const bool unfl = (l < D) && (w_d > 0.0);
  const unsigned long long m = G::ballot(unfl);
  double sall = 0.0;
  if (l < D) {
    if (unfl) {
      const int p = G::rank(m);
      sall = v0[p];
    } else {
      // C[l][idx p]: idx p = p-th set bit of m
      unsigned long long mm = m;
      int p = 0;
      while (mm) {
        const int q = __builtin_ctzll(mm);
        sall += L.C[l * L.cld + q] * v1[p];
        mm &= mm - 1;
        ++p;
      }
    }
  }
  lds_sync();
  if (l < D) v2[l] = sall;
  lds_sync();
  if (l < D) {
    double sh = 0.0;
#pragma unroll kMatVecUnroll
    for (int p = 0; p < D; ++p) sh += L.U[p * ld + l] * v2[p];
    const double lm = L.lam[l];
    v0[l] = fabs(lm) > kPinvAtol ? sh / lm : 0.0;
  }
  lds_sync();
  double wa = 0.0;
  if (l < D)
#pragma unroll kMatVecUnroll
    for (int r = 0; r < D; ++r) wa += L.U[l * ld + r] * v0[r];
  lds_sync();
  white_d = wa;
  resid_d = phi_d - model_value<M>(screen_type, sall);
}

// LEAN (fast class, every slot's unflagged weights equal -- the 0/1 weights
// of the benchmarks): no per-slot G / subset-basis copies in LDS -- a flagged
// slot reads its subset basis straight from the pool (L1/L2) -- so the
// per-slot LDS is the 3 KiB of vectors and 2.7x (D = 20) to 4x (D = 50) more
// waves fit on a CU; the kernel is latency-bound, so occupancy is its speed.
#ifndef SF_FIT_MINW
#define SF_FIT_MINW 4  // waves per SIMD of the two-slot fast pass (128 VGPRs)
#endif
template <bool SLOW, int SPW, bool LEAN>
__global__ __launch_bounds__(256, SLOW ? 1 : SF_FIT_MINW) void kl_fit_pass_kernel(
    int it, int niter, int64_t S, int F, int A, int D,
    const double* __restrict__ phase, const double* __restrict__ refph,
    int ref_sub, const double* __restrict__ g_u, const double* __restrict__ g_c,
    const double* __restrict__ g_eig, const int* __restrict__ st_order,
    const uint8_t* __restrict__ cls, int* __restrict__ pos,
    const int* __restrict__ ids, unsigned long long* __restrict__ keys, int cap,
    const double* __restrict__ pool, int pool_cap, int* __restrict__ counters,
    int screen_type, double nsigma, int adjust_order, double* __restrict__ coef,
    double* __restrict__ resid, float* __restrict__ w_out,
    int32_t* __restrict__ order_out, const long long* __restrict__ list) {
#pragma clang fp contract(off)
  extern __shared__ double smem[];
  const int ld = odd_ld(D);
  using G = Group<SPW>;
  using M = FitMath<!SLOW>;
  const G tm;
  constexpr bool CG = SPW == 1;  // C read from global (L2), not LDS
  const int nwaves = blockDim.x / 64;
  const int nslots = nwaves * SPW;                  // slots in flight per WG
  const int wv = (threadIdx.x / 64) * SPW + G::index();  // slot of the WG
  const int d = G::lane();
  double* sU = smem;
  double* sC = CG ? nullptr : sU + D * ld;
  double* sl = sU + (CG ? 1 : 2) * D * ld;
  for (int e = threadIdx.x; e < D * D; e += blockDim.x) {
    const int r = e / D, c = e % D;
    sU[r * ld + c] = g_u[e];
    if (!CG) sC[r * ld + c] = g_c[e];
  }
  for (int e = threadIdx.x; e < 64; e += blockDim.x) sl[e] = e < D ? g_eig[e] : 0.0;
  __syncthreads();
  FastLds L;
  L.U = sU;
  L.C = CG ? g_c : sC;
  L.cld = CG ? D : ld;
  L.lam = sl;
  double* wb = sl + 64 + (size_t)wv * (fast_wave_bytes(D, SLOW, LEAN) / sizeof(double));
  if (LEAN) {
    L.Vs = L.G = L.M = L.lams = nullptr;
    L.vec = wb;
    L.cs = nullptr;
    L.pr = nullptr;
  } else {
    L.Vs = wb;
    L.G = wb + D * ld;
    L.M = L.G + D * ld;
    L.lams = (SLOW ? L.M + D * ld : L.G + D * ld);
    L.vec = L.lams + 64;
    L.cs = reinterpret_cast<double2*>(L.vec + 6 * 64);
    L.pr = reinterpret_cast<int2*>(L.cs + 64);
  }
  const uint8_t want = SLOW ? 2 : 0;

  // list (kl_fit_lane.h): the fast-class slots of a fit whose other slots
  // the lane kernel took, each with the first pass it is owed; its length is
  // read here, the host never sees it.  Null: every slot.
  const int64_t n_work = list ? (int64_t)counters[kCntList] : S;
  for (int64_t i = (int64_t)blockIdx.x * nslots + wv; i < n_work;
       i += (int64_t)gridDim.x * nslots) {
    int64_t s = i;
    if (list) {
      const long long e = list[i];
      if (list_first(e) > it) continue;
      s = list_slot(e);
    }
    // the slot's independent loads go out together (class, mask position,
    // phases, weights, state): checked one after another they were 4-5
    // serial global round trips per slot, the pass's main cost.  The rare
    // SLOW class tests its class first (it skips almost every slot).
    if (SLOW && cls[s] != want) continue;
    const uint8_t cl = SLOW ? want : cls[s];
    const int a = (int)(s % A);
    const int p0 = pos[s];
    const int64_t base = s * D;
    double phi_d = 0.0, w_d = 0.0, white_d = 0.0, resid_d = 0.0;
    if (d < D) {
      phi_d = phase_ref(phase, refph, ref_sub, s, a, A, D, d);
      w_d = (double)w_out[base + d];
      // pass 0 starts from zero (kl_classify_kernel leaves them unwritten)
      white_d = it == 0 ? 0.0 : coef[base + d];
      resid_d = it == 0 ? 0.0 : resid[base + d];
    }
    double order = (double)order_out[s];
    const double station_order = (double)st_order[a];
    if (cl != want) continue;
    int id = -1;
    if (p0 >= 0) {
      id = ids[p0];
      if (id < 0 || id >= pool_cap) {  // cannot happen: flag it loudly
        if (d == 0) atomicOr(counters + kCntError, kErrLookupMiss);
        continue;
      }
    } else if (p0 == -3) {
      if (d == 0) atomicOr(counters + kCntError, kErrTableFull);
      continue;
    }
    const bool unfl = (d < D) && (w_d > 0.0);
    const unsigned long long um = G::ballot(unfl);
    const int n_unfl = __popcll(um);

    Basis B;
    B.n = n_unfl;
    B.full = (n_unfl == D);
    B.ld = ld;
    if (B.full) {
      B.U = L.U;
      B.lam = L.lam;
    } else if (n_unfl > 0) {
      const double* e = pool + (size_t)id * (D * D + D);
      if (LEAN) {
        B.U = e;
        B.ld = D;
        B.lam = e + D * D;
      } else {
        for (int r = 0; r < n_unfl; ++r)
          if (d < n_unfl) L.Vs[r * ld + d] = e[r * D + d];
        if (d < n_unfl) L.lams[d] = e[D * D + d];
        lds_sync();
        B.U = L.Vs;
        B.lam = L.lams;
      }
    }
    // unflagged directions onto lanes p < n
    double phi_p = 0.0, w_p = 0.0;
    {
      double* v4 = L.vec + 256;
      double* v5 = L.vec + 320;
      if (unfl) {
        const int p = G::rank(um);
        v4[p] = phi_d;
        v5[p] = w_d;
      }
      lds_sync();
      if (d < n_unfl) {
        phi_p = v4[d];
        w_p = v5[d];
      }
      lds_sync();
    }
    const double wmax = G::max(unfl ? w_d : -INFINITY);
    const double wmin = -G::max(unfl ? -w_d : -INFINITY);
    const bool uniform = (wmax == wmin);
    if (LEAN && n_unfl > 0 && !uniform) {  // classify counted none: flag it loudly
      if (d == 0) atomicOr(counters + kCntError, kErrLeanNonUniform);
      continue;
    }

    if (n_unfl > 0) {
      if (order > n_unfl - 1) order = n_unfl - 1;
      if (it == 0) {
        fit_once<SLOW, SPW, LEAN>(L, B, D, ld, (int)order, screen_type, uniform, wmin,
                       phi_p, w_p, phi_d, w_d, white_d, resid_d);
      } else if (adjust_order) {
        OrderWalk walk;
        for (int oi = 0; oi < 4; ++oi) {
          // oi == 0: the weights always compare equal (quirk Q2) -> no fit
          if (oi > 0)
            fit_once<SLOW, SPW, LEAN>(L, B, D, ld, (int)order, screen_type, uniform, wmin,
                           phi_p, w_p, phi_d, w_d, white_d, resid_d);
          if (walk.done()) break;
          const double redchi2 = slot_redchi2<M>(tm, screen_type, d < D, unfl, phi_d,
                                                 w_d, resid_d, n_unfl, order);
          if (walk.template step<M>(oi, redchi2, n_unfl, station_order, order)) break;
        }
      }
    }
    // phase: outlier flagging for the next pass, per slot (the circular
    // sigma is per time across directions, stationscreen.py:303-350);
    // tec / amplitude: one sigma per station block -> kl_block_sigma/flag
    if (it + 1 < niter && screen_type == SF_SCREEN_PHASE) {
      const bool live = d < D;
      if (G::any(live && w_d > 0.0) &&
          G::any(flag_circular_outliers<M>(tm, live, nsigma, resid_d, w_d))) {
        const unsigned long long nm = G::ballot(live && w_d > 0.0);
        if (d == 0) pos[s] = (nm == 0ull) ? -2 : table_insert(keys, cap, nm);
      }
    }
    if (d < D) {
      coef[base + d] = white_d;
      resid[base + d] = resid_d;
      w_out[base + d] = (float)w_d;
    }
    if (d == 0) order_out[s] = (int32_t)order;
  }
}

// 3. tec / amplitude outlier sigma per (station, freq) block
//    (stationscreen.py:338-344: fancy indexing flattens the block, so ONE
//    weighted rms over all its times and directions, quirk Q6)
__global__ __launch_bounds__(256) void kl_block_sigma_kernel(
    int T, int F, int A, int D, const double* __restrict__ phase,
    const double* __restrict__ refph, int ref_sub,
    const uint8_t* __restrict__ skip, int ref_skip, int screen_type,
    const double* __restrict__ resid, const float* __restrict__ w_out,
    double* __restrict__ sigma) {
  __shared__ double red[2][256];
  const int blk = blockIdx.x;  // f * A + a
  const int f = blk / A, a = blk % A;
  double sw = 0.0, swr = 0.0;
  if (!(skip[blk] || a == ref_skip)) {
    for (int e = threadIdx.x; e < T * D; e += blockDim.x) {
      const int t = e / D, d = e % D;
      const int64_t s = ((int64_t)t * F + f) * A + a;
      const double w = (double)w_out[s * D + d];
      if (w > 0.0) {
        const double v = phase_ref(phase, refph, ref_sub, s, a, A, D, d);
        const double sd = screen_diff(screen_type, v, resid[s * D + d]);
        swr += w * (sd * sd);
        sw += w;
      }
    }
  }
  red[0][threadIdx.x] = sw;
  red[1][threadIdx.x] = swr;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) sigma[blk] = sqrt(red[1][0] / red[0][0]);
}

// 4. apply the block sigma: |diff| > nsigma sigma -> weight 0, new mask
__global__ __launch_bounds__(256) void kl_block_flag_kernel(
    int64_t S, int F, int A, int D, const double* __restrict__ phase,
    const double* __restrict__ refph, int ref_sub,
    const uint8_t* __restrict__ cls, int screen_type, double nsigma,
    const double* __restrict__ sigma, const double* __restrict__ resid,
    float* __restrict__ w_out, unsigned long long* __restrict__ keys, int cap,
    int* __restrict__ pos) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S || (cls[s] != 0 && cls[s] != 2)) return;
  const SlotGeom g(s, F, A);  // a skipped slot has class 1
  const int a = g.a;
  const double sig = sigma[g.blk];
  unsigned long long m = 0ull;
  bool changed = false;
  for (int d = 0; d < D; ++d) {
    float w = w_out[s * D + d];
    const double v = phase_ref(phase, refph, ref_sub, s, a, A, D, d);
    const double sd = screen_diff(screen_type, v, resid[s * D + d]);
    if (fabs(sd) > nsigma * sig && w != 0.0f) {
      w = 0.0f;
      w_out[s * D + d] = w;
      changed = true;
    }
    if (w > 0.0f) m |= 1ull << d;
  }
  if (changed) {
    pos[s] = (m == 0ull) ? -2 : (m == full_mask(D) ? -1 : table_insert(keys, cap, m));
  }
}

// ---------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------
// One pass over the slots of one class.  The fast class packs two slots into
// one wavefront (two 32-lane groups) while the directions fit in half a wave:
// D <= 20 leaves 44 of 64 lanes idle otherwise, and the per-slot instruction
// stream is the fit's cost.  lean: no slot has non-uniform weights.
static int launch_pass(sf_ctx* ctx, bool slow, int it, const sf_fit_params* p,
                       const RefSpec& r, int64_t S, int F, int A,
                       const double* phase, double* coef, double* resid,
                       float* w_out, int32_t* order_out, bool lean,
                       const long long* list) {
  const int D = ctx->D;
  const int spw = !slow && D <= 32 && ctx->fit_pack ? 2 : 1;
  lean = !slow && lean && ctx->fit_lean;
  // [slow class, else lean][slots per wave - 1]; the slow class never packs
  // (its two-slot kernel is built, as it always was, and never launched)
  decltype(&kl_fit_pass_kernel<false, 1, false>) const kernels[3][2] = {
      {kl_fit_pass_kernel<false, 1, false>, kl_fit_pass_kernel<false, 2, false>},
      {kl_fit_pass_kernel<false, 1, true>, kl_fit_pass_kernel<false, 2, true>},
      {kl_fit_pass_kernel<true, 1, false>, kl_fit_pass_kernel<true, 2, false>}};
  const auto kernel = kernels[slow ? 2 : lean][spw - 1];
  const size_t shared = fast_shared_bytes(D, spw == 1);
  const size_t slot = fast_wave_bytes(D, slow, lean);  // per-slot LDS scratch
  // waves per workgroup (<= 4): the most resident waves per CU under the
  // 160 KiB LDS of a gfx950 CU (the per-slot subset basis is D^2 doubles,
  // so at D = 50 only 2 waves fit; the smaller workgroup wins ties)
  int nw = 1, best = 0;
  for (int k = 1; k <= 4; ++k) {
    const size_t per_wg = shared + (size_t)k * spw * slot;
    if (per_wg > kLdsBytes) break;
    const int waves = k * (int)(kLdsBytes / per_wg);
    if (waves > best) {
      best = waves;
      nw = k;
    }
  }
  const size_t shm = shared + (size_t)nw * spw * slot;
  SF_TRY(allow_lds(kernel, shm));
  int64_t blocks = (S + nw * spw - 1) / (nw * spw);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64 * nw), shm,
                     ctx->stream, it, p->niter, S, F, A, D, phase, r.refph, r.sub,
                     ctx->d_u, ctx->d_c, ctx->d_eig, ctx->d_st_order, ctx->d_class,
                     ctx->d_pos, ctx->d_ids, ctx->d_keys, (int)ctx->d_keys.size(),
                     ctx->d_pool, (int)ctx->d_pool_mask.size(), ctx->d_counters,
                     p->screen_type, p->nsigma, p->adjust_order, coef, resid, w_out,
                     order_out, list);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

int launch_block_sigma(sf_ctx* ctx, int T, int F, int A, const double* phase,
                       const RefSpec& r, int screen_type, const double* resid,
                       const float* w_out) {
  hipLaunchKernelGGL(kl_block_sigma_kernel, dim3(F * A), dim3(256), 0,
                     ctx->stream, T, F, A, ctx->D, phase, r.refph, r.sub,
                     ctx->d_skip, r.skip, screen_type, resid, w_out,
                     ctx->d_sigma);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

// What every fit launcher needs beside its own tables: the block sigma, the
// counters, and scratch for the outputs the caller does not want (they carry
// the state from pass to pass).
int fit_buffers(sf_ctx* ctx, int64_t S, int F, int A, double** resid,
                float** w_out, int32_t** order_out) {
  const size_t n = (size_t)S * ctx->D;
  if (!*resid) {
    SF_TRY(ctx->d_scratch.reserve(n, kFitAlloc));
    *resid = ctx->d_scratch;
  }
  if (!*w_out) {
    SF_TRY(ctx->d_wscratch.reserve(n, kFitAlloc));
    *w_out = ctx->d_wscratch;
  }
  if (!*order_out) {
    SF_TRY(ctx->d_oscratch.reserve((size_t)S, kFitAlloc));
    *order_out = ctx->d_oscratch;
  }
  SF_TRY(ctx->d_sigma.reserve((size_t)F * A, kFitAlloc));
  SF_TRY(ctx->d_counters.reserve((size_t)kFitCounters, kFitAlloc));
  return SF_OK;
}

int launch_fit(sf_ctx* ctx, const double* phase, const float* weight, int T,
               int F, int A, const sf_fit_params* p, double* coef,
               double* resid, float* w_out, int32_t* order_out) {
  if (ctx->wide)
    return launch_fit_wide(ctx, phase, weight, T, F, A, p, coef, resid, w_out,
                           order_out);
  const int D = ctx->D;
  const int64_t S = (int64_t)T * F * A;
  const RefSpec r = ref_spec(p, A);
  SF_TRY(launch_skip(ctx, phase, weight, T, F, A, r));

  static const char* env = std::getenv("SCREENFIT_FIT");
  if (ctx->force_general || (env && env[0] == 'g')) {
    if (p->screen_type == SF_SCREEN_AMPLITUDE ||
        (p->niter > 1 && p->screen_type != SF_SCREEN_PHASE)) {
      set_error("the general fit kernel handles phase (any niter) and tec (niter 1) only");
      return SF_EINVAL;
    }
    return launch_fit_general(ctx, phase, weight, T, F, A, p, r, coef, resid,
                              w_out, order_out);
  }
  SF_TRY(fit_buffers(ctx, S, F, A, &resid, &w_out, &order_out));
  SF_TRY(reserve_pair(ctx->d_pos, (size_t)S, ctx->d_class, (size_t)S, kFitAlloc));
  // every pass inserts at most one mask per slot
  const size_t tcap = next_pow2((size_t)(2 * p->niter + 2) * (size_t)S + 64, 1);
  SF_TRY(reserve_pair(ctx->d_keys, tcap, ctx->d_ids, tcap, kFitAlloc));
  SF_TRY(ensure_pool(ctx, 1024));
  // (the table may be a larger power of two than tcap: an earlier call's)
  const int cap = (int)ctx->d_keys.size();
  SF_HIP(hipMemsetAsync(ctx->d_keys, 0, cap * sizeof(unsigned long long), ctx->stream));
  SF_HIP(hipMemsetAsync(ctx->d_ids, 0xff, cap * sizeof(int), ctx->stream));
  SF_HIP(hipMemsetAsync(ctx->d_counters, 0, kFitCounters * sizeof(int), ctx->stream));
  // lane-per-slot kernel (kl_fit_lane.h): classify sets its slots aside, the
  // lane kernel lists the others for the fast pass
  const bool lane_fit = fit_lane_applies(ctx, p);
  if (lane_fit) SF_TRY(ctx->d_list.reserve((size_t)S, kFitAlloc));
  long long* const list = lane_fit ? ctx->d_list : nullptr;

  {
    // lane groups of GW >= D lanes per slot, 4 waves per workgroup
    const int gw = D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64;
    const int64_t per_block = 4 * (64 / gw);
    const dim3 grid((unsigned)((S + per_block - 1) / per_block));
    const auto classify = gw == 8    ? kl_classify_kernel<8>
                          : gw == 16 ? kl_classify_kernel<16>
                          : gw == 32 ? kl_classify_kernel<32>
                                     : kl_classify_kernel<64>;
    hipLaunchKernelGGL(classify, grid, dim3(256), 0, ctx->stream, weight, S, F, A, D,
                       ctx->d_st_order, ctx->d_skip, r.skip, ctx->d_keys, cap,
                       ctx->d_pos, ctx->d_class, ctx->d_counters, coef, resid, w_out,
                       order_out, lane_fit ? 1 : 0);
    SF_HIP(hipGetLastError());
  }

  const bool block_flags = p->screen_type != SF_SCREEN_PHASE;
  for (int it = 0; it < p->niter; ++it) {
    int n_slow = 0, n_nonuniform = 0;
    SF_TRY(number_and_decompose(ctx, &n_slow, &n_nonuniform));
    // every pass of the lane slots, where pass 0 starts: the masks of their
    // pass-0 flags enter the table before the next numbering, as the pass
    // kernel's do; the same launch lists the fast-class slots
    if (it == 0 && lane_fit)
      SF_TRY(launch_fit_lane(ctx, p, r, S, A, phase, coef, resid, w_out, order_out));
    SF_TRY(launch_pass(ctx, false, it, p, r, S, F, A, phase, coef, resid, w_out,
                          order_out, n_nonuniform == 0, list));
    if (n_slow > 0)
      SF_TRY(launch_pass(ctx, true, it, p, r, S, F, A, phase, coef, resid, w_out,
                            order_out, false, nullptr));
    if (block_flags && it + 1 < p->niter) {
      SF_TRY(launch_block_sigma(ctx, T, F, A, phase, r, p->screen_type, resid,
                                 w_out));
      hipLaunchKernelGGL(kl_block_flag_kernel, dim3((unsigned)((S + 255) / 256)),
                         dim3(256), 0, ctx->stream, S, F, A, D, phase, r.refph,
                         r.sub, ctx->d_class, p->screen_type, p->nsigma,
                         ctx->d_sigma, resid, w_out, ctx->d_keys, cap,
                         ctx->d_pos);
      SF_HIP(hipGetLastError());
    }
  }
  int err = 0;
  SF_HIP(hipMemcpyAsync(&err, ctx->d_counters + kCntError, sizeof(int),
                        hipMemcpyDeviceToHost, ctx->stream));
  SF_HIP(hipStreamSynchronize(ctx->stream));
  // FitError bits; kErrLeanNonUniform: kl_classify_kernel counted the slot
  // uniform, an internal inconsistency
  SF_REQUIRE((err & (kErrLookupMiss | kErrTableFull)) == 0, SF_EIO,
             "sf_kl_fit: internal mask table overflow");
  SF_REQUIRE((err & kErrLeanNonUniform) == 0, SF_EIO,
             "sf_kl_fit: lean fit pass saw non-uniform weights in a slot "
             "classified uniform (slot left unwritten)");
  SF_REQUIRE((err & kErrFullMaskInPool) == 0, SF_EIO,
             "sf_kl_fit: a mask with every direction unflagged entered the "
             "subset-basis pool (its basis is the global one; left unbuilt)");
  return SF_OK;
}

}  // namespace sf
