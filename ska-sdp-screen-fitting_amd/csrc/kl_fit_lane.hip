// kl_fit_lane.hip -- the lane-per-slot phase fit (gfx950, float64).
//
// kl_fit_pass_kernel<false, 2, true> spends a half-wave on a slot: at D = 20
// 40 of 64 lanes work, every per-slot scalar (hypot, log, sqrt, pow) runs on
// all of them, every sum across directions is a five-step shuffle butterfly
// and a slot crosses about ten LDS ordering points.  Most slots of a phase
// fit need none of that generality: every direction unflagged, one weight.
// Here one LANE fits such a slot (class kClassLane): a wavefront takes 64
// consecutive slots, D is a compile-time constant, the slot's component
// vectors live in registers, U and lambda are wave-uniform (LDS broadcast
// reads) and the sums across directions are in-lane.
//
// Same bits as the pass kernel, by construction:
//  - pass 0 restates fit_once<false, 2, true> for B.full: each of its sums
//    is already serial in one lane there, so the order carries over;
//  - the two cross-lane sums (flag_circular_outliers, slot_redchi2) are
//    Group<2>::sum, an xor butterfly over 32 lanes with offsets 16, 8, 4, 2, 1
//    whose lanes >= D hold +0.0: tree_sum3() is that tree in one lane,
//    additions of +0.0 included;
//  - the transcendentals are the functions FitMath names (inlined);
//  - a later pass is taken only while it needs no fit: where the order walk
//    moves at its first step, or a referenced phase is not finite (NaN
//    payloads depend on the butterfly's operand order), the slot's state is
//    left as the previous pass left it, its class goes back to kClassFast
//    and it joins the pass kernel's work list from that pass on.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kl_fit_lane.h"
#include "kl_fit_masks.h"
#include "kl_fit_steps.h"
#include "sf_internal.h"

#pragma clang fp contract(off)

namespace sf {

// the transcendentals inlined (kl_fit_steps.h: the same bits as called); each
// stands once in a loop over the directions that is NOT unrolled, see below
using LaneMath = FitMath<false>;

// Code size and registers decide this kernel's shape.  Fully unrolled over
// the directions (every vector in registers) it is ~150 KiB of straight-line
// code with 4 D inlined transcendentals whose constants alone hold ~130 VGPRs:
// at D = 20 it spilled.  So every loop over the directions p that holds a
// transcendental or a row of U is a real loop (`unroll 1`; 24 KiB of code at
// D = 20): what it indexes by p lives in LDS (the slot's vector X,
// column-major so a lane's element p is X[p][lane]; the rows of U), what it
// indexes by the component k in registers, with the k loops unrolled inside
// the body.

// Group<2>::sum of three series at once: leaf(p, v) gives the three terms of
// direction p < D; the lanes D .. 31 of the half-wave hold +0.0.  The
// butterfly's lane 0 adds lanes 16 apart, then the results 8 apart, 4, 2, 1
// (a + b == b + a: every lane ends with its bits).  The same tree depth
// first: five nested two-trip loops, bit 4 of p innermost, each level adding
// its second subtree to its first; one copy of the leaf's code.
template <int D, class Leaf>
__device__ __forceinline__ void tree_sum3(double (&out)[3], Leaf leaf) {
  static_assert(D <= 32, "a half-wave of directions");
  double t5[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
  for (int b0 = 0; b0 < 2; ++b0) {
    double t4[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int b1 = 0; b1 < 2; ++b1) {
      double t3[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
      for (int b2 = 0; b2 < 2; ++b2) {
        double t2[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
        for (int b3 = 0; b3 < 2; ++b3) {
          double t1[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
          for (int b4 = 0; b4 < 2; ++b4) {
            const int p = b0 + 2 * b1 + 4 * b2 + 8 * b3 + 16 * b4;
            double x[3] = {0.0, 0.0, 0.0};
            if (p < D) leaf(p, x);
#pragma unroll
            for (int k = 0; k < 3; ++k) t1[k] = b4 == 0 ? x[k] : t1[k] + x[k];
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) t2[k] = b3 == 0 ? t1[k] : t2[k] + t1[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) t3[k] = b2 == 0 ? t2[k] : t3[k] + t2[k];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) t4[k] = b1 == 0 ? t3[k] : t4[k] + t3[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) t5[k] = b0 == 0 ? t4[k] : t5[k] + t4[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = t5[k];
}

// rows (slots) of the wave's block whose bit is set in `rows`, from X to dst:
// consecutive lanes, consecutive addresses
template <int D, int LDX, class T>
__device__ __forceinline__ void store_rows(T* dst, const double* X, int n_elem,
                                           unsigned long long rows) {
  for (int e = lane(); e < n_elem; e += 64) {
    const int r = e / D, d = e % D;
    if ((rows >> r) & 1ull) dst[e] = (T)X[d * LDX + r];
  }
}

// The pass kernel's work list and the lane slots' count, after classify: a
// wavefront takes kGroups x 64 slots, its fast-class ones join the list, its
// lane-class ones are counted -- one 64-bit atomic for both (a single address
// takes ~5 ns per atomic: one per two slots, from the classify kernel, cost
// config 4 45 ms).
constexpr int kGroups = 16;
__global__ __launch_bounds__(256) void kl_lane_list_kernel(
    const uint8_t* __restrict__ cls, int64_t S, int* __restrict__ counters,
    long long* __restrict__ list) {
  const int l = lane();
  const int64_t sb = ((int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64) *
                     (64 * kGroups);
  if (sb >= S) return;
  int my_at[kGroups];  // this lane's slot of group g: its place in the list
  int n_fast = 0, n_lane = 0;
#pragma unroll
  for (int g = 0; g < kGroups; ++g) {
    const int64_t sg = sb + g * 64 + l;
    const uint8_t c = sg < S ? cls[sg] : kClassSkipped;
    const unsigned long long fast_rows = __ballot(c == kClassFast);
    my_at[g] = c == kClassFast ? n_fast + Group<1>::rank(fast_rows) : -1;
    n_fast += __popcll(fast_rows);
    n_lane += __popcll(__ballot(c == kClassLane));
  }
  unsigned long long old = 0ull;
  if (l == 0 && (n_fast | n_lane) != 0)
    old = atomicAdd(reinterpret_cast<unsigned long long*>(counters + kCntLane),
                    (unsigned long long)n_lane | ((unsigned long long)n_fast << 32));
  const int base = (int)(__shfl(old, 0) >> 32);
#pragma unroll
  for (int g = 0; g < kGroups; ++g)
    if (my_at[g] >= 0) list[base + my_at[g]] = list_entry(sb + g * 64 + l, 0);
}

template <int D>
__global__ __launch_bounds__(64, 2) void kl_fit_lane_kernel(
    int niter, int64_t S, int A, const double* __restrict__ phase,
    const double* __restrict__ refph, int ref_sub,
    const double* __restrict__ g_u, const double* __restrict__ g_eig,
    const int* __restrict__ st_order, uint8_t* __restrict__ cls,
    int* __restrict__ pos, unsigned long long* __restrict__ keys, int cap,
    int* __restrict__ counters, long long* __restrict__ list, double nsigma,
    int adjust_order, double* __restrict__ coef, double* __restrict__ resid,
    float* __restrict__ w_out, int32_t* __restrict__ order_out) {
  // X[p][lane], row stride 65: a lane's walk over p and the block's walk
  // over (slot, p) in memory order both spread over the banks
  constexpr int LDX = 65;
  __shared__ double X[D * LDX];
  __shared__ double sU[D * D + D];  // U by rows, then lambda
  __shared__ long long row_tf[64];
  __shared__ int row_a[64];
  const int l = lane();
  const int64_t s0 = (int64_t)blockIdx.x * 64;
  const int64_t s = s0 + l;
  const bool mine = s < S && cls[s] == kClassLane;
  if (__ballot(mine) == 0ull) return;
  const int n_elem = (int)(S - s0 < 64 ? S - s0 : 64) * D;
  const int a = (int)(s % A);
  const double* sLam = sU + D * D;
  for (int e = l; e < D * D; e += 64) sU[e] = g_u[e];
  if (l < D) sU[D * D + l] = g_eig[l];
  row_a[l] = a;
  row_tf[l] = (long long)(s / A);
  lds_sync();
  // referenced phases (phase_ref) of the 64 slots, coalesced, into X
  for (int e = l; e < n_elem; e += 64) {
    const int r = e / D, d = e % D;
    double v = phase[s0 * D + e];
    if (refph) v -= refph[row_tf[r] * D + d];
    else if (ref_sub >= 0) v -= phase[(s0 + r + (ref_sub - row_a[r])) * D + d];
    X[d * LDX + r] = v;
  }
  lds_sync();
  double* x = X + l;  // this lane's element p: x[p * LDX]

  bool run = mine;
  int defer = -1;  // first pass the pass kernel owes this slot
  if (run) {
    bool finite = true;
#pragma unroll 1
    for (int p = 0; p < D; ++p) finite = finite && __builtin_isfinite(x[p * LDX]);
    if (!finite) {
      defer = 0;
      run = false;
    }
  }
  const bool fitted = run;
  const double wu = mine ? (double)w_out[s * D] : 1.0;
  const double station_order = mine ? (double)st_order[a] : 0.0;
  double order = station_order;

  if (run) {
    // ---- pass 0: fit_once<false, 2, true>, B.full, n = D.  Every sum adds
    // its terms in the pass kernel's order (p, k or r ascending).
    if (order > D - 1) order = D - 1;
    const int K = (int)order;
    double v0[D], v1[D];
#pragma unroll
    for (int k = 0; k < D; ++k) v0[k] = v1[k] = 0.0;
#pragma unroll 1
    for (int p = 0; p < D; ++p) {
      double sn, cn;
      LaneMath::sin_cos(x[p * LDX], &sn, &cn);
      const double rc = wu * cn;
      const double rs = wu * sn;
      const double* ur = sU + p * D;
#pragma unroll
      for (int k = 0; k < D - 1; ++k) {
        const double u = ur[k];
        v0[k] += u * rc;
        v1[k] += u * rs;
      }
    }
    // the pass kernel's lanes l >= K compute no component and its sums run
    // over k < K.  Here the components k >= K are +0.0 and the sums run over
    // every k: a sum that starts from +0.0 is never -0.0 (x + y is -0.0 only
    // for x = y = -0.0), so adding U[p][k] * 0.0 = +-0.0 (U is finite) leaves
    // its bits alone
#pragma unroll
    for (int k = 0; k < D - 1; ++k) {
      const bool keep = k < K && fabs(sLam[k]) > kPinvAtol;
      v0[k] = keep ? v0[k] / wu : 0.0;
      v1[k] = keep ? v1[k] / wu : 0.0;
    }
    double sh[D];
#pragma unroll
    for (int k = 0; k < D; ++k) sh[k] = 0.0;
#pragma unroll 1
    for (int p = 0; p < D; ++p) {
      const double* ur = sU + p * D;
      double re = 0.0, im = 0.0;
#pragma unroll
      for (int k = 0; k < D - 1; ++k) {
        const double u = ur[k];
        re += u * v0[k];
        im += u * v1[k];
      }
      const double screen = LaneMath::arctan2(im, re);
#pragma unroll
      for (int k = 0; k < D; ++k) sh[k] += ur[k] * screen;
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double lm = sLam[k];
      const bool keep = fabs(lm) > kPinvAtol;
      v0[k] = keep ? sh[k] / lm : 0.0;
      v1[k] = keep ? sh[k] : 0.0;
    }
    // white straight to the slot's row of coef, 16 bytes a store: a lane
    // completes its own lines over the loop; the residual replaces the phase
    double* crow = coef + s * D;
#pragma unroll 1
    for (int p = 0; p < D; p += 2) {
      double wh[2] = {0.0, 0.0}, cw[2] = {0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (p + q < D) {
          const double* ur = sU + (p + q) * D;
#pragma unroll
          for (int r = 0; r < D; ++r) {
            const double u = ur[r];
            wh[q] += u * v0[r];
            cw[q] += u * v1[r];
          }
          x[(p + q) * LDX] = x[(p + q) * LDX] - cw[q];
        }
      }
      if (p + 1 < D) {
        __builtin_memcpy(crow + p, wh, 16);
      } else {
        crow[p] = wh[0];
      }
    }
  }

  // residuals out, coalesced; X keeps them for the later passes
  lds_sync();
  store_rows<D, LDX>(resid + s0 * D, X, n_elem, __ballot(fitted));
  lds_sync();

  // ---- the outlier test of every pass and the later passes' order step
  constexpr unsigned kFull = D == 32 ? ~0u : (1u << D) - 1u;
  unsigned um = kFull;  // unflagged directions: weight wu, the others 0
  bool alive = run;
  for (int it = 0; it < niter; ++it) {
    if (__ballot(alive) == 0ull) break;
    if (alive && it > 0) {
      const int n_unfl = __popc(um);
      double o = order;
      if (o > n_unfl - 1) o = n_unfl - 1;
      if (adjust_order) {
        // slot_redchi2 (phase) on the post-flag weights
        double r[3];
        tree_sum3<D>(r, [&](int p, double(&v)[3]) {
          const bool unfl = (um >> p) & 1u;
          double sn = 0.0, cn = 0.0;
          if (unfl) LaneMath::sin_cos(x[p * LDX], &sn, &cn);
          const double ww = unfl ? wu : 0.0;
          v[0] = ww;
          v[1] = sn * sn * ww;
          v[2] = cn * cn * ww;
        });
        const double m1 = r[1] / r[0];
        const double m2 = r[2] / r[0];
        const double redchi2 = (1.0 - hypot(m1, m2)) * r[0] / (n_unfl - o);
        OrderWalk walk;
        double moved = o;
        if (!walk.template step<LaneMath>(0, redchi2, n_unfl, station_order, moved)) {
          // the walk moves: the slot needs a fit -- hand it back as pass
          // it - 1 left it
          defer = it;
          alive = false;
        }
      }
      if (alive) order = o;
    }
    if (alive && it + 1 < niter) {
      // flag_circular_outliers
      const auto wrapped = [&](int p) {
        double r = LaneMath::mod(x[p * LDX], 2.0 * M_PI);
        if (r < -M_PI) r += 2.0 * M_PI;
        if (r > M_PI) r -= 2.0 * M_PI;
        return r;
      };
      double t[3];
      tree_sum3<D>(t, [&](int p, double(&v)[3]) {
        const double r = wrapped(p);
        const bool inc = ((um >> p) & 1u) && !isnan(r);
        double sn = 0.0, cn = 0.0;
        if (inc) LaneMath::sin_cos(r, &sn, &cn);
        v[0] = inc ? 1.0 : 0.0;
        v[1] = sn;
        v[2] = cn;
      });
      const double ms = t[1] / t[0];
      const double mc = t[2] / t[0];
      const double stdv = sqrt(-2.0 * LaneMath::ln(hypot(ms, mc)));
      const double thr = nsigma * stdv;
      unsigned outl = 0u;
#pragma unroll 1
      for (int p = 0; p < D; ++p)
        if (fabs(wrapped(p)) > thr) outl |= 1u << p;
      if (outl) {
        um &= ~outl;
        int np = -2;
        if (um != 0u) {
          np = table_insert(keys, cap, (unsigned long long)um);
          if (np == -3) atomicOr(counters + kCntError, kErrTableFull);
        }
        pos[s] = np;
        if (um == 0u) alive = false;  // nothing left to fit or flag
      }
    }
  }

  // ---- weights of the slots that lost a direction, the order, the hand-back
  lds_sync();
  const bool lost = fitted && um != kFull;
  if (lost) {
#pragma unroll 1
    for (int p = 0; p < D; ++p) x[p * LDX] = ((um >> p) & 1u) ? wu : 0.0;
  }
  lds_sync();
  store_rows<D, LDX>(w_out + s0 * D, X, n_elem, __ballot(lost));
  if (fitted) order_out[s] = (int32_t)order;
  const int dat = number_fresh(defer >= 0, counters + kCntList);
  if (defer >= 0) {
    cls[s] = kClassFast;
    list[dat] = list_entry(s, defer);
  }
  const unsigned long long nd = __ballot(defer >= 0);
  if (l == 0 && nd != 0ull) atomicAdd(counters + kCntLaneDeferred, __popcll(nd));
}

template <int D>
static void launch_lane(sf_ctx* ctx, const sf_fit_params* p, const RefSpec& r,
                        int64_t S, int A, const double* phase, double* coef,
                        double* resid, float* w_out, int32_t* order_out) {
  hipLaunchKernelGGL(kl_fit_lane_kernel<D>, dim3((unsigned)((S + 63) / 64)), dim3(64), 0,
                     ctx->stream, p->niter, S, A, phase, r.refph, r.sub, ctx->d_u,
                     ctx->d_eig, ctx->d_st_order, ctx->d_class, ctx->d_pos, ctx->d_keys,
                     (int)ctx->d_keys.size(), ctx->d_counters, ctx->d_list, p->nsigma,
                     p->adjust_order, coef, resid, w_out, order_out);
}

int launch_fit_lane(sf_ctx* ctx, const sf_fit_params* p, const RefSpec& r,
                    int64_t S, int A, const double* phase, double* coef,
                    double* resid, float* w_out, int32_t* order_out) {
  const int64_t per_block = 4 * 64 * kGroups;
  hipLaunchKernelGGL(kl_lane_list_kernel, dim3((unsigned)((S + per_block - 1) / per_block)),
                     dim3(256), 0, ctx->stream, ctx->d_class, S, ctx->d_counters,
                     ctx->d_list);
  SF_HIP(hipGetLastError());
#define SF_LANE_CASE(d)                                                        \
  case d:                                                                      \
    launch_lane<d>(ctx, p, r, S, A, phase, coef, resid, w_out, order_out);     \
    break;
  switch (ctx->D) {
    SF_LANE_CASE(3) SF_LANE_CASE(4) SF_LANE_CASE(5) SF_LANE_CASE(6)
    SF_LANE_CASE(7) SF_LANE_CASE(8) SF_LANE_CASE(9) SF_LANE_CASE(10)
    SF_LANE_CASE(11) SF_LANE_CASE(12) SF_LANE_CASE(13) SF_LANE_CASE(14)
    SF_LANE_CASE(15) SF_LANE_CASE(16) SF_LANE_CASE(17) SF_LANE_CASE(18)
    SF_LANE_CASE(19) SF_LANE_CASE(20) SF_LANE_CASE(21) SF_LANE_CASE(22)
    SF_LANE_CASE(23)
    default:
      set_error("sf_kl_fit: no lane kernel for this number of directions");
      return SF_EINVAL;
  }
#undef SF_LANE_CASE
  static_assert(kLaneMinD == 3 && kLaneMaxD == 23, "the cases above");
  SF_HIP(hipGetLastError());
  return SF_OK;
}

}  // namespace sf
