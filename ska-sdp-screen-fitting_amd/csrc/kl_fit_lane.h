// kl_fit_lane.h -- the lane-per-slot phase fit (kl_fit_lane.hip) and the
// work list it shares with the pass kernel (kl_fit_fast.hip).
//
// A slot that enters pass 0 with every direction unflagged and one weight
// (class kClassLane, kl_classify_kernel) is fitted by one LANE: a wavefront
// takes 64 consecutive slots, the number of directions is a compile-time
// constant and the slot's component vectors live in registers.  The lane restates
// fit_once<false, 2, true> for the full basis, the outlier test and the
// order walk's first step sum for sum, so it writes the bits the pass kernel
// writes; a slot it cannot finish that way (the walk moves, a phase is not
// finite) goes back to the pass kernel through the work list, untouched.
#pragma once

#include <cstdint>

#include "sf_internal.h"

namespace sf {

constexpr uint8_t kClassFast = 0, kClassSkipped = 1, kClassSlow = 2, kClassLane = 3;

// directions the lane kernel is instantiated for: D = 24 is the first whose
// component vectors do not fit the 256 VGPRs of two waves per SIMD (12 bytes
// of scratch per lane, 36 at 25, 76 at 26)
constexpr int kLaneMinD = 3;
constexpr int kLaneMaxD = 23;

// A work-list entry: the slot and the first pass the pass kernel owes it
constexpr int kListPassShift = 56;
__host__ __device__ inline long long list_entry(int64_t s, int first) {
  return (long long)s | ((long long)first << kListPassShift);
}
__host__ __device__ inline int64_t list_slot(long long e) {
  return (int64_t)(e & ((1ll << kListPassShift) - 1));
}
__host__ __device__ inline int list_first(long long e) {
  return (int)(e >> kListPassShift);
}

// Does the lane kernel serve this fit?  (The half-wave sums it restates are
// those of the two-slot pass, so SF_OPT_FIT_PACK = 0 keeps it off.)
inline bool fit_lane_applies(const sf_ctx* ctx, const sf_fit_params* p) {
  return ctx->fit_lane && ctx->fit_pack && !ctx->wide &&
         p->screen_type == SF_SCREEN_PHASE && ctx->D >= kLaneMinD &&
         ctx->D <= kLaneMaxD;
}

// passes 0 .. niter - 1 of every class-kClassLane slot (after pass 0's
// number_and_decompose, before pass 0's pass kernel)
int launch_fit_lane(sf_ctx* ctx, const sf_fit_params* p, const RefSpec& r,
                    int64_t S, int A, const double* phase, double* coef,
                    double* resid, float* w_out, int32_t* order_out);

}  // namespace sf
