// kl_eval_rt.h -- what the evaluation kernels that take the k-step count at
// run time share: the k-loop (kl_eval_wide.hip, kl_values.hip, kl_points.hip),
// the Jones epilogue of one accumulator row (wide, points; pol) and the launch
// geometry of the pixel-block walk (wide, values).  The device parts are
// inlined into the kernel that calls them: each kernel stays in its own unit,
// under that unit's compiler flags (csrc/Makefile).  The functors a kernel
// passes capture by value: a loop variable captured by reference stays in
// memory until late in the pipeline and costs registers (4 VGPRs measured in
// the point kernel).
#pragma once
#include "kl_eval_launch.h"

namespace sf {

constexpr int kMaxSets = 3;  // coefficient sets of a contraction: phase, XX, YY

// The contraction of 16 slots with NT 16-column B tiles over ks_pad k-steps,
// KC per trip (ks_pad % KC == 0), for NSET coefficient sets that share the B
// operand (1, 3 for gain in the order phase, XX, YY, or 2 / 4 for polarized
// phases: phase XX, phase YY, amplitude XX, YY -- kl_eval_pol.hip, whose row
// array has its own length kPolSets: with kMaxSets itself at 4 the code objects
// of kl_tec.o and kl_points.o moved, profiles/README.md).  row[s] is the
// lane's coefficient row (a clamped one when !srow), dl = l >> 4 its
// direction within a k-step, bfrag(k, t) the lane's B fragment of k-step k,
// tile t.  The raw fragments of a trip are unconditional loads of clamped
// addresses (load_coef's reasoning), put into the contraction's units by
// scaled(s, x) -- the identity where there is no scale: no multiply -- and
// masked when used; the next trip's loads are issued before this trip's
// v_mfma_f64_16x16x4_f64 (the last trip reloads its own: no branch).  Only
// the accumulator tiles stay in registers across the loop.
template <int KC, int NT, int NSET, typename Scaled, typename BFrag, int NROW>
__device__ __forceinline__ void rt_contract(v4d (&acc)[NSET][NT],
                                            const double* const (&row)[NROW],
                                            bool srow, int D, int ks_pad, int dl,
                                            Scaled scaled, BFrag bfrag) {
  static_assert(NSET >= 1 && NSET <= NROW, "a row per coefficient set");
#pragma unroll
  for (int s = 0; s < NSET; ++s)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[s][t] = v4d{0.0, 0.0, 0.0, 0.0};
  double raw[NSET][KC];
  auto load_raw = [&](int k0) {
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const int d = 4 * (k0 + j) + dl;
      const int dc = d < D ? d : D - 1;
#pragma unroll
      for (int s = 0; s < NSET; ++s) raw[s][j] = row[s][dc];
    }
  };
  load_raw(0);
#pragma unroll 1
  for (int k0 = 0; k0 < ks_pad; k0 += KC) {
    double a[NSET][KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const bool ok = srow && 4 * (k0 + j) + dl < D;
#pragma unroll
      for (int s = 0; s < NSET; ++s) a[s][j] = keep_if(ok, scaled(s, raw[s][j]));
    }
    load_raw(k0 + KC < ks_pad ? k0 + KC : k0);
#pragma unroll
    for (int j = 0; j < KC; ++j) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const double b = bfrag(k0 + j, t);
#pragma unroll
        for (int s = 0; s < NSET; ++s)
          acc[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][j], b, acc[s][t], 0, 0, 0);
      }
    }
  }
}

// Register r of the accumulators (4 slot rows x the lane's NT columns) as the
// Jones planes pv = Re XX, Im XX, Re YY, Im YY.  FAST: the exact reduction
// rev - rint(rev) (the fixed-point kRevMagic reduction holds only to
// kMagicMaxKS k-steps) and the hardware sincos, else the fp64 sincos; gain:
// 10^x of sets 1, 2.  Phase screens on the fast path scrub the reduced
// argument (cos 1, sin 0), every other the products: v_cmp_u of a PAIR flags
// either being NaN, and the selects run only when some lane of the wave has
// one (a wave-uniform branch).
template <bool FAST, bool GAIN, int NT>
__device__ __forceinline__ void jones_row(float (&pv)[4][NT],
                                          const v4d (&acc)[GAIN ? 3 : 1][NT], int r,
                                          bool scrub) {
  float fr[NT];
  if constexpr (FAST) {
    double rv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) rv[t] = acc[0][t][r];
    rev_reduce_n<NT>(fr, rv, !GAIN && scrub);
  }
  constexpr bool kScrubValues = GAIN || !FAST;
  bool bad = false;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float sn, cs;
    if constexpr (FAST) sincos_rev(fr[t], sn, cs);
    else sincos_rev_f64(acc[0][t][r], sn, cs);
    if constexpr (GAIN) {
      if constexpr (FAST) {
        const float ax = amp2f(acc[1][t][r]);
        const float ay = amp2f(acc[2][t][r]);
        pv[0][t] = ax * cs;
        pv[1][t] = ax * sn;
        pv[2][t] = ay * cs;
        pv[3][t] = ay * sn;
      } else {
        // reference: A (fp64) * cos (fp64), one cast to float32
        const double ax = exp10(acc[1][t][r]);
        const double ay = exp10(acc[2][t][r]);
        pv[0][t] = (float)(ax * (double)cs);
        pv[1][t] = (float)(ax * (double)sn);
        pv[2][t] = (float)(ay * (double)cs);
        pv[3][t] = (float)(ay * (double)sn);
      }
    } else {
      pv[0][t] = pv[2][t] = cs;
      pv[1][t] = pv[3][t] = sn;
    }
    if (kScrubValues)
      bad |= __builtin_isunordered(pv[0][t], pv[1][t]) |
             __builtin_isunordered(pv[2][t], pv[3][t]);
  }
  if (kScrubValues && scrub && __builtin_amdgcn_ballot_w64(bad) != 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (isnan(pv[q][t])) pv[q][t] = (q & 1) ? 0.0f : 1.0f;
  }
}

// jones_row for polarized phases (kl_eval_pol.hip): sets 0 / 1 are the XX / YY
// phases in turns, sets 2 / 3 (GAIN) the XX / YY log-amplitudes.  Per pixel two
// reductions and two sincos, pol p into planes 2 p, 2 p + 1 with jones_row's
// arithmetic, so equal XX and YY phases give jones_row's bits.  The scrub is
// jones_row's too, per plane pair: a NaN of one pol leaves the other's planes
// alone.
template <bool FAST, bool GAIN, int NT>
__device__ __forceinline__ void jones_row_pol(float (&pv)[4][NT],
                                              const v4d (&acc)[GAIN ? 4 : 2][NT], int r,
                                              bool scrub) {
  float fr[2][NT];
  if constexpr (FAST) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      double rv[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) rv[t] = acc[p][t][r];
      rev_reduce_n<NT>(fr[p], rv, !GAIN && scrub);
    }
  }
  constexpr bool kScrubValues = GAIN || !FAST;
  bool bad = false;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float sn, cs;
      if constexpr (FAST) sincos_rev(fr[p][t], sn, cs);
      else sincos_rev_f64(acc[p][t][r], sn, cs);
      if constexpr (GAIN) {
        if constexpr (FAST) {
          const float a = amp2f(acc[2 + p][t][r]);
          pv[2 * p][t] = a * cs;
          pv[2 * p + 1][t] = a * sn;
        } else {
          // reference: A (fp64) * cos (fp64), one cast to float32
          const double a = exp10(acc[2 + p][t][r]);
          pv[2 * p][t] = (float)(a * (double)cs);
          pv[2 * p + 1][t] = (float)(a * (double)sn);
        }
      } else {
        pv[2 * p][t] = cs;
        pv[2 * p + 1][t] = sn;
      }
      if (kScrubValues) bad |= __builtin_isunordered(pv[2 * p][t], pv[2 * p + 1][t]);
    }
  }
  if (kScrubValues && scrub && __builtin_amdgcn_ballot_w64(bad) != 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (isnan(pv[q][t])) pv[q][t] = (q & 1) ? 0.0f : 1.0f;
  }
}

// Launch geometry of the kernels whose workgroups walk (64-pixel block, chunk
// of ring groups) items with the block's Cpix fragments in LDS, for a trip of
// kc k-steps (kl_eval_wide_kernel, kl_values_kernel, kl_eval_pol_kernel)
struct BlockWalkLaunch {
  int ks_pad, groups;
  size_t lds;    // ks_pad x 2 KiB <= 64 KiB
  int64_t n_wpb, n_sc, nblk;
  unsigned fl;   // flags + the XCD map and band bits of eval_block
  bool vec4, nt;
};

// work items: (64-pixel block, chunk of `groups` 16-entry ring groups), the
// ring cut to <= S by the caller, so a ring that does not alias is the plain
// slot-major split.  One launch: past the dispatch limit the workgroups walk
// the items (eval_grid).  float4 stores take P % 4 == 0 and a 16-byte aligned
// output.
inline BlockWalkLaunch block_walk_launch(const sf_ctx* ctx, int kc, int64_t ring,
                                         unsigned flags, const float* out) {
  BlockWalkLaunch g;
  g.ks_pad = (ctx->ksteps + kc - 1) / kc * kc;
  g.lds = (size_t)g.ks_pad * kTiles * 64 * sizeof(double);
  g.n_wpb = ctx->n_pix_blocks * kEvalWaves;
  g.groups = eval_chunk_groups(g.n_wpb, ring, ctx->eval_groups ? ctx->eval_groups : 64, 4096);
  flags &= ~(kEvalXcdInterleave | kEvalBandMask);
  if (ctx->eval_xcd_map > 0) flags |= kEvalXcdInterleave;
  g.fl = flags | eval_band_flags(ctx, g.n_wpb);
  g.vec4 = (ctx->n_pix % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  g.nt = (flags & SF_EVAL_NT_STORES) && g.vec4;
  g.n_sc = eval_chunks(ring, g.groups);
  g.nblk = eval_grid(ctx, g.n_wpb, g.n_sc, 256);
  return g;
}

}  // namespace sf
