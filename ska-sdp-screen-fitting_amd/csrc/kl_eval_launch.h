// kl_eval_launch.h -- host side of the D <= 60 evaluation kernels of
// kl_eval_impl.h: one description of a call (EvalCall), one launch plan per
// kernel family (EvalPlan, the plan_* functions: the only home of the measured
// tuning constants) and one split loop (eval_split); the run-time-bool ->
// template-argument dispatch (with_bools, also used by the wide and value
// launchers) is sf_dispatch.h's.  No kernel lives here.
#pragma once
#include "kl_eval_impl.h"
#include "sf_dispatch.h"

namespace sf {

// One evaluation call as sf_kl_eval* hands it to launch_eval
struct EvalCall {
  sf_ctx* ctx;
  const double *coef, *cxx, *cyy;  // [S_all][D]; cxx / cyy: gain screens only
  int64_t S_all;
  float* out;
  int64_t ring;
  unsigned flags;
  unsigned* sums;  // slot checksums (sf_kl_eval_sums) or null
};

// How one kernel family runs a call
struct EvalPlan {
  int64_t n_items;  // work items along pixels: pixel blocks of the family
  int threads;      // per workgroup
  int groups;       // 16-slot groups per (pixel block, slot chunk) item
  int64_t per;      // slots per launch
  unsigned flags;   // the kernel's flag word: the call's + bands + XCD map
  bool ic;          // integer-digit contraction: digit prepass per launch
};

// One launch of the split loop: slots [b, b + S) of the call
struct EvalStep {
  int64_t b, S, n_sc, nblk;      // n_sc slot chunks, nblk workgroups
  const double *cb, *cxb, *cyb;  // the call's coefficients at slot b
  unsigned* sb;                  // the call's sums at slot b (or null)
  int64_t ring_base;             // b % ring
};

// slot chunks of S slots at `groups` 16-slot groups per chunk
inline int64_t eval_chunks(int64_t S, int groups) {
  return (S + 16 * groups - 1) / (16 * groups);
}

// Grid of an eval launch: one workgroup per (pixel block, slot chunk) up to
// the dispatch limit of 2^32 work-items (kept at 2^31), a multiple of 8 so
// the XCD mapping of eval_block holds for every item a workgroup walks.
inline int64_t eval_grid(const sf_ctx* ctx, int64_t n_pb, int64_t n_sc,
                         int threads) {
  int64_t n = n_pb * n_sc;
  if ((n_pb & 7) == 0) n = ((n + 7) / 8) * 8;
  int64_t cap = ((int64_t)1 << 31) / threads;
  if (ctx->eval_max_blocks > 0 && ctx->eval_max_blocks < cap)
    cap = ctx->eval_max_blocks;
  cap = cap < 8 ? 8 : cap & ~(int64_t)7;
  return n < cap ? n : cap;
}

// 16-slot groups per (pixel block, slot chunk) work item: as many as keep
// >= min_items items (the grid fills the chip), at most max_groups
// (SF_OPT_EVAL_GROUPS, else the family's default).  Every item loads its
// pixel block's Cpix fragments once, so long chunks keep that reload small
// against the item's output: at 512^2 x D = 50 the Cpix of one XCD's pixel
// blocks (13.6 MB) outgrows its 4 MiB L2, and 16 groups per item re-read
// 3.6 TB of it per 8.2 M-slot launch (FETCH_SIZE, 10 % of the writes; 64
// groups: 0.9 TB, +2 %); at 256^2 x D = 20 the slices stay in L2 and 16 groups
// keep each XCD's coefficient rows there too
// (profiles/round2e_eval_groups_ab.txt, round2f_eval_groups_bench.txt).
inline int eval_chunk_groups(int64_t n_pb, int64_t S, int max_groups,
                             int64_t min_items) {
  int groups = max_groups;
  while (groups > 1 && n_pb * eval_chunks(S, groups) < min_items) groups >>= 1;
  return groups;
}

// Slots per launch that keep one workgroup per work item: the dispatch caps
// a grid at 2^31 work-items (eval_grid); past that the workgroups would walk
// several items each, which measured 3-8 % slower than one-shot workgroups
// dispatched in slot order (profiles/round2k_eval_split.txt), so a call
// longer than that is split into consecutive launches.  SF_OPT_EVAL_MAX_BLOCKS
// is the test hook of that walk: with it the call stays one launch, whatever
// its length, so the capped grid really walks.
inline int64_t eval_launch_slots(const sf_ctx* ctx, int64_t n_pb, int groups,
                                 int threads) {
  int64_t cap = ((int64_t)1 << 31) / threads;
  if (ctx->eval_max_blocks > 0) return INT64_MAX;
  const int64_t chunks = cap / n_pb;
  return (chunks < 1 ? 1 : chunks) * 16 * groups;
}

// Slots per launch of the integer contraction: its per-slot digit rows
// (384 B) live in a context buffer of at most this many slots; launches of
// 1 M slots are ~0.7 s at 512^2 x D = 50, so the cut costs no measurable tail
constexpr int64_t kDigChunk = (int64_t)1 << 20;

inline int ensure_kdig(sf_ctx* ctx, int64_t slots) {
  // (hipFree waits for the device, so no reader of the old buffers remains)
  return reserve_pair(ctx->d_kdig, (size_t)slots * kDigits * 64, ctx->d_kflag, (size_t)slots,
                      "sf_kl_eval: hipMalloc of the integer-contraction digits failed");
}

// Prepass of one integer-contraction launch: the digit rows and flags of S
// slots.  The buffers are the context's, so a launch on another stream may
// still be reading them: the prepass waits for the last reader first
// (kdig_read, recorded by kdig_done after every integer launch; on the same
// stream the wait is already satisfied by stream order).
inline int run_kdig(sf_ctx* ctx, const double* cb, int64_t S) {
  if (!ctx->kdig_read)
    SF_HIP(hipEventCreateWithFlags(&ctx->kdig_read, hipEventDisableTiming));
  else
    SF_HIP(hipStreamWaitEvent(ctx->stream, ctx->kdig_read, 0));
  hipLaunchKernelGGL(kl_kdig_kernel<0>, dim3((unsigned)((S + 3) / 4)), dim3(256), 0,
                     ctx->stream, cb, ctx->D, S, kInv2Pi, ctx->d_kdig, ctx->d_kflag);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

// after the launch that read the digits run_kdig wrote
inline int kdig_done(sf_ctx* ctx) {
  SF_HIP(hipEventRecord(ctx->kdig_read, ctx->stream));
  return SF_OK;
}

// digit operands of a launch (IC) or none
template <bool IC>
DigArgs dig_args(const sf_ctx* ctx) {
  DigArgs dg{};
  if (IC) {
    dg.cdig = reinterpret_cast<const v4i*>(ctx->d_cdig.get());
    dg.kdig = ctx->d_kdig;
    dg.kflag = ctx->d_kflag;
  }
  return dg;
}

// The part every plan shares: the family's default group count and min_items
// give `groups`, the dispatch limit gives `per`, cut to whole items of at most
// kDigChunk slots when the integer contraction is on.
inline EvalPlan eval_plan(const EvalCall& c, int64_t n_items, int threads, int def_groups,
                          int64_t min_items, bool ic, unsigned map_flags) {
  const sf_ctx* ctx = c.ctx;
  EvalPlan p;
  p.n_items = n_items;
  p.threads = threads;
  p.groups = eval_chunk_groups(n_items, c.S_all, ctx->eval_groups ? ctx->eval_groups : def_groups,
                               min_items);
  p.per = eval_launch_slots(ctx, n_items, p.groups, threads);
  if (ic) {
    const int64_t gs = 16 * (int64_t)p.groups;
    const int64_t cap = kDigChunk < gs ? gs : (kDigChunk / gs) * gs;
    if (p.per > cap) p.per = cap;
  }
  p.flags = c.flags | map_flags;
  p.ic = ic;
  return p;
}

// Band and XCD-map bits of the register-tile families over n_items pixel
// blocks.  Large grids (>= 1024 blocks of 256 px: 512^2 and up): auto bands
// of 128 x 256 pixels with the XCD-interleaved map -- 512^2 x D = 50 0.706 ->
// 0.732 of 8 TB/s; 2, 4 or 16 bands and the contiguous map measured no better
// (profiles/round2u_eval_bands.txt).  Two families deliberately do not come
// here: the fp64 SHB tile takes SF_OPT_EVAL_BANDS only (plan_shb), and the
// LDS-staged kernels have an XCD rule of their own (plan_lds).
inline unsigned eval_auto_map_flags(const sf_ctx* ctx, int64_t n_items) {
  const int64_t n_pb = ctx->n_pix_blocks;
  const int auto_bands = n_pb >= 1024 ? (int)(n_pb / 128 < 128 ? n_pb / 128 : 128) : 1;
  unsigned fl = eval_band_flags(ctx, n_items, auto_bands);
  if (ctx->eval_xcd_map < 0 && ctx->eval_bands == 0 && auto_bands > 1)
    fl |= kEvalXcdInterleave;
  return fl;
}

// fp64 register tile: 256-pixel blocks.  (64 groups also at 512^2: 8 measured
// 0.725 vs 0.691 of 8 TB/s in tools/eval_variants.py but 0.703 vs 0.714 in
// the config-5 bench step, profiles/round3y_eval_items_512.txt,
// round3ad_c5_fp64_g8.json)
inline EvalPlan plan_tile(const EvalCall& c) {
  const int64_t n_pb = c.ctx->n_pix_blocks;
  return eval_plan(c, n_pb, 256, 64, 2048, false, eval_auto_map_flags(c.ctx, n_pb));
}

// Register tile on the integer-digit contraction: workgroup pixel blocks of
// NWV x 64 pixels (the wave blocks of the Cpix / digit fragments are 64
// pixels either way).  Large grids (>= 1024 blocks of 256 px: 512^2 and up):
// items of 4 groups (the digit fragments are 6 KB per wave block, a quarter
// of the fp64 ones, so short items cost little reload): 512^2 x D = 50 0.691
// (64 groups) -> 0.744 of 8 TB/s, 2 / 8 groups 0.723 / 0.731
// (profiles/round3y_eval_items_512.txt).  Bands / XCD map as the fp64 tile.
template <int NWV>
EvalPlan plan_int_tile(const EvalCall& c) {
  const sf_ctx* ctx = c.ctx;
  const int64_t n_pb = (ctx->n_pix_blocks * kEvalWaves + NWV - 1) / NWV;
  return eval_plan(c, n_pb, 64 * NWV, ctx->n_pix_blocks >= 1024 ? 4 : 64,
                   2048 * kEvalWaves / NWV, true, eval_auto_map_flags(ctx, n_pb));
}

// SHB tile: one workgroup per (64-pixel wave block, chunk).  fp64: chunks of
// 4 x 16 groups, SF_OPT_EVAL_BANDS but neither auto bands nor the auto XCD
// map (deliberately kept as this variant always ran).  Integer contraction:
// 4 groups per wave (the register tile's 4-group items), bands and map as
// that tile.
inline EvalPlan plan_shb(const EvalCall& c, bool ic) {
  const int64_t n_wpb = c.ctx->n_pix_blocks * kEvalWaves;
  return eval_plan(c, n_wpb, 256, ic ? 16 : 64, 4096, ic,
                   ic ? eval_auto_map_flags(c.ctx, n_wpb) : eval_band_flags(c.ctx, n_wpb));
}

// LDS-staged kernels: pixel blocks of the shape's store run.
// Small grids (n_pb <= 64: 256^2 and below, pixel blocks dealt to the XCDs
// interleaved): the shortest items whose Cpix reload (8 x 4 KS bytes per
// pixel) stays <= ~1/3 of their output (16 x 16 g bytes per pixel):
// KS <= 2 -> 1 group, 3-5 -> 2, 6-11 -> 4, else 8.  Measured in the bench
// setting (profiles/round2l_eval_chunks.txt): 256^2 x D = 20 0.72 (16
// groups) -> 0.79 (2 groups) of 8 TB/s, 1 group 0.67; 128^2 x D = 7 0.61
// -> 0.75 (1 group).  Larger grids keep 16 (their Cpix outgrows L2 and the
// long items won at 512^2, round2k_eval_split.txt).
// XCD map (this family's own rule, no auto bands): interleave the pixel
// blocks over the XCDs when each XCD's contiguous eighth would be <= 8 blocks
// (measured: 256^2 at 4 KiB runs +2-3 %, 512^2 -3 %;
// profiles/round1e_eval_xcd_map.txt).
// The integer-digit contraction where it applies (phase screens).
template <int KS, int NW, int TPW, bool GAIN>
EvalPlan plan_lds(const EvalCall& c) {
  const sf_ctx* ctx = c.ctx;
  const int64_t run = EvalLds<NW, TPW, GAIN>::kRun;
  const int64_t n_pb = (ctx->n_pix + run - 1) / run;
  const int def_groups = n_pb > 64 ? 16 : KS <= 2 ? 1 : KS <= 5 ? 2 : KS <= 11 ? 4 : 8;
  const bool ic = !GAIN && eval_int_applies(ctx, false, c.flags,
                                            (reinterpret_cast<uintptr_t>(c.out) & 15) == 0);
  unsigned fl = eval_band_flags(ctx, n_pb);
  if (ctx->eval_xcd_map < 0 && (n_pb & 7) == 0 && n_pb / 8 <= 8) fl |= kEvalXcdInterleave;
  return eval_plan(c, n_pb, 64 * NW, def_groups, 1024, ic, fl);
}

inline EvalStep eval_step(const EvalCall& c, const EvalPlan& p, int64_t b, int64_t S) {
  const int64_t D = c.ctx->D;
  EvalStep s;
  s.b = b;
  s.S = S;
  s.n_sc = eval_chunks(S, p.groups);
  s.nblk = eval_grid(c.ctx, p.n_items, s.n_sc, p.threads);
  s.cb = c.coef + b * D;
  s.cxb = c.cxx ? c.cxx + b * D : nullptr;
  s.cyb = c.cyy ? c.cyy + b * D : nullptr;
  s.sb = c.sums ? c.sums + b : nullptr;
  s.ring_base = b % c.ring;
  return s;
}

// The split loop of every family: launch(step) for consecutive steps of
// plan.per slots, bracketed by the digit prepass and its reader event when
// the plan runs the integer contraction; the first error ends the call.
template <class F>
int eval_split(const EvalCall& c, const EvalPlan& p, F&& launch) {
  sf_ctx* ctx = c.ctx;
  if (p.ic) SF_TRY(ensure_kdig(ctx, c.S_all < p.per ? c.S_all : p.per));
  for (int64_t b = 0; b < c.S_all; b += p.per) {
    const EvalStep s = eval_step(c, p, b, c.S_all - b < p.per ? c.S_all - b : p.per);
    if (p.ic) SF_TRY(run_kdig(ctx, s.cb, s.S));
    launch(s);
    SF_HIP(hipGetLastError());
    if (p.ic) SF_TRY(kdig_done(ctx));
  }
  return SF_OK;
}

// The variants of kl_eval_kernel the library holds (KS = 1..15 each; the
// launchers below reach no other, so no other is compiled):
//   * NT stores are float4 stores: NT only with VEC4;
//   * fp64 register tile, float4 + fast sincos (every hot call): the byte
//     order compiled in (BEM 0 / 1), with direct addressing up to kMagicMaxKS
//     k-steps and without; every other fp64 tile reads the byte order from
//     the flags (BEM 2) and never addresses directly;
//   * fp64 SHB tile: phase screens, float4, BEM 2;
//   * integer-digit contraction (register tile at 4 or 8 waves, SHB tile at
//     4): from 12 k-steps (D >= 45, eval_int_applies), phase screens, float4 +
//     fast sincos, BEM 0 / 1, no direct addressing (measured 2 % slower at
//     D = 50 with fp64, profiles/round3o_eval_direct_ab.txt).
template <int KS, bool V, bool F, bool N, bool G, bool SHB, int BEM, bool DIR, bool IC, int NWV>
constexpr bool tile_variant_exists() {
  if (N && !V) return false;
  if (IC) return KS >= 12 && V && F && !G && BEM != 2 && !DIR && (NWV == kEvalWaves || !SHB);
  if (NWV != kEvalWaves) return false;
  if (SHB) return V && !G && BEM == 2 && !DIR;
  if ((BEM != 2) != (V && F)) return false;
  return !DIR || (V && F && KS <= kMagicMaxKS);
}

// The one launch site of kl_eval_kernel: the slots of `s` (a step of the
// split loop or a part of one)
template <int KS, int MINW, bool V, bool F, bool N, bool G, bool SHB, int BEM, bool DIR,
          bool IC = false, int NWV = kEvalWaves>
void launch_tile(const EvalCall& c, const EvalPlan& p, const EvalStep& s) {
  static_assert(tile_variant_exists<KS, V, F, N, G, SHB, BEM, DIR, IC, NWV>(),
                "not a kl_eval_kernel variant of the library");
  const sf_ctx* ctx = c.ctx;
  hipLaunchKernelGGL((kl_eval_kernel<KS, MINW, V, F, N, G, SHB, BEM, DIR, IC, NWV>),
                     dim3((unsigned)s.nblk), dim3(p.threads), 0, ctx->stream, ctx->d_cfrag,
                     s.cb, s.cxb, s.cyb, ctx->D, s.S, ctx->n_pix, p.n_items, s.n_sc, p.groups,
                     c.out, c.ring, s.ring_base, p.flags, s.sb, ctx->d_trash, ctx->rev_thr,
                     dig_args<IC>(ctx));
}

// fp64 register tile at MINW waves / SIMD
template <int KS, int MINW>
int launch_eval_ks(const EvalCall& c) {
  const EvalPlan p = plan_tile(c);
  const int64_t P = c.ctx->n_pix;
  const bool vec4 = (P % 4 == 0) && ((reinterpret_cast<uintptr_t>(c.out) & 15) == 0);
  const bool fast = c.flags & SF_EVAL_FAST_SINCOS;
  const bool nt = c.flags & SF_EVAL_NT_STORES;
  const bool be = c.flags & SF_EVAL_BIG_ENDIAN;
  return eval_split(c, p, [&](const EvalStep& s) {
    // float4 + fast sincos, 64-pixel blocks inside the grid and a ring of
    // whole 16-slot groups: the direct-addressing kernel over the whole groups
    // of the launch, the general one over a ragged tail (< 16 slots)
    // (up to D = 44: at D = 50 it measured 2 % slower, like the fixed-point
    // reduction -- profiles/round3o_eval_direct_ab.txt)
    const bool direct = KS <= kMagicMaxKS && vec4 && fast && P % kWavePix == 0 &&
                        c.ring % 16 == 0 && s.ring_base % 16 == 0;
    const int64_t S_dir = direct ? (s.S & ~(int64_t)15) : 0;
    with_bools(
        [&](auto V, auto F, auto N, auto G, auto BE) {
          constexpr bool v = decltype(V)::value, f = decltype(F)::value;
          constexpr bool n = decltype(N)::value, g = decltype(G)::value;
          if constexpr (v && f) {
            constexpr int bem = decltype(BE)::value ? 1 : 0;
            if constexpr (KS <= kMagicMaxKS) {
              if (S_dir > 0)
                launch_tile<KS, MINW, v, f, n, g, false, bem, true>(c, p, eval_step(c, p, s.b, S_dir));
            }
            if (s.S > S_dir)
              launch_tile<KS, MINW, v, f, n, g, false, bem, false>(
                  c, p, eval_step(c, p, s.b + S_dir, s.S - S_dir));
          } else if constexpr (!decltype(BE)::value && (v || !n)) {
            launch_tile<KS, MINW, v, f, n, g, false, 2, false>(c, p, s);
          }
        },
        vec4, fast, nt && vec4, c.cxx != nullptr, be && vec4 && fast);
  });
}

// SHB register tile (phase screens, float4-aligned output)
template <int KS>
int launch_eval_shb(const EvalCall& c) {
  const EvalPlan p = plan_shb(c, false);
  return eval_split(c, p, [&](const EvalStep& s) {
    with_bools(
        [&](auto F, auto N) {
          launch_tile<KS, 4, true, decltype(F)::value, decltype(N)::value, false, true, 2, false>(
              c, p, s);
        },
        bool(c.flags & SF_EVAL_FAST_SINCOS), bool(c.flags & SF_EVAL_NT_STORES));
  });
}

// The integer-digit contraction (phase, D >= 45) on the register tile --
// NWV = 4 (256-pixel workgroup blocks) or 8 (512, SF_OPT_EVAL_WG_WAVES), 2
// waves / SIMD -- or on the SHB tile (SF_EVAL_KERNEL_SHB): the 4 waves of a
// workgroup share one 64-pixel block, its pixel digits in LDS, and take its
// 16-slot groups round-robin, 3 waves / SIMD.  KS < 12 never comes here
// (eval_int_applies) and launches nothing.
template <int KS, int NWV, bool SHB>
int launch_eval_int(const EvalCall& c) {
  const EvalPlan p = SHB ? plan_shb(c, true) : plan_int_tile<NWV>(c);
  return eval_split(c, p, [&](const EvalStep& s) {
    with_bools(
        [&](auto N, auto BE) {
          if constexpr (KS >= 12)
            launch_tile<KS, SHB ? 3 : 2, true, true, decltype(N)::value, false, SHB,
                        decltype(BE)::value ? 1 : 0, false, true, NWV>(c, p, s);
        },
        bool(c.flags & SF_EVAL_NT_STORES), bool(c.flags & SF_EVAL_BIG_ENDIAN));
  });
}

// LDS-staged kernels; the integer variant only where it can apply (phase
// screens from 12 k-steps: a plan with ic below that, which eval_int_applies
// never gives, launches nothing)
template <int KS, int NW, int TPW, bool GAIN = false>
int launch_eval_lds(const EvalCall& c) {
  const EvalPlan p = plan_lds<KS, NW, TPW, GAIN>(c);
  const sf_ctx* ctx = c.ctx;
  return eval_split(c, p, [&](const EvalStep& s) {
    with_bools(
        [&](auto N, auto I) {
          constexpr bool ic = decltype(I)::value;
          if constexpr (!ic || (KS >= 12 && !GAIN))
            hipLaunchKernelGGL((kl_eval_lds_kernel<KS, NW, TPW, decltype(N)::value, ic, GAIN>),
                               dim3((unsigned)s.nblk), dim3(p.threads), 0, ctx->stream,
                               ctx->d_cfrag, s.cb, s.cxb, s.cyb, ctx->D, ctx->ksteps, s.S,
                               ctx->n_pix, p.n_items, s.n_sc, p.groups, c.out, c.ring,
                               s.ring_base, p.flags, ctx->eval_sleep, s.sb, ctx->rev_thr,
                               dig_args<ic>(ctx));
        },
        bool(c.flags & SF_EVAL_NT_STORES), p.ic);
  });
}

#define SF_EVAL_PICK_ARGS                                                    \
  sf_ctx* ctx, const double* coef, const double* cxx, const double* cyy,   \
      int64_t S, float* out, int64_t ring, unsigned flags, unsigned* sums

template <int KS>
int launch_eval_pick(SF_EVAL_PICK_ARGS) {
  const EvalCall c{ctx, coef, cxx, cyy, S, out, ring, flags, sums};
  const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int v = pick_eval_kernel(ctx, cxx != nullptr, flags, aligned);
  // the integer-digit contraction: the LDS-staged kernels take it themselves
  // (plan_lds), the register and SHB tiles through launch_eval_int
  if (eval_int_applies(ctx, cxx != nullptr, flags, aligned)) {
    if (v == SF_EVAL_KERNEL_TILE || v == SF_EVAL_KERNEL_TILE3)
      return ctx->eval_wg_waves == 8 ? launch_eval_int<KS, 8, false>(c)
                                     : launch_eval_int<KS, kEvalWaves, false>(c);
    if (v == SF_EVAL_KERNEL_SHB) return launch_eval_int<KS, kEvalWaves, true>(c);
  }
  // gain screens (round 6): the LDS-staged shapes whose three-plane tile
  // fits LDS (pick_eval_kernel maps LDS16 to LDS16H), up to kGainLdsMaxKS
  if (cxx != nullptr) {
    if constexpr (KS <= kGainLdsMaxKS) {
      switch (v) {
        case SF_EVAL_KERNEL_LDS4: return launch_eval_lds<KS, 4, 4, true>(c);
        case SF_EVAL_KERNEL_LDS8: return launch_eval_lds<KS, 8, 4, true>(c);
        case SF_EVAL_KERNEL_LDS8H: return launch_eval_lds<KS, 8, 2, true>(c);
        case SF_EVAL_KERNEL_LDS16H: return launch_eval_lds<KS, 16, 2, true>(c);
        default: break;
      }
    }
    // (pick_eval_kernel gives gain screens no other LDS-staged shape)
    if (v != SF_EVAL_KERNEL_TILE && v != SF_EVAL_KERNEL_TILE3) {
      set_error("sf_kl_eval_gain: no LDS-staged gain kernel for this shape");
      return SF_EINVAL;
    }
  }
  switch (v) {
    case SF_EVAL_KERNEL_LDS4: return launch_eval_lds<KS, 4, 4>(c);
    case SF_EVAL_KERNEL_LDS8: return launch_eval_lds<KS, 8, 4>(c);
    case SF_EVAL_KERNEL_LDS16: return launch_eval_lds<KS, 16, 4>(c);
    case SF_EVAL_KERNEL_LDS8H: return launch_eval_lds<KS, 8, 2>(c);
    case SF_EVAL_KERNEL_LDS16H: return launch_eval_lds<KS, 16, 2>(c);
    case SF_EVAL_KERNEL_SHB: return launch_eval_shb<KS>(c);
    // below 8 k-steps the register tile fits 4 waves/SIMD anyway
    case SF_EVAL_KERNEL_TILE3: return launch_eval_ks<KS, (KS >= 8 ? 3 : 2)>(c);
    default: return launch_eval_ks<KS, 2>(c);
  }
}

#define SF_EVAL_KS_LIST(X) \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)
#define SF_EVAL_EXTERN(k) extern template int launch_eval_pick<k>(SF_EVAL_PICK_ARGS);
#define SF_EVAL_INSTANTIATE(k) template int launch_eval_pick<k>(SF_EVAL_PICK_ARGS);

}  // namespace sf
