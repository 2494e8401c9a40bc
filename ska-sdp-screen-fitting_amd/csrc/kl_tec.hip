// kl_tec.hip -- TEC screens to Jones cubes at many channels (sf_kl_eval_tec).
//
// The phase of a TEC screen at frequency nu is kappa * dTEC / nu, so the
// pixel values of all F output channels of one (time, station) differ by a
// scalar only: per slot s = t * A + a and pixel p
//     tec[s][p] = sum_d Cpix[p][d] * tec_coef[t][i][a][d]            (TECU)
//     ph [s][p] = sum_d Cpix[p][d] * phase_coef[t][i][a][d] / 2 pi   (turns)
//     out[t][f][a][.][p] = (cos, sin, cos, sin)(2 pi (tec * k_f + ph))
// for every channel f that takes its screens from TEC frequency i, k_f =
// rad_per_tecu[f] / 2 pi.  The fp64 contraction runs ONCE per slot and the
// channels pay the epilogue only: the MFMA work of an F-channel cube is 1 / F
// of what sf_kl_eval spends on the replicated, pre-scaled coefficients.
//
// A third sibling of kl_eval_wide.hip and kl_values.hip, one kernel for
// 1 <= D <= SF_MAX_EVAL_DIR, on their shape:
//   * the 4 waves of a workgroup share ONE 64-pixel wave block, whose Cpix
//     fragments (ctx->d_cfrag, [kstep][tile][lane]) sit in LDS, the k-step
//     count rounded up to a multiple of 2 with zero fragments, and take the
//     item's 16-slot groups round-robin;
//   * one launch serves one TEC frequency i: a group is 16 consecutive slots
//     s = t * A + a of it, the coefficient row of slot s is
//     ((t * F_tec + i) * A + a) * D (the launcher folds i into the base
//     pointer), and the launch's channels are a list (index f, scale k_f) in a
//     context-owned device buffer, read with wave-uniform (scalar) loads;
//   * the contraction is rt_contract (kl_eval_rt.h) with NSET = 1 (TEC, no
//     scale) or 2 (plus the phase, scaled to turns as the wide kernel does):
//     only the 4 or 8 accumulator tiles stay in registers across the k-loop
//     and then across the channel loop -- in VGPRs: the unit is built with the
//     VGPR form of the MFMAs (csrc/Makefile).  Both loops of this kernel are
//     run-time loops; AGPR accumulators are copied to VGPRs and back on every
//     trip of the k-loop (kl_values.hip measured that), and the channel loop
//     reads every accumulator register with the VALU, F times;
//   * per channel: rev = acc_tec * k_f (+ acc_ph), one fp64 multiply (and add)
//     on the contracted value, then jones_row (the exact reduction in
//     revolutions), byte swap, float4 stores (trash block for dead rows) or
//     scalar stores for odd grids / unaligned output, to output slot
//     (t * F + f) * A + a.  t and a of the lane's 4 accumulator rows are
//     computed once per group.
// No ring, no checksums.

#include "kl_eval_rt.h"

namespace sf {

// k-steps per trip of the contraction loop: the value kernel's 2 (the zero
// k-steps of the last trip are real MFMAs, which a one-channel call pays in
// full)
constexpr int kTecKC = 2;

template <bool VEC4, bool FAST, bool NT, bool PH>
__global__ __launch_bounds__(64 * kEvalWaves) void kl_tec_kernel(
    const double* __restrict__ cfrag, const double* __restrict__ tec,
    const double* __restrict__ phase, int D, int ks, int ks_pad, unsigned S,
    unsigned A, int64_t row_stride, int64_t out_stride, int64_t P, int64_t n_pb,
    int64_t n_sc, int chunk_groups, const int* __restrict__ ch_f,
    const double* __restrict__ ch_k, int n_ch, float* __restrict__ out,
    unsigned flags, float* __restrict__ trash) {
  extern __shared__ double tec_bsh[];  // [ks_pad][kTiles][64]
  constexpr int NSET = PH ? 2 : 1;
  const int l = threadIdx.x & 63;
  // wave index, wave-uniform: keeps the group arithmetic on the SALU
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_frag = ks * kTiles * 64;          // Cpix doubles of a wave block
  const int n_frag_pad = ks_pad * kTiles * 64;  // with the zero k-steps
  const bool scrub = flags & SF_EVAL_NAN_SCRUB;
  const bool be = flags & SF_EVAL_BIG_ENDIAN;
  const int dl = l >> 4;
  const int64_t n_blocks = n_pb * n_sc;
  for (int64_t bb = blockIdx.x; bb < n_blocks; bb += gridDim.x) {
    int64_t wpb, sc;
    eval_block(bb, n_pb, n_sc, wpb, sc, flags);
    if (sc >= n_sc) continue;  // uniform per workgroup
    __syncthreads();           // the previous item's reads of the fragments are done
    if (wpb * kWavePix < P) {
      const double* src = cfrag + wpb * n_frag;
      for (int i = threadIdx.x; i < n_frag_pad; i += 64 * kEvalWaves)
        tec_bsh[i] = i < n_frag ? src[i] : 0.0;
    }
    __syncthreads();
    if (wpb * kWavePix >= P) continue;  // uniform per workgroup
    const int64_t p0 = wpb * kWavePix + (int64_t)(l & 15) * kTiles;
    // n_sc counts chunks of chunk_groups 16-slot groups (S < 2^31: the launcher)
    const int64_t slot_base = sc * (int64_t)chunk_groups * 16;
    for (int g = w; g < chunk_groups; g += kEvalWaves) {
      const int64_t s0l = slot_base + (int64_t)g * 16;
      if (s0l >= S) break;
      const unsigned s0 = (unsigned)s0l;
      // ---- contraction: 16 slots x the block's 64 pixels
      const unsigned sa = s0 + (l & 15);
      const bool srow = sa < S;
      const unsigned sc_ = srow ? sa : S - 1;
      const unsigned ta = sc_ / A;
      const int64_t roff = ((int64_t)ta * row_stride + (sc_ - ta * A)) * D;
      const double* const rows[kMaxSets] = {tec + roff, PH ? phase + roff : nullptr, nullptr};
      v4d acc[NSET][kTiles];  // TEC in TECU, phase in turns
      rt_contract<kTecKC, kTiles, NSET>(
          acc, rows, srow, D, ks_pad, dl,
          [=](int s, double x) { return s == 0 ? x : x * kInv2Pi; },
          [=](int k, int t) { return tec_bsh[(k * kTiles + t) * 64 + l]; });
      // ---- output place of the lane's 4 accumulator rows, channel 0 of the
      // cube: float offset of ((t * F) * A + a) * 4 * P
      int64_t obase[4];
      bool olive[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned s = s0 + acc_row(l, r);
        olive[r] = s < S;
        const unsigned sl = olive[r] ? s : S - 1;
        const unsigned t = sl / A;
        obase[r] = ((int64_t)t * out_stride + (sl - t * A)) * 4 * P;
      }
      // ---- epilogue per channel of this TEC frequency (wave-uniform loop)
#pragma unroll 1
      for (int c = 0; c < n_ch; ++c) {
        const double kf = ch_k[c];
        const int64_t foff = (int64_t)ch_f[c] * A * 4 * P;
        v4d rev[1][kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
          rev[0][t] = acc[0][t] * kf;
          if constexpr (PH) rev[0][t] += acc[1][t];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool live = olive[r] && (!VEC4 || p0 < P);
          float pv[4][kTiles];  // planes Re XX, Im XX, Re YY, Im YY
          jones_row<FAST, false, kTiles>(pv, rev, r, scrub);
          if (be) {
#pragma unroll
            for (int t = 0; t < kTiles; ++t)
#pragma unroll
              for (int q = 0; q < 4; ++q) pv[q][t] = bswapf(pv[q][t]);
          }
          if constexpr (VEC4) {
            // P % 4 == 0: a lane's 4 pixels are all inside the grid or all
            // out; dead rows and pixels store into the context's trash block
            float* o = live ? out + obase[r] + foff + p0 : trash + 4 * l;
            const int64_t qstride = live ? P : 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const v4f v = {pv[q][0], pv[q][1], pv[q][2], pv[q][3]};
              store4<NT>(o + q * qstride, v);
            }
          } else if (live) {
            float* o = out + obase[r] + foff + p0;
#pragma unroll
            for (int t = 0; t < kTiles; ++t) {
              if (p0 + t < P) {
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q * P + t] = pv[q][t];
              }
            }
          }
        }
      }  // channels
    }
  }  // workgroup walk
}

// One launch per TEC frequency that has channels (ctx->tec_used): slots
// s = t * A + a of frequency i, its channels the range tec_off[j] ..
// tec_off[j + 1] of the lists in ctx->d_tec_ch.  A frequency without channels
// is never read.
int launch_eval_tec(sf_ctx* ctx, const double* tec, const double* phase, int64_t T,
                    int A, float* out, unsigned flags) {
  const int ks = ctx->ksteps;
  if (ks < 1 || ks > kEvalWideMaxKS) {
    set_error("sf_kl_eval_tec: unsupported number of directions");
    return SF_EINVAL;
  }
  const int64_t S = T * A;
  const int F = ctx->tec_F, F_tec = ctx->tec_F_tec;
  const BlockWalkLaunch g = block_walk_launch(ctx, kTecKC, S, flags, out);
  const bool fast = flags & SF_EVAL_FAST_SINCOS;
  const int* ch_f = reinterpret_cast<const int*>(ctx->d_tec_ch + F);
  for (size_t j = 0; j < ctx->tec_used.size(); ++j) {
    const int c0 = ctx->tec_off[j], n_ch = ctx->tec_off[j + 1] - c0;
    const int64_t foff = (int64_t)ctx->tec_used[j] * A * ctx->D;
    // 12 variants: NT stores are float4 stores (g.nt implies g.vec4)
    with_bools(
        [&](auto V, auto FS, auto N, auto PHS) {
          constexpr bool v = decltype(V)::value, n = decltype(N)::value;
          if constexpr (v || !n)
            hipLaunchKernelGGL(
                (kl_tec_kernel<v, decltype(FS)::value, n, decltype(PHS)::value>),
                dim3((unsigned)g.nblk), dim3(64 * kEvalWaves), g.lds, ctx->stream,
                ctx->d_cfrag, tec + foff, phase ? phase + foff : nullptr, ctx->D, ks,
                g.ks_pad, (unsigned)S, (unsigned)A, (int64_t)F_tec * A, (int64_t)F * A,
                ctx->n_pix, g.n_wpb, g.n_sc, g.groups, ch_f + c0, ctx->d_tec_ch + c0, n_ch,
                out, g.fl, ctx->d_trash);
        },
        g.vec4, fast, g.nt, phase != nullptr);
    SF_HIP(hipGetLastError());
  }
  return SF_OK;
}

}  // namespace sf
