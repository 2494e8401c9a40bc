// kl_eval_pol.hip -- KL screen evaluation with polarized phases
// (sf_kl_eval_pol): the XX and YY Jones terms of a diagonal gain each take
// their own phase screen,
//     out[s % ring][4][ny][nx] = (a_xx cos phi_xx, a_xx sin phi_xx,
//                                 a_yy cos phi_yy, a_yy sin phi_yy),
//     phi_p = sum_d Cpix[.][d] phase_p[s][d],  a_p = 10^(sum_d Cpix amp_p) or 1.
// The reference renders no such table (kl_screen.py:319-378 takes one phase
// per slot); the only other way to this cube is two sf_kl_eval passes and a
// plane copy, i.e. every output byte written twice or more.
//
// One kernel for 1 <= D <= SF_MAX_EVAL_DIR on kl_eval_wide.hip's shape (the
// walk is that kernel's, spelled out here too for kl_values.hip's reason):
//   * the 4 waves of a workgroup share ONE 64-pixel wave block, whose Cpix
//     fragments (ctx->d_cfrag, [kstep][tile][lane]) sit in LDS, the k-step
//     count rounded up to the trip with zero fragments (4..64 KiB of dynamic
//     LDS), and take the item's 16-entry ring groups round-robin;
//   * a group is 16 consecutive ring entries, and the wave that owns it
//     evaluates every slot that lands there in ascending order: with a ring
//     shorter than the call an entry ends up holding its last slot;
//   * the contraction is rt_contract (kl_eval_rt.h) with 2 sets (the XX and
//     YY phases, in turns) or 4 (plus the XX and YY log-amplitudes).  The sets
//     share the B operand: one LDS read of a Cpix fragment feeds the MFMAs of
//     every set, so the LDS traffic per MFMA is a half / a quarter of a
//     one-set kernel's;
//   * the epilogue is jones_row_pol (kl_eval_rt.h): two exact reductions and
//     two sincos per pixel, then the wide kernel's store code (byte swap,
//     float4 stores with the trash block for dead rows, scalar stores for
//     P % 4 != 0 or an unaligned output).  No checksums.
// With phase_yy == phase_xx the operands, their order and the epilogue's
// arithmetic are kl_eval_wide_kernel's: the same bits.
//
// Build choices (csrc/Makefile), both read from this unit's ISA (float4 /
// fast-sincos variants, phase-only | with amplitudes; profiles/README.md):
//   * the VGPR form of the MFMAs (-mllvm -amdgpu-mfma-vgpr-form).  8 | 16 v4d
//     accumulator tiles live across the run-time k-loop and are then read by
//     the VALU epilogue.  With AGPR accumulators the compiler carries them in
//     VGPRs over the loop's back edge and copies them to AGPRs and back on
//     every trip: 128 | 256 v_accvgpr moves beside 16 | 32 MFMAs, on the VALU
//     the fp64 MFMAs hold, and 180 | 308 registers.  In VGPR form: no moves,
//     122 | 206 VGPRs (4 | 2 waves per SIMD), no scratch -- the value
//     kernel's finding, at 2 and 4 times its accumulators;
//   * 2 k-steps per trip, as kl_values.hip and not the wide kernel's 4.  The
//     zero k-steps of the last trip are real MFMAs, times 2 | 4 sets here
//     (D = 20: 6 k-steps instead of 8 for 5), and from D ~ 50 the fp64 MFMAs,
//     not the stores, are expected to bound this kernel.  4 per trip also
//     costs registers, 157 | 239 (3 | 2 waves per SIMD), for nothing it
//     hides: a 2-step trip already puts 16 | 32 MFMAs of 8 passes each
//     behind its 4 | 8 coefficient loads.  A trip reads each Cpix fragment
//     from LDS once for all sets (4 ds_read2st64_b64 per 16 | 32 MFMAs).

#include "kl_eval_rt.h"

namespace sf {

constexpr int kPolKC = 2;  // k-steps per trip of the contraction loop
// coefficient sets: phase XX, phase YY, amplitude XX, YY (kl_eval_rt.h's
// kMaxSets stays 3: its four users' code objects are then unchanged)
constexpr int kPolSets = 4;

template <bool VEC4, bool FAST, bool NT, bool GAIN>
__global__ __launch_bounds__(64 * kEvalWaves) void kl_eval_pol_kernel(
    const double* __restrict__ cfrag, const double* __restrict__ ph_xx,
    const double* __restrict__ ph_yy, const double* __restrict__ amp_xx,
    const double* __restrict__ amp_yy, int D, int ks, int ks_pad, int64_t S, int64_t P,
    int64_t n_pb, int64_t n_sc, int chunk_groups, float* __restrict__ out, int64_t ring,
    unsigned flags, float* __restrict__ trash) {
  extern __shared__ double pol_bsh[];  // [ks_pad][kTiles][64]
  constexpr int NSET = GAIN ? 4 : 2;   // phase XX, phase YY, amplitude XX, YY
  const int l = threadIdx.x & 63;
  // wave index, wave-uniform: keeps slot / ring arithmetic on the SALU
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_frag = ks * kTiles * 64;          // Cpix doubles of a wave block
  const int n_frag_pad = ks_pad * kTiles * 64;  // with the zero k-steps
  const bool scrub = flags & SF_EVAL_NAN_SCRUB;
  const bool be = flags & SF_EVAL_BIG_ENDIAN;
  const double sx = FAST ? kLog2of10 : 1.0;
  const int dl = l >> 4;
  // n_pb counts 64-pixel wave blocks
  const int64_t n_blocks = n_pb * n_sc;
  for (int64_t bb = blockIdx.x; bb < n_blocks; bb += gridDim.x) {
    int64_t wpb, sc;
    eval_block(bb, n_pb, n_sc, wpb, sc, flags);
    if (sc >= n_sc) continue;  // uniform per workgroup
    __syncthreads();           // the previous item's reads of the fragments are done
    if (wpb * kWavePix < P) {
      const double* src = cfrag + wpb * n_frag;
      for (int i = threadIdx.x; i < n_frag_pad; i += 64 * kEvalWaves)
        pol_bsh[i] = i < n_frag ? src[i] : 0.0;
    }
    __syncthreads();
    if (wpb * kWavePix >= P) continue;  // uniform per workgroup
    const int64_t p0 = wpb * kWavePix + (int64_t)(l & 15) * kTiles;
    // n_sc counts chunks of chunk_groups ring groups (ring <= S: the launcher)
    const int64_t entry_base = sc * (int64_t)chunk_groups * 16;
    for (int g = w; g < chunk_groups; g += kEvalWaves) {
      const int64_t e0 = entry_base + (int64_t)g * 16;
      if (e0 >= ring) break;
      // the slots of ring entries e0 .. e0 + 15, lap by lap
      for (int64_t s0 = e0; s0 < S; s0 += ring) {
        // ---- contraction: 16 slots x the block's 64 pixels, every set
        const int64_t sa = s0 + (l & 15);
        const bool srow = e0 + (l & 15) < ring && sa < S;
        const int64_t roff = (srow ? sa : S - 1) * D;
        const double* const rows[kPolSets] = {ph_xx + roff, ph_yy + roff,
                                              GAIN ? amp_xx + roff : nullptr,
                                              GAIN ? amp_yy + roff : nullptr};
        v4d acc[NSET][kTiles];
        rt_contract<kPolKC, kTiles, NSET>(
            acc, rows, srow, D, ks_pad, dl,
            // phases in turns, log-amplitudes as the epilogue takes them
            [=](int s, double x) { return x * (s < 2 ? kInv2Pi : sx); },
            [=](int k, int t) { return pol_bsh[(k * kTiles + t) * 64 + l]; });
        // ---- epilogue: accumulator row r = 4 slot rows x this lane's 4 pixels
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = acc_row(l, r);
          const int64_t so = e0 + row;  // ring entry
          const bool srow_live = so < ring && s0 + row < S;
          float pv[4][kTiles];  // planes Re XX, Im XX, Re YY, Im YY
          jones_row_pol<FAST, GAIN, kTiles>(pv, acc, r, scrub);
          if (be) {
#pragma unroll
            for (int t = 0; t < kTiles; ++t)
#pragma unroll
              for (int q = 0; q < 4; ++q) pv[q][t] = bswapf(pv[q][t]);
          }
          if constexpr (VEC4) {
            // P % 4 == 0: a lane's 4 pixels are all inside the grid or all out;
            // dead rows and pixels store into the context's trash block
            const bool live = srow_live && p0 < P;
            float* o = live ? out + (so * 4) * P + p0 : trash + 4 * l;
            const int64_t qstride = live ? P : 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const v4f v = {pv[q][0], pv[q][1], pv[q][2], pv[q][3]};
              store4<NT>(o + q * qstride, v);
            }
          } else if (srow_live) {
            float* o = out + (so * 4) * P + p0;
#pragma unroll
            for (int t = 0; t < kTiles; ++t) {
              if (p0 + t < P) {
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q * P + t] = pv[q][t];
              }
            }
          }
        }
      }  // laps
    }
  }  // workgroup walk
}

int launch_eval_pol(sf_ctx* ctx, const double* ph_xx, const double* ph_yy,
                    const double* amp_xx, const double* amp_yy, int64_t S, float* out,
                    int64_t ring, unsigned flags) {
  const int ks = ctx->ksteps;
  if (ks < 1 || ks > kEvalWideMaxKS) {
    set_error("sf_kl_eval_pol: unsupported number of directions");
    return SF_EINVAL;
  }
  // a ring longer than the call changes nothing (slot s -> entry s)
  if (ring > S) ring = S;
  const BlockWalkLaunch g = block_walk_launch(ctx, kPolKC, ring, flags, out);
  const bool fast = flags & SF_EVAL_FAST_SINCOS;
  const bool gain = amp_xx != nullptr;
  // 12 variants: NT stores are float4 stores (g.nt implies g.vec4)
  with_bools(
      [&](auto V, auto F, auto N, auto G) {
        constexpr bool v = decltype(V)::value, n = decltype(N)::value;
        if constexpr (v || !n)
          hipLaunchKernelGGL(
              (kl_eval_pol_kernel<v, decltype(F)::value, n, decltype(G)::value>),
              dim3((unsigned)g.nblk), dim3(64 * kEvalWaves), g.lds, ctx->stream, ctx->d_cfrag,
              ph_xx, ph_yy, amp_xx, amp_yy, ctx->D, ks, g.ks_pad, S, ctx->n_pix, g.n_wpb,
              g.n_sc, g.groups, out, ring, g.fl, ctx->d_trash);
      },
      g.vec4, fast, g.nt, gain);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

}  // namespace sf
