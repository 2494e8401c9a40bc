// kl_eval_wide.hip -- KL screen evaluation for 61..128 directions
// (16..32 k-steps of 4 directions; SF_EVAL_KERNEL_WIDE).
//
// The kernels of kl_eval_impl.h are templates on the k-step count and keep a
// wave's Cpix fragments (8 KS registers) and coefficient fragments (2 KS, 6 KS
// for gain) in registers: at KS = 32 that is far over the 512-VGPR budget, so
// their dispatch stops at 15 k-steps (D = 60).  This kernel takes the k-step
// count at run time instead:
//   * the 4 waves of a workgroup share ONE 64-pixel wave block, whose Cpix
//     fragments sit in LDS in kl_cpix_kernel's order [kstep][tile][lane]
//     (2 KiB per k-step, the count rounded up to a multiple of 4 with zero
//     fragments: 32..64 KiB of dynamic LDS), and take the work item's groups
//     round-robin -- the SHB shape of kl_eval_kernel;
//   * a group is 16 consecutive RING ENTRIES, and the wave that owns it
//     evaluates every slot that lands there (s = entry, entry + ring, ...) in
//     ascending order: with a ring shorter than the call all writers of an
//     entry are one lane of one wave in program order, so the entry ends up
//     holding its last slot (the slot-major kernels leave that unspecified);
//     with ring >= S it is the plain 16-slot group;
//   * a group's contraction is rt_contract (kl_eval_rt.h), 4 k-steps per
//     trip: only the accumulator tiles (4, or 12 for gain: phase, XX, YY)
//     stay in registers across the loop;
//   * the epilogue is jones_row (kl_eval_rt.h: the register tile's, with the
//     exact reduction), then byte swap, float4 stores (trash block for dead
//     rows) or scalar stores for odd grids / unaligned output, and per-slot
//     checksums.
// The contraction is fp64 everywhere (SF_EVAL_CONTRACTION_F64): the
// integer-digit contraction for D > 64 would take two K = 64 halves per digit
// pair and is not built.

#include "kl_eval_rt.h"

namespace sf {

constexpr int kWideKC = 4;  // k-steps per trip of the contraction loop

template <bool VEC4, bool FAST, bool NT, bool GAIN>
__global__ __launch_bounds__(64 * kEvalWaves) void kl_eval_wide_kernel(
    const double* __restrict__ cfrag, const double* __restrict__ coef,
    const double* __restrict__ coef_xx, const double* __restrict__ coef_yy,
    int D, int ks, int ks_pad, int64_t S, int64_t P, int64_t n_pb, int64_t n_sc,
    int chunk_groups, float* __restrict__ out, int64_t ring, unsigned flags,
    unsigned* __restrict__ sums, float* __restrict__ trash) {
  extern __shared__ double wide_bsh[];  // [ks_pad][kTiles][64]
  const int l = threadIdx.x & 63;
  // wave index, wave-uniform: keeps slot / ring arithmetic on the SALU
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_frag = ks * kTiles * 64;          // Cpix doubles of a wave block
  const int n_frag_pad = ks_pad * kTiles * 64;  // with the zero k-steps
  const bool scrub = flags & SF_EVAL_NAN_SCRUB;
  const bool be = flags & SF_EVAL_BIG_ENDIAN;
  const double sx = FAST ? kLog2of10 : 1.0;
  const int dl = l >> 4;
  // n_pb counts 64-pixel wave blocks (as the SHB launch of kl_eval_kernel)
  const int64_t n_blocks = n_pb * n_sc;
  for (int64_t bb = blockIdx.x; bb < n_blocks; bb += gridDim.x) {
    int64_t wpb, sc;
    eval_block(bb, n_pb, n_sc, wpb, sc, flags);
    if (sc >= n_sc) continue;  // uniform per workgroup
    __syncthreads();           // the previous item's reads of the fragments are done
    if (wpb * kWavePix < P) {
      const double* src = cfrag + wpb * n_frag;
      for (int i = threadIdx.x; i < n_frag_pad; i += 64 * kEvalWaves)
        wide_bsh[i] = i < n_frag ? src[i] : 0.0;
    }
    __syncthreads();
    if (wpb * kWavePix >= P) continue;  // uniform per workgroup
    const int64_t p0 = wpb * kWavePix + (int64_t)(l & 15) * kTiles;
    // n_sc counts chunks of chunk_groups ring groups (ring <= S: launch_eval)
    const int64_t entry_base = sc * (int64_t)chunk_groups * 16;
    for (int g = w; g < chunk_groups; g += kEvalWaves) {
      const int64_t e0 = entry_base + (int64_t)g * 16;
      if (e0 >= ring) break;
      // the slots of ring entries e0 .. e0 + 15, lap by lap
      for (int64_t s0 = e0; s0 < S; s0 += ring) {
      // ---- contraction: 16 slots x the block's 64 pixels
      const int64_t sa = s0 + (l & 15);
      const bool srow = e0 + (l & 15) < ring && sa < S;
      const int64_t roff = (srow ? sa : S - 1) * D;
      const double* const rows[kMaxSets] = {coef + roff, GAIN ? coef_xx + roff : nullptr,
                                            GAIN ? coef_yy + roff : nullptr};
      v4d acc[GAIN ? 3 : 1][kTiles];  // phase, XX, YY
      rt_contract<kWideKC, kTiles, GAIN ? 3 : 1>(
          acc, rows, srow, D, ks_pad, dl,
          // phase in turns, log-amplitudes as the epilogue takes them
          [=](int s, double x) { return x * (s == 0 ? kInv2Pi : sx); },
          [=](int k, int t) { return wide_bsh[(k * kTiles + t) * 64 + l]; });
      // ---- epilogue: accumulator row r = 4 slot rows x this lane's 4 pixels
      unsigned part[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = acc_row(l, r);
        const int64_t s = s0 + row;
        const int64_t so = e0 + row;  // ring entry
        const bool srow_live = so < ring && s < S;
        const bool live = srow_live && (!VEC4 || p0 < P);
        float pv[4][kTiles];  // planes Re XX, Im XX, Re YY, Im YY
        jones_row<FAST, GAIN, kTiles>(pv, acc, r, scrub);
        if (be) {
#pragma unroll
          for (int t = 0; t < kTiles; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) pv[q][t] = bswapf(pv[q][t]);
        }
        unsigned cs32 = 0u;
        if constexpr (VEC4) {
          // P % 4 == 0: a lane's 4 pixels are all inside the grid or all out;
          // dead rows and pixels store into the context's trash block
          float* o = live ? out + (so * 4) * P + p0 : trash + 4 * l;
          const int64_t qstride = live ? P : 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const v4f v = {pv[q][0], pv[q][1], pv[q][2], pv[q][3]};
            store4<NT>(o + q * qstride, v);
          }
          if (sums && live) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int t = 0; t < kTiles; ++t) cs32 += fbits(pv[q][t]);
          }
        } else if (srow_live) {
          float* o = out + (so * 4) * P + p0;
#pragma unroll
          for (int t = 0; t < kTiles; ++t) {
            if (p0 + t < P) {
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                o[q * P + t] = pv[q][t];
                if (sums) cs32 += fbits(pv[q][t]);
              }
            }
          }
        }
        part[r] = cs32;
      }
      if (sums) {
        // lane i of a DPP row gets the row total of part[i >> 2], i.e. of
        // slot row (l >> 4) + 4 (i >> 2): one lane of each quad adds it
        const unsigned tot = row_sum16_x4(part, l & 15);
        const int row = 4 * ((l >> 2) & 3) + (l >> 4);
        if ((l & 3) == 0 && e0 + row < ring && s0 + row < S)
          atomicAdd(sums + s0 + row, tot);
      }
      }  // laps
    }
  }  // workgroup walk
}

int launch_eval_wide(sf_ctx* ctx, const double* coef, const double* cxx,
                     const double* cyy, int64_t S_all, float* out, int64_t ring,
                     unsigned flags, unsigned* sums) {
  const int ks = ctx->ksteps;
  if (ks <= kEvalMaxKS || ks > kEvalWideMaxKS) {
    set_error("sf_kl_eval: unsupported number of directions");
    return SF_EINVAL;
  }
  const BlockWalkLaunch g = block_walk_launch(ctx, kWideKC, ring, flags, out);
  const bool fast = flags & SF_EVAL_FAST_SINCOS;
  const bool gain = cxx != nullptr;
  // 12 variants: NT stores are float4 stores (g.nt implies g.vec4)
  with_bools(
      [&](auto V, auto F, auto N, auto G) {
        constexpr bool v = decltype(V)::value, n = decltype(N)::value;
        if constexpr (v || !n)
          hipLaunchKernelGGL(
              (kl_eval_wide_kernel<v, decltype(F)::value, n, decltype(G)::value>),
              dim3((unsigned)g.nblk), dim3(64 * kEvalWaves), g.lds, ctx->stream, ctx->d_cfrag,
              coef, cxx, cyy, ctx->D, ks, g.ks_pad, S_all, ctx->n_pix, g.n_wpb, g.n_sc,
              g.groups, out, ring, g.fl, sums, ctx->d_trash);
      },
      g.vec4, fast, g.nt, gain);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

}  // namespace sf
