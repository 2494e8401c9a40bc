// kl_values.hip -- KL screen VALUES on the pixel grid (sf_kl_eval_values).
//
// calculate_kl_screen (kl_screen.py:411-449) gives, per slot s and pixel p,
//     value[s][p] = sum_d Cpix[p][d] * coef[s][d]          (float64)
// and the reference's "tec" a-term cube (processing_utils.py:187-190) stores
// that value itself, one float32 per pixel, where the Jones cube stores its
// cos / sin.  This kernel writes out[(s % ring)][ny][nx] = (float)value:
// 4 N^2 bytes per slot, a quarter of the Jones cube's stores for the same
// MFMAs, so from D ~ 20 the fp64 MFMAs and not the stores bound it.
//
// One kernel for 1 <= D <= SF_MAX_EVAL_DIR, on kl_eval_wide.hip's shape (the
// walk below is that kernel's, spelled out here too: routed through a shared
// template with the stores as functors, this kernel measured 0.3-1 % slower,
// profiles/rt_kloop_isa.txt):
//   * the 4 waves of a workgroup share ONE 64-pixel wave block, whose Cpix
//     fragments (sf_set_grid's ctx->d_cfrag, [kstep][tile][lane]) sit in LDS,
//     the k-step count rounded up to a multiple of 2 with zero fragments
//     (4..64 KiB of dynamic LDS), and take the item's 16-entry ring groups
//     round-robin;
//   * a group is 16 consecutive ring entries, and the wave that owns it
//     evaluates every slot that lands there in ascending order: with a ring
//     shorter than the call an entry ends up holding its last slot;
//   * the contraction walks the k-steps 2 at a time at run time (one kernel
//     for every D, no template on the k-step count): rt_contract of
//     kl_eval_rt.h without a scale, the B operands from LDS per MFMA, and
//     only the 4 accumulator tiles stay in registers across the loop -- in
//     VGPRs: the unit is built with the VGPR
//     form of the MFMAs (csrc/Makefile), since AGPR accumulators were copied
//     to VGPRs and back on every trip of a run-time loop;
//   * fp64 all the way, one cast at the store (Q12).  The integer-digit
//     contraction is exact only modulo 2^32 turns and fp32 MFMAs lose the
//     value to cancellation, so neither applies;
//   * epilogue: cast, NaN scrub (-> 0.0f, the value whose Jones term is the
//     1 / 0 the gain scrub writes), byte swap, one float4 store per slot row
//     (trash block for dead rows) or scalar stores for grids with P % 4 != 0
//     and outputs that are not 16-byte aligned.

#include "kl_eval_rt.h"

namespace sf {

// k-steps per trip of the contraction loop.  2, not the wide kernel's 4: the
// zero k-steps of the last trip are real MFMAs here (D = 20: 6 k-steps instead
// of 8 for 5), and with this kernel MFMA-bound they are what the trip size
// costs (DESIGN.md §14 has the three shapes measured)
constexpr int kValKC = 2;

template <bool VEC4, bool NT>
__global__ __launch_bounds__(64 * kEvalWaves) void kl_values_kernel(
    const double* __restrict__ cfrag, const double* __restrict__ coef, int D,
    int ks, int ks_pad, int64_t S, int64_t P, int64_t n_pb, int64_t n_sc,
    int chunk_groups, float* __restrict__ out, int64_t ring, unsigned flags,
    float* __restrict__ trash) {
  extern __shared__ double val_bsh[];  // [ks_pad][kTiles][64]
  const int l = threadIdx.x & 63;
  // wave index, wave-uniform: keeps slot / ring arithmetic on the SALU
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_frag = ks * kTiles * 64;          // Cpix doubles of a wave block
  const int n_frag_pad = ks_pad * kTiles * 64;  // with the zero k-steps
  const bool scrub = flags & SF_EVAL_NAN_SCRUB;
  const bool be = flags & SF_EVAL_BIG_ENDIAN;
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
        val_bsh[i] = i < n_frag ? src[i] : 0.0;
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
        // ---- contraction: 16 slots x the block's 64 pixels
        const int64_t sa = s0 + (l & 15);
        const bool srow = e0 + (l & 15) < ring && sa < S;
        const double* const row[kMaxSets] = {coef + (srow ? sa : S - 1) * D, nullptr, nullptr};
        v4d acc[1][kTiles];
        rt_contract<kValKC, kTiles, 1>(
            acc, row, srow, D, ks_pad, dl, [](int, double x) { return x; },
            [=](int k, int t) { return val_bsh[(k * kTiles + t) * 64 + l]; });
        // ---- epilogue: accumulator row r = 4 slot rows x this lane's 4 pixels
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = acc_row(l, r);
          const int64_t so = e0 + row;  // ring entry
          const bool srow_live = so < ring && s0 + row < S;
          float pv[kTiles];
#pragma unroll
          for (int t = 0; t < kTiles; ++t) {
            float v = (float)acc[0][t][r];
            if (scrub && isnan(v)) v = 0.0f;
            pv[t] = be ? bswapf(v) : v;
          }
          if constexpr (VEC4) {
            // P % 4 == 0: a lane's 4 pixels are all inside the grid or all
            // out; dead rows and pixels store into the context's trash block
            const bool live = srow_live && p0 < P;
            float* o = live ? out + so * P + p0 : trash + 4 * l;
            store4<NT>(o, v4f{pv[0], pv[1], pv[2], pv[3]});
          } else if (srow_live) {
            float* o = out + so * P + p0;
#pragma unroll
            for (int t = 0; t < kTiles; ++t)
              if (p0 + t < P) o[t] = pv[t];
          }
        }
      }  // laps
    }
  }  // workgroup walk
}

int launch_eval_values(sf_ctx* ctx, const double* coef, int64_t S, float* out,
                       int64_t ring, unsigned flags) {
  const int ks = ctx->ksteps;
  if (ks < 1 || ks > kEvalWideMaxKS) {
    set_error("sf_kl_eval_values: unsupported number of directions");
    return SF_EINVAL;
  }
  // a ring longer than the call changes nothing (slot s -> entry s)
  if (ring > S) ring = S;
  const BlockWalkLaunch g = block_walk_launch(ctx, kValKC, ring, flags, out);
  // 3 variants: NT stores are float4 stores (g.nt implies g.vec4)
  with_bools(
      [&](auto V, auto N) {
        constexpr bool v = decltype(V)::value, n = decltype(N)::value;
        if constexpr (v || !n)
          hipLaunchKernelGGL((kl_values_kernel<v, n>), dim3((unsigned)g.nblk),
                             dim3(64 * kEvalWaves), g.lds, ctx->stream, ctx->d_cfrag, coef,
                             ctx->D, ks, g.ks_pad, S, ctx->n_pix, g.n_wpb, g.n_sc, g.groups,
                             out, ring, g.fl, ctx->d_trash);
      },
      g.vec4, g.nt);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

}  // namespace sf
