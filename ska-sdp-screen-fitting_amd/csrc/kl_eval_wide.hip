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
//   * a group's contraction walks the k-steps 4 at a time: the coefficient
//     fragments of the next 4 k-steps (one double each; three for gain) are
//     loaded while the v_mfma_f64_16x16x4_f64 of the current 4 run, the B
//     operands come from LDS per MFMA, and only the accumulator tiles (4, or
//     12 for gain: phase, XX, YY) stay in registers across the loop;
//   * the epilogue is the register tile's, from the helpers of
//     kl_eval_impl.h: the exact reduction rev - rint(rev) (the fixed-point
//     kRevMagic reduction holds only to kMagicMaxKS k-steps) and the hardware
//     sincos under SF_EVAL_FAST_SINCOS, else the fp64 sincos; 10^x for gain;
//     NaN scrub; byte swap; float4 stores (trash block for dead rows) or
//     scalar stores for odd grids / unaligned output; per-slot checksums.
// The contraction is fp64 everywhere (SF_EVAL_CONTRACTION_F64): the
// integer-digit contraction for D > 64 would take two K = 64 halves per digit
// pair and is not built.

#include "kl_eval_impl.h"

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
      const double* rp = coef + roff;
      const double* rxp = GAIN ? coef_xx + roff : nullptr;
      const double* ryp = GAIN ? coef_yy + roff : nullptr;
      v4d acc[kTiles], accx[GAIN ? kTiles : 1], accy[GAIN ? kTiles : 1];
#pragma unroll
      for (int t = 0; t < kTiles; ++t) {
        acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
        if constexpr (GAIN) {
          accx[t] = v4d{0.0, 0.0, 0.0, 0.0};
          accy[t] = v4d{0.0, 0.0, 0.0, 0.0};
        }
      }
      // raw fragments of k-steps k0 .. k0 + 3: unconditional loads of clamped
      // addresses (load_coef's reasoning), masked and scaled when used
      double rf[kWideKC], rx[GAIN ? kWideKC : 1], ry[GAIN ? kWideKC : 1];
      auto load_raw = [&](int k0) {
#pragma unroll
        for (int j = 0; j < kWideKC; ++j) {
          const int d = 4 * (k0 + j) + dl;
          const int dc = d < D ? d : D - 1;
          rf[j] = rp[dc];
          if constexpr (GAIN) {
            rx[j] = rxp[dc];
            ry[j] = ryp[dc];
          }
        }
      };
      load_raw(0);
#pragma unroll 1
      for (int k0 = 0; k0 < ks_pad; k0 += kWideKC) {
        double af[kWideKC], ax[GAIN ? kWideKC : 1], ay[GAIN ? kWideKC : 1];
#pragma unroll
        for (int j = 0; j < kWideKC; ++j) {
          const bool ok = srow && 4 * (k0 + j) + dl < D;
          af[j] = keep_if(ok, rf[j] * kInv2Pi);  // phase in turns
          if constexpr (GAIN) {
            ax[j] = keep_if(ok, rx[j] * sx);
            ay[j] = keep_if(ok, ry[j] * sx);
          }
        }
        // the next trip's loads (the last trip reloads its own: no branch)
        load_raw(k0 + kWideKC < ks_pad ? k0 + kWideKC : k0);
#pragma unroll
        for (int j = 0; j < kWideKC; ++j) {
          const double* bk = wide_bsh + ((k0 + j) * kTiles) * 64 + l;
#pragma unroll
          for (int t = 0; t < kTiles; ++t) {
            const double b = bk[t * 64];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[j], b, acc[t], 0, 0, 0);
            if constexpr (GAIN) {
              accx[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ax[j], b, accx[t], 0, 0, 0);
              accy[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ay[j], b, accy[t], 0, 0, 0);
            }
          }
        }
      }
      // ---- epilogue: accumulator row r = 4 slot rows x this lane's 4 pixels
      unsigned part[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = acc_row(l, r);
        const int64_t s = s0 + row;
        const int64_t so = e0 + row;  // ring entry
        const bool srow_live = so < ring && s < S;
        const bool live = srow_live && (!VEC4 || p0 < P);
        // fast epilogue: the exact reduction; phase screens scrub the
        // reduced argument (cos 1, sin 0), gain screens the products
        float fr[kTiles];
        if constexpr (FAST) {
          double rv[kTiles];
#pragma unroll
          for (int t = 0; t < kTiles; ++t) rv[t] = acc[t][r];
          rev_reduce_n<kTiles>(fr, rv, !GAIN && scrub);
        }
        float pv[4][kTiles];  // planes Re XX, Im XX, Re YY, Im YY
        constexpr bool kScrubValues = GAIN || !FAST;
        bool bad = false;
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
          float sn, cs;
          if constexpr (FAST) sincos_rev(fr[t], sn, cs);
          else sincos_rev_f64(acc[t][r], sn, cs);
          if constexpr (GAIN) {
            if constexpr (FAST) {
              const float ax = amp2f(accx[t][r]);
              const float ay = amp2f(accy[t][r]);
              pv[0][t] = ax * cs;
              pv[1][t] = ax * sn;
              pv[2][t] = ay * cs;
              pv[3][t] = ay * sn;
            } else {
              // reference: A (fp64) * cos (fp64), one cast at the FITS store
              const double ax = exp10(accx[t][r]);
              const double ay = exp10(accy[t][r]);
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
          for (int t = 0; t < kTiles; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (isnan(pv[q][t])) pv[q][t] = (q & 1) ? 0.0f : 1.0f;
        }
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
  const int ks_pad = (ks + kWideKC - 1) / kWideKC * kWideKC;
  const size_t lds = (size_t)ks_pad * kTiles * 64 * sizeof(double);  // <= 64 KiB
  const int64_t P = ctx->n_pix;
  const int64_t n_wpb = ctx->n_pix_blocks * kEvalWaves;
  // work items: (64-pixel block, chunk of `groups` 16-entry ring groups);
  // launch_eval has cut the ring to <= S, so a ring that does not alias is
  // the plain slot-major split.  One launch: past the dispatch limit the
  // workgroups walk the items (eval_grid)
  const int groups = eval_chunk_groups(n_wpb, ring, ctx->eval_groups ? ctx->eval_groups : 64, 4096);
  flags &= ~(kEvalXcdInterleave | kEvalBandMask);
  if (ctx->eval_xcd_map > 0) flags |= kEvalXcdInterleave;
  const unsigned fl = flags | eval_band_flags(ctx, n_wpb);
  const bool vec4 = (P % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  const bool fast = flags & SF_EVAL_FAST_SINCOS;
  const bool nt = (flags & SF_EVAL_NT_STORES) && vec4;
  const bool gain = cxx != nullptr;
  {
    const int64_t n_sc = (ring + 16 * groups - 1) / (16 * groups);
    const int64_t nblk = eval_grid(ctx, n_wpb, n_sc, 256);
#define SF_LAUNCH_WIDE(V, F, N, G)                                               \
  hipLaunchKernelGGL((kl_eval_wide_kernel<V, F, N, G>), dim3((unsigned)nblk),    \
                     dim3(64 * kEvalWaves), lds, ctx->stream, ctx->d_cfrag,      \
                     coef, cxx, cyy, ctx->D, ks, ks_pad, S_all, P, n_wpb, n_sc,  \
                     groups, out, ring, fl, sums, ctx->d_trash)
#define SF_LAUNCH_WIDE_G(V, F, N)              \
  do {                                         \
    if (gain) SF_LAUNCH_WIDE(V, F, N, true);   \
    else SF_LAUNCH_WIDE(V, F, N, false);       \
  } while (0)
    if (vec4) {
      if (fast) {
        if (nt) SF_LAUNCH_WIDE_G(true, true, true); else SF_LAUNCH_WIDE_G(true, true, false);
      } else {
        if (nt) SF_LAUNCH_WIDE_G(true, false, true); else SF_LAUNCH_WIDE_G(true, false, false);
      }
    } else {
      if (fast) SF_LAUNCH_WIDE_G(false, true, false); else SF_LAUNCH_WIDE_G(false, false, false);
    }
#undef SF_LAUNCH_WIDE_G
#undef SF_LAUNCH_WIDE
    SF_HIP(hipGetLastError());
  }
  return SF_OK;
}

}  // namespace sf
