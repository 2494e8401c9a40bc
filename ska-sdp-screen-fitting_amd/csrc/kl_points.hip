// kl_points.hip -- KL screens sampled at a list of positions
// (sf_set_points, sf_kl_eval_points, sf_kl_eval_point_values).
//
// calculate_kl_screen (kl_screen.py:411-449) evaluates a screen at ONE
// position; make_matrix calls it for every pixel of the a-term image.  The
// question the reference's acceptance test asks -- what do the screens hold at
// the calibrator patches -- needs P ~ D positions per slot, not N^2 pixels:
// 8 D bytes read and 16 P written per slot instead of 16 N^2.  The kernels of
// kl_eval_impl.h are pixel-block-major (a wave keeps one 64-pixel block and
// streams slots through it, every store is a piece of a [ny][nx] plane); this
// one is SLOT-major:
//   * output planes are [S][4][P] float32 (the cube's plane order with the
//     pixel axes replaced by the point index), values [S][P] float64, so the
//     16 consecutive slots of a wave form ONE contiguous run of 256 P
//     (128 P) bytes;
//   * the point basis Cpix[p][d] (kl_points_cpix_kernel: pix_cov's expression
//     in pix_cov's order, so a point at (X[i], Y[j]) carries the bits of the
//     grid's entry for pixel (j, i)) is stored as v_mfma_f64_16x16x4_f64 B
//     fragments [16-point tile][k-step][lane], zero-padded to whole passes of
//     kPtTiles tiles and to kPtKC k-steps.  A workgroup copies all of it into
//     LDS once when two workgroups of that size fit a CU, else every MFMA
//     reads its fragment through L1 / L2 (P x D up to 4096 x 128: 4 MiB);
//   * a wave takes 16 consecutive slots and walks the point tiles kPtTiles at
//     a time; the k-loop runs ceil(D / 4) k-steps at run time (one kernel for
//     D = 1..128, the coefficient fragments of the next trip loaded while the
//     MFMAs of this one run, rows past S and directions past D from a clamped
//     address and masked, as kl_eval_wide.hip);
//   * three epilogues: Jones planes of phase screens (cos, sin, cos, sin),
//     of gain screens (three contractions), both from the helpers of
//     kl_eval_impl.h (exact reduction in revolutions + hardware sincos under
//     SF_EVAL_FAST_SINCOS, fp64 sincos otherwise, 10^x, NaN scrub), and the
//     raw fp64 contraction (values: the coefficients' own units, no 1 / 2 pi
//     round trip, no scrub -- NaN passes through);
//   * the pass's [rows][32 points] tile goes through a wave-private LDS
//     stage, from which lanes write 16-byte pieces at 16-byte aligned
//     addresses wherever a row's run covers one, and single elements at a
//     run's unaligned head and tail -- whatever P and the alignment of the
//     output pointer (4 bytes for planes, 8 for values) are.  Dead slot rows
//     (S % 16) and dead point columns (P % 16) are never stored.

#include "kl_eval_impl.h"

namespace sf {

constexpr int kPtTiles = 2;               // 16-point MFMA tiles per pass
constexpr int kPtPass = 16 * kPtTiles;    // points per pass
constexpr int kPtKC = 2;                  // k-steps per trip of the k-loop
constexpr int kPtWaves = 4;               // waves (16-slot groups) per workgroup
constexpr int kPtPlanes = 0, kPtGain = 1, kPtValues = 2;

// pix_cov of kl_eval.hip: the same expression in the same order
__device__ inline double point_cov(double ppx, double ppy, double ppz, double x,
                                   double y, double r0sq, double half_beta) {
#pragma clang fp contract(off)
  const double dx = ppx - x;
  const double dy = ppy - y;
  const double dz = ppz - 0.0;
  const double d2 = (dx * dx + dy * dy) + dz * dz;
  return -pow(d2 / r0sq, half_beta) / 2.0;
}

// Cpix of the points in MFMA B-fragment order [point tile][k-step][lane]:
// lane l of (tile, kk) holds point 16 tile + (l & 15), direction 4 kk + (l >> 4)
// (0 past P or D).
__global__ __launch_bounds__(256) void kl_points_cpix_kernel(
    const double* __restrict__ pp, int D, double r0, double beta,
    const double* __restrict__ xy, int P, int ks_pad, int n_elems,
    double* __restrict__ pfrag) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_elems) return;
  const int l = e & 63;
  const int kk = (e >> 6) % ks_pad;
  const int tile = (e >> 6) / ks_pad;
  const int p = 16 * tile + (l & 15);
  const int d = 4 * kk + (l >> 4);
  double v = 0.0;
  if (p < P && d < D)
    v = point_cov(pp[3 * d], pp[3 * d + 1], pp[3 * d + 2], xy[2 * p], xy[2 * p + 1],
                  r0 * r0, beta / 2.0);
  pfrag[e] = v;
}

template <int MODE>
struct PtOut {
  using T = std::conditional_t<MODE == kPtValues, double, float>;
  static constexpr int kRowsPerSlot = MODE == kPtValues ? 1 : 4;
  static constexpr int kRows = 16 * kRowsPerSlot;          // rows of a 16-slot group
  static constexpr int kVec = 16 / (int)sizeof(T);         // elements per 16 bytes
  static constexpr int kLd = kPtPass + kVec;               // stage row stride
  static constexpr int kPieces = kPtPass / kVec + 1;       // 16-byte pieces a row can touch
  static constexpr size_t kStageBytes = (size_t)kPtWaves * kRows * kLd * sizeof(T);
};

template <int MODE, bool FAST, bool LDSB>
__global__ __launch_bounds__(64 * kPtWaves) void kl_eval_points_kernel(
    const double* __restrict__ pfrag, const double* __restrict__ coef,
    const double* __restrict__ coef_xx, const double* __restrict__ coef_yy, int D,
    int ks_pad, int64_t S, int P, int n_pt, int64_t n_items, void* __restrict__ out_v,
    unsigned flags) {
  using O = PtOut<MODE>;
  using T = typename O::T;
  typedef T vecT __attribute__((ext_vector_type(O::kVec)));
  constexpr bool GAIN = MODE == kPtGain;
  extern __shared__ double pt_sh[];  // [n_pt][ks_pad][64] when LDSB, then the stages
  const int l = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_b = LDSB ? n_pt * ks_pad * 64 : 0;
  T* stage = reinterpret_cast<T*>(pt_sh + n_b) + w * (O::kRows * O::kLd);
  if constexpr (LDSB) {
    for (int i = threadIdx.x; i < n_b; i += 64 * kPtWaves) pt_sh[i] = pfrag[i];
  }
  __syncthreads();
  T* out = static_cast<T*>(out_v);
  // elements by which the output pointer is past a 16-byte boundary
  const int oa = (int)((reinterpret_cast<uintptr_t>(out_v) / sizeof(T)) & (O::kVec - 1));
  const bool scrub = flags & SF_EVAL_NAN_SCRUB;
  const double sc_ph = MODE == kPtValues ? 1.0 : kInv2Pi;  // planes: phase in turns
  const double sx = FAST ? kLog2of10 : 1.0;
  const int dl = l >> 4;
  // every wave of the workgroup runs every trip of both loops (the barriers
  // round the stage are workgroup barriers): a group past S computes on
  // masked rows and stores nothing
  for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const int64_t s0 = (it * kPtWaves + w) * 16;
    const int64_t sa = s0 + (l & 15);
    const bool srow = sa < S;
    const int64_t roff = (srow ? sa : S - 1) * D;
    const double* rp = coef + roff;
    const double* rxp = GAIN ? coef_xx + roff : nullptr;
    const double* ryp = GAIN ? coef_yy + roff : nullptr;
    const int64_t left = S - s0;
    const int n_rows = (left >= 16 ? 16 : left > 0 ? (int)left : 0) * O::kRowsPerSlot;
    for (int pt0 = 0; pt0 < n_pt; pt0 += kPtTiles) {
      // ---- contraction: 16 slots x the pass's kPtTiles x 16 points
      v4d acc[kPtTiles], accx[GAIN ? kPtTiles : 1], accy[GAIN ? kPtTiles : 1];
#pragma unroll
      for (int t = 0; t < kPtTiles; ++t) {
        acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
        if constexpr (GAIN) {
          accx[t] = v4d{0.0, 0.0, 0.0, 0.0};
          accy[t] = v4d{0.0, 0.0, 0.0, 0.0};
        }
      }
      double rf[kPtKC], rx[GAIN ? kPtKC : 1], ry[GAIN ? kPtKC : 1];
      auto load_raw = [&](int k0) {
#pragma unroll
        for (int j = 0; j < kPtKC; ++j) {
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
      for (int k0 = 0; k0 < ks_pad; k0 += kPtKC) {
        double af[kPtKC], ax[GAIN ? kPtKC : 1], ay[GAIN ? kPtKC : 1];
#pragma unroll
        for (int j = 0; j < kPtKC; ++j) {
          const bool ok = srow && 4 * (k0 + j) + dl < D;
          af[j] = keep_if(ok, rf[j] * sc_ph);
          if constexpr (GAIN) {
            ax[j] = keep_if(ok, rx[j] * sx);
            ay[j] = keep_if(ok, ry[j] * sx);
          }
        }
        // the next trip's loads (the last trip reloads its own: no branch)
        load_raw(k0 + kPtKC < ks_pad ? k0 + kPtKC : k0);
#pragma unroll
        for (int j = 0; j < kPtKC; ++j) {
#pragma unroll
          for (int t = 0; t < kPtTiles; ++t) {
            const int bi = ((pt0 + t) * ks_pad + k0 + j) * 64 + l;
            const double b = LDSB ? pt_sh[bi] : pfrag[bi];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[j], b, acc[t], 0, 0, 0);
            if constexpr (GAIN) {
              accx[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ax[j], b, accx[t], 0, 0, 0);
              accy[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ay[j], b, accy[t], 0, 0, 0);
            }
          }
        }
      }
      // ---- epilogue into the wave's stage: accumulator register r of lane l
      // is slot row (l >> 4) + 4 r, point column 16 t + (l & 15)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = acc_row(l, r);
        if constexpr (MODE == kPtValues) {
#pragma unroll
          for (int t = 0; t < kPtTiles; ++t)
            stage[row * O::kLd + 16 * t + (l & 15)] = acc[t][r];
        } else {
          float fr[kPtTiles];
          if constexpr (FAST) {
            double rv[kPtTiles];
#pragma unroll
            for (int t = 0; t < kPtTiles; ++t) rv[t] = acc[t][r];
            rev_reduce_n<kPtTiles>(fr, rv, !GAIN && scrub);
          }
          float pv[4][kPtTiles];  // planes Re XX, Im XX, Re YY, Im YY
          constexpr bool kScrubValues = GAIN || !FAST;
          bool bad = false;
#pragma unroll
          for (int t = 0; t < kPtTiles; ++t) {
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
                // reference: A (fp64) * cos (fp64), one cast to float32
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
            for (int t = 0; t < kPtTiles; ++t)
#pragma unroll
              for (int q = 0; q < 4; ++q)
                if (isnan(pv[q][t])) pv[q][t] = (q & 1) ? 0.0f : 1.0f;
          }
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int t = 0; t < kPtTiles; ++t)
              stage[(row * 4 + q) * O::kLd + 16 * t + (l & 15)] = pv[q][t];
        }
      }
      __syncthreads();
      // ---- stores: row j of the group (slot row j / kRowsPerSlot, plane
      // j % kRowsPerSlot) holds the pass's n_cols live points at elements
      // g .. g + n_cols - 1 of the output; piece q of the row is the q-th
      // 16-byte aligned block that run touches
      const int n_cols = P - 16 * pt0 < kPtPass ? P - 16 * pt0 : kPtPass;
      for (int i = l; i < O::kRows * O::kPieces; i += 64) {
        const int j = i / O::kPieces;
        const int q = i - j * O::kPieces;
        if (j >= n_rows) break;
        const int64_t g = (s0 * O::kRowsPerSlot + j) * P + 16 * pt0;
        const int a = (int)((g + oa) & (O::kVec - 1));
        const int c0 = q * O::kVec - a;  // the piece's first column (may be < 0)
        const T* src = stage + j * O::kLd;
        T* dst = out + g + c0;
        if (c0 >= 0 && c0 + O::kVec <= n_cols) {
          vecT v;
#pragma unroll
          for (int e = 0; e < O::kVec; ++e) v[e] = src[c0 + e];
          *reinterpret_cast<vecT*>(dst) = v;
        } else {
#pragma unroll
          for (int e = 0; e < O::kVec; ++e)
            if (c0 + e >= 0 && c0 + e < n_cols) dst[e] = src[c0 + e];
        }
      }
      __syncthreads();  // the stage is free for the next pass
    }
  }
}

int launch_points_cpix(sf_ctx* ctx) {
  const int n = ctx->pt_tiles * ctx->pt_ks_pad * 64;
  hipLaunchKernelGGL(kl_points_cpix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256),
                     0, ctx->stream, ctx->d_pp, ctx->D, ctx->r0, ctx->beta, ctx->d_pxy,
                     ctx->n_points, ctx->pt_ks_pad, n, ctx->d_pfrag);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

int points_ks_pad(int D) { return ((D + 3) / 4 + kPtKC - 1) / kPtKC * kPtKC; }
int points_tiles(int P) { return ((P + 15) / 16 + kPtTiles - 1) / kPtTiles * kPtTiles; }

namespace {

constexpr size_t kLdsPerCu = 160 * 1024;

template <int MODE, bool FAST, bool LDSB>
int launch_points_one(sf_ctx* ctx, const double* coef, const double* cxx,
                      const double* cyy, int64_t S, void* out, unsigned flags) {
  const size_t basis = (size_t)ctx->pt_tiles * ctx->pt_ks_pad * 64 * sizeof(double);
  const size_t shm = (LDSB ? basis : 0) + PtOut<MODE>::kStageBytes;
  if (shm > 64 * 1024)
    SF_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&kl_eval_points_kernel<MODE, FAST, LDSB>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
  // persistent workgroups (each loads the basis once): as many as the LDS and
  // the 2048 threads of a CU hold
  const int64_t n_items = (S + 16 * kPtWaves - 1) / (16 * kPtWaves);
  int64_t per_cu = (int64_t)(kLdsPerCu / shm);
  if (per_cu > 8) per_cu = 8;
  int64_t blocks = (int64_t)ctx->pt_cus * per_cu;
  if (blocks > n_items) blocks = n_items;
  hipLaunchKernelGGL((kl_eval_points_kernel<MODE, FAST, LDSB>), dim3((unsigned)blocks),
                     dim3(64 * kPtWaves), shm, ctx->stream, ctx->d_pfrag, coef, cxx, cyy,
                     ctx->D, ctx->pt_ks_pad, S, ctx->n_points, ctx->pt_tiles, n_items, out,
                     flags);
  SF_HIP(hipGetLastError());
  return SF_OK;
}

template <int MODE, bool FAST>
int launch_points_lds(sf_ctx* ctx, const double* coef, const double* cxx,
                      const double* cyy, int64_t S, void* out, unsigned flags) {
  // the basis in LDS while two workgroups (8 waves) still fit a CU
  const size_t basis = (size_t)ctx->pt_tiles * ctx->pt_ks_pad * 64 * sizeof(double);
  if (2 * (basis + PtOut<MODE>::kStageBytes) <= kLdsPerCu)
    return launch_points_one<MODE, FAST, true>(ctx, coef, cxx, cyy, S, out, flags);
  return launch_points_one<MODE, FAST, false>(ctx, coef, cxx, cyy, S, out, flags);
}

}  // namespace

int launch_eval_points(sf_ctx* ctx, const double* coef, const double* cxx,
                       const double* cyy, int64_t S, float* planes, unsigned flags) {
  const bool fast = flags & SF_EVAL_FAST_SINCOS;
  if (cxx) {
    return fast ? launch_points_lds<kPtGain, true>(ctx, coef, cxx, cyy, S, planes, flags)
                : launch_points_lds<kPtGain, false>(ctx, coef, cxx, cyy, S, planes, flags);
  }
  return fast ? launch_points_lds<kPtPlanes, true>(ctx, coef, nullptr, nullptr, S, planes, flags)
              : launch_points_lds<kPtPlanes, false>(ctx, coef, nullptr, nullptr, S, planes, flags);
}

int launch_eval_point_values(sf_ctx* ctx, const double* coef, int64_t S, double* values) {
  return launch_points_lds<kPtValues, false>(ctx, coef, nullptr, nullptr, S, values, 0u);
}

}  // namespace sf
