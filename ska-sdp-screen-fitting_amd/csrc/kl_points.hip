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
//   * the point basis Cpix[p][d] (kl_points_cpix_kernel: kl_cov against
//     (x, y, 0) as kl_cpix_kernel, so a point at (X[i], Y[j]) carries the bits
//     of the grid's entry for pixel (j, i)) is stored as v_mfma_f64_16x16x4_f64 B
//     fragments [16-point tile][k-step][lane], zero-padded to whole passes of
//     kPtTiles tiles and to kPtKC k-steps.  A workgroup copies all of it into
//     LDS once when two workgroups of that size fit a CU, else every MFMA
//     reads its fragment through L1 / L2 (P x D up to 4096 x 128: 4 MiB);
//   * a wave takes 16 consecutive slots and walks the point tiles kPtTiles at
//     a time; the k-loop runs ceil(D / 4) k-steps at run time (one kernel for
//     D = 1..128: rt_contract of kl_eval_rt.h, the wide kernel's loop);
//   * three epilogues: Jones planes of phase screens (cos, sin, cos, sin),
//     of gain screens (three contractions), both by jones_row of
//     kl_eval_rt.h (exact reduction in revolutions + hardware sincos under
//     SF_EVAL_FAST_SINCOS, fp64 sincos otherwise, 10^x, NaN scrub), and the
//     raw fp64 contraction (values: the coefficients' own units, no 1 / 2 pi
//     round trip, no scrub -- NaN passes through);
//   * the pass's [rows][32 points] tile goes through a wave-private LDS
//     stage, from which lanes write 16-byte pieces at 16-byte aligned
//     addresses wherever a row's run covers one, and single elements at a
//     run's unaligned head and tail -- whatever P and the alignment of the
//     output pointer (4 bytes for planes, 8 for values) are.  Dead slot rows
//     (S % 16) and dead point columns (P % 16) are never stored.

#include "kl_cov.h"
#include "kl_eval_rt.h"

namespace sf {

constexpr int kPtTiles = 2;               // 16-point MFMA tiles per pass
constexpr int kPtPass = 16 * kPtTiles;    // points per pass
constexpr int kPtKC = 2;                  // k-steps per trip of the k-loop
constexpr int kPtWaves = 4;               // waves (16-slot groups) per workgroup
constexpr int kPtPlanes = 0, kPtGain = 1, kPtValues = 2;

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
    v = kl_cov(pp[3 * d], pp[3 * d + 1], pp[3 * d + 2], xy[2 * p], xy[2 * p + 1], 0.0,
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
    const double* const rows[kMaxSets] = {coef + roff, GAIN ? coef_xx + roff : nullptr,
                                          GAIN ? coef_yy + roff : nullptr};
    const int64_t left = S - s0;
    const int n_rows = (left >= 16 ? 16 : left > 0 ? (int)left : 0) * O::kRowsPerSlot;
    for (int pt0 = 0; pt0 < n_pt; pt0 += kPtTiles) {
      // ---- contraction: 16 slots x the pass's kPtTiles x 16 points
      v4d acc[GAIN ? 3 : 1][kPtTiles];  // phase, XX, YY
      rt_contract<kPtKC, kPtTiles, GAIN ? 3 : 1>(
          acc, rows, srow, D, ks_pad, dl,
          [=](int s, double x) {
            if constexpr (MODE == kPtValues) return x;  // the coefficients' own units
            else return x * (s == 0 ? kInv2Pi : sx);    // phase in turns
          },
          [=](int k, int t) {
            const int bi = ((pt0 + t) * ks_pad + k) * 64 + l;
            return LDSB ? pt_sh[bi] : pfrag[bi];
          });
      // ---- epilogue into the wave's stage: accumulator register r of lane l
      // is slot row (l >> 4) + 4 r, point column 16 t + (l & 15)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = acc_row(l, r);
        if constexpr (MODE == kPtValues) {
#pragma unroll
          for (int t = 0; t < kPtTiles; ++t)
            stage[row * O::kLd + 16 * t + (l & 15)] = acc[0][t][r];
        } else {
          float pv[4][kPtTiles];  // planes Re XX, Im XX, Re YY, Im YY
          jones_row<FAST, GAIN, kPtTiles>(pv, acc, r, scrub);
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
  SF_TRY(allow_lds(kl_eval_points_kernel<MODE, FAST, LDSB>, shm));
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
