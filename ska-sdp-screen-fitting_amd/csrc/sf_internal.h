// sf_internal.h -- shared definitions of libscreenfit (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "screenfit.h"

namespace sf {

// error plumbing -------------------------------------------------------------
void set_error(const std::string& msg);

#define SF_HIP(call)                                                        \
  do {                                                                      \
    hipError_t e_ = (call);                                                 \
    if (e_ != hipSuccess) {                                                 \
      ::sf::set_error(std::string(#call) + ": " + hipGetErrorString(e_));   \
      return SF_EIO;                                                        \
    }                                                                       \
  } while (0)

#define SF_REQUIRE(cond, code, msg) \
  do {                              \
    if (!(cond)) {                  \
      ::sf::set_error(msg);         \
      return (code);                \
    }                               \
  } while (0)

#define SF_TRY(x)                  \
  do {                             \
    int rc_ = (x);                 \
    if (rc_ != SF_OK) return rc_;  \
  } while (0)

// Device memory that a context (or a call) owns: the pointer and its size in
// elements, never one without the other.  Reads as a plain T* wherever a
// kernel argument, a copy or a test for "allocated" wants one.  hipFree waits
// for the device, so no queued kernel still uses a buffer that is let go.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t size() const { return n_; }

  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  void swap(DevBuf& o) {
    std::swap(p_, o.p_);
    std::swap(n_, o.n_);
  }

  // At least `need` elements, contents not kept: the old buffer is freed
  // before the new one (exactly `need`) is allocated, so the two never
  // coexist.  A failure leaves the buffer empty.
  int reserve(size_t need, const char* what) {
    if (n_ >= need) return SF_OK;
    reset();
    if (hipMalloc(reinterpret_cast<void**>(&p_), need * sizeof(T)) != hipSuccess) {
      p_ = nullptr;
      set_error(what);
      return SF_ENOMEM;
    }
    n_ = need;
    return SF_OK;
  }

  // At least `need` elements with the old ones copied over (the caller has
  // synchronised the streams that write them).  Old and new coexist during
  // the copy; a failure leaves the old buffer as it was.
  int reserve_keep(size_t need, const char* what) {
    if (n_ >= need) return SF_OK;
    DevBuf q;
    SF_TRY(q.reserve(need, what));
    if (n_ > 0 && hipMemcpy(q.p_, p_, n_ * sizeof(T), hipMemcpyDeviceToDevice) != hipSuccess) {
      set_error(std::string(what) + " (copy of the old contents)");
      return SF_EIO;
    }
    swap(q);
    return SF_OK;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// Two buffers sized together: when either is too small both are freed before
// either is allocated, so the old and the new pair never coexist.
template <typename T, typename U>
int reserve_pair(DevBuf<T>& p, size_t np, DevBuf<U>& q, size_t nq, const char* what) {
  if (p.size() >= np && q.size() >= nq) return SF_OK;
  p.reset();
  q.reset();
  SF_TRY(p.reserve(np, what));
  return q.reserve(nq, what);
}

// what a failed allocation of the fit's tables, pool and scratch reports
constexpr const char* kFitAlloc = "hipMalloc failed (fit scratch)";

// A kernel launched with more than 64 KiB of dynamic LDS has to be allowed it
template <typename K>
int allow_lds(K* kernel, size_t shm) {
  if (shm > 64 * 1024)
    SF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
  return SF_OK;
}

// ctx->d_counters: kFitCounters ints, zeroed at the start of every fit
enum FitCounter {
  kCntIds = 0,         // <= 60 directions: pool ids issued so far
  kCntWideDecomp = 0,  // wide fit: subset decompositions run.  An alias of
                       // kCntIds (the wide fit issues no ids there), so
                       // sf_get_fit_stats reports either as n_masks
  kCntPassStart = 1,   // start of this pass's id range [start, ids)
  kCntSlow = 2,        // slow-class slots (a weight in (0, 1.001e-3])
  kCntError = 3,       // FitError bits
  kCntNonUniform = 4,  // fast-class slots with unequal positive weights
  kCntMaxLevel = 5,    // deepest deletion level among this pass's new masks
  kCntWideMasks = 6,   // wide fit: distinct masks numbered
  kCntLaneDeferred = 7,  // lane slots handed back to the pass kernel
  kCntLane = 8,        // slots the lane kernel took (kl_fit_lane.hip) ...
  kCntList = 9,        // ... entries of the pass kernel's work list: an
                       // aligned pair, one 64-bit atomic adds to both
};
constexpr int kFitCounters = 12;
enum FitError {
  kErrLookupMiss = 1,      // a slot's mask has no pool id
  kErrTableFull = 2,       // the mask table took no further key
  kErrLeanNonUniform = 4,  // the lean pass met non-uniform weights
  kErrFullMaskInPool = 8,  // a mask with no flagged direction in the pool
};

// pixel tiling of the evaluation kernel (kl_eval.hip) -------------------------
constexpr int kTiles = 4;                       // 16x16 MFMA tiles per wave, interleaved
constexpr int kWavePix = 16 * kTiles;           // 64 consecutive pixels per wave
constexpr int kEvalWaves = 4;                   // waves per workgroup
constexpr int kBlockPix = kWavePix * kEvalWaves; // 256 pixels per workgroup

// integer-digit contraction (kl_eval_int.h): balanced base-256 digits per
// operand
constexpr int kDigits = 6;

}  // namespace sf

struct sf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // shared KL basis (sf_set_basis) or evaluation-only geometry
  // (sf_set_piercepoints: D, r0, beta, d_pp / h_pp only)
  int D = 0;
  int has_basis = 0;           // 1: d_c / d_pinv / d_u / d_eig belong to D
  int wide = 0;                // 1: the basis came from sf_set_basis_wide with
                               // D > SF_MAX_DIR (kl_fit_wide.hip fits it)
  double r0 = 100.0;
  double beta = 5.0 / 3.0;
  sf::DevBuf<double> d_pp;      // [D][3]
  sf::DevBuf<double> d_c;       // [D][D]
  sf::DevBuf<double> d_pinv;    // [D][D]
  sf::DevBuf<double> d_u;       // [D][D] (columns sorted by |lambda| desc)
  sf::DevBuf<double> d_eig;     // [D]    (signed eigenvalues, sorted)
  // wide fit (kl_fit_wide.hip): the matrices of the basis kernel, then of the
  // fit workgroups that do not fit the LDS
  sf::DevBuf<double> d_wide_ws;
  // mask cache of the wide fit: every distinct flag mask of a call's input is
  // decomposed once (128-bit keys; rebuilt by every sf_kl_fit)
  int wide_cache = 1;          // SF_OPT_FIT_WIDE_CACHE
  int wide_pool_mb = 0;        // SF_OPT_FIT_WIDE_POOL_MB (0 = 2048)
  int wide_pool_max = 0;       // SF_OPT_FIT_WIDE_POOL_MAX (0 = no entry cap)
  sf::DevBuf<unsigned long long> d_wkeys;  // [S][2] initial mask of every slot
  sf::DevBuf<int> d_wslot;      // [S] table slot, then pool id, of that mask
  sf::DevBuf<unsigned long long> d_wtab;   // [power of two] claimant slot + 1 (0 = empty)
  sf::DevBuf<int> d_wtab_id;    // [as d_wtab] pool id of a claimed table entry
  sf::DevBuf<unsigned long long> d_wpool_mask;  // [entries][2]
  sf::DevBuf<double> d_wpool;   // [wide_pool_n][D (D | 1) + 2 D]: V, lam, perm
  int wide_pool_n = 0;         // entries the last fit built (for this D)
  // pixel grid (sf_set_grid)
  int nx = 0, ny = 0;
  int64_t n_pix = 0;
  int64_t n_pix_blocks = 0;    // workgroup pixel blocks (kBlockPix)
  int ksteps = 0;              // ceil(D / 4)
  sf::DevBuf<double> d_cfrag;   // [wave pixel blocks][ksteps][kTiles][64]
  // fixed-point phase epilogue: a lane's |coef| sum (turns) below rev_thr
  // bounds its phases below 2^17 turns (kl_eval_impl.h group_rev_safe)
  double rev_thr = 0.0;
  // integer-digit contraction (kl_eval_int.h): Cpix as 6 balanced base-256
  // digits of rint(Cpix * 2^36) in i8 MFMA B-fragment order (phase screens,
  // D >= 45), and whether the grid fits the digits
  sf::DevBuf<int8_t> d_cdig;    // [wave pixel blocks][6][kTiles][64][16 B]
  int dig_ok = 0;              // 1: max |Cpix| * 2^36 fits 6 digits
  int eval_int = -1;           // SF_OPT_EVAL_INT (-1 auto, 0 off)
  int eval_wg_waves = 0;       // SF_OPT_EVAL_WG_WAVES (0 = 4, or 8)
  // per-call slot digits of the integer contraction (kl_kdig_kernel)
  sf::DevBuf<int8_t> d_kdig;    // [slot][6][64]
  sf::DevBuf<uint8_t> d_kflag;  // [slot]: 1 = integer path
  // recorded after every launch that reads d_kdig / d_kflag: the next
  // prepass (on whatever stream) waits for it before rewriting them
  hipEvent_t kdig_read = nullptr;
  double h_pp[3 * SF_MAX_EVAL_DIR] = {};  // host copy of the piercepoints
  // screen positions (sf_set_points, kl_points.hip)
  int n_points = 0;            // 0: none bound
  int pt_tiles = 0;            // 16-point tiles, padded to whole passes
  int pt_ks_pad = 0;           // k-steps, padded to the k-loop's trip
  int pt_cus = 0;              // compute units of the device
  sf::DevBuf<double> d_pxy;     // [P][2]
  sf::DevBuf<double> d_pfrag;   // [pt_tiles][pt_ks_pad][64] MFMA B fragments
  // output channels of sf_kl_eval_tec (sf_set_tec_freqs, kl_tec.hip), grouped
  // by TEC frequency; independent of the geometry
  int tec_F = 0;               // channels bound (0: none)
  int tec_F_tec = 0;           // TEC frequencies of the coefficient arrays
  std::vector<int> tec_used;   // the TEC frequencies that have channels, ascending
  std::vector<int> tec_off;    // [used + 1] their ranges in the lists
  sf::DevBuf<double> d_tec_ch;  // [F] scale in turns per TECU, then [F] int
                               // channel index, both in list order
  // fit scratch
  sf::DevBuf<uint8_t> d_skip;   // [F][A] block skip flags
  sf::DevBuf<int> d_st_order;   // [A]
  // mask-keyed cache of flagged-subset bases (kl_fit_fast.hip)
  sf::DevBuf<unsigned long long> d_keys;  // [power of two] hash table keys (0 = empty)
  sf::DevBuf<int> d_ids;                  // [as d_keys] hash table values (-1 = unassigned)
  sf::DevBuf<unsigned long long> d_pool_mask;  // [pool entries] mask of pool entry
  sf::DevBuf<double> d_pool;              // [pool entries][D*D + D] (U_sub, lam)
  int fit_eig_waves = 0;                 // SF_OPT_FIT_EIG_WAVES (0 = 3)
  int fit_subset_deletion = 1;           // SF_OPT_FIT_SUBSET_DELETION: 1 from ancestors (default), 2 from the global basis, 0 Jacobi
  sf::DevBuf<uint8_t> d_pool_status;      // [>= pool entries] deletion kernel: 0 done, 1 Jacobi
  int pool_D = 0;
  sf::DevBuf<int> d_pos;                  // [S] table slot of the current mask
  sf::DevBuf<uint8_t> d_class;            // [S] 0 fast, 1 skipped, 2 slow, 3 lane
  sf::DevBuf<long long> d_list;           // [S] work list of the fast pass (kl_fit_lane.h)
  sf::DevBuf<double> d_sigma;             // [F][A] tec/amplitude block sigma
  sf::DevBuf<int> d_counters;  // [kFitCounters], indexed by sf::FitCounter
  sf::DevBuf<double> d_scratch;           // resid / state when caller passes NULL
  sf::DevBuf<float> d_wscratch;           // w_out / order_out likewise
  sf::DevBuf<int32_t> d_oscratch;
  // Gaussian weights of sf_tess_fill / sf_smooth, pass buffer of sf_smooth
  sf::DevBuf<double> d_gw;
  double gw_sigma = -1.0;                // sigma whose weights d_gw holds
  sf::DevBuf<float> d_trash;  // 1 KiB sink of the eval's out-of-range stores
  sf::DevBuf<float> d_smooth;
  sf::DevBuf<float> d_tess_tab;           // tessellated value table [S][D+1][4] (value fill: [S][D+1])
  // fast-path switch (SCREENFIT_FIT=general forces the general kernel)
  int force_general = 0;
  // evaluation kernel (SF_OPT_EVAL_KERNEL)
  int eval_kernel = SF_EVAL_KERNEL_AUTO;
  int64_t eval_max_blocks = 0;  // SF_OPT_EVAL_MAX_BLOCKS (0 = dispatch limit)
  int eval_ks_pad = 0;          // SF_OPT_EVAL_KS_PAD: extra zero k-steps
  int eval_sleep = 0;           // SF_OPT_EVAL_SLEEP: x 64 cycles per group
  int eval_xcd_map = -1;        // SF_OPT_EVAL_XCD_MAP (-1 = auto)
  int eval_groups = 0;          // SF_OPT_EVAL_GROUPS (0 = auto = 256)
  int eval_bands = 0;           // SF_OPT_EVAL_BANDS (0 = auto = 1)
  int tess_slots = 0;           // SF_OPT_TESS_SLOTS (0 = auto = 16)
  int tess_waves = 0;           // SF_OPT_TESS_WAVES (0 = auto = 16)
  int tess_tile = 0;            // SF_OPT_TESS_TILE (1: round-1 fused tile kernel)
  int tess_box = -1;            // SF_OPT_TESS_BOX (-1 auto, 0 wide-tile, 1 interior lookups)
  int fit_pack = 1;             // SF_OPT_FIT_PACK: 2 slots per wave for D <= 32
  int fit_lean = 1;             // SF_OPT_FIT_LEAN: lean pass when weights are uniform
  int fit_lane = 1;             // SF_OPT_FIT_LANE: lane-per-slot kernel + work list
};

namespace sf {
// Does the integer-digit contraction (kl_eval_int.h) serve this call?  Phase
// screens from D = 45 (below, the fp64 MFMA share of the SIMD is small and
// the LDS-staged kernels are store-bound already) on the fast epilogue with
// float4-aligned output; SF_OPT_EVAL_INT = 0 and grids whose |Cpix| does not
// fit the digits keep the fp64 contraction, and so does the wide kernel
// (D > 60, kl_eval_wide.hip).
constexpr int kEvalMaxKS = 15;   // k-steps of the kl_eval_impl.h templates
constexpr int kEvalWideMaxKS = SF_MAX_EVAL_DIR / 4;
inline bool eval_int_applies(const sf_ctx* ctx, bool gain, unsigned flags,
                             bool out_aligned16) {
  return !gain && ctx->dig_ok && ctx->d_cdig && ctx->eval_int != 0 &&
         (flags & SF_EVAL_FAST_SINCOS) && ctx->n_pix % 4 == 0 && out_aligned16 &&
         ctx->ksteps >= 12 && ctx->ksteps <= kEvalMaxKS;
}

struct RefSpec {
  int sub = -1;                 // local station whose phases are subtracted
  const double* refph = nullptr;  // or: external reference phases [T][F][D]
  int skip = -1;                // local station skipped as the reference
};
RefSpec ref_spec(const sf_fit_params* p, int A);
int launch_skip(sf_ctx* ctx, const double* phase, const float* weight, int T,
                int F, int A, const RefSpec& r);
int launch_fit_general(sf_ctx* ctx, const double* phase, const float* weight,
                       int T, int F, int A, const sf_fit_params* p,
                       const RefSpec& r, double* coef, double* resid,
                       float* w_out, int32_t* order_out);
int launch_basis(sf_ctx* ctx);
// tec / amplitude outlier sigma per (station, freq) block into ctx->d_sigma
// (kl_block_sigma_kernel, kl_fit_fast.hip; any D)
int launch_block_sigma(sf_ctx* ctx, int T, int F, int A, const double* phase,
                       const RefSpec& r, int screen_type, const double* resid,
                       const float* w_out);
// block sigma, counters and scratch for NULL outputs of a fit of S slots
// (kl_fit_fast.hip; every fit launcher)
int fit_buffers(sf_ctx* ctx, int64_t S, int F, int A, double** resid,
                float** w_out, int32_t** order_out);
// 60 < D <= SF_MAX_FIT_DIR: kl_fit_wide.hip
int launch_basis_wide(sf_ctx* ctx);
int launch_fit_wide(sf_ctx* ctx, const double* phase, const float* weight,
                    int T, int F, int A, const sf_fit_params* p, double* coef,
                    double* resid, float* w_out, int32_t* order_out);
// the wide fit's pool of subset bases in sf_get_fit_pool's layout (host)
int read_fit_pool_wide(sf_ctx* ctx, uint64_t* masks, double* entries, int k);
int launch_cpix(sf_ctx* ctx, const double* d_x, const double* d_y);
int launch_cdig(sf_ctx* ctx, const double* d_x, const double* d_y, int* d_bad);
int launch_fit(sf_ctx* ctx, const double* phase, const float* weight, int T,
               int F, int A, const sf_fit_params* p, double* coef,
               double* resid, float* w_out, int32_t* order_out);
int pick_eval_kernel(const sf_ctx* ctx, bool gain, unsigned flags,
                     bool out_aligned16);
int launch_eval(sf_ctx* ctx, const double* coef, const double* cxx,
                const double* cyy, int64_t S, float* out, int64_t ring,
                unsigned flags, unsigned* sums);
// D > 60 (kEvalMaxKS < ksteps <= kEvalWideMaxKS): kl_eval_wide.hip
int launch_eval_wide(sf_ctx* ctx, const double* coef, const double* cxx,
                     const double* cyy, int64_t S, float* out, int64_t ring,
                     unsigned flags, unsigned* sums);
// polarized phases (XX / YY), amplitudes both given or both null, any D
// (kl_eval_pol.hip)
int launch_eval_pol(sf_ctx* ctx, const double* ph_xx, const double* ph_yy,
                    const double* amp_xx, const double* amp_yy, int64_t S, float* out,
                    int64_t ring, unsigned flags);
// screen values on the pixel grid, any D (kl_values.hip)
int launch_eval_values(sf_ctx* ctx, const double* coef, int64_t S, float* out,
                       int64_t ring, unsigned flags);
// Jones cubes of TEC screens at the bound channels, any D (kl_tec.hip)
int launch_eval_tec(sf_ctx* ctx, const double* tec, const double* phase, int64_t T,
                    int A, float* out, unsigned flags);
// screen positions (kl_points.hip): padded shapes of the point basis, its
// kernel (d_pxy -> d_pfrag) and the slot-major evaluation at the points
int points_ks_pad(int D);
int points_tiles(int P);
int launch_points_cpix(sf_ctx* ctx);
int launch_eval_points(sf_ctx* ctx, const double* coef, const double* cxx,
                       const double* cyy, int64_t S, float* planes, unsigned flags);
int launch_eval_point_values(sf_ctx* ctx, const double* coef, int64_t S,
                             double* values);
// phase_yy: the YY phases of a polarized table, or null (planes 2 / 3 take
// the phase of planes 0 / 1)
int launch_tess(sf_ctx* ctx, const int32_t* labels, int nx, int ny,
                const double* phase, const double* phase_yy, const double* amp_xx,
                const double* amp_yy, int D, int64_t S, float* out,
                int64_t ring, const double* d_w, int R, unsigned flags);
int launch_tess_tile(sf_ctx* ctx, const int32_t* labels, int nx, int ny,
                const double* phase, const double* phase_yy, const double* amp_xx,
                const double* amp_yy, int D, int64_t S, float* out,
                int64_t ring, const double* d_w, int R, unsigned flags);
int launch_smooth(sf_ctx* ctx, float* cube, int nx, int ny, int64_t n_img,
                  const double* d_w, int R, unsigned flags);
constexpr int kTessMaxR = 24;  // Gaussian radius of the fused tess kernel
// one-plane value fill (tess_values.hip): table pass + gather (R = 0) or the
// fused tile kernel (R <= kTessMaxR); the two passes for any R over one-plane
// images, scrubbing NaN to 0
int launch_tess_values(sf_ctx* ctx, const int32_t* labels, int nx, int ny,
                       const double* values, int D, int64_t S, float* out, int64_t ring,
                       const double* d_w, int R, unsigned flags);
int launch_values_smooth(sf_ctx* ctx, float* cube, int nx, int ny, int64_t n_img,
                         const double* d_w, int R, unsigned flags);
}  // namespace sf
