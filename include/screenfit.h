/*
 * screenfit.h -- C ABI of the MI355X-native KL a-term screen library
 * (libscreenfit.so, hand-written HIP for gfx950).
 *
 * Drop-in boundary for the hot path of ska-sdp-screen-fitting v0.1.0
 * (reference at /root/reference, paths below relative to
 * src/ska_sdp_screen_fitting/).  The reference is pure Python with no FFI;
 * each entry point names the Python interface it replaces:
 *
 *   sf_set_basis  <- stationscreen._calculate_piercepoints / _calculate_svd
 *                    (stationscreen.py:70-110, 390-430; run :1046-1053)
 *   sf_kl_fit     <- stationscreen.run -> _process_single_freq ->
 *                    _process_station -> _fit_screen
 *                    (stationscreen.py:858-1161, 785-855, 597-782, 433-594)
 *   sf_set_piercepoints <- the piercepoint / r_0 / beta attributes that
 *                    KLScreen.make_matrix reads from the screen soltab and
 *                    hands to calculate_kl_screen (kl_screen.py:228-261,
 *                    411-449): the evaluation-only geometry, no eigen-basis
 *   sf_set_grid   <- KLScreen.make_matrix coordinate block
 *                    (kl_screen.py:228-261)
 *   sf_kl_eval    <- KLScreen.make_matrix + calculate_kl_screen + the NaN
 *                    scrub of Screen.write (kl_screen.py:192-449,
 *                    screen.py:343-378)
 *   sf_set_points / sf_kl_eval_points / sf_kl_eval_point_values <-
 *                    calculate_kl_screen at a list of positions instead of
 *                    every pixel (kl_screen.py:411-449) and the Jones terms
 *                    make_matrix forms from it (kl_screen.py:319-378)
 *   sf_set_tec_freqs / sf_kl_eval_tec <- no counterpart: the reference fits
 *                    tec soltabs (stationscreen.py:858-1161) but never turns
 *                    them into phases.  The Jones cube of TEC screens (and a
 *                    frequency-independent phase screen) at many channels,
 *                    one contraction per (time, station)
 *
 * Conventions
 *  - Plain C types only.  Return 0 on success, a negative errno-style code
 *    on failure (SF_EINVAL bad shape/argument, SF_ENOMEM, SF_EIO HIP
 *    failure, SF_ENODEV no usable gfx950 device); sf_last_error() gives a
 *    thread-local message.
 *  - Array arguments of sf_kl_fit / sf_kl_eval are DEVICE pointers (HBM,
 *    e.g. from sf_alloc or any HIP allocator); small geometry arrays
 *    (piercepoints, grid coordinates, per-station orders) are HOST pointers.
 *    The caller owns every buffer it passes; the library never frees caller
 *    memory.  Device scratch (basis, pixel matrix) is owned by the context.
 *  - Work is enqueued on the context's stream (sf_set_stream); calls return
 *    once enqueued except sf_set_basis/sf_get_basis/sf_copy_* which
 *    synchronise.  Calls on one context must be serialised by the caller;
 *    contexts on different devices may be driven from different threads.
 *  - Slot layout is the H5parm scalarphase layout [time][freq][ant][dir]
 *    (stationscreen.py:936-963, kl_screen.py:269-272): slot index
 *    s = (t * F + f) * A + a.  The evaluated cube is the FITS a-term cube
 *    layout [time][freq][ant][4][y][x] (screen.py:319-351), native-endian
 *    float32, planes (Re XX, Im XX, Re YY, Im YY).
 */
#ifndef SCREENFIT_H
#define SCREENFIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_OK 0
#define SF_EINVAL (-22)
#define SF_ENOMEM (-12)
#define SF_EIO (-5)
#define SF_ENODEV (-19)

#define SF_MAX_DIR 60 /* directions per slot of sf_set_basis / sf_kl_fit (one
                         wavefront lane each; LDS-bound) */
/* directions per slot of sf_set_basis_wide and of sf_kl_fit after it (above
 * SF_MAX_DIR: one workgroup per slot, kl_fit_wide.hip) */
#define SF_MAX_FIT_DIR 128
/* directions per slot of the pixel side: sf_set_piercepoints, sf_set_grid,
 * sf_kl_eval / _gain / _sums and sf_tess_fill */
#define SF_MAX_EVAL_DIR 128

/* screen types of stationscreen.run (stationscreen.py:922-928) */
#define SF_SCREEN_PHASE 0
#define SF_SCREEN_TEC 1
#define SF_SCREEN_AMPLITUDE 2 /* log10 fit; sigma per station block (Q6) */

/* sf_kl_eval flags */
#define SF_EVAL_NAN_SCRUB 1u /* NaN -> 1 (real planes), 0 (imag) (screen.py:368-378) */
#define SF_EVAL_FAST_SINCOS (1u << 8) /* exact fp64 reduction of the phase in
                                         revolutions + hardware fp32 sincos
                                         (|err| <= 2.3e-7) instead of fp64
                                         sincos */
#define SF_EVAL_NT_STORES (1u << 9) /* non-temporal (streaming) cube stores */
#define SF_EVAL_BIG_ENDIAN (1u << 10) /* store big-endian float32 (the FITS
                                         byte order), for direct file writes */

typedef struct sf_ctx sf_ctx;

/* Operator parameters of stationscreen.run (stationscreen.py:858-871). */
typedef struct sf_fit_params {
  int screen_type;  /* SF_SCREEN_PHASE, _TEC or _AMPLITUDE */
  int niter;        /* outlier-flagging iterations (phase: 2), 1..64: anything
                       else is SF_EINVAL */
  double nsigma;    /* outlier threshold in circular sigmas (5.0) */
  int adjust_order; /* adapt the order toward reduced chi^2 ~ 1 (1) */
  int ref_ant;      /* GLOBAL reference station index, -1 = none */
  int ant_offset;   /* global index of this call's station 0 (ant shards) */
  const double* ref_phase; /* device [T][F][D] phases of the reference
                              station when it is not in this shard; NULL =
                              read them from station ref_ant - ant_offset.
                              SF_SCREEN_TEC with ref_ant == -1 is referenced
                              to the LAST station of the whole soltab (quirk
                              Q15): ref_phase holds that station's values;
                              NULL = this call's last station, right only
                              for an unsharded call or the shard that holds
                              the global last station.  Never read for
                              SF_SCREEN_AMPLITUDE, nor for SF_SCREEN_PHASE
                              with ref_ant == -1 */
} sf_fit_params;

/* Library / device management */
const char* sf_version(void);
const char* sf_last_error(void);
int sf_create(int device, sf_ctx** out);
int sf_destroy(sf_ctx* ctx);
int sf_set_stream(sf_ctx* ctx, void* hip_stream); /* NULL = default stream */
int sf_synchronize(sf_ctx* ctx);
/* A HIP stream whose kernels may only use the compute units NOT listed in
 * reserve_cus (CU indices 0..n_cu-1; the reserved units stay free for work
 * on other streams, e.g. the fit of the next time chunk while the current
 * chunk is evaluated).  n_reserve = 0 gives an ordinary stream. */
int sf_stream_create(sf_ctx* ctx, const int* reserve_cus, int n_reserve,
                     void** hip_stream);
int sf_stream_destroy(sf_ctx* ctx, void* hip_stream);
int sf_device_cus(sf_ctx* ctx, int* n_cu);
/* Options: SF_OPT_FIT_GENERAL = 1 routes every slot through the general
 * (per-slot Jacobi) fit kernel instead of the mask-cached eigenbasis
 * pipeline; both give the reference's results (used to cross-check). */
#define SF_OPT_FIT_GENERAL 1
/* SF_OPT_EVAL_KERNEL selects the evaluation kernel of sf_kl_eval (all give
 * the same values): AUTO (default), TILE = register-tile stores (4 slots x
 * 256 B per store instruction; always used for fp64 sincos and gain
 * screens), LDS4 / LDS8 / LDS16 = LDS-staged stores with 1 / 2 / 4 KiB
 * contiguous runs per (slot, plane).  Ignored for D > 60
 * (SF_EVAL_KERNEL_WIDE). */
#define SF_OPT_EVAL_KERNEL 2
/* SF_OPT_EVAL_MAX_BLOCKS caps the workgroups of an evaluation launch (0 =
 * the dispatch limit); each workgroup then walks several (pixel block, slot
 * chunk) items.  For tests of that walk. */
#define SF_OPT_EVAL_MAX_BLOCKS 3
/* SF_OPT_FIT_PACK = 0 runs one slot per wavefront in the fit also for
 * D <= 32 (default 1: two slots per wavefront; same results bit for bit). */
#define SF_OPT_FIT_PACK 4
/* SF_OPT_EVAL_KS_PAD = n (0..3) runs the evaluation contraction with n extra
 * all-zero k-steps of 4 directions (same values; tuning / diagnostics). */
#define SF_OPT_EVAL_KS_PAD 5 /* (ignored for D > 60) */
/* SF_OPT_EVAL_SLEEP = n: LDS-staged evaluation waves sleep n x 64 cycles
 * after each 16-slot contraction (store-throttling experiments; default 0). */
#define SF_OPT_EVAL_SLEEP 6
/* SF_OPT_EVAL_XCD_MAP: workgroup -> pixel-block map of the evaluation
 * kernels.  0: XCD x (workgroups are dealt round-robin over the 8 XCDs)
 * takes a contiguous eighth of the pixel blocks; 1: XCD x takes the pixel
 * blocks pb = x (mod 8); -1 (default): 1 when an XCD's eighth is at most 8
 * pixel blocks (256^2 with 4 KiB runs: +2-3 % measured), else 0. */
#define SF_OPT_EVAL_XCD_MAP 7
/* SF_OPT_EVAL_GROUPS = g (1..256, power of two; 0 = auto: 64 for the
 * register-tile kernels, 16 for the LDS-staged ones): most 16-slot groups per
 * evaluation work item (each item loads its pixel block's basis once, so
 * longer items re-read less of it). */
#define SF_OPT_EVAL_GROUPS 8
/* SF_OPT_EVAL_BANDS = b (1..128, power of two; 0 = auto): the evaluation
 * runs its work items band-major over b pixel bands (every slot chunk of the
 * first 1/b of the pixel blocks, then the next ...), so each XCD's live slice
 * of the pixel basis is 1/b of its share.  Auto: bands of 128 pixel blocks
 * (with the interleaved XCD map) for the register-tile kernels on grids of
 * >= 1024 blocks (512^2 and up), else 1.  Ignored where the pixel blocks of a
 * band would not divide by 8.  Outputs are identical for every b. */
#define SF_OPT_EVAL_BANDS 9
/* SF_OPT_FIT_LEAN = 0 / 1 (default 1): when every slot's unflagged weights
 * are equal (counted by the classify kernel), the fit passes run a variant
 * with no per-slot normal-matrix / subset-basis copies in LDS (flagged slots
 * read their subset basis from the pool), for 2.7-4x the resident waves.
 * Same results bit for bit; 0 forces the general layout. */
#define SF_OPT_FIT_LEAN 10
/* SF_OPT_TESS_SLOTS = n (0 = auto 16, else 1..256): slots per work item of
 * the unsmoothed tessellated fill (the item's value-table slice sits in
 * LDS); SF_OPT_TESS_WAVES = 4, 8 or 16 (0 = auto 16): its waves per
 * workgroup, each writing whole 4 KiB runs of its own slots.  Outputs are
 * identical for every setting. */
#define SF_OPT_TESS_SLOTS 11
#define SF_OPT_TESS_WAVES 12
/* SF_OPT_TESS_TILE = 1 runs sf_tess_fill (radius <= 24) on the round-1 fused
 * 16 x 16 tile kernel instead of the table + gather / wide-tile smoothing
 * kernels (same bits; for cross-checks). */
#define SF_OPT_TESS_TILE 13
/* SF_OPT_TESS_BOX = 1: sf_tess_fill with smoothing (radius <= 24) stores
 * the pixels whose whole (2R + 1)^2 neighbourhood is one cell from a
 * per-(slot, cell) value and sums only the others (kl_tess_box_kernel); 0:
 * the wide-tile kernel that sums every pixel; -1 (default): the first for
 * four planes (XX / YY amplitudes) at radius <= 5, else the second.  Same
 * bits. */
#define SF_OPT_TESS_BOX 14
/* SF_OPT_EVAL_INT = 0 evaluates with the fp64 MFMA contraction everywhere;
 * -1 (default): the integer-digit contraction -- Cpix and the coefficients
 * as 6 balanced base-256 digits of 36- / 44-bit fixed point, contracted
 * exactly on i8 MFMAs (64x the fp64 MFMA rate per product) modulo 2^32
 * turns -- for phase screens with D >= 45, on the fast (hardware sincos)
 * epilogue with float4-aligned output (gain screens keep fp64); slots whose
 * coefficients are not finite or out of the digit range take the fp64
 * contraction.  |error| < 2^-27 turn of phase over the allowed ranges
 * (7.06e-9 turn at D = 60, |coef / 2 pi| = 8.03 turns, |Cpix| = 1905 with
 * every rounding aligned; ~2^-32 at the BASELINE configs), below the fp32
 * rounding of the reduced phase (up to 2^-26 turn); it runs in the register
 * tile, the SHB tile (pixel digits shared in LDS by 4 waves) and the
 * LDS-staged kernels alike (same bits; sf_get_eval_kernel /
 * sf_get_eval_contraction say which).  Ignored for D > 60 (fp64). */
#define SF_OPT_EVAL_INT 15
/* SF_OPT_EVAL_WG_WAVES: waves per workgroup of the integer-digit register
 * tile -- 4 (0 = default: 256 pixels, 1 KiB store runs per (slot, plane)) or
 * 8 (512 pixels, 2 KiB runs).  Same bits.  It acts ONLY on the register tile
 * (SF_EVAL_KERNEL_TILE / TILE3) running the integer-digit contraction
 * (sf_get_eval_contraction == 1); the fp64 contraction, the LDS-staged
 * kernels and SF_EVAL_KERNEL_SHB always run 4-wave workgroups and ignore it
 * (the Python binding's eval_kernel() names the 8-wave variant when it runs).
 * Ignored for D > 60. */
#define SF_OPT_EVAL_WG_WAVES 16
/* SF_OPT_FIT_EIG_WAVES: waves per flagged-direction mask of the subset-basis
 * Jacobi in sf_kl_fit -- 1..4 (0 = default: 3).  Every count writes the same
 * bits (the rotations and their per-element arithmetic do not depend on how
 * a round's column pairs are split over the waves). */
#define SF_OPT_FIT_EIG_WAVES 17
/* SF_OPT_FIT_SUBSET_DELETION: the flagged-direction subset bases by
 * secular-equation deletions (Loewner-corrected vectors), one per flagged
 * direction, the Jacobi solve only for the masks the deletions cannot
 * separate.  3 = each mask starts from its nearest ancestor in the mask
 * table that the deletions built (the mask with its lowest flagged
 * directions unflagged; the global basis when none is), one launch per
 * number of flagged directions; 2 = every mask from the global basis, one
 * launch; 1 (default) = 3 for a fit pass with many new masks, else 2;
 * 0 = the Jacobi solve for every mask.  1, 2 and 3 write the same bits. */
#define SF_OPT_FIT_SUBSET_DELETION 18
/* SF_OPT_FIT_WIDE_CACHE: the mask cache of the fit above SF_MAX_DIR
 * directions (sf_set_basis_wide) -- 1 (default): every distinct flag mask of
 * a call's input is decomposed once, into a pool that the slots carrying the
 * mask share; 0: every flagged slot decomposes its own subset covariance.
 * Same bits either way; any other value is SF_EINVAL.  Ignored for
 * D <= SF_MAX_DIR. */
#define SF_OPT_FIT_WIDE_CACHE 19
/* SF_OPT_FIT_WIDE_POOL_MB: cap of that pool's device memory in MiB, 1..65536
 * (0 = default: 2048).  An entry takes (D (D | 1) + 2 D) doubles: 2 GiB hold
 * 16,008 masks at D = 128, 40,427 at D = 80.  Masks beyond the cap get no
 * entry: their slots decompose their own subset (same bits). */
#define SF_OPT_FIT_WIDE_POOL_MB 20
/* SF_OPT_FIT_WIDE_POOL_MAX: cap of the pool's number of entries (0 = default:
 * none beyond the byte cap); a small value forces the fallback above. */
#define SF_OPT_FIT_WIDE_POOL_MAX 21
/* SF_OPT_FIT_LANE = 0 / 1 (default 1): phase fits with 3..23 directions give
 * the slots that start with every direction unflagged and one weight to a
 * kernel that fits one slot per lane (64 consecutive slots per wavefront),
 * and the pass kernel walks a list of the other slots instead of all of
 * them.  A lane slot whose order walk moves, or with a phase that is not
 * finite, goes back to the pass kernel.  Same results bit for bit; 0 (and
 * SF_OPT_FIT_PACK = 0) runs every slot through the pass kernel. */
#define SF_OPT_FIT_LANE 22
#define SF_EVAL_KERNEL_AUTO 0
#define SF_EVAL_KERNEL_TILE 1
#define SF_EVAL_KERNEL_LDS4 2
#define SF_EVAL_KERNEL_LDS8 3
#define SF_EVAL_KERNEL_LDS16 4
#define SF_EVAL_KERNEL_LDS8H 5 /* LDS-staged, 2 MFMA tiles per wave (large D) */
#define SF_EVAL_KERNEL_LDS16H 6
#define SF_EVAL_KERNEL_TILE3 7 /* register tile at 3 waves per SIMD */
#define SF_EVAL_KERNEL_SHB 8 /* register tile, Cpix (or its digits) shared in LDS by 4 waves */
/* D > 60 (16..32 k-steps, after sf_set_piercepoints): the wide kernel
 * (kl_eval_wide.hip) -- run-time k-loop, Cpix of a 64-pixel block in LDS,
 * fp64 contraction (SF_EVAL_CONTRACTION_F64), exact phase reduction.  It is
 * the only kernel there: SF_OPT_EVAL_KERNEL, SF_OPT_EVAL_INT,
 * SF_OPT_EVAL_KS_PAD and SF_OPT_EVAL_WG_WAVES are ignored above 60 directions
 * (SF_OPT_EVAL_MAX_BLOCKS, _GROUPS, _BANDS and _XCD_MAP are honoured).  As a
 * value of SF_OPT_EVAL_KERNEL it is accepted and means AUTO for D <= 60. */
#define SF_EVAL_KERNEL_WIDE 9
/* The evaluation kernel sf_kl_eval (gain = 0) or sf_kl_eval_gain (gain = 1)
 * runs for the current grid and these flags on a 16-byte aligned output
 * (one of SF_EVAL_KERNEL_TILE / _LDS4 / _LDS8 / _LDS16 ..., or
 * SF_EVAL_KERNEL_WIDE for every call with D > 60). */
int sf_get_eval_kernel(sf_ctx* ctx, int gain, unsigned flags, int* kernel);
/* The contraction of that evaluation: SF_EVAL_CONTRACTION_F64 (fp64 MFMAs) or
 * SF_EVAL_CONTRACTION_I8_DIGITS (the integer-digit contraction,
 * SF_OPT_EVAL_INT). */
#define SF_EVAL_CONTRACTION_F64 0
#define SF_EVAL_CONTRACTION_I8_DIGITS 1
int sf_get_eval_contraction(sf_ctx* ctx, int gain, unsigned flags, int* contraction);
int sf_set_option(sf_ctx* ctx, int option, int value);
int sf_alloc(sf_ctx* ctx, size_t bytes, void** dev_ptr);
int sf_free(sf_ctx* ctx, void* dev_ptr);
int sf_copy_h2d(sf_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int sf_copy_d2h(sf_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/*
 * Shared KL basis from the D piercepoints (host, [D][3] float64, the
 * "piercepoint" array of the screen soltab): C[i][j] =
 * -(|pp_i - pp_j|^2 / r0^2)^(beta/2) / 2, its pseudo-inverse with absolute
 * cutoff 1e-3 (scipy>=1.7 pinv(rcond=1e-3) semantics) and U = the left
 * singular vectors of C ordered by descending singular value.  Computed on
 * the device (wavefront Jacobi eigen-solver).  1 <= D <= SF_MAX_DIR.
 */
int sf_set_basis(sf_ctx* ctx, const double* pp_host, int D, double r0,
                 double beta);
/*
 * sf_set_basis for 1 <= D <= SF_MAX_FIT_DIR.  For D <= SF_MAX_DIR it IS
 * sf_set_basis (basis, fit and evaluation bit for bit).  For 61..128
 * directions it computes C, pinv(C) (absolute cutoff 1e-3), U (columns by
 * descending |lambda|, ties by index) and the eigenvalues on the device with
 * a workgroup Jacobi solver, binds the evaluation geometry exactly as
 * sf_set_piercepoints does (sf_set_grid and sf_kl_eval* afterwards write the
 * same bytes as after sf_set_piercepoints) and marks the context as holding
 * a wide basis.  It synchronises and invalidates the pixel grid; a failed
 * call leaves the context usable (no geometry, as after sf_create).
 * On a wide-basis context:
 *  - sf_get_basis returns the basis in the same layout;
 *  - sf_kl_fit keeps its contract (screen types, niter, nsigma,
 *    adjust_order, ref_ant / ant_offset / ref_phase, the block and
 *    reference-station skips, NULL resid / w_out / order_out) on the wide
 *    fit: one workgroup per slot.  Every distinct flag mask of the call's
 *    input is decomposed once, before the first pass, into a pool of subset
 *    bases keyed by the 128-bit mask (SF_OPT_FIT_WIDE_CACHE, _POOL_MB,
 *    _POOL_MAX); a slot whose mask has an entry reads it, and a slot whose
 *    mask has none -- the cache off, the pool full, or a mask that outlier
 *    flags created in a later pass and that no slot of the input carries --
 *    decomposes its own subset covariance.  Same bits in every case.  Every
 *    sf_kl_fit rebuilds the pool; it lives until the next sf_kl_fit,
 *    sf_set_basis*, sf_set_piercepoints or sf_destroy, so an idle context
 *    can hold up to the pool cap (2 GiB by default; the largest pool any
 *    call on this geometry built) plus up to 68 bytes per slot of the
 *    largest call for the keys and the table and 16 bytes per entry.  The
 *    other SF_OPT_FIT_* options are
 *    ignored above SF_MAX_DIR directions.  The context keeps a workspace
 *    for the matrices that do not fit the LDS: (3 - m) D (D | 1) doubles
 *    per workgroup of the persistent grid, m = matrices that fit 160 KiB,
 *    one workgroup per CU (64.5 MiB at D = 128 on 256 CUs, 19 MiB at D = 96,
 *    13 MiB at D = 80, none for D <= 79),
 *    freed by sf_destroy and by the next sf_set_basis* / sf_set_piercepoints;
 *  - sf_get_fit_stats reports in n_masks the number of subset
 *    decompositions the last fit ran -- pool entries built plus the
 *    decompositions slots ran for themselves -- and n_general = 0.  With the
 *    cache on it is never above the count with the cache off.  When the pool
 *    overflows, which masks get entries follows the order the masks were
 *    numbered in, which is not deterministic: the count may then vary from
 *    run to run (the fit's output does not);
 *  - sf_get_fit_pool returns SF_EINVAL (its mask keys are 64-bit);
 *    sf_get_fit_pool_wide returns the pool.
 */
int sf_set_basis_wide(sf_ctx* ctx, const double* pp_host, int D, double r0,
                      double beta);
/* Copy the device basis back (host [D][D] each; any pointer may be NULL).
 * SF_EINVAL on a context whose geometry came from sf_set_piercepoints. */
int sf_get_basis(sf_ctx* ctx, double* c_host, double* pinv_c_host,
                 double* u_host, double* eig_host);

/*
 * Evaluation-only geometry: the D piercepoints (host, [D][3] float64), r0
 * and beta that sf_set_grid and sf_kl_eval* read -- the pixel basis
 * Cpix[p][d] = -(|pp_d - (x_p, y_p, 0)|^2 / r0^2)^(beta/2) / 2 of
 * calculate_kl_screen (kl_screen.py:411-449) needs nothing else.
 * 1 <= D <= SF_MAX_EVAL_DIR, r0 > 0.  No eigen-basis is computed or
 * allocated: on such a context sf_kl_fit and sf_get_basis return SF_EINVAL
 * until sf_set_basis is called (which makes it a full context again).  Like
 * sf_set_basis it invalidates the pixel grid; a failed call leaves the
 * context usable (no geometry, as after sf_create).  For D <= SF_MAX_DIR the
 * evaluation is bit for bit the one after sf_set_basis with the same
 * arguments.
 */
int sf_set_piercepoints(sf_ctx* ctx, const double* pp_host, int D, double r0,
                        double beta);

/*
 * Batched KL least-squares fit of all T*F*A slots (one scalar-phase or tec
 * soltab, one pol).  Device inputs: phase [T][F][A][D] float64 (radians,
 * NOT yet referenced -- the reference-station subtraction of
 * stationscreen.py:994-997 is done here), weight [T][F][A][D] float32.
 * Host input: station_order [A] (the initial per-station order,
 * stationscreen.py:999-1034).  Device outputs (any may be NULL except
 * coef): coef [T][F][A][D] float64 (the "phase_screen000" values),
 * resid [T][F][A][D] float64, w_out [T][F][A][D] float32 (weights after
 * outlier flagging), order_out [T][F][A] int32 (orders, the weights of the
 * "...resid" soltab).  Requires sf_set_basis (D <= SF_MAX_DIR) or
 * sf_set_basis_wide (D <= SF_MAX_FIT_DIR) with the same D
 * (sf_set_piercepoints does not serve: SF_EINVAL).
 */
int sf_kl_fit(sf_ctx* ctx, const double* phase, const float* weight, int T,
              int F, int A, const int* station_order_host,
              const sf_fit_params* params, double* coef, double* resid,
              float* w_out, int32_t* order_out);

/* Statistics of the last sf_kl_fit (synchronises): number of distinct
 * flagged-direction masks whose subset basis was decomposed, and number of
 * slots that took the general (tiny-weight) path.  (Wide-basis context:
 * see sf_set_basis_wide.) */
int sf_get_fit_stats(sf_ctx* ctx, int* n_masks, int* n_general);

/* Of the last sf_kl_fit (synchronises): the slots the lane-per-slot kernel
 * took (SF_OPT_FIT_LANE) and how many of those it handed back to the pass
 * kernel.  Both 0 where that kernel did not run. */
int sf_get_fit_lane_stats(sf_ctx* ctx, int64_t* n_lane, int64_t* n_deferred);

/* The subset bases the last sf_kl_fit decomposed (a test / inspection
 * hook; every call renumbers and rebuilds its pool): up to max_masks
 * entries, each its direction mask (masks_host[i], bit d = direction d
 * unflagged, n bits set) and a [D][D] block whose leading n x n part holds
 * the subset's eigenvectors (row = unflagged direction in index order,
 * columns sorted by |lambda| descending) followed by D slots whose first n
 * hold its eigenvalues (entries_host[i * (D*D + D)]); the rest of an entry
 * is unspecified.  Entries are in the order the
 * masks were numbered, which is not deterministic; *n_masks = how many
 * exist.  Synchronises.  SF_EINVAL on a wide-basis context. */
int sf_get_fit_pool(sf_ctx* ctx, uint64_t* masks_host, double* entries_host,
                    int max_masks, int* n_masks);
/* sf_get_fit_pool on a wide-basis context (sf_set_basis_wide with more than
 * SF_MAX_DIR directions), with 128-bit keys: the pool entries the last
 * sf_kl_fit built (none with SF_OPT_FIT_WIDE_CACHE = 0).  masks_host[2 i]
 * holds the bits of directions 0..63 of entry i and masks_host[2 i + 1] those
 * of directions 64..127 (bit = direction unflagged, n bits set in all);
 * entries_host[i * (D*D + D)] is a [D][D] block whose leading n x n part
 * holds the subset's eigenvectors (row = unflagged direction in index order,
 * columns sorted by |lambda| descending, ties by index) followed by D slots
 * whose first n hold its eigenvalues; the rest of an entry is zero.  Entries
 * are in the order the masks were numbered, which is not deterministic;
 * *n_masks = how many exist.  Synchronises.  SF_EINVAL on a context that
 * does not hold a wide basis. */
int sf_get_fit_pool_wide(sf_ctx* ctx, uint64_t* masks_host, double* entries_host,
                         int max_masks, int* n_masks);

/*
 * Pixel grid of the a-term image: X[nx], Y[ny] screen coordinates of the
 * diagonal pixels (kl_screen.py:247-259, quirk Q8: pixel (y=j, x=i) is
 * evaluated at (X[i], Y[j])).  Builds the [nx*ny][D] pixel basis on the
 * device in MFMA fragment order.  Requires sf_set_basis or
 * sf_set_piercepoints first (D <= SF_MAX_EVAL_DIR).
 */
int sf_set_grid(sf_ctx* ctx, const double* x_host, int nx,
                const double* y_host, int ny);

/*
 * KL pixel evaluation of S slots: phase[s][p] = sum_d Cpix[p][d]*coef[s][d]
 * (float64, MFMA), written as the 4 Jones planes (cos, sin, cos, sin) in
 * float32 to out[(s % ring_slots)][4][ny][nx] (device).  ring_slots >= S
 * writes every slot to its own place; smaller rings let a benchmark stream
 * an output volume larger than HBM.  coef: device [S][D] float64.
 * D <= SF_MAX_EVAL_DIR (above SF_MAX_DIR: SF_EVAL_KERNEL_WIDE); the same
 * holds for sf_kl_eval_gain and sf_kl_eval_sums.
 */
int sf_kl_eval(sf_ctx* ctx, const double* coef, int64_t S, float* out,
               int64_t ring_slots, unsigned flags);

/*
 * Gain screens (kl_screen.py:319-378): three KL screens on the same pixel
 * basis -- phase and the XX / YY log10-amplitude screens -- written as
 * (10^xx cos, 10^xx sin, 10^yy cos, 10^yy sin).  Device coef arrays [S][D].
 */
int sf_kl_eval_gain(sf_ctx* ctx, const double* coef_phase,
                    const double* coef_xx, const double* coef_yy, int64_t S,
                    float* out, int64_t ring_slots, unsigned flags);
/* sf_kl_eval / sf_kl_eval_gain (coef_xx = coef_yy = NULL: phase screens)
 * that also ADD, mod 2^32, to slot_sums[s] (device, uint32, zeroed by the
 * caller) the checksum of slot s's output: the sum mod 2^32 of the 4 N^2
 * 32-bit words written for it (as stored, after the NaN scrub / byte swap;
 * SURVEY.md §8(d) "per-slot sum of fp32 words").  Order-free
 * integer sums, so a slot streamed through a ring in a large run and the same
 * slot evaluated alone give the same value: the discard + checksum mode of
 * volumes that do not fit HBM. */
int sf_kl_eval_sums(sf_ctx* ctx, const double* coef_phase,
                    const double* coef_xx, const double* coef_yy, int64_t S,
                    float* out, int64_t ring, unsigned flags,
                    uint32_t* slot_sums);

/*
 * Screen VALUES on the pixel grid (kl_values.hip): what calculate_kl_screen
 * (kl_screen.py:411-449) returns, and what the reference's "tec" a-term cube
 * stores per pixel (processing_utils.py:187-190), without the cos / sin of the
 * Jones planes:
 *   out[(s % ring_slots)][ny][nx] = (float) sum_d Cpix[p][d] * coef[s][d]
 * (device float32; rad, TECU or log10 amplitude, whatever was fitted).  The
 * contraction is float64 with one cast at the store (Q12); pixel order and grid
 * are sf_kl_eval's (Q8, sf_set_grid).  coef: device [S][D] float64.  Needs
 * sf_set_grid on the geometry of sf_set_basis, sf_set_basis_wide or
 * sf_set_piercepoints; one kernel serves 1 <= D <= SF_MAX_EVAL_DIR.
 * flags: SF_EVAL_NAN_SCRUB (NaN -> 0.0f, the value whose Jones term is the
 * 1 / 0 of the gain scrub), SF_EVAL_NT_STORES (honoured for 16-byte-aligned
 * output and nx * ny % 4 == 0), SF_EVAL_BIG_ENDIAN; any other bit is
 * SF_EINVAL.  Without the scrub a NaN coefficient gives a NaN plane for its
 * slot and leaves the others alone.  ring_slots >= S gives every slot its own
 * place; with a shorter ring an entry ends up holding the last slot that maps
 * to it.  The output needs 4-byte alignment only (unaligned or odd-sized
 * outputs take scalar stores).  SF_OPT_EVAL_MAX_BLOCKS, _GROUPS, _BANDS and
 * _XCD_MAP are honoured.  Enqueued on the context stream; does not
 * synchronise.
 */
int sf_kl_eval_values(sf_ctx* ctx, const double* coef, int64_t S, float* out,
                      int64_t ring_slots, unsigned flags);

/*
 * Polarized phase screens (kl_eval_pol.hip): the a-term of a DIAGONAL gain
 * whose XX and YY terms each carry their own phase, as the phase000 soltab of
 * a diagonal-mode solve does on its pol axis.  Extends the gain screens of
 * kl_screen.py:319-378, which take ONE phase per slot; the reference has no
 * polarized-phase rendering.  Device coefficient arrays [S][D] float64 on the
 * same pixel basis; with phi_p = sum_d Cpix[.][d] * phase_p[s][d] and
 * a_p = 10^(sum_d Cpix[.][d] * amp_p[s][d]) it writes
 *   out[(s % ring_slots)][4][ny][nx] =
 *       (a_xx cos phi_xx, a_xx sin phi_xx, a_yy cos phi_yy, a_yy sin phi_yy)
 * (device float32).  phase_xx and phase_yy are both required; amp_xx and
 * amp_yy are both given or both NULL (a_p = 1); anything else is SF_EINVAL.
 * The contractions are float64 and share the Cpix operand; the reduction in
 * revolutions is exact (SF_EVAL_FAST_SINCOS; without the flag fp64 sincos and
 * fp64 10^x with one cast).  With phase_yy == phase_xx the cube is bit for bit
 * what SF_EVAL_KERNEL_WIDE gives for sf_kl_eval / sf_kl_eval_gain.  Needs
 * sf_set_grid on the geometry of sf_set_basis, sf_set_basis_wide or
 * sf_set_piercepoints; one kernel serves 1 <= D <= SF_MAX_EVAL_DIR.
 * flags: SF_EVAL_NAN_SCRUB, SF_EVAL_FAST_SINCOS, SF_EVAL_NT_STORES (honoured
 * for 16-byte-aligned output and nx * ny % 4 == 0), SF_EVAL_BIG_ENDIAN; any
 * other bit is SF_EINVAL.  The output needs 4-byte alignment only.  NaN
 * semantics are per polarization: a NaN coefficient of phase_yy or amp_yy in
 * slot k gives NaN in planes 2 and 3 of slot k (1 / 0 under the scrub) and
 * touches nothing else -- planes 0 and 1 of slot k are the bits of a clean run
 * -- and likewise for XX.  ring_slots >= S gives every slot its own place; with
 * a shorter ring an entry ends up holding the last slot that maps to it.  No
 * checksums.  SF_OPT_EVAL_MAX_BLOCKS, _GROUPS, _BANDS and _XCD_MAP are
 * honoured.  Enqueued on the context stream; does not synchronise.
 */
int sf_kl_eval_pol(sf_ctx* ctx, const double* phase_xx, const double* phase_yy,
                   const double* amp_xx, const double* amp_yy, int64_t S,
                   float* out, int64_t ring_slots, unsigned flags);

/*
 * Jones cubes of TEC screens at many channels (kl_tec.hip).  The phase of a
 * TEC screen at frequency nu is rad_per_tecu * dTEC with rad_per_tecu =
 * tec_to_phase / nu, so the F channels of one (time, station) share one
 * contraction and differ in the epilogue only.
 */
#define SF_MAX_TEC_FREQ 4096
/* Bind the F output channels (host arrays): channel f takes its screens from
 * TEC frequency tec_index[f] in 0..F_tec-1 (NULL = 0 for every f) and
 * multiplies them by rad_per_tecu[f].  F_tec is the frequency extent of the
 * coefficient arrays sf_kl_eval_tec will be given.  Synchronises, like
 * sf_set_points.  The binding lives until the next sf_set_tec_freqs or
 * sf_destroy; it does not depend on the geometry, so sf_set_basis* and
 * sf_set_piercepoints do not drop it.  SF_EINVAL for F outside
 * 1..SF_MAX_TEC_FREQ, F_tec < 1, an index out of range, a non-finite scale or
 * a NULL scale pointer; a failed call keeps the previous binding. */
int sf_set_tec_freqs(sf_ctx* ctx, const double* rad_per_tecu_host,
                     const int* tec_index_host, int F, int F_tec);
/*
 * Device inputs: tec_coef [T][F_tec][A][D] float64 in TECU (the layout of
 * "tec_screen000"); phase_coef NULL or the same shape in radians, the
 * frequency-independent phase screens of a tecandphase solution.  Device
 * output: out [T][F][A][4][ny][nx] float32, the FITS a-term layout, planes as
 * sf_kl_eval:
 *   out[t][f][a][.][p] = (cos, sin, cos, sin)(
 *       rad_per_tecu[f] * sum_d Cpix[p][d] * tec[t][i_f][a][d]
 *                       + sum_d Cpix[p][d] * ph[t][i_f][a][d] ),  i_f = tec_index[f].
 * Both contractions are float64 and run once per (t, TEC frequency, a); the
 * scale is applied to the contracted value, one float64 multiply in turns,
 * and the reduction in revolutions is exact (as sf_kl_eval with
 * SF_EVAL_FAST_SINCOS; without the flag, fp64 sincos).  Needs sf_set_grid on
 * the geometry of sf_set_basis, sf_set_basis_wide or sf_set_piercepoints, and
 * sf_set_tec_freqs (else SF_EINVAL, the message names the missing call); one
 * kernel serves 1 <= D <= SF_MAX_EVAL_DIR.  T * A < 2^31.
 * flags: SF_EVAL_NAN_SCRUB, SF_EVAL_FAST_SINCOS, SF_EVAL_NT_STORES (honoured
 * for 16-byte-aligned output and nx * ny % 4 == 0), SF_EVAL_BIG_ENDIAN; any
 * other bit is SF_EINVAL.  The output needs 4-byte alignment only.  A NaN
 * coefficient gives NaN planes in all F channels of its own (t, a) -- those of
 * its TEC frequency -- and nowhere else; with the scrub they are 1 / 0.  A TEC
 * frequency that no channel refers to is never read.  No ring and no
 * checksums.  SF_OPT_EVAL_MAX_BLOCKS, _GROUPS, _BANDS and _XCD_MAP are
 * honoured.  Enqueued on the context stream (one launch per TEC frequency that
 * has channels); does not synchronise.
 */
int sf_kl_eval_tec(sf_ctx* ctx, const double* tec_coef, const double* phase_coef,
                   int64_t T, int A, float* out, unsigned flags);

/*
 * Screens sampled at positions (kl_points.hip): the value
 * calculate_kl_screen (kl_screen.py:411-449) gives at each of P positions,
 * without a pixel grid or a cube.  The point basis Cpix[p][d] =
 * -(|pp_d - (x_p, y_p, 0)|^2 / r0^2)^(beta/2) / 2 is sf_set_grid's expression:
 * a point at (X[i], Y[j]) evaluates as pixel (y=j, x=i) of that grid.
 */
#define SF_MAX_POINTS 4096
/* P screen positions (host [P][2] float64: x, y in piercepoint coordinates).
 * Needs the geometry of sf_set_basis / sf_set_basis_wide / sf_set_piercepoints
 * (else SF_EINVAL); the next of those calls drops the points, as it drops the
 * grid.  Independent of sf_set_grid: both may be bound at once.  Synchronises. */
int sf_set_points(sf_ctx* ctx, const double* xy_host, int P);
/* Jones planes at the bound points (kl_screen.py:319-378 at positions):
 * device out [S][4][P] float32, planes as sf_kl_eval.  coef_xx and coef_yy
 * both NULL (phase screens) or both given (gain; as sf_kl_eval_gain).  Device
 * coef arrays [S][D] float64; the output needs 4-byte alignment only.  flags:
 * SF_EVAL_NAN_SCRUB, SF_EVAL_FAST_SINCOS; any other bit is SF_EINVAL. */
int sf_kl_eval_points(sf_ctx* ctx, const double* coef_phase, const double* coef_xx,
                      const double* coef_yy, int64_t S, float* planes, unsigned flags);
/* Screen values sum_d Cpix[p][d] coef[s][d] (kl_screen.py:411-449; rad, TECU
 * or log10 amplitude, whatever was fitted; NaN coefficients give NaN): device
 * out [S][P] float64. */
int sf_kl_eval_point_values(sf_ctx* ctx, const double* coef, int64_t S, double* values);

/*
 * Tessellated (Voronoi) screens: fill every pixel with the values of the
 * direction whose cell contains it, then (smooth_pix > 0) apply the Gaussian
 * of Screen.write.  Replaces VoronoiScreen.make_matrix + the smoothing loop
 * (voronoi_screen.py:132-216, screen.py:353-362).  Device inputs: labels
 * [ny][nx] int32 in 1..D, D <= SF_MAX_EVAL_DIR (the template of
 * make_rasertize_template), phase
 * [S][D] float64 (already referenced), amp_xx / amp_yy [S][D] float64 or NULL
 * (phase-only: amplitude 1).  Output as sf_kl_eval.  smooth_pix <= 6 runs
 * fused in one LDS-tiled kernel; larger values (any sigma, as scipy) gather
 * first and then run the passes of sf_smooth, which needs ring_slots >= S.
 * A label outside 1..D (the template never makes one) gives NaN pixels (1 / 0
 * under SF_EVAL_NAN_SCRUB); no table entry is read for it.
 */
int sf_tess_fill(sf_ctx* ctx, const int32_t* labels, int nx, int ny,
                 const double* phase, const double* amp_xx,
                 const double* amp_yy, int D, int64_t S, float* out,
                 int64_t ring_slots, double smooth_pix, unsigned flags);
/*
 * sf_tess_fill for tables with polarized phases: phase_yy [S][D] float64
 * (device, already referenced) is the phase of the YY term, so planes 2 and 3
 * take A_yy cos / sin of phase_yy where sf_tess_fill repeats the phase of
 * planes 0 and 1.  Extends voronoi_screen.py:132-216, which fills one phase
 * per direction; the reference has no polarized-phase rendering.  With
 * phase_yy == NULL it IS sf_tess_fill, bit for bit (sf_tess_fill is this
 * call).  Every smoothing path serves: fused up to smooth_pix = 6, sf_smooth
 * above (ring_slots >= S); labels outside 1..D give NaN (1 / 0 under the
 * scrub) in all four planes.
 */
int sf_tess_fill_pol(sf_ctx* ctx, const int32_t* labels, int nx, int ny,
                     const double* phase, const double* phase_yy,
                     const double* amp_xx, const double* amp_yy, int D, int64_t S,
                     float* out, int64_t ring_slots, double smooth_pix,
                     unsigned flags);

/*
 * Tessellated VALUE fill (tess_values.hip): one float32 plane per slot, the
 * values themselves instead of their Jones terms.  Extends
 * voronoi_screen.py:132-216 (VoronoiScreen.make_matrix) to values -- dTEC in
 * TECU, or anything else solved per direction -- and gives the tessellated
 * path the aterm_type="tec" cube of processing_utils.py:144-292; it is to
 * sf_tess_fill what sf_kl_eval_values is to sf_kl_eval.  Device inputs:
 * labels [ny][nx] int32 in 1..D (nx * ny < 2^31), values [S][D] float64
 * (already referenced), 1 <= D <= SF_MAX_EVAL_DIR.  Device output
 *   out[(s % ring_slots)][ny][nx] = g((float) values[s][labels[y][x] - 1])
 * float32, g the identity (smooth_pix = 0) or the Gaussian of sf_smooth per
 * image: float64 sums in scipy's order (centre first, then the pairs from the
 * outermost inwards, no contraction), float32 between the y pass and the x
 * pass, 'reflect' borders, truncated at 4 sigma -- where finite, bit for bit
 * plane 0 of sf_tess_fill(phase = 0, amp_xx = values).  A label outside 1..D
 * gives NaN and reads no table entry.  flags: SF_EVAL_NAN_SCRUB (NaN -> 0.0f
 * after smoothing: the value sf_kl_eval_values scrubs to, whose Jones term is
 * 1 / 0), SF_EVAL_BIG_ENDIAN, SF_EVAL_NT_STORES (honoured for 16-byte-aligned
 * output and nx * ny % 4 == 0); any other bit is SF_EINVAL.  ring_slots in
 * 1..INT32_MAX: with ring_slots < S an entry ends up holding the last slot
 * that maps to it.  smooth_pix in [0, 1e4]: a radius int(4 smooth_pix + 0.5)
 * <= 24 runs fused in one LDS-tiled kernel; a larger one gathers unscrubbed
 * and then runs the two separable passes, which needs ring_slots >= S.  The
 * output needs 4-byte alignment only (an unaligned output, or nx * ny % 4 !=
 * 0, takes scalar stores).  S = 0 is a no-op.  SF_OPT_TESS_SLOTS and
 * SF_OPT_TESS_WAVES are honoured by the unsmoothed fill.  Enqueued on the
 * context stream; does not synchronise, except for the weight upload when
 * smooth_pix changes (as sf_tess_fill).
 */
int sf_tess_fill_values(sf_ctx* ctx, const int32_t* labels, int nx, int ny,
                        const double* values, int D, int64_t S, float* out,
                        int64_t ring_slots, double smooth_pix, unsigned flags);

/*
 * The Gaussian smoothing of Screen.write (screen.py:353-362:
 * scipy.ndimage.gaussian_filter(., sigma=(0, smooth_pix, smooth_pix)) per
 * image, float32 between the y and x passes, 'reflect' borders, truncate
 * 4 sigma) in place on n_img images [n_img][ny][nx] float32 on the device --
 * the cube [S][4][ny][nx] is n_img = 4 S images (n_img must be a multiple of
 * 4).  SF_EVAL_NAN_SCRUB / SF_EVAL_BIG_ENDIAN in flags apply after smoothing,
 * as the reference scrubs after smoothing: evaluate without them, then
 * smooth with them.  Any smooth_pix (device pass buffer <= 256 MiB).
 */
int sf_smooth(sf_ctx* ctx, float* cube, int nx, int ny, int64_t n_img,
              double smooth_pix, unsigned flags);

#ifdef __cplusplus
}
#endif
#endif /* SCREENFIT_H */
