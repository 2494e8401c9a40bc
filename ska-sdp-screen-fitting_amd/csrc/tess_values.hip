// tess_values.hip -- tessellated (Voronoi) VALUE fill: one float32 plane per
// slot instead of the four Jones planes of tess.hip.
//
// Extends VoronoiScreen.make_matrix (voronoi_screen.py:132-216) to the values
// themselves -- the tessellated counterpart of sf_kl_eval_values and of the
// aterm_type="tec" cube of processing_utils.py:144-292:
//   out[s % ring][y][x] = g((float) values[s][label[y][x] - 1])
// with g = identity or the separable Gaussian of Screen.write (axis y then
// axis x, float32 between the passes, 'reflect' borders, scipy's
// symmetric-kernel summation order in float64: centre first, then the pairs
// from the outermost in, contraction off) -- the arithmetic of tess.hip on
// one plane, so a value fill is bit for bit plane 0 of
// sf_tess_fill(phase = 0, amp_xx = values) where that is finite.
//
// sf_tess_fill_values runs a per-slot value-table pass ([S][D + 1] float32,
// entry D = NaN for labels outside 1..D) and then
//  * tess_values_gather_kernel (no smoothing): scrub and byte swap are applied
//    to the table entries, the kernel is a pure gather-store;
//  * tess_values_smooth_kernel (radius 1..kTessMaxR): an LDS tile kernel, the
//    raw table widened to double per slot;
//  * above kTessMaxR the unscrubbed gather, then tess_values_pass_kernel
//    twice (axis y into a pass buffer, axis x back), scrubbing to 0.
// Ring entries are owned: the slots s, s + ring, s + 2 ring, ... of one entry
// are written by the same wave in ascending order, so an entry ends up holding
// the last slot that maps to it.
//
// reflect / walk_grid repeat tess.hip's: that file's code generation is pinned
// (profiles/tess_launch_isa.txt), so nothing of it moves to a header.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "sf_dispatch.h"
#include "sf_internal.h"

namespace sf {
namespace {

typedef float val_v4f __attribute__((ext_vector_type(4)));

constexpr int kValRun = 1024;      // pixels per gather work item (4 KiB)
// slots (ring entries) per gather work item and waves per workgroup
// (SF_OPT_TESS_SLOTS / SF_OPT_TESS_WAVES override them): 16 x 4 waves, 0.711 /
// 0.668 of 8 TB/s at 256^2 with D = 20 / 128, level with 32 x 8 (0.701 /
// 0.678) and ahead of tess.hip's 16 x 16 (0.454 / 0.419): four slots per wave
// and item amortise the labels and the table slice, which weigh four times as
// much per output byte as in the Jones fill (profiles/tess_values_sweep.txt)
constexpr int kValSlotsAuto = 16;
constexpr int kValWavesAuto = 4;
constexpr int kValTabCap = 65;                       // D <= 64
constexpr int kValTabCapWide = SF_MAX_EVAL_DIR + 1;  // D <= 128
constexpr int kValTW = 256;        // smoothing tile: pixels per row ...
constexpr int kValTH = 8;          // ... rows (wave w: rows w, w + 4) ...
constexpr int kValSmSlots = 8;     // ... and ring entries per work item
constexpr int kValMaxR = kTessMaxR;

__device__ __forceinline__ int val_reflect(int i, int n) {
  // scipy.ndimage mode 'reflect' (d c b a | a b c d | d c b a), closed form
  if (i >= 0 && i < n) return i;
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

// a finished value: NaN -> 0 under the scrub (the value whose Jones term is
// 1 / 0, as sf_kl_eval_values), then the FITS byte order
__device__ __forceinline__ float val_finish(float x, bool scrub, bool be) {
  if (scrub && isnan(x)) x = 0.0f;
  if (be) x = __uint_as_float(__builtin_bswap32(__float_as_uint(x)));
  return x;
}

// [S][D + 1] float32: (float)values[s][d], entry D = NaN; flags: the scrub
// and swap of an unsmoothed fill (the table entry IS the pixel), 0 otherwise
__global__ __launch_bounds__(256) void tess_values_table_kernel(
    const double* __restrict__ values, int D, int64_t S, float* __restrict__ tab,
    unsigned flags) {
  const int DT = D + 1;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S * DT) return;
  const int64_t s = e / DT;
  const int d = (int)(e - s * DT);
  const float v = d < D ? (float)values[s * D + d] : __builtin_nanf("");
  tab[e] = val_finish(v, flags & SF_EVAL_NAN_SCRUB, flags & SF_EVAL_BIG_ENDIAN);
}

// Unsmoothed fill.  A work item is a run of kValRun consecutive pixels times
// a chunk of `chunk` columns; column c holds the slots c, c + n_col, ... of
// the launch (n_col = min(ring, S): one column per ring entry in use), so the
// item's waves own its ring entries.  Each lane loads its 16 labels (pixels
// 256 c + 4 l + j) once per item; lap by lap the chunk's table slice goes to
// LDS and wave w takes the columns w, w + NW, ...: 16 LDS reads and four
// float4 stores per lane and slot, one wave writing the run's 4 KiB.
template <int NW, bool VEC4>
__global__ __launch_bounds__(64 * NW) void tess_values_gather_kernel(
    const int32_t* __restrict__ labels, int64_t P, const float* __restrict__ tab,
    int D, int64_t S, float* __restrict__ out, int64_t ring, int64_t ring_base,
    int64_t n_col, int64_t n_pb, int64_t n_cc, int chunk, int nt) {
  extern __shared__ float vtab[];  // [chunk][D + 1]
  constexpr int kC = kValRun / 256;
  const int DT = D + 1;
  const int l = threadIdx.x & 63;
  // wave index, wave-uniform: slot and ring arithmetic stay on the SALU
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t bb = blockIdx.x; bb < n_pb * n_cc; bb += gridDim.x) {
    const int64_t pb = bb % n_pb, cc = bb / n_pb;
    const int64_t c0 = cc * chunk;
    const int nc = (int)((n_col - c0) < chunk ? (n_col - c0) : chunk);
    const int64_t p0 = pb * kValRun + 4 * l;
    int lab[kC][4];
#pragma unroll
    for (int c = 0; c < kC; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t p = p0 + 256 * c + j;
        const int lb = p < P ? labels[p] - 1 : 0;
        lab[c][j] = (lb >= 0 && lb < D) ? lb : D;  // entry D: NaN
      }
    for (int64_t s0 = c0; s0 < S; s0 += n_col) {  // laps of the ring
      const int ns = (int)((S - s0) < nc ? (S - s0) : nc);
      __syncthreads();  // the previous lap's table reads are done
      for (int e = threadIdx.x; e < ns * DT; e += blockDim.x) vtab[e] = tab[s0 * DT + e];
      __syncthreads();
      for (int k = w; k < ns; k += NW) {
        const float* t = vtab + k * DT;
        // ring entry (ring < 2^31: sf_tess_fill_values)
        const int64_t so = (c0 + k + ring_base) % ring;
        float* o = out + so * P + p0;
#pragma unroll
        for (int c = 0; c < kC; ++c) {
          if (VEC4) {
            if (p0 + 256 * c < P) {
              const val_v4f v{t[lab[c][0]], t[lab[c][1]], t[lab[c][2]], t[lab[c][3]]};
              val_v4f* q = reinterpret_cast<val_v4f*>(o + 256 * c);
              if (nt)
                __builtin_nontemporal_store(v, q);
              else
                *q = v;
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (p0 + 256 * c + j < P) o[256 * c + j] = t[lab[c][j]];
          }
        }
      }
    }
  }
}

// Smoothed fill, 1 <= R <= kValMaxR, one plane of kl_tess_smooth_kernel with
// the radius at run time: a workgroup (4 waves) owns a tile of kValTH rows x
// kValTW pixels and a chunk of columns (ring entries).  The tile's labels +
// halo sit in LDS as bytes; per slot the raw table entries, widened to double,
// go to LDS (double-buffered), the y pass writes the halo columns of the tile
// rows as float (scipy's float32 intermediate), the x pass each wave's rows,
// then scrub, swap and the stores (4 pixels per lane).  TC: table capacity.
template <int TC>
__global__ __launch_bounds__(256) void tess_values_smooth_kernel(
    const int32_t* __restrict__ labels, int nx, int ny, const float* __restrict__ tab,
    int D, int64_t S, float* __restrict__ out, int64_t ring, int64_t ring_base,
    int64_t n_col, const double* __restrict__ gw, int R, int64_t n_tiles,
    int64_t n_cc, unsigned flags) {
#pragma clang fp contract(off)
  __shared__ unsigned char lab[(kValTH + 2 * kValMaxR) * (kValTW + 2 * kValMaxR)];
  __shared__ float ybuf[kValTH * (kValTW + 2 * kValMaxR)];
  __shared__ double tbl[2][TC];
  __shared__ double w[2 * kValMaxR + 1];
  const int DT = D + 1;
  const int W2 = kValTW + 2 * R;  // halo tile width
  const int H2 = kValTH + 2 * R;
  const int tiles_x = (nx + kValTW - 1) / kValTW;
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool scrub = flags & SF_EVAL_NAN_SCRUB;
  const bool be = flags & SF_EVAL_BIG_ENDIAN;
  const bool vec = (nx % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  const bool nt = vec && (flags & SF_EVAL_NT_STORES);
  const int64_t P = (int64_t)nx * ny;
  for (int e = threadIdx.x; e < 2 * R + 1; e += blockDim.x) w[e] = gw[e];
  for (int64_t bb = blockIdx.x; bb < n_tiles * n_cc; bb += gridDim.x) {
    const int64_t tile = bb % n_tiles, cc = bb / n_tiles;
    const int tx0 = (int)(tile % tiles_x) * kValTW;
    const int ty0 = (int)(tile / tiles_x) * kValTH;
    const int64_t c0 = cc * kValSmSlots;
    const int nc = (int)((n_col - c0) < kValSmSlots ? (n_col - c0) : kValSmSlots);
    // the item's slots, lap by lap: i -> c0 + i % nc + (i / nc) n_col (only
    // the last lap can be short)
    const int64_t laps = (S - c0 + n_col - 1) / n_col;
    const int64_t tail = S - (c0 + (laps - 1) * n_col);
    const int64_t n_it = (laps - 1) * nc + (tail < nc ? tail : nc);
    auto slot_of = [&](int64_t i) { return c0 + i % nc + (i / nc) * n_col; };
    __syncthreads();  // the previous item is done with lab / tbl / ybuf
    for (int e = threadIdx.x; e < H2 * W2; e += blockDim.x) {
      const int hy = e / W2, hx = e - hy * W2;
      const int gy = val_reflect(ty0 + hy - R, ny);
      const int gx = val_reflect(tx0 + hx - R, nx);
      const int lb = labels[(int64_t)gy * nx + gx] - 1;
      lab[e] = (unsigned char)((lb >= 0 && lb < D) ? lb : D);
    }
    for (int e = threadIdx.x; e < DT; e += blockDim.x)
      tbl[0][e] = (double)tab[slot_of(0) * DT + e];
    for (int64_t i = 0; i < n_it; ++i) {
      __syncthreads();  // tbl[i & 1] (and, at i = 0, lab) complete; ybuf free
      const double* t = tbl[i & 1];
      // y pass over the tile rows and every halo column
      for (int e = threadIdx.x; e < kValTH * W2; e += blockDim.x) {
        const int r = e / W2, c = e - r * W2;
        const unsigned char* col = lab + (r + R) * W2 + c;
        double acc = t[col[0]] * w[R];
#pragma unroll 4
        for (int j = R; j >= 1; --j) {
          const double a = t[col[-j * W2]], b = t[col[j * W2]];
          acc += (a + b) * w[R - j];
        }
        ybuf[e] = (float)acc;
      }
      // the next slot's table, into the other buffer (its last readers
      // finished the y pass of slot i - 1 before the barrier above)
      if (i + 1 < n_it)
        for (int e = threadIdx.x; e < DT; e += blockDim.x)
          tbl[(i + 1) & 1][e] = (double)tab[slot_of(i + 1) * DT + e];
      __syncthreads();
      // x pass: wave w takes rows w, w + 4; 4 pixels per lane
      const int gx0 = tx0 + 4 * l;
      const int64_t so = (c0 + i % nc + ring_base) % ring;
      for (int rr = wv; rr < kValTH; rr += 4) {
        const int gy = ty0 + rr;
        if (gy >= ny || gx0 >= nx) continue;
        float v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const float* row = ybuf + rr * W2 + R + 4 * l + p;
          double acc = (double)row[0] * w[R];
#pragma unroll 4
          for (int j = R; j >= 1; --j) acc += ((double)row[-j] + (double)row[j]) * w[R - j];
          v[p] = val_finish((float)acc, scrub, be);
        }
        float* o = out + so * P + (int64_t)gy * nx + gx0;
        if (vec) {
          const val_v4f q{v[0], v[1], v[2], v[3]};
          if (nt)
            __builtin_nontemporal_store(q, reinterpret_cast<val_v4f*>(o));
          else
            *reinterpret_cast<val_v4f*>(o) = q;
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (gx0 + p < nx) o[p] = v[p];
        }
      }
    }
  }
}

// One 1-D pass of the Gaussian for any radius over n_img one-plane images
// (smooth_pass_kernel of tess.hip with the value scrub: NaN -> 0 whatever the
// image index): one thread per output pixel, neighbours from L1 / L2; flags
// (scrub, swap) on the second pass only.
__global__ __launch_bounds__(256) void tess_values_pass_kernel(
    const float* __restrict__ in, float* __restrict__ out, int nx, int ny, int64_t n,
    const double* __restrict__ gw, int R, int axis, unsigned flags) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int64_t P = (int64_t)nx * ny;
  const int64_t img = e / P;
  const int rem = (int)(e - img * P);
  const int y = rem / nx, x = rem % nx;
  const float* base = in + img * P;
  auto at = [&](int o) -> double {
    return axis == 0 ? (double)base[(int64_t)val_reflect(y + o, ny) * nx + x]
                     : (double)base[(int64_t)y * nx + val_reflect(x + o, nx)];
  };
  double acc = at(0) * gw[R];
  for (int j = R; j >= 1; --j) acc += (at(-j) + at(j)) * gw[R - j];
  out[e] = val_finish((float)acc, flags & SF_EVAL_NAN_SCRUB, flags & SF_EVAL_BIG_ENDIAN);
}

// Workgroups of `threads` for n_items work items: one each up to the dispatch
// limit (kept at 2^31 work-items); past it the workgroups walk the rest
unsigned val_walk_grid(int64_t n_items, int threads) {
  const int64_t cap = ((int64_t)1 << 31) / threads;
  return (unsigned)(n_items < cap ? n_items : cap);
}

}  // namespace

int launch_tess_values(sf_ctx* ctx, const int32_t* labels, int nx, int ny,
                       const double* values, int D, int64_t S, float* out, int64_t ring,
                       const double* d_w, int R, unsigned flags) {
  const int64_t DT = D + 1;
  const int64_t P = (int64_t)nx * ny;
  hipStream_t stream = ctx->stream;
  // gather: slots per work item (its table slice in LDS: at most 64 KiB) and
  // waves per workgroup (SF_OPT_TESS_SLOTS / _WAVES; the scalar-store kernel
  // exists at 4 waves only)
  int chunk = kValSmSlots, threads = 256;
  const bool vec4 = (P % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  if (R == 0) {
    chunk = ctx->tess_slots > 0 ? ctx->tess_slots : kValSlotsAuto;
    if (chunk * DT * 4 > 65536) chunk = (int)(65536 / (DT * 4));
    const int nw = ctx->tess_waves;
    threads = 64 * (!vec4 || nw == 4 ? 4 : nw == 8 ? 8 : nw == 16 ? 16 : kValWavesAuto);
  }
  // the value table of at most `per` slots (<= 256 MiB of scratch) in the
  // context's scratch buffer.  A batch holds whole laps of the ring when the
  // ring is shorter than it, so within a launch a ring entry's slots belong
  // to one column; batches follow each other on the stream
  int64_t per = ((int64_t)256 << 20) / (DT * 4);
  if (ring < per) per = per / ring * ring;
  if (per > S) per = S;
  SF_TRY(ctx->d_tess_tab.reserve((size_t)(per * DT),
                                 "sf_tess_fill_values: hipMalloc of the value table failed"));
  float* tab = ctx->d_tess_tab.get();
  for (int64_t b = 0; b < S; b += per) {
    const int64_t Sb = S - b < per ? S - b : per;
    hipLaunchKernelGGL(tess_values_table_kernel, dim3((unsigned)((Sb * DT + 255) / 256)),
                       dim3(256), 0, stream, values + b * D, D, Sb, tab,
                       R == 0 ? flags : 0u);
    SF_HIP(hipGetLastError());
    const int64_t n_col = Sb < ring ? Sb : ring;
    const int64_t ring_base = b % ring;  // 0 whenever n_col == ring
    const int64_t n_cc = (n_col + chunk - 1) / chunk;
    if (R == 0) {
      const int64_t n_pb = (P + kValRun - 1) / kValRun;
      const dim3 grid(val_walk_grid(n_pb * n_cc, threads)), block(threads);
      const size_t lds = (size_t)chunk * DT * 4;
      const int nt = (flags & SF_EVAL_NT_STORES) && vec4;
      auto gather = [&](auto NW, auto V) {
        hipLaunchKernelGGL(
            (tess_values_gather_kernel<decltype(NW)::value, decltype(V)::value>), grid, block,
            lds, stream, labels, P, tab, D, Sb, out, ring, ring_base, n_col, n_pb, n_cc, chunk,
            nt);
      };
      if (!vec4)
        gather(std::integral_constant<int, 4>{}, std::false_type{});
      else if (threads == 64 * 4)
        gather(std::integral_constant<int, 4>{}, std::true_type{});
      else if (threads == 64 * 8)
        gather(std::integral_constant<int, 8>{}, std::true_type{});
      else
        gather(std::integral_constant<int, 16>{}, std::true_type{});
    } else {
      const int64_t tiles_x = (nx + kValTW - 1) / kValTW;
      const int64_t n_tiles = tiles_x * ((ny + kValTH - 1) / kValTH);
      const dim3 grid(val_walk_grid(n_tiles * n_cc, 256)), block(256);
      with_bools(
          [&](auto WIDE) {
            constexpr int TC = decltype(WIDE)::value ? kValTabCapWide : kValTabCap;
            hipLaunchKernelGGL(tess_values_smooth_kernel<TC>, grid, block, 0, stream, labels,
                               nx, ny, tab, D, Sb, out, ring, ring_base, n_col, d_w, R,
                               n_tiles, n_cc, flags);
          },
          DT > kValTabCap);
    }
    SF_HIP(hipGetLastError());
  }
  return SF_OK;
}

int launch_values_smooth(sf_ctx* ctx, float* cube, int nx, int ny, int64_t n_img,
                         const double* d_w, int R, unsigned flags) {
  const int64_t P = (int64_t)nx * ny;
  // the y pass goes to scratch, the x pass back into the cube, in chunks of
  // images that keep the scratch at <= 256 MiB
  int64_t chunk = ((int64_t)256 << 20) / (P * (int64_t)sizeof(float));
  if (chunk < 1) chunk = 1;
  if (chunk > n_img) chunk = n_img;
  SF_TRY(ctx->d_smooth.reserve((size_t)(chunk * P),
                               "sf_tess_fill_values: hipMalloc of the pass buffer failed"));
  for (int64_t i0 = 0; i0 < n_img; i0 += chunk) {
    const int64_t ni = (n_img - i0 < chunk) ? n_img - i0 : chunk;
    const int64_t n = ni * P;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    float* c = cube + i0 * P;
    hipLaunchKernelGGL(tess_values_pass_kernel, dim3(blocks), dim3(256), 0, ctx->stream, c,
                       ctx->d_smooth.get(), nx, ny, n, d_w, R, 0, 0u);
    SF_HIP(hipGetLastError());
    hipLaunchKernelGGL(tess_values_pass_kernel, dim3(blocks), dim3(256), 0, ctx->stream,
                       ctx->d_smooth.get(), c, nx, ny, n, d_w, R, 1, flags);
    SF_HIP(hipGetLastError());
  }
  return SF_OK;
}

}  // namespace sf
