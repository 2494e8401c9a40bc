// kl_fit_masks.h -- what the fit's two mask caches share: the 64-bit keys of
// kl_fit_pool.h (<= 60 directions) and the 128-bit claimants of
// kl_fit_wide.hip hash with one mixer and number their new entries with one
// wave-aggregated step.  The tables themselves differ (exact 64-bit key
// equality against a two-word compare through the claimant's row) and stay
// with their files.
#pragma once

#include <hip/hip_runtime.h>

#include "sf_wave.h"

namespace sf {

// splitmix64's finaliser
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// every one of D <= 64 directions unflagged
__host__ __device__ inline unsigned long long full_mask(int D) {
  return D == 64 ? ~0ull : (1ull << D) - 1ull;
}

inline size_t next_pow2(size_t x, size_t floor) {
  size_t p = floor;
  while (p < x) p <<= 1;
  return p;
}

constexpr unsigned long long kEmptyKey = 0ull;

// Insert `key` (non-zero) into the open-addressing table; returns its slot
// or -3 when the table is full.  Only ever inserts, never waits on other
// threads (ids are assigned by a later kernel).
__device__ inline int table_insert(unsigned long long* keys, int cap,
                            unsigned long long key) {
  int h = (int)(mix64(key) & (unsigned long long)(cap - 1));
  for (int probe = 0; probe < cap; ++probe) {
    // a plain load first: most slots share a few masks, whose entries are
    // taken long before most inserts arrive -- no atomic on those
    unsigned long long prev = keys[h];
    if (prev == kEmptyKey) prev = atomicCAS(keys + h, kEmptyKey, key);
    if (prev == kEmptyKey || prev == key) return h;
    h = (h + 1) & (cap - 1);
  }
  return -3;
}

// Bound of a grid-stride loop of one thread per table entry i whose trips
// are wave-uniform: a wave goes on while its first lane is inside the table,
// so number_fresh below meets whole waves (entry i itself may lie beyond cap)
__device__ __forceinline__ bool wave_in_table(int i, int cap) {
  return i - lane() < cap;
}

// The next free ids of *counter for the wave's `fresh` lanes: one atomic per
// wavefront, each fresh lane its rank among them; -1 on the other lanes.  The
// order of the ids is immaterial (every entry is decomposed on its own, the
// readers of a pool sort by mask).  Called by the whole wave.
__device__ __forceinline__ int number_fresh(bool fresh, int* counter) {
  const unsigned long long nb = __ballot(fresh);
  if (nb == 0ull) return -1;  // wave-uniform: most of a table is empty
  int base = 0;
  if (lane() == 0) base = atomicAdd(counter, __popcll(nb));
  base = __shfl(base, 0);
  return fresh ? base + Group<1>::rank(nb) : -1;
}

}  // namespace sf
