// Coordinate hashing shared by every voxel table of the library (coordmap.hip, kmap.hip, conv1.hip, voxelmean.hip,
// tsdf.hip, tsdfmesh.hip): the hash, the look-ups, the ONE probe-and-claim loop and the host helper that sizes a table.
// COO coordinates are int32 rows [batch, x_0 .. x_{D-1}] (NC = 1 + D ints).  The hash table is
// open addressing with linear probing; entries are row indices (-1 = empty) into the coordinate
// array that owns the keys, so a probe is: 4-byte table read (L2-resident: 2 x N entries) and,
// only on an occupied slot, an NC-int row compare.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dgr_internal.h"

#define DGR_EMPTY (-1)

// Slots of the table of n rows: a power of two >= max(64, 2 n), at most 2^31 (the most a 32-bit mask addresses).  Up to
// n = 2^30 rows the load is at most 1/2; beyond, up to the 2^31 - 1 rows an int32 row index can name, at least one slot
// stays empty.  Either way every probe loop below meets an empty slot or its key and ends.
// (gtmatch.hip's sets of 64-bit keys are addressed with a 64-bit mask and pass a higher limit.)
static inline uint64_t dgr_table_slots(int64_t n, uint64_t max_slots = 1ull << 31) {
  uint64_t cap = 64;
  while (cap < 2 * (uint64_t)n && cap < max_slots) cap <<= 1;
  return cap;
}

// a cleared table for n rows (n < 2^31), from the arena
static inline int dgr_table_make(DgrArena &arena, int64_t n, int32_t **table_out, uint32_t *mask_out, hipStream_t stream) {
  DGR_REQUIRE(n >= 0 && n < (1ll << 31), "hash table: %lld rows", (long long)n);
  const uint64_t cap = dgr_table_slots(n);
  DGR_ALLOC(*table_out, arena, int32_t, cap);
  *mask_out = (uint32_t)(cap - 1);
  DGR_HIP_CHECK(hipMemsetAsync(*table_out, 0xff, (size_t)cap * sizeof(int32_t), stream));
  return DGR_OK;
}

__device__ __forceinline__ uint32_t dgr_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

template <int NC>
__device__ __forceinline__ uint32_t dgr_hash_row(const int32_t *c) {
  uint32_t h = 0x9747b28cu;
#pragma unroll
  for (int d = 0; d < NC; ++d) {
    uint32_t k = (uint32_t)c[d];
    k *= 0xcc9e2d51u;
    k = dgr_rotl(k, 15);
    k *= 0x1b873593u;
    h ^= k;
    h = dgr_rotl(h, 13);
    h = h * 5u + 0xe6546b64u;
  }
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

template <int NC>
__device__ __forceinline__ bool dgr_rows_equal(const int32_t *a, const int32_t *b) {
  bool eq = true;
#pragma unroll
  for (int d = 0; d < NC; ++d) eq &= (a[d] == b[d]);
  return eq;
}

// The probe-and-claim loop: walks from the hash of row r's key to the first slot that is empty or holds a row with the
// same key.  Returns DGR_EMPTY if r took an empty slot, else the row that was seen holding the slot; *slot_out = the slot.
// Ends because the table has an empty slot (dgr_table_slots); every key it compares against must have been written by a
// kernel that has finished.
template <int NC>
__device__ __forceinline__ int dgr_claim(int32_t *table, uint32_t mask, const int32_t *__restrict__ keys, int r,
                                         uint32_t *slot_out) {
  int32_t me[NC];
#pragma unroll
  for (int d = 0; d < NC; ++d) me[d] = keys[(int64_t)r * NC + d];
  uint32_t slot = dgr_hash_row<NC>(me) & mask;
  int cur;
  while (true) {
    cur = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == DGR_EMPTY) {
      cur = atomicCAS(&table[slot], DGR_EMPTY, r);
      if (cur == DGR_EMPTY) break;
    }
    if (dgr_rows_equal<NC>(keys + (int64_t)cur * NC, me)) break;
    slot = (slot + 1) & mask;
  }
  *slot_out = slot;
  return cur;
}

// table[slot] ends up holding the SMALLEST row among the inserted rows that share a key, whatever the order the threads
// are served in.  A row that sees a smaller row of its key leaves without the atomic: a slot's value only ever falls.
template <int NC>
__device__ __forceinline__ void dgr_insert_first(int32_t *table, uint32_t mask, const int32_t *__restrict__ keys, int r) {
  uint32_t slot;
  const int prev = dgr_claim<NC>(table, mask, keys, r, &slot);
  if (prev > r) atomicMin(&table[slot], r);
}

// Row index of `q` in (coords, table) or -1.
template <int NC>
__device__ __forceinline__ int dgr_lookup(const int32_t *__restrict__ table, uint32_t mask,
                                          const int32_t *__restrict__ coords, const int32_t *q) {
  uint32_t slot = dgr_hash_row<NC>(q) & mask;
  while (true) {
    int v = table[slot];
    if (v == DGR_EMPTY) return -1;
    if (dgr_rows_equal<NC>(coords + (int64_t)v * NC, q)) return v;
    slot = (slot + 1) & mask;
  }
}

// U independent look-ups at once: the U table reads are issued together, then the key rows of the occupied
// slots, so a thread pays two memory latencies for U probes instead of 2 U (collisions fall back to the
// sequential probe loop, continuing behind the first slot).
template <int NC, int U>
__device__ __forceinline__ void dgr_lookup_many(const int32_t *__restrict__ table, uint32_t mask,
                                                const int32_t *__restrict__ coords, const int32_t (*q)[NC],
                                                int *found) {
  uint32_t slot[U];
  int v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    slot[u] = dgr_hash_row<NC>(q[u]) & mask;
    v[u] = table[slot[u]];
  }
  bool eq[U];
#pragma unroll
  for (int u = 0; u < U; ++u) eq[u] = dgr_rows_equal<NC>(coords + (int64_t)max(v[u], 0) * NC, q[u]);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (v[u] == DGR_EMPTY) {
      found[u] = -1;
    } else if (eq[u]) {
      found[u] = v[u];
    } else {   // collision: keep probing
      uint32_t s2 = (slot[u] + 1) & mask;
      int r = -1;
      while (true) {
        const int w = table[s2];
        if (w == DGR_EMPTY) break;
        if (dgr_rows_equal<NC>(coords + (int64_t)w * NC, q[u])) { r = w; break; }
        s2 = (s2 + 1) & mask;
      }
      found[u] = r;
    }
  }
}
