// Kernel maps: for every output coordinate and every kernel offset delta_k, probe the input
// coordinate hash for (out + delta_k * ts_in).  Replaces MinkowskiEngine's kernel-map
// construction behind ME.MinkowskiConvolution(Transpose) (model/residual_block.py:15-80).
//
// Output layout (rule-major COO): pairs sorted by (k, out) -- pair_in[p], pair_out[p] for
// p in [rule_ptr[k], rule_ptr[k+1]) -- plus tile_ptr[k], the exclusive prefix of
// ceil(P_k / DGR_TILE_M) used by the sparse-conv kernel to enumerate MFMA tiles.
// Offset enumeration: first spatial dimension fastest -- kept in ONE place:
// `offset_of`.  Deterministic: two passes (count, fill) with block-level ranks, no atomics on
// the pair positions.
#include <string.h>

#include <algorithm>

#include "dgr_internal.h"
#include "hash.h"

constexpr int KM_THREADS = 256;

// delta for offset index k, in units of ts (first spatial dimension fastest)
template <int D>
__device__ __forceinline__ void offset_of(int k, int ks, int ts, int32_t *delta) {
  const int half = ks >> 1;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    delta[d] = ((k % ks) - half) * ts;
    k /= ks;
  }
}

template <int D>
__device__ __forceinline__ int probe(const int32_t *__restrict__ out_coords, int64_t o,
                                     const int32_t *delta, const int32_t *__restrict__ in_coords,
                                     const int32_t *__restrict__ in_table, uint32_t in_mask) {
  constexpr int NC = D + 1;
  int32_t q[NC];
  q[0] = out_coords[o * NC];
#pragma unroll
  for (int d = 0; d < D; ++d) q[1 + d] = out_coords[o * NC + 1 + d] + delta[d];
  return dgr_lookup<NC>(in_table, in_mask, in_coords, q);
}

// ---- pass 1, generic: grid = (row blocks, K).  Probes every (output row, offset); the hit (or -1)
// is cached in hits[k * n_cap + o] so that pass 2 never probes again, and the number of hits of
// offset k among the rows of block rb goes to block_counts[k * RB + rb].
template <int D>
__global__ void __launch_bounds__(KM_THREADS)
    kmap_search(const int32_t *__restrict__ out_coords, const int32_t *n_out_dev,
                const int32_t *__restrict__ in_coords, const int32_t *__restrict__ in_table,
                uint32_t in_mask, int ks, int ts_in, int RB, int64_t n_cap, int32_t *__restrict__ hits,
                int32_t *__restrict__ block_counts, int KW, uint32_t *mask_out, uint32_t *mask_in) {
  __shared__ int wave_cnt[KM_THREADS / 64];
  const int rb = blockIdx.x, k = blockIdx.y;
  const int n_out = *n_out_dev;
  if (rb * KM_THREADS >= n_out) {
    if (threadIdx.x == 0) block_counts[(int64_t)k * RB + rb] = 0;
    return;
  }
  int32_t delta[D];
  offset_of<D>(k, ks, ts_in, delta);
  const int64_t o = (int64_t)rb * KM_THREADS + threadIdx.x;
  int hit = -1;
  if (o < n_out) {
    hit = probe<D>(out_coords, o, delta, in_coords, in_table, in_mask);
    hits[(int64_t)k * n_cap + o] = hit;
    if (hit >= 0) {
      atomicOr(&mask_out[o * KW + (k >> 5)], 1u << (k & 31));
      if (mask_in) atomicOr(&mask_in[(int64_t)hit * KW + (k >> 5)], 1u << (k & 31));
    }
  }
  unsigned long long m = __ballot(hit >= 0);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < KM_THREADS / 64; ++w) s += wave_cnt[w];
    block_counts[(int64_t)k * RB + rb] = s;
  }
}

__device__ __forceinline__ int mask_rank(const uint32_t *__restrict__ m, int k) {
  int r = 0;
  const int w = k >> 5;
  for (int i = 0; i < w; ++i) r += __popc(m[i]);
  return r + __popc(m[w] & ((1u << (k & 31)) - 1u));
}

__global__ void mask_count_kernel(const uint32_t *__restrict__ mask, int KW, const int32_t *n_dev, int64_t n_cap,
                                  int32_t *__restrict__ cnt) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_cap) return;
  int c = 0;
  if (r < *n_dev)
    for (int i = 0; i < KW; ++i) c += __popc(mask[r * KW + i]);
  cnt[r] = c;
}
// the same for the bit matrices of the input rows of the three strided 6-D maps in ONE launch (blockIdx.y = matrix), the
// row's words requested together (a loop that alternates loads and stores: 23 dependent round trips per row), plus
// wpre: pairs of the row in the mask words before word i (a row can have all K = 729 offsets: 16 bits)
constexpr int KM_MAXJOBS = 8;   // kernel maps per multi-map launch (blockIdx.y = map): the 6-D builder passes seven
struct MaskCountJobs {
  const uint32_t *mask[KM_MAXJOBS];
  const int32_t *n_dev[KM_MAXJOBS];
  long long n_cap[KM_MAXJOBS];
  int32_t *cnt[KM_MAXJOBS];
  unsigned short *wpre[KM_MAXJOBS];
};
template <int KW>
__global__ void mask_count_multi(MaskCountJobs J) {
  const int m = blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= J.n_cap[m]) return;
  int c = 0;
  if (r < *J.n_dev[m]) {
    uint32_t w[KW];
#pragma unroll
    for (int i = 0; i < KW; ++i) w[i] = J.mask[m][r * KW + i];
#pragma unroll
    for (int i = 0; i < KW; ++i) {
      J.wpre[m][r * KW + i] = (unsigned short)c;
      c += __popc(w[i]);
    }
  }
  J.cnt[m][r] = c;
}
// rank of offset k among the row's set offsets, with the per-word prefix of the row
__device__ __forceinline__ int mask_rank_pre(const uint32_t *__restrict__ m, const unsigned short *__restrict__ pre, int k) {
  return pre[k >> 5] + __popc(m[k >> 5] & ((1u << (k & 31)) - 1u));
}

// =========================== D = 6: bit-matrix pipeline =====================================
// A 6-D map has 729 offsets but only 2..45 neighbours per row (0.3..6 % density), so nothing of
// size [K, N] is ever materialised except ONE BIT per (row, offset):
//   bits     the search (pruned_search6) sets mask_out[o][k] (and mask_in[i][k] for maps that are
//            also used swapped).  Same-stride maps are symmetric -- (o, k) -> i  <=>  (i, K-1-k) -> o
//            -- so only offsets below the centre are searched and every hit sets both bits.
//            Every hit is also APPENDED as a record (offset, row, input row) to a hit list -- in no particular
//            order, into the searching wave's own region (HitList below: no global counter); the records replace a
//            re-probe of every set bit in the placing pass.
//   colmask  transposes the bit matrix per 64-row group (one ballot per offset), counts the pairs of every
//            (offset, 256-row block) cell -> exclusive scan = cell bases -- and of every row (CSR row pointers).
//   place    one thread per hit record: ranks the pair inside its row (CSR slot) and inside its cell (rule-major
//            position) with popcounts.  The positions depend on the bit matrix only, not on the order of the list.
// Result identical to the generic path: pairs sorted by (k, out), CSR slots in ascending k.
// All seven maps of a sparse tensor go through these phases TOGETHER (build_kernel_maps6): one clear, one multi-array
// scan, one finalisation and one tile-descriptor launch for all of them.

// hit record: offset k (10 bits) | output row (27 bits) | input row (27 bits)
__device__ __forceinline__ unsigned long long hit_pack(int k, int64_t o, int64_t in) {
  return ((unsigned long long)k << 54) | ((unsigned long long)o << 27) | (unsigned long long)in;
}
// The hit list needs no global counter (one that is bumped per hit, per wave-call or even per 128-slot chunk serialises
// on its one address at ~40 ns per atomic: measured 13 / 5.3 ms instead of 2.4 ms per batch): every wave of the search
// owns a fixed REGION of the list, hands slots out from a cursor in LDS and leaves its record count in
// wave_count[wave id].  Round 3 sized a region for the most records 64 threads can produce (3456 for the pruned
// symmetric search: 6 KB of arena per output row, of which a few per cent were ever written).  Now a region holds
// KM_REGION records -- several times what a wave of the benchmark's maps produces -- and a wave that runs out of slots
// marks itself (count -1): the bit matrix is complete either way, and the placing kernel REPLAYS the search of a marked
// wave and places its pairs directly (positions depend on the bit matrix only).  Arena per output row: 0.9 KB
// (symmetric maps) / 1.7 KB (strided maps).
constexpr int KM_REGION = 512;
// (a wave = 64 rows under one first-half offset: a dozen records at the fine levels and in the strided maps, ~180 in
// the stride-8 map with its 39 neighbours per row, several times that in its dense corners)
constexpr int km_region_of(int ts_in, bool symmetric) { return (ts_in >= 8 && symmetric) ? 2 * KM_REGION : KM_REGION / 2; }
struct HitList {
  unsigned long long *recs;   // [waves][region]
  int32_t *wave_count;        // [waves]; -1: the region overflowed, replay the wave
  int region;                 // records per wave
};
__device__ __forceinline__ void hit_begin(volatile int *cur) {
  if ((threadIdx.x & 63) == 0) cur[threadIdx.x >> 6] = 0;
}
// First of `n` (1 or 2) consecutive slots for this lane, or -1 once the wave's region is full.  Called from divergent
// code by the lanes that found a pair: the active lanes of the wave share one cursor update.
__device__ __forceinline__ int64_t hit_slots(int n, const HitList &h, volatile int *cur, int wave_id) {
  const unsigned long long act = __ballot(1), two = __ballot(n == 2);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  int base = 0;
  if (lane == __ffsll((long long)act) - 1) {
    base = cur[w];
    const int need = __popcll(act) + __popcll(two);
    if (base >= 0 && base + need <= h.region) {
      cur[w] = base + need;
    } else {
      cur[w] = -1;
      base = -1;
    }
  }
  base = __builtin_amdgcn_readfirstlane(base);   // the first ACTIVE lane is the one that moved the cursor
  if (base < 0) return -1;
  return (int64_t)wave_id * h.region + base + __popcll(act & below) + __popcll(two & below);
}
__device__ __forceinline__ void hit_end(const HitList &h, volatile int *cur, int wave_id) {
  if ((threadIdx.x & 63) == 0) h.wave_count[wave_id] = cur[threadIdx.x >> 6];
}

// pruned search: one thread per (output row, first-half offset).  A 6-D neighbour (ca + da, cb + db) can only exist
// among the rows whose first half equals ca + da: look that bucket up once (27 -- symmetric: 14 -- look-ups per row
// instead of 729 probes) and test the second half of its entries, which lie contiguously in `hb.second` (sequential
// 16-byte reads; round 3 read a row index and then, dependently, the row's coordinates per candidate -- at tensor
// stride 8, where a bucket holds tens to hundreds of rows, that made the generic 364-probe search the cheaper one:
// 449 us for the one stride-8 map of a batch).  `emit(k, o, in)` is called, from divergent code, by the lane that
// found input row `in` under offset k of output row o; the search kernel sets bits and records the hit, the placing
// kernel's replay of an overflowed wave places the pair.
struct PrunedArgs {
  const int32_t *out_coords, *n_out_dev;
  const int4 *out_order;   // the OUTPUT map's rows in the order of its own first-half buckets: (x1, y1, z1, row)
  int64_t n_cap;           // row capacity of the output map (thread t = ja * n_cap + position in out_order)
  DgrHalfBuckets hb;       // first-half buckets of the INPUT map
  int ts_in, symmetric;
};
// Thread t = (first-half offset ja, position p in the output map's bucket order): the 64 lanes of a wave are 64
// consecutive rows of (mostly) ONE first-half bucket under the SAME first-half offset, so they scan the same neighbour
// bucket in lock step -- every load of the loop below is one address for the whole wave -- and a wave's records are
// spread over 64 rows instead of all offsets of 4.6 rows (rows with hundreds of neighbours overflowed a region alone).
template <class Emit>
__device__ __forceinline__ void pruned_search6(const PrunedArgs &a, int64_t t, Emit &&emit) {
  const int NJ = a.symmetric ? 14 : 27;
  const int ts_in = a.ts_in;
  const int ja = (int)(t / a.n_cap);
  const int64_t p = t - (int64_t)ja * a.n_cap;
  int b = -1;
  int64_t o = 0;
  int c4 = 0, c5 = 0, c6 = 0;
  if (ja < NJ && p < *a.n_out_dev) {
    const int4 me = a.out_order[p];
    o = me.w; c4 = me.x; c5 = me.y; c6 = me.z;
    const int32_t *co = a.out_coords + o * 7;
    int32_t q[4];
    q[0] = co[0];
    q[1] = co[1] + ((ja % 3) - 1) * ts_in;
    q[2] = co[2] + (((ja / 3) % 3) - 1) * ts_in;
    q[3] = co[3] + ((ja / 9) - 1) * ts_in;
    b = dgr_lookup<4>(a.hb.table, a.hb.mask, a.hb.bkeys, q);
  }
  const int beg = b >= 0 ? a.hb.start[b] : 0, end = b >= 0 ? a.hb.start[b + 1] : 0;
  // four bucket entries per trip, fetched together
  for (int p0 = beg; p0 < end; p0 += 4) {
    int4 e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) e[u] = a.hb.second[min(p0 + u, end - 1)];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (p0 + u >= end) break;
      const int d4 = e[u].x - c4, d5 = e[u].y - c5, d6 = e[u].z - c6;
      // every component must be -ts, 0 or +ts (all coordinates of a level are multiples of ts)
      if (abs(d4) <= ts_in && abs(d5) <= ts_in && abs(d6) <= ts_in) {
        const int k = ja + 27 * ((d4 / ts_in + 1) + 3 * (d5 / ts_in + 1) + 9 * (d6 / ts_in + 1));
        if (a.symmetric && ja == 13 && k > 364) continue;  // ja == 13 mirrors onto itself: upper half found from the other row
        emit(k, o, e[u].w);
      }
    }
  }
}

// Everything the three kernels of the 6-D builder (search, transposing pass, placing pass) need of ONE map; the host
// fills the record once (build_kernel_maps6) and every kernel takes all records by value, blockIdx.y = map, and reads
// the fields it uses from its map's record.
struct Map6 {
  PrunedArgs s;                          // the search, and its replay for an overflowed wave in the placing pass
  HitList hl;
  int search_blocks, hit_waves;          // blocks of the search; its waves = regions of the hit list
  int place_blocks;                      // the placing pass: that many blocks stride over the regions
  int RB;                                // 256-row blocks of the output map
  uint32_t *mask_out, *mask_in;          // bit matrices [rows + 1][KW]; mask_in: maps with an in-major CSR, else NULL
  unsigned short *wpre_out, *wpre_in;    // per-word prefixes of the rows' pair counts
  int4 *cell;                            // transposed bit matrix (kmap_colmask)
  int32_t *counts, *base;                // pairs per (offset, 256-row block) cell [K * RB] and their exclusive scan
  int32_t *cnt_out;                      // pairs per output row -> km.out_ptr
  DgrKernelMap km;                       // the lasting arrays (a copy of the caller's map once they are allocated)
  // host side only
  int32_t *total, *cnt_in;               // pairs of the map; pairs per input row -> km.in_ptr (with mask_in)
  int64_t n_in_cap;
};
struct Maps6 {
  Map6 m[KM_MAXJOBS];
};
static_assert(sizeof(Maps6) <= 4096, "the records of the 6-D builder travel as ONE by-value kernel argument (HIP: 4 KB)");

// The searches of ALL maps of a sparse tensor in one launch (round 5; round 4 launched map after map: seven grids of
// 38-250 us each with their tails idle): blockIdx.y = map, blockIdx.x = the map's search block (surplus blocks of the
// smaller maps exit at once).
__global__ void __launch_bounds__(KM_THREADS)
    kmap_bits_pruned6(Maps6 J, int KW) {
  __shared__ int hit_cur[KM_THREADS / 64];
  const Map6 &M = J.m[blockIdx.y];
  if ((int)blockIdx.x >= M.search_blocks) return;
  const PrunedArgs &a = M.s;
  uint32_t *const mask_out = M.mask_out, *const mask_in = M.mask_in;
  const HitList &hl = M.hl;
  hit_begin(hit_cur);
  const int wid = (int)(blockIdx.x * (KM_THREADS / 64) + (threadIdx.x >> 6));
  // (no early return: every wave leaves its record count behind)
  pruned_search6(a, (int64_t)blockIdx.x * KM_THREADS + threadIdx.x, [&](int k, int64_t o, int in) {
    atomicOr(&mask_out[o * KW + (k >> 5)], 1u << (k & 31));
    const int km = 728 - k;
    if (a.symmetric) {
      if (km != k) atomicOr(&mask_out[(int64_t)in * KW + (km >> 5)], 1u << (km & 31));
    } else if (mask_in) {
      atomicOr(&mask_in[(int64_t)in * KW + (k >> 5)], 1u << (k & 31));
    }
    const int n = (a.symmetric && km != k) ? 2 : 1;
    const int64_t s = hit_slots(n, hl, hit_cur, wid);
    if (s >= 0) {
      hl.recs[s] = hit_pack(k, o, in);
      if (n == 2) hl.recs[s + 1] = hit_pack(km, in, o);
    }
  });
  hit_end(hl, hit_cur, wid);
}

// transposed bit matrix: cell[g * K + k] = {rows of 64-row group g that have offset k (one ballot, 2 words),
// rule-major position of the group's first pair of that offset, 0}; counts[k * RB + rb] = pairs of the
// (offset, 256-row block) cell.  A pair's position = cell base (exclusive scan of counts) + the pairs of the earlier
// groups of the same block (here) + its rank inside the group's ballot (place_pair).
constexpr int KM_KMAX = 736;
__global__ void __launch_bounds__(KM_THREADS)
    kmap_colmask(Maps6 J, int K, int KW) {   // blockIdx.y = map, blockIdx.x = 256-row block of the map
  __shared__ unsigned long long bal[KM_THREADS / 64][KM_KMAX];
  const Map6 &M = J.m[blockIdx.y];
  const int RB = M.RB;
  if ((int)blockIdx.x >= RB) return;
  const uint32_t *__restrict__ mask_out = M.mask_out;
  const int32_t *n_out_dev = M.s.n_out_dev;
  int4 *__restrict__ cell = M.cell;
  int32_t *__restrict__ counts = M.counts, *__restrict__ row_cnt = M.cnt_out;
  unsigned short *__restrict__ wpre = M.wpre_out;
  const int rb = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_out = *n_out_dev;
  const int64_t o = (int64_t)rb * KM_THREADS + threadIdx.x;
  int row_pairs = 0;
  // the row's whole mask first (KW <= 24 words, all loads in flight together: the loop below alternates ballots and
  // stores, which kept the loads one memory round trip apart -- 23 dependent trips per wave)
  constexpr int KW_MAX = (KM_KMAX + 31) / 32;
  uint32_t words[KW_MAX];
#pragma unroll
  for (int w = 0; w < KW_MAX; ++w) words[w] = (w < KW && o < n_out) ? mask_out[o * KW + w] : 0u;
#pragma unroll
  for (int w = 0; w < KW_MAX; ++w) {
    if (w < KW) {   // (uniform)
      const uint32_t word = words[w];
      if (o < n_out) wpre[o * KW + w] = (unsigned short)row_pairs;
      row_pairs += __popc(word);
      unsigned long long mine = 0;
#pragma unroll
      for (int b = 0; b < 32; ++b) {
        const unsigned long long m = __ballot((word >> b) & 1u);
        if (lane == b) mine = m;
      }
      if (lane < 32 && 32 * w + lane < KM_KMAX) bal[wave][32 * w + lane] = mine;
    }
  }
  if (o < n_out) row_cnt[o] = row_pairs;   // (rows beyond the count: cleared together with the bit matrix)
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += KM_THREADS) {
    int run = 0;
#pragma unroll
    for (int g = 0; g < KM_THREADS / 64; ++g) {
      const unsigned long long m = bal[g][k];
      cell[((int64_t)rb * (KM_THREADS / 64) + g) * K + k] = make_int4((int)(m & 0xffffffffull), (int)(m >> 32), run, 0);
      run += __popcll(m);
    }
    counts[(int64_t)k * RB + rb] = run;
  }
}

// puts ONE pair (k, o) -> in into map p.  km.pair_out / km.pair_k may be NULL (maps whose consumers never read them):
// two random stores less per pair.
__device__ __forceinline__ void place_pair(const Map6 &p, int K, int KW, int32_t *overflow, int k, int64_t o, int64_t in) {
  const int64_t slot = (int64_t)p.km.out_ptr[o] + mask_rank_pre(p.mask_out + o * KW, p.wpre_out + o * KW, k);
  const int64_t g = o >> 6;
  const int4 c = p.cell[g * K + k];   // ONE 16-byte read: column ballot + pairs of the block's earlier groups
  const unsigned long long cm = ((unsigned long long)(uint32_t)c.y << 32) | (uint32_t)c.x;
  const int64_t pos = (int64_t)p.base[(int64_t)k * p.RB + (g >> 2)] + c.z + __popcll(cm & ((1ull << (o & 63)) - 1ull));
  if (pos < p.km.pair_cap && slot < p.km.pair_cap) {
    p.km.pair_in[pos] = (int32_t)in;
    if (p.km.pair_out) p.km.pair_out[pos] = (int32_t)o;
    if (p.km.pair_k) p.km.pair_k[pos] = (uint16_t)k;
    p.km.out_pos[slot] = (int32_t)pos;
    if (p.mask_in) p.km.in_pos[p.km.in_ptr[in] + mask_rank_pre(p.mask_in + in * KW, p.wpre_in + in * KW, k)] = (int32_t)pos;
  } else {
    *overflow = 2;
  }
}

// one wave per region of the hit list: one lane per record places the pair; a wave whose region overflowed during the
// search (count -1) repeats that wave's search and places what it finds.  blockIdx.y = map; the map's blocks stride
// over its hit-list regions.
__global__ void __launch_bounds__(KM_THREADS)
    kmap_place_hits(Maps6 J, int K, int KW, int32_t *overflow) {
  const Map6 &p = J.m[blockIdx.y];
  const int nblk = p.place_blocks;
  if ((int)blockIdx.x >= nblk) return;
  const HitList &h = p.hl;
  const PrunedArgs &replay = p.s;
  const int n_waves = p.hit_waves;
  const int lane = threadIdx.x & 63;
  for (int r = blockIdx.x * (KM_THREADS / 64) + (threadIdx.x >> 6); r < n_waves; r += nblk * (KM_THREADS / 64)) {
    const int n = h.wave_count[r];
    if (n < 0) {
      pruned_search6(replay, (int64_t)r * 64 + lane, [&](int k, int64_t o, int in) {
        place_pair(p, K, KW, overflow, k, o, in);
        if (replay.symmetric && 728 - k != k) place_pair(p, K, KW, overflow, 728 - k, in, o);
      });
      continue;
    }
    for (int e = lane; e < n; e += 64) {
      const unsigned long long rec = h.recs[(int64_t)r * h.region + e];
      place_pair(p, K, KW, overflow, (int)(rec >> 54), (int64_t)((rec >> 27) & 0x7ffffffull), (int64_t)(rec & 0x7ffffffull));
    }
  }
}

// ---- pass 2: grid = (row blocks, K / 8).  A block owns 256 output rows and 8 consecutive offsets:
// it reads the 8 cell counts, and for the non-empty cells (a few % in 6-D) ranks the cached hits
// inside the block (row order) and writes the pairs at cell_base + rank.  Sorted by (k, out), no
// atomics, no probing; 8x fewer (mostly empty) blocks than one block per cell.
constexpr int KM_KGROUP = 8;
__global__ void __launch_bounds__(KM_THREADS)
    kmap_fill(const int32_t *n_out_dev, int RB, int K, int64_t n_cap, const int32_t *__restrict__ hits,
              const int32_t *__restrict__ block_counts, const int32_t *__restrict__ block_base,
              int32_t *__restrict__ pair_in, int32_t *__restrict__ pair_out, int64_t pair_cap,
              int32_t *overflow, int KW, const uint32_t *__restrict__ mask_out,
              const int32_t *__restrict__ out_ptr, int32_t *__restrict__ out_pos,
              const uint32_t *__restrict__ mask_in, const int32_t *__restrict__ in_ptr,
              int32_t *__restrict__ in_pos, uint16_t *__restrict__ pair_k) {
  __shared__ int wave_cnt[2][KM_THREADS / 64];
  const int rb = blockIdx.x;
  const int n_out = *n_out_dev;
  if (rb * KM_THREADS >= n_out) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t o = (int64_t)rb * KM_THREADS + threadIdx.x;
  int parity = 0;
  for (int kk = 0; kk < KM_KGROUP; ++kk) {
    const int k = blockIdx.y * KM_KGROUP + kk;
    if (k >= K) break;
    const int64_t cell = (int64_t)k * RB + rb;
    if (block_counts[cell] == 0) continue;      // block-uniform
    int hit = -1;
    if (o < n_out) hit = hits[(int64_t)k * n_cap + o];
    const unsigned long long m = __ballot(hit >= 0);
    if (lane == 0) wave_cnt[parity][wave] = __popcll(m);
    __syncthreads();                            // double-buffered counts: one barrier per live cell
    if (hit >= 0) {
      int base = block_base[cell];
      for (int w = 0; w < wave; ++w) base += wave_cnt[parity][w];
      const int64_t pos = base + __popcll(m & ((1ull << lane) - 1ull));
      if (pos < pair_cap) {
        pair_in[pos] = hit;
        if (pair_out) pair_out[pos] = (int32_t)o;
        if (pair_k) pair_k[pos] = (uint16_t)k;
        // CSR slot = row start + number of this row's offsets below k (ascending-k order per row)
        out_pos[out_ptr[o] + mask_rank(mask_out + o * KW, k)] = (int32_t)pos;
        if (mask_in) in_pos[in_ptr[hit] + mask_rank(mask_in + (int64_t)hit * KW, k)] = (int32_t)pos;
      } else {
        *overflow = 2;
      }
    }
    parity ^= 1;
  }
}

// Finalisation of up to KM_MAXJOBS kernel maps in ONE launch each (blockIdx.x / blockIdx.y = map): the seven 6-D maps of
// a forward reach this point together (build_kernel_maps6).
struct FinalizeJobs {
  const int32_t *base[KM_MAXJOBS], *total[KM_MAXJOBS];
  int32_t *rule_ptr[KM_MAXJOBS], *tile_ptr[KM_MAXJOBS];
  int4 *desc[KM_MAXJOBS];
  long long tile_cap[KM_MAXJOBS];
  int K[KM_MAXJOBS], RB[KM_MAXJOBS];
};
// rule_ptr[k] = block_base[k * RB], rule_ptr[K] = total; tile_ptr = exclusive scan of ceil(P_k / DGR_TILE_M).
// One block per map, K <= 1024.
__global__ void __launch_bounds__(1024) kmap_finalize(FinalizeJobs j) {
  __shared__ int s[1024];
  const int m = blockIdx.x, K = j.K[m], RB = j.RB[m];
  const int32_t *block_base = j.base[m];
  const int k = threadIdx.x;
  int start = 0, end = 0;
  if (k < K) {
    start = block_base[(int64_t)k * RB];
    end = (k + 1 < K) ? block_base[(int64_t)(k + 1) * RB] : *j.total[m];
    j.rule_ptr[m][k] = start;
    if (k == K - 1) j.rule_ptr[m][K] = end;
  }
  const int tiles = (end - start + DGR_TILE_M - 1) / DGR_TILE_M;
  s[k] = tiles;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = (k >= d) ? s[k - d] : 0;
    __syncthreads();
    s[k] += v;
    __syncthreads();
  }
  if (k < K) j.tile_ptr[m][k] = s[k] - tiles;
  if (k == K - 1) j.tile_ptr[m][K] = s[k];
}

// one thread per tile: (k, first pair, pair count) so that the conv kernels fetch a tile with ONE
// 16-byte load instead of a 10-step binary search over tile_ptr on their critical path
__device__ __forceinline__ void tile_desc_one(const int32_t *__restrict__ tile_ptr, const int32_t *__restrict__ rule_ptr, int K,
                                              int4 *__restrict__ desc, int64_t tile_cap, int64_t t, int tile_m) {
  if (t >= tile_cap || t >= tile_ptr[K]) return;
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_ptr[mid] <= t) lo = mid; else hi = mid;
  }
  const int pstart = rule_ptr[lo] + ((int)t - tile_ptr[lo]) * tile_m;
  desc[t] = make_int4(lo, pstart, min(tile_m, rule_ptr[lo + 1] - pstart), 0);
}
__global__ void tile_desc_kernel(FinalizeJobs j) {
  const int m = blockIdx.y;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  tile_desc_one(j.tile_ptr[m], j.rule_ptr[m], j.K[m], j.desc[m], j.tile_cap[m], t, DGR_TILE_M);
}

// What a map keeps besides pair_in and the out-major CSR.  `lean` (the network forward): pair_out is only read by the
// transposed convs (strided maps used swapped, which also need the in-major CSR), pair_k only by the small-Cin conv1
// (same[0] / the conv1 map); the stand-alone maps object keeps everything.  The same for D = 3 and D = 6.
struct MapKeep {
  bool in_csr, pair_out, pair_k;
};
enum MapRole { MAP_SAME, MAP_CONV1, MAP_DOWN, MAP_LIST };   // same[level], conv1 (ks != 3), down[level], a list made from a table
static MapKeep map_keep(const DgrMapsMode &mode, MapRole role, int level) {
  switch (role) {
    case MAP_SAME: return {false, !mode.lean, !mode.lean || level == 0};
    case MAP_CONV1: return {false, !mode.lean, true};
    case MAP_DOWN: return {true, true, !mode.lean};
    default: return {false, false, false};
  }
}

// the parts of a kernel map that outlive the build
static int alloc_kernel_map(DgrArena &arena, int K, int64_t n_cap, int64_t n_in_cap, int max_pairs_per_row, MapKeep keep,
                            DgrKernelMap *km) {
  DGR_REQUIRE(K <= 1024, "kernel volume %d > 1024 not supported", K);
  km->K = K;
  const int64_t per_row = K < max_pairs_per_row ? K : max_pairs_per_row;
  km->pair_cap = per_row * n_cap;
  DGR_REQUIRE(km->pair_cap < (1ll << 31), "kernel map too large (%lld pairs)", (long long)km->pair_cap);
  DGR_ALLOC(km->rule_ptr, arena, int32_t, K + 1);
  DGR_ALLOC(km->tile_ptr, arena, int32_t, K + 1);
  DGR_ALLOC(km->pair_in, arena, int32_t, km->pair_cap);
  km->pair_out = nullptr;
  if (keep.pair_out) DGR_ALLOC(km->pair_out, arena, int32_t, km->pair_cap);
  km->tile_cap = km->pair_cap / DGR_TILE_M + K;
  DGR_ALLOC(km->tile_desc, arena, int4, km->tile_cap);
  DGR_ALLOC(km->out_ptr, arena, int32_t, n_cap + 1);
  DGR_ALLOC(km->out_pos, arena, int32_t, km->pair_cap);
  km->pair_k = nullptr;
  if (keep.pair_k) DGR_ALLOC(km->pair_k, arena, uint16_t, km->pair_cap);
  km->in_ptr = km->in_pos = nullptr;
  if (keep.in_csr) {
    DGR_ALLOC(km->in_ptr, arena, int32_t, n_in_cap + 1);
    DGR_ALLOC(km->in_pos, arena, int32_t, km->pair_cap);
  }
  return DGR_OK;
}

// The closing pass of every builder, for all maps of a call together: ONE multi-array scan -- per map the row counts
// -> km->out_ptr, the per-(offset, 256-row block) counts -> base and total, the input-row counts -> km->in_ptr where
// the map has an in-major CSR --, one finalisation launch (rule_ptr, tile_ptr) and one tile-descriptor launch.
struct MapClose {
  const int32_t *counts;    // [km->K * RB]
  int32_t *base, *total;
  int RB;
  const int32_t *cnt_out;   // [n_out]
  int64_t n_out;
  const int32_t *cnt_in;    // [n_in], or NULL
  int64_t n_in;
  DgrKernelMap *km;
};
static int close_maps(DgrArena &arena, const MapClose *maps, int nj, hipStream_t stream) {
  DGR_REQUIRE(nj >= 1 && nj <= KM_MAXJOBS, "kernel maps: %d maps per closing pass", nj);
  const int32_t *ins[DGR_SCAN_MAX];
  int32_t *outs[DGR_SCAN_MAX], *tots[DGR_SCAN_MAX];
  int64_t ns[DGR_SCAN_MAX];
  int c = 0;
  FinalizeJobs fj = {};
  int64_t max_tiles = 0;
  for (int m = 0; m < nj; ++m) {
    const MapClose &M = maps[m];
    const DgrKernelMap *km = M.km;
    DGR_REQUIRE(c + (M.cnt_in ? 3 : 2) <= DGR_SCAN_MAX, "kernel maps: more than %d arrays to scan", DGR_SCAN_MAX);
    ins[c] = M.cnt_out; outs[c] = km->out_ptr; tots[c] = nullptr; ns[c++] = M.n_out;
    ins[c] = M.counts; outs[c] = M.base; tots[c] = M.total; ns[c++] = (int64_t)km->K * M.RB;
    if (M.cnt_in) { ins[c] = M.cnt_in; outs[c] = km->in_ptr; tots[c] = nullptr; ns[c++] = M.n_in; }
    fj.base[m] = M.base; fj.total[m] = M.total; fj.K[m] = km->K; fj.RB[m] = M.RB;
    fj.rule_ptr[m] = km->rule_ptr; fj.tile_ptr[m] = km->tile_ptr;
    fj.desc[m] = km->tile_desc; fj.tile_cap[m] = km->tile_cap;
    max_tiles = std::max<int64_t>(max_tiles, km->tile_cap);
  }
  DGR_CHECK(dgr_exclusive_scan_multi(arena, c, ins, outs, ns, tots, stream));
  kmap_finalize<<<nj, 1024, 0, stream>>>(fj);
  tile_desc_kernel<<<dim3((unsigned)dgr_ceil_div(max_tiles, 256), (unsigned)nj), 256, 0, stream>>>(fj);
  return DGR_OK;
}

// D = 3 (rule-major maps of 3-D nets that do not run on neighbour tables; the stand-alone maps object): one map per call
static int build_kernel_map3(DgrArena &arena, const DgrCoordMap &in, const DgrCoordMap &out, int ks, int max_pairs_per_row,
                             MapKeep keep, DgrKernelMap *km, int32_t *overflow, hipStream_t stream) {
  constexpr int D = 3;
  const int K = ks * ks * ks;
  const int64_t n_cap = out.n_cap, n_in_cap = in.n_cap;
  const int RB = (int)dgr_ceil_div(n_cap, KM_THREADS);
  DGR_CHECK(alloc_kernel_map(arena, K, n_cap, n_in_cap, max_pairs_per_row, keep, km));
  const int KW = (K + 31) / 32;
  // transients (released after the last pass): per-(offset, block) counts, row bitmasks and the dense hit cache [K, n_cap]
  DgrArena::Mark mk = arena.mark();
  int32_t *counts, *base, *total;
  DGR_ALLOC(counts, arena, int32_t, (int64_t)K * RB);
  DGR_ALLOC(base, arena, int32_t, (int64_t)K * RB);
  DGR_ALLOC(total, arena, int32_t, 1);
  uint32_t *mask_out, *mask_in = nullptr;
  int32_t *cnt_out, *cnt_in = nullptr;
  {
    const size_t w_out = (size_t)(n_cap + 1) * KW, w_in = keep.in_csr ? (size_t)(n_in_cap + 1) * KW : 0;
    DGR_ALLOC(mask_out, arena, uint32_t, w_out + w_in);
    if (keep.in_csr) mask_in = mask_out + w_out;
    DGR_HIP_CHECK(hipMemsetAsync(mask_out, 0, (w_out + w_in) * sizeof(uint32_t), stream));
  }
  DGR_ALLOC(cnt_out, arena, int32_t, n_cap + 1);
  if (keep.in_csr) DGR_ALLOC(cnt_in, arena, int32_t, n_in_cap + 1);
  int32_t *hits;
  DGR_ALLOC(hits, arena, int32_t, (int64_t)K * n_cap);
  kmap_search<D><<<dim3(RB, K), KM_THREADS, 0, stream>>>(out.coords, out.n_dev, in.coords, in.table, in.table_mask, ks,
                                                         in.ts, RB, n_cap, hits, counts, KW, mask_out, mask_in);
  DGR_LAUNCH_CHECK();
  // per-row pair counts -> CSR row pointers (out rows; in rows for maps used swapped)
  mask_count_kernel<<<(int)dgr_ceil_div(n_cap + 1, 256), 256, 0, stream>>>(mask_out, KW, out.n_dev, n_cap + 1, cnt_out);
  if (keep.in_csr)
    mask_count_kernel<<<(int)dgr_ceil_div(n_in_cap + 1, 256), 256, 0, stream>>>(mask_in, KW, in.n_dev, n_in_cap + 1, cnt_in);
  const MapClose mc = {counts, base, total, RB, cnt_out, n_cap + 1, cnt_in, n_in_cap + 1, km};
  DGR_CHECK(close_maps(arena, &mc, 1, stream));
  kmap_fill<<<dim3(RB, (K + KM_KGROUP - 1) / KM_KGROUP), KM_THREADS, 0, stream>>>(
      out.n_dev, RB, K, n_cap, hits, counts, base, km->pair_in, km->pair_out, km->pair_cap, overflow, KW, mask_out,
      km->out_ptr, km->out_pos, mask_in, km->in_ptr, km->in_pos, km->pair_k);
  DGR_LAUNCH_CHECK();
  arena.rewind(mk);
  km->built = true;
  return DGR_OK;
}

// D = 6: ALL kernel maps of a sparse tensor (four same-stride maps, three strided ones) are built phase by phase
// together -- one clear for all bit matrices, the searches and transposing passes back to back, ONE multi-array scan
// (17 arrays), one finalisation launch, one tile-descriptor launch, then the placing passes.  Round 3 built map after
// map: 21 scan launches, 7 finalisations, 7 descriptor launches and 7 clears per forward, ~5 us each and nothing else
// running next to them.
struct Kmap6Job {
  const DgrCoordMap *in, *out;
  const DgrHalfBuckets *hb;     // first-half buckets of `in`
  const DgrHalfBuckets *hb_out; // ... of `out` (the order the search walks the output rows in)
  MapKeep keep;
  DgrKernelMap *km;
};
static int build_kernel_maps6(DgrArena &arena, const Kmap6Job *jobs, int nj, int max_pairs_per_row, int32_t *overflow,
                              hipStream_t stream) {
  constexpr int K = 729, KW = (K + 31) / 32;
  DGR_REQUIRE(nj >= 1 && nj <= KM_MAXJOBS, "6-D kernel maps: %d jobs", nj);
  Maps6 R = {};
  int max_sb = 0, max_rb = 0, max_pb = 0;
  for (int m = 0; m < nj; ++m) {
    const Kmap6Job &J = jobs[m];
    Map6 &r = R.m[m];
    DGR_REQUIRE(J.hb && J.hb->built && J.hb_out && J.hb_out->built, "6-D kernel map: first-half buckets missing");
    const int64_t n_cap = J.out->n_cap;
    r.n_in_cap = J.in->n_cap;
    DGR_REQUIRE(n_cap < (1ll << 27) && r.n_in_cap < (1ll << 27), "6-D kernel maps: more than 2^27 rows");
    DGR_CHECK(alloc_kernel_map(arena, K, n_cap, r.n_in_cap, max_pairs_per_row, J.keep, J.km));
    r.km = *J.km;
    r.RB = (int)dgr_ceil_div(n_cap, KM_THREADS);
    // same-stride maps (in and out are the SAME coordinate set) are symmetric: search half the offsets
    const int symmetric = (J.in->coords == J.out->coords && !J.keep.in_csr) ? 1 : 0;
    r.s = PrunedArgs{J.out->coords, J.out->n_dev, J.hb_out->second, n_cap, *J.hb, J.in->ts, symmetric};
    // hit list: one region per wave of the search (thread = (first-half offset, row in bucket order)); a wave whose
    // region overflows is replayed by the placing kernel
    const int64_t search_blocks = dgr_ceil_div(n_cap * (symmetric ? 14 : 27), KM_THREADS);
    DGR_REQUIRE(search_blocks * (KM_THREADS / 64) < (1ll << 31), "6-D kernel map: too many search waves");
    r.search_blocks = (int)search_blocks;
    r.hit_waves = r.search_blocks * (KM_THREADS / 64);
    r.place_blocks = std::min(r.search_blocks, 16384);
    r.hl.region = km_region_of(J.in->ts, symmetric);
    max_sb = std::max(max_sb, r.search_blocks);
    max_rb = std::max(max_rb, r.RB);
    max_pb = std::max(max_pb, r.place_blocks);
  }
  DgrArena::Mark mk = arena.mark();
  // the bit matrices (out rows; in rows for maps used swapped) and the row counts of ALL maps: one allocation, one clear
  // (kmap_colmask leaves cnt_out of the rows beyond the count to this clear)
  {
    size_t words = 0;
    for (int m = 0; m < nj; ++m)
      words += (size_t)(R.m[m].s.n_cap + 1) * (KW + 1) + (jobs[m].keep.in_csr ? (size_t)(R.m[m].n_in_cap + 1) * KW : 0);
    uint32_t *pool;
    DGR_ALLOC(pool, arena, uint32_t, words);
    DGR_HIP_CHECK(hipMemsetAsync(pool, 0, words * sizeof(uint32_t), stream));
    for (int m = 0; m < nj; ++m) {
      Map6 &r = R.m[m];
      r.mask_out = pool; pool += (size_t)(r.s.n_cap + 1) * KW;
      if (jobs[m].keep.in_csr) { r.mask_in = pool; pool += (size_t)(r.n_in_cap + 1) * KW; }
      r.cnt_out = reinterpret_cast<int32_t *>(pool); pool += (size_t)(r.s.n_cap + 1);
    }
  }
  MapClose mc[KM_MAXJOBS];
  MaskCountJobs mj = {};   // the input rows of the maps with an in-major CSR
  int nm = 0;
  long long max_rows = 0;
  for (int m = 0; m < nj; ++m) {
    Map6 &r = R.m[m];
    const int64_t n_cap = r.s.n_cap;
    const bool in_csr = jobs[m].keep.in_csr;
    DGR_ALLOC(r.counts, arena, int32_t, (int64_t)K * r.RB);
    DGR_ALLOC(r.base, arena, int32_t, (int64_t)K * r.RB);
    DGR_ALLOC(r.total, arena, int32_t, 1);
    if (in_csr) DGR_ALLOC(r.cnt_in, arena, int32_t, r.n_in_cap + 1);
    DGR_ALLOC(r.cell, arena, int4, (int64_t)r.RB * (KM_THREADS / 64) * K);
    DGR_ALLOC(r.hl.recs, arena, unsigned long long, (int64_t)r.hit_waves * r.hl.region);
    DGR_ALLOC(r.hl.wave_count, arena, int32_t, r.hit_waves);
    DGR_ALLOC(r.wpre_out, arena, unsigned short, (n_cap + 1) * KW);
    if (in_csr) {
      DGR_ALLOC(r.wpre_in, arena, unsigned short, (r.n_in_cap + 1) * KW);
      mj.mask[nm] = r.mask_in; mj.n_dev[nm] = jobs[m].in->n_dev; mj.n_cap[nm] = r.n_in_cap + 1;
      mj.cnt[nm] = r.cnt_in; mj.wpre[nm] = r.wpre_in;
      max_rows = std::max(max_rows, mj.n_cap[nm]);
      ++nm;
    }
    mc[m] = MapClose{r.counts, r.base, r.total, r.RB, r.cnt_out, n_cap + 1, r.cnt_in, r.n_in_cap + 1, jobs[m].km};
  }
  // ---- search (bits + hit records) of all maps in one launch, then the transposing / counting passes in one launch each
  kmap_bits_pruned6<<<dim3((unsigned)max_sb, (unsigned)nj), KM_THREADS, 0, stream>>>(R, KW);
  kmap_colmask<<<dim3((unsigned)max_rb, (unsigned)nj), KM_THREADS, 0, stream>>>(R, K, KW);
  if (nm) mask_count_multi<KW><<<dim3((unsigned)dgr_ceil_div(max_rows, 256), (unsigned)nm), 256, 0, stream>>>(mj);
  DGR_LAUNCH_CHECK();
  // ---- every scan of every map (CSR row pointers, cell bases), rule and tile pointers, tile descriptors
  DGR_CHECK(close_maps(arena, mc, nj, stream));
  // ---- place: all maps in one launch
  kmap_place_hits<<<dim3((unsigned)max_pb, (unsigned)nj), KM_THREADS, 0, stream>>>(R, K, KW, overflow);
  DGR_LAUNCH_CHECK();
  arena.rewind(mk);
  for (int m = 0; m < nj; ++m) jobs[m].km->built = true;
  return DGR_OK;
}

// =========================== D = 3: dense neighbour tables =====================================
// One launch per (input map, output map) pair: a thread owns an output row and one z-slab of the 3^3
// offsets (9 probes issued together).  SIGN = +1: q = o + delta_k * ts (same-stride and strided convs,
// out = the output map's rows); SIGN = -1: q = f - delta_k * ts (transposed convs: fine output row f,
// coarse input c with f = c + delta_k * ts_fine).  Rows beyond the device-side count get -1.
// All ten tables of a 3-D sparse tensor in ONE launch (round 5; round 4: ten launches of 11-130 us with idle tails):
// blockIdx.z = table, blockIdx.y = z-slab, blockIdx.x = row block of the table (surplus blocks of the smaller tables exit).
constexpr int NBR_JOBS = 10;
struct NbrJobs {
  const int32_t *out_coords[NBR_JOBS], *n_out_dev[NBR_JOBS], *in_coords[NBR_JOBS], *in_table[NBR_JOBS];
  uint32_t in_mask[NBR_JOBS];
  int ts[NBR_JOBS];        // signed: +ts for q = o + delta ts, -ts for q = f - delta ts (transposed convs)
  long long n_pad[NBR_JOBS];
  int32_t *nbr[NBR_JOBS];
};
__global__ void __launch_bounds__(KM_THREADS) nbr_search3(NbrJobs J) {
  const int jm = blockIdx.z;
  const int64_t n_pad = J.n_pad[jm];
  const int64_t o = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
  if (o >= n_pad) return;
  int32_t *__restrict__ nbr = J.nbr[jm];
  const int kz = blockIdx.y;
  if (o >= *J.n_out_dev[jm]) {
#pragma unroll
    for (int u = 0; u < 9; ++u) nbr[(int64_t)(9 * kz + u) * n_pad + o] = -1;
    return;
  }
  const int sts = J.ts[jm];
  const int4 c = *reinterpret_cast<const int4 *>(J.out_coords[jm] + o * 4);
  int32_t q[9][4];
#pragma unroll
  for (int u = 0; u < 9; ++u) {   // offset index k = x + 3 y + 9 z (first spatial dimension fastest: offset_of)
    q[u][0] = c.x;
    q[u][1] = c.y + ((u % 3) - 1) * sts;
    q[u][2] = c.z + ((u / 3) - 1) * sts;
    q[u][3] = c.w + (kz - 1) * sts;
  }
  int hit[9];
  dgr_lookup_many<4, 9>(J.in_table[jm], J.in_mask[jm], J.in_coords[jm], q, hit);
#pragma unroll
  for (int u = 0; u < 9; ++u) nbr[(int64_t)(9 * kz + u) * n_pad + o] = hit[u];
}

// ---- the rows of a (fine) map grouped by the parity class of their coordinates (DgrNbrTable::perm; conv_up.hip): a
// stable counting sort in two small launches for the three fine levels together -- per 256-row block the eight class
// counts, then every block adds up the counts of the blocks before it and places its rows.  (One atomic per wave and
// class on eight global counters instead: +0.3 ms per forward, the counters serialise at ~40 ns per atomic.)
struct ClsJobs {
  const int32_t *coords[3], *n_dev[3];
  int ts[3], nb[3];
  int32_t *blk_cnt[3], *perm[3], *cls_count[3];
  long long cls_cap[3];
};
__device__ __forceinline__ int parity_class(const int32_t *coords, int64_t o, int ts) {
  const int4 c = *reinterpret_cast<const int4 *>(coords + o * 4);
  return ((c.y / ts) & 1) | (((c.z / ts) & 1) << 1) | (((c.w / ts) & 1) << 2);
}
__global__ void __launch_bounds__(KM_THREADS) cls_count_kernel(ClsJobs J) {
  __shared__ int wcnt[KM_THREADS / 64][8];
  const int l = blockIdx.y, b = blockIdx.x;
  if (b >= J.nb[l]) return;
  const int64_t o = (int64_t)b * KM_THREADS + threadIdx.x;
  const int cls = o < *J.n_dev[l] ? parity_class(J.coords[l], o, J.ts[l]) : 8;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const unsigned long long m = __ballot(cls == c);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6][c] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    int n = 0;
    for (int w = 0; w < KM_THREADS / 64; ++w) n += wcnt[w][threadIdx.x];
    J.blk_cnt[l][b * 8 + threadIdx.x] = n;
  }
}
__global__ void __launch_bounds__(KM_THREADS) cls_fill_kernel(ClsJobs J) {
  __shared__ int part[KM_THREADS / 64][8], before[8], wcnt[KM_THREADS / 64][8];
  const int l = blockIdx.y, b = blockIdx.x;
  if (b >= J.nb[l]) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // rows of every class in the blocks before this one
  int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int bb = threadIdx.x; bb < b; bb += KM_THREADS) {
    const int4 lo = *reinterpret_cast<const int4 *>(J.blk_cnt[l] + bb * 8), hi = *reinterpret_cast<const int4 *>(J.blk_cnt[l] + bb * 8 + 4);
    acc[0] += lo.x; acc[1] += lo.y; acc[2] += lo.z; acc[3] += lo.w;
    acc[4] += hi.x; acc[5] += hi.y; acc[6] += hi.z; acc[7] += hi.w;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    int v = acc[c];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if (lane == 0) part[wave][c] = v;
  }
  const int64_t o = (int64_t)b * KM_THREADS + threadIdx.x;
  const int cls = o < *J.n_dev[l] ? parity_class(J.coords[l], o, J.ts[l]) : 8;
  int rank = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const unsigned long long m = __ballot(cls == c);
    if (lane == 0) wcnt[wave][c] = __popcll(m);
    if (cls == c) rank = __popcll(m & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    int n = 0;
    for (int w = 0; w < KM_THREADS / 64; ++w) n += part[w][threadIdx.x];
    before[threadIdx.x] = n;
    if (b == J.nb[l] - 1) {   // the last block knows every class's total
      for (int w = 0; w < KM_THREADS / 64; ++w) n += wcnt[w][threadIdx.x];
      J.cls_count[l][threadIdx.x] = n;
    }
  }
  __syncthreads();
  if (cls < 8) {
    int pos = before[cls] + rank;
    for (int w = 0; w < wave; ++w) pos += wcnt[w][cls];
    J.perm[l][(int64_t)cls * J.cls_cap[l] + pos] = (int32_t)o;
  }
}

// queue one table (allocation here, the search in nbr_tables_launch)
static int build_nbr_table(DgrArena &arena, const DgrCoordMap &in, const DgrCoordMap &out, int ts, int sign,
                           DgrNbrTable *t, NbrJobs *jobs, int *nj, int32_t *cls_count = nullptr) {
  t->K = 27;
  t->n_pad = dgr_ceil_div(out.n_cap, DGR_OS_ROWS) * DGR_OS_ROWS;
  DGR_ALLOC(t->nbr, arena, int32_t, t->n_pad * 27);
  t->perm = nullptr; t->cls_count = nullptr; t->cls_cap = 0;
  if (cls_count) {   // (the row list and the counts are written by cls_fill_kernel)
    t->cls_cap = t->n_pad;
    t->cls_count = cls_count;
    DGR_ALLOC(t->perm, arena, int32_t, 8 * t->cls_cap);
  }
  DGR_REQUIRE(*nj < NBR_JOBS, "neighbour tables: more than %d per launch", NBR_JOBS);
  const int m = (*nj)++;
  jobs->out_coords[m] = out.coords; jobs->n_out_dev[m] = out.n_dev; jobs->in_coords[m] = in.coords;
  jobs->in_table[m] = in.table; jobs->in_mask[m] = in.table_mask; jobs->ts[m] = sign > 0 ? ts : -ts;
  jobs->n_pad[m] = t->n_pad; jobs->nbr[m] = t->nbr;
  t->built = true;
  return DGR_OK;
}
static int nbr_tables_launch(const NbrJobs &jobs, int nj, hipStream_t stream) {
  long long n_max = 0;
  for (int m = 0; m < nj; ++m) n_max = std::max(n_max, jobs.n_pad[m]);
  if (nj == 0) return DGR_OK;
  nbr_search3<<<dim3((unsigned)dgr_ceil_div(n_max, KM_THREADS), 3, (unsigned)nj), KM_THREADS, 0, stream>>>(jobs);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}

__global__ void nbr_count_kernel(const int32_t *__restrict__ nbr, int64_t n_pad, const int32_t *n_out_dev,
                                 unsigned long long *__restrict__ counts) {
  const int k = blockIdx.y;
  const int n = *n_out_dev;
  int c = 0;
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < n; o += (int64_t)gridDim.x * blockDim.x)
    c += nbr[(int64_t)k * n_pad + o] >= 0;
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&counts[k], (unsigned long long)c);
}

int dgr_nbr_counts(const DgrNbrTable &t, const int32_t *n_out_dev, int64_t counts[27]) {
  unsigned long long *dev;
  DGR_HIP_CHECK(hipMalloc((void **)&dev, 27 * sizeof(unsigned long long)));
  DGR_HIP_CHECK(hipMemset(dev, 0, 27 * sizeof(unsigned long long)));
  nbr_count_kernel<<<dim3(64, 27), 256>>>(t.nbr, t.n_pad, n_out_dev, dev);
  unsigned long long host[27];
  hipError_t e = hipMemcpy(host, dev, sizeof(host), hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  DGR_HIP_CHECK(e);
  for (int k = 0; k < 27; ++k) counts[k] = (int64_t)host[k];
  return DGR_OK;
}

// ---- D = 3: rule-major lists FROM a neighbour table, for the layers of the 3-D net that run on the wide rule-major
// kernel (conv_wide.hip + dgr_reduce_rows): rule k = the rows o with nbr[k][o] >= 0 in ascending o, a row's out_pos
// entries = its valid offsets in ascending k -- the contract of a lean rule-major map without a second
// hash search.  Counting per (offset, 256-row block) and per row, ONE multi-array scan, one fill; the maps of a forward
// go through each launch together (blockIdx.y = map).  No atomics: every position is a prefix sum, two builds are equal.
constexpr int NL_JOBS = 3;
struct NbrListJobs {
  const int32_t *nbr[NL_JOBS], *n_out_dev[NL_JOBS];
  long long n_pad[NL_JOBS], n_cap[NL_JOBS];
  int RB[NL_JOBS];                                       // 256-row blocks covering rows 0 .. n_cap (out_ptr has n_cap + 1 entries)
  int32_t *counts[NL_JOBS], *cnt_out[NL_JOBS];           // pass 1: pairs per (offset, block) [27 * RB] and per row [n_cap + 1]
  const int32_t *base[NL_JOBS], *out_ptr[NL_JOBS];       // ... scanned
  int32_t *pair_in[NL_JOBS], *out_pos[NL_JOBS];
};
__global__ void __launch_bounds__(KM_THREADS) nbr_list_count(NbrListJobs J) {
  __shared__ int wcnt[KM_THREADS / 64][27];
  const int m = blockIdx.y, b = blockIdx.x;
  if (b >= J.RB[m]) return;
  const int64_t o = (int64_t)b * KM_THREADS + threadIdx.x, n_pad = J.n_pad[m];
  const int32_t *__restrict__ nbr = J.nbr[m];
  const bool live = o < *J.n_out_dev[m];   // (n_out <= n_cap <= n_pad: a live row lies inside the table)
  int mine = 0;
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    const bool hit = live && nbr[(int64_t)k * n_pad + o] >= 0;
    mine += hit;
    const unsigned long long bal = __ballot(hit);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6][k] = __popcll(bal);
  }
  __syncthreads();
  if (threadIdx.x < 27) {
    int n = 0;
    for (int w = 0; w < KM_THREADS / 64; ++w) n += wcnt[w][threadIdx.x];
    J.counts[m][(int64_t)threadIdx.x * J.RB[m] + b] = n;
  }
  if (o <= J.n_cap[m]) J.cnt_out[m][o] = mine;
}
__global__ void __launch_bounds__(KM_THREADS) nbr_list_fill(NbrListJobs J) {
  __shared__ int wcnt[KM_THREADS / 64][27];
  const int m = blockIdx.y, b = blockIdx.x;
  if (b >= J.RB[m]) return;
  const int64_t o = (int64_t)b * KM_THREADS + threadIdx.x, n_pad = J.n_pad[m];
  const int32_t *__restrict__ nbr = J.nbr[m];
  if ((int64_t)b * KM_THREADS >= *J.n_out_dev[m]) return;   // (the whole block: no barrier is skipped by a part of it)
  const bool live = o < *J.n_out_dev[m];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    const unsigned long long bal = __ballot(live && nbr[(int64_t)k * n_pad + o] >= 0);
    if (lane == 0) wcnt[wave][k] = __popcll(bal);
  }
  __syncthreads();
  int slot = live ? J.out_ptr[m][o] : 0;
  int32_t *__restrict__ pair_in = J.pair_in[m], *__restrict__ out_pos = J.out_pos[m];
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    const int v = live ? nbr[(int64_t)k * n_pad + o] : -1;
    const unsigned long long bal = __ballot(v >= 0);
    if (v < 0) continue;
    int pos = J.base[m][(int64_t)k * J.RB[m] + b] + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wcnt[w][k];
    pair_in[pos] = v;        // pos < 27 n_cap = pair_cap: at most one pair per (offset, row)
    out_pos[slot++] = pos;   // the row's slots [out_ptr[o], out_ptr[o + 1]) in ascending k
  }
}

// Lists for `nj` tables (in, out level, table, map); the scanned temporaries are released before returning.
struct NbrListSpec {
  const DgrNbrTable *t;
  const DgrCoordMap *out;
  DgrKernelMap *km;
};
static int build_nbr_lists3(DgrArena &arena, const NbrListSpec *specs, int nj, MapKeep keep, hipStream_t stream) {
  DGR_REQUIRE(nj >= 1 && nj <= NL_JOBS, "neighbour-table lists: %d maps per call", nj);
  DGR_REQUIRE(!keep.in_csr && !keep.pair_out && !keep.pair_k, "neighbour-table lists: pair_in and the out-major CSR only");
  NbrListJobs J = {};
  for (int m = 0; m < nj; ++m) {
    const int64_t n_cap = specs[m].out->n_cap;
    DGR_REQUIRE(specs[m].t->built && specs[m].t->n_pad >= n_cap, "neighbour-table lists: table %d is not built", m);
    DGR_CHECK(alloc_kernel_map(arena, 27, n_cap, 0, 27, keep, specs[m].km));   // at most one pair per (offset, row)
  }
  DgrArena::Mark mk = arena.mark();
  MapClose mc[NL_JOBS];
  int max_rb = 0;
  for (int m = 0; m < nj; ++m) {
    DgrKernelMap *km = specs[m].km;
    const int64_t n_cap = specs[m].out->n_cap;
    const int RB = (int)dgr_ceil_div(n_cap + 1, KM_THREADS);
    int32_t *counts, *base, *total, *cnt_out;
    DGR_ALLOC(counts, arena, int32_t, (int64_t)27 * RB);
    DGR_ALLOC(base, arena, int32_t, (int64_t)27 * RB);
    DGR_ALLOC(total, arena, int32_t, 1);
    DGR_ALLOC(cnt_out, arena, int32_t, n_cap + 1);
    J.nbr[m] = specs[m].t->nbr; J.n_out_dev[m] = specs[m].out->n_dev; J.n_pad[m] = specs[m].t->n_pad; J.n_cap[m] = n_cap;
    J.RB[m] = RB; J.counts[m] = counts; J.cnt_out[m] = cnt_out; J.base[m] = base; J.out_ptr[m] = km->out_ptr;
    J.pair_in[m] = km->pair_in; J.out_pos[m] = km->out_pos;
    mc[m] = MapClose{counts, base, total, RB, cnt_out, n_cap + 1, nullptr, 0, km};
    max_rb = std::max(max_rb, RB);
  }
  nbr_list_count<<<dim3((unsigned)max_rb, (unsigned)nj), KM_THREADS, 0, stream>>>(J);
  DGR_LAUNCH_CHECK();
  DGR_CHECK(close_maps(arena, mc, nj, stream));
  nbr_list_fill<<<dim3((unsigned)max_rb, (unsigned)nj), KM_THREADS, 0, stream>>>(J);
  DGR_LAUNCH_CHECK();
  arena.rewind(mk);
  for (int m = 0; m < nj; ++m) specs[m].km->built = true;
  return DGR_OK;
}

int dgr_build_maps(DgrArena &arena, const int32_t *coords, int64_t N, int D, int conv1_ks,
                   DgrMapSet *ms, hipStream_t stream, DgrMapsMode mode) {
  DGR_REQUIRE(D == 3 || D == 6, "D=%d not supported (the DGR path uses D=3 and D=6)", D);
  DGR_REQUIRE(!mode.tables || D == 3, "neighbour tables are a D = 3 structure");
  DGR_REQUIRE(!mode.lists || (mode.lean && mode.tables), "lists from neighbour tables go with lean maps and D = 3");
  DGR_REQUIRE(conv1_ks % 2 == 1 && conv1_ks >= 1, "conv1 kernel size must be odd");
  DGR_REQUIRE(N > 0 && N < (1ll << 30), "N=%lld out of range", (long long)N);
  ms->D = D;
  ms->nc = D + 1;
  ms->conv1_ks = conv1_ks;
  if (!ms->overflow) {  // callers may pre-set a flag word that outlives arena rewinds
    DGR_ALLOC(ms->overflow, arena, int32_t, 1);
    DGR_HIP_CHECK(hipMemsetAsync(ms->overflow, 0, sizeof(int32_t), stream));
  }
  DGR_CHECK(dgr_build_coord_maps(arena, coords, N, ms, stream));
  if (mode.tables) {
    // D = 3 network forward: ten dense neighbour tables, ONE launch for all of them -- no pair lists, no CSR, no scans
    ms->use_nbr = true;
    NbrJobs nbj = {};
    int n_nbj = 0;
    int32_t *cls;   // parity-class row counts of the three fine maps the transposed convs write
    DGR_ALLOC(cls, arena, int32_t, 3 * 8);
    for (int l = 0; l < 4; ++l) DGR_CHECK(build_nbr_table(arena, ms->cm[l], ms->cm[l], ms->cm[l].ts, +1, &ms->nsame[l], &nbj, &n_nbj));
    for (int l = 0; l < 3; ++l) {
      DGR_CHECK(build_nbr_table(arena, ms->cm[l], ms->cm[l + 1], ms->cm[l].ts, +1, &ms->ndown[l], &nbj, &n_nbj));
      DGR_CHECK(build_nbr_table(arena, ms->cm[l + 1], ms->cm[l], ms->cm[l].ts, -1, &ms->nup[l], &nbj, &n_nbj, cls + 8 * l));
    }
    DGR_CHECK(nbr_tables_launch(nbj, n_nbj, stream));
    {
      ClsJobs cj = {};
      int max_nb = 0;
      for (int l = 0; l < 3; ++l) {
        cj.coords[l] = ms->cm[l].coords; cj.n_dev[l] = ms->cm[l].n_dev; cj.ts[l] = ms->cm[l].ts;
        cj.nb[l] = (int)dgr_ceil_div(ms->cm[l].n_cap, KM_THREADS);
        DGR_ALLOC(cj.blk_cnt[l], arena, int32_t, (int64_t)cj.nb[l] * 8);
        cj.perm[l] = ms->nup[l].perm; cj.cls_count[l] = ms->nup[l].cls_count; cj.cls_cap[l] = ms->nup[l].cls_cap;
        max_nb = std::max(max_nb, cj.nb[l]);
      }
      cls_count_kernel<<<dim3((unsigned)max_nb, 3), KM_THREADS, 0, stream>>>(cj);
      cls_fill_kernel<<<dim3((unsigned)max_nb, 3), KM_THREADS, 0, stream>>>(cj);
      DGR_LAUNCH_CHECK();
    }
    if (mode.lists) {
      // ... plus rule-major lists of the two coarse same-stride tables and the level 2 -> 3 strided one: the 128 / 256-channel
      // layers there run on the wide rule-major kernel (net.hip, layer_kind)
      const NbrListSpec specs[3] = {{&ms->nsame[2], &ms->cm[2], &ms->same[2]}, {&ms->nsame[3], &ms->cm[3], &ms->same[3]},
                                    {&ms->ndown[2], &ms->cm[3], &ms->down[2]}};
      DGR_CHECK(build_nbr_lists3(arena, specs, 3, map_keep(mode, MAP_LIST, 0), stream));
    }
    // the network forward needs nothing else: conv1 runs fused with its neighbour search, whatever its kernel size
    if (mode.lean) return DGR_OK;
  }
  // capacity per output row: exact (K) in 3-D; in 6-D 3^6 = 729 offsets but measured mean
  // occupancy is 2..40 neighbours -- reserve 160 per row and raise the overflow flag beyond.
  const int cap_row = (D == 3) ? 1024 : 160;
  if (D == 6) {
    DGR_REQUIRE(conv1_ks == 3, "6-D kernel maps support kernel size 3 only (got %d)", conv1_ks);
    // first-half buckets of every level: the pruned search of all seven maps (since round 4 also at tensor stride 8)
    // (the coarse maps are numbered in bucket order on the way; level 0 keeps the caller's row order)
    DGR_CHECK(dgr_build_half_buckets(arena, ms->cm, ms->hb, 4, 1, stream));
    Kmap6Job jobs[7];
    for (int l = 0; l < 4; ++l) jobs[l] = {&ms->cm[l], &ms->cm[l], &ms->hb[l], &ms->hb[l], map_keep(mode, MAP_SAME, l), &ms->same[l]};
    for (int l = 0; l < 3; ++l)
      jobs[4 + l] = {&ms->cm[l], &ms->cm[l + 1], &ms->hb[l], &ms->hb[l + 1], map_keep(mode, MAP_DOWN, l), &ms->down[l]};
    DGR_CHECK(build_kernel_maps6(arena, jobs, 7, cap_row, ms->overflow, stream));
    ms->conv1 = ms->same[0];
    return DGR_OK;
  }
  auto build = [&](const DgrCoordMap &in, const DgrCoordMap &out, int ks, MapRole role, int l, DgrKernelMap *km) -> int {
    return build_kernel_map3(arena, in, out, ks, cap_row, map_keep(mode, role, l), km, ms->overflow, stream);
  };
  for (int l = 0; l < 4; ++l) DGR_CHECK(build(ms->cm[l], ms->cm[l], 3, MAP_SAME, l, &ms->same[l]));
  if (conv1_ks == 3)
    ms->conv1 = ms->same[0];
  else
    DGR_CHECK(build(ms->cm[0], ms->cm[0], conv1_ks, MAP_CONV1, 0, &ms->conv1));
  for (int l = 0; l < 3; ++l) DGR_CHECK(build(ms->cm[l], ms->cm[l + 1], 3, MAP_DOWN, l, &ms->down[l]));
  return DGR_OK;
}
