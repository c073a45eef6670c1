// split_kernels.hpp — the stable LDS-staged multi-split of up to three 8-byte columns (the fast path of
// sqlrs_hash_partition, partition.hip, and of sqlrs_range_partition, range_partition.hip), generic over the
// function that maps a row to its part:
//   * HashPart   p = part_of(key): the hash exchange (join / group-by keys);
//   * RangePart  p = number of splitters <= (encoded key, global row position): the ORDER BY exchange.
// A part function owns SMEM_TUPLES 16-byte words of LDS that setup() fills (the range splitters); the kernels
// put a barrier between setup() and the first use when SMEM_TUPLES > 0.  HashPart has none, so its kernels are the
// code they were before the split into this header.
#pragma once

#include "device_utils.hpp"

namespace sq {

__device__ __forceinline__ uint32_t part_of(uint64_t key, uint32_t parts) {
  uint64_t h = mix64(key ^ 0x5851f42d4c957f2dULL);
  return (uint32_t)(((h >> 32) * (uint64_t)parts) >> 32);
}

constexpr int SP_WG = 512, SP_WAVES = 8, SP_ITEMS = 8, SP_TILE = SP_WG * SP_ITEMS;

struct HashPart {
  uint32_t parts;
  static constexpr int SMEM_TUPLES = 0;
  __device__ __forceinline__ void setup(u64x2 *) const {}
  __device__ __forceinline__ uint32_t operator()(const u64x2 *, uint64_t key, int64_t) const { return part_of(key, parts); }
};

// ORDER BY one int64 (KIND 0) / float64 (KIND 1) key without NULLs.  Tuple of a row = (encoded key, row_base + row):
// the encoding of the local Order (i64_to_ordered / f64_to_ordered, complemented for DESC: ops.hip sort_key_kernel).
// The splitters (parts - 1 tuples, nondecreasing) are padded in LDS to p2 - 1 entries (p2 = the power of two >= parts)
// with all-ones tuples, which no row reaches (positions stay below 2^63): the part is found in log2(p2) steps of a
// branch-free binary search, one 16-byte LDS read per step.
template <int KIND> struct RangePart {
  uint32_t parts, p2;
  uint64_t flip; // ~0 for DESC
  int64_t row_base;
  const u64x2 *spl; // parts - 1 tuples (device)
  static constexpr int SMEM_TUPLES = 255;
  __device__ __forceinline__ void setup(u64x2 *s) const {
    for (uint32_t t = threadIdx.x; t + 1 < p2; t += SP_WG) {
      u64x2 v;
      v.x = ~0ull;
      v.y = ~0ull;
      s[t] = t + 1 < parts ? spl[t] : v;
    }
  }
  __device__ __forceinline__ uint64_t encode(uint64_t bits) const {
    return (KIND == 0 ? i64_to_ordered((int64_t)bits) : f64_to_ordered(__longlong_as_double((long long)bits))) ^ flip;
  }
  __device__ __forceinline__ uint32_t operator()(const u64x2 *s, uint64_t bits, int64_t row) const {
    const uint64_t k = encode(bits), pos = (uint64_t)(row_base + row);
    uint32_t at = 0;
    for (uint32_t step = p2 >> 1; step; step >>= 1) {
      const u64x2 t = s[at + step - 1];
      if (t.x < k || (t.x == k && t.y <= pos)) at += step;
    }
    return at;
  }
};

// pass 1: per (part, tile) row counts (part-major: the exclusive scan of the matrix gives every (tile, part) run its
// start).  WRITE_IDS: the part of every row is also stored as one byte for the scatter pass (READ_IDS there).
template <class P, bool WRITE_IDS = false>
__global__ __launch_bounds__(SP_WG) void split_hist_kernel(const uint64_t *__restrict__ keys, int64_t n, P pf,
                                                           int64_t ntiles, uint32_t *__restrict__ hist,
                                                           uint8_t *__restrict__ ids = nullptr) {
  __shared__ uint32_t h[256];
  __shared__ u64x2 psm[P::SMEM_TUPLES > 0 ? P::SMEM_TUPLES : 1];
  if (threadIdx.x < 256) h[threadIdx.x] = 0;
  if (P::SMEM_TUPLES > 0) pf.setup(psm);
  const int64_t base = (int64_t)blockIdx.x * SP_TILE + threadIdx.x;
  uint64_t k[SP_ITEMS];
#pragma unroll
  for (int r = 0; r < SP_ITEMS; r++) k[r] = keys[min(base + r * SP_WG, n - 1)];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SP_ITEMS; r++)
    if (base + r * SP_WG < n) {
      const uint32_t d = pf(psm, k[r], base + r * SP_WG);
      atomicAdd(&h[d], 1u);
      if (WRITE_IDS) ids[base + r * SP_WG] = (uint8_t)d;
    }
  __syncthreads();
  if (threadIdx.x < pf.parts) hist[(int64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// pass 2: same scheme as the radix sort's stable scatter (sort.hip): row order inside the tile is (wave,
// chunk, lane); lanes of a chunk with the same partition find each other with 8 ballots, the first
// of them bumps the wave's own counter, a prefix over waves and partitions gives the tile-local
// position, the tile is staged partition-major in LDS and leaves as one run per partition.
// The key is column `kc` of the carried ones; READ_IDS: the part comes from the byte pass 1 wrote.
template <class P, int NC, bool READ_IDS = false>
__global__ __launch_bounds__(SP_WG) void split_scatter_kernel(
    const uint64_t *__restrict__ c0, const uint64_t *__restrict__ c1, const uint64_t *__restrict__ c2, int kc,
    int64_t n, P pf, int64_t ntiles, const uint32_t *__restrict__ offsets, uint64_t *__restrict__ o0,
    uint64_t *__restrict__ o1, uint64_t *__restrict__ o2, const uint8_t *__restrict__ ids = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sp_smem[];
  uint64_t *s0 = (uint64_t *)sp_smem;
  uint64_t *s1 = s0 + SP_TILE;
  uint64_t *s2 = s1 + (NC >= 2 ? SP_TILE : 0);
  uint8_t *spart = (uint8_t *)(s2 + (NC >= 3 ? SP_TILE : 0));
  __shared__ uint32_t wcnt[SP_WAVES][256];
  __shared__ uint32_t dstart[256];
  __shared__ int64_t gbase[256];
  __shared__ uint32_t s_wsum[4];
  __shared__ u64x2 psm[P::SMEM_TUPLES > 0 && !READ_IDS ? P::SMEM_TUPLES : 1];
  const int w = wave_id(), lane = lane_id();
  const int64_t tbase = (int64_t)blockIdx.x * SP_TILE;
  const int64_t wrow = tbase + (int64_t)w * (SP_ITEMS * 64) + lane;
  uint64_t a[SP_ITEMS], b[NC >= 2 ? SP_ITEMS : 1], c[NC >= 3 ? SP_ITEMS : 1];
  uint32_t idv[READ_IDS ? SP_ITEMS : 1];
#pragma unroll
  for (int j = 0; j < SP_ITEMS; j++) {
    const int64_t i = min(wrow + j * 64, n - 1);
    a[j] = c0[i];
    if (NC >= 2) b[j] = c1[i];
    if (NC >= 3) c[j] = c2[i];
    if (READ_IDS) idv[READ_IDS ? j : 0] = ids[i];
  }
  uint32_t goff = threadIdx.x < pf.parts ? offsets[(int64_t)threadIdx.x * ntiles + blockIdx.x] : 0;
#pragma unroll
  for (int q = 0; q < 4; q++) wcnt[w][lane + 64 * q] = 0;
  if (P::SMEM_TUPLES > 0 && !READ_IDS) {
    pf.setup(psm);
    __syncthreads();
  }
  uint32_t rnk[SP_ITEMS], prt[SP_ITEMS];
#pragma unroll
  for (int j = 0; j < SP_ITEMS; j++) {
    const bool valid = wrow + j * 64 < n;
    const uint64_t key = kc == 0 ? a[j] : (kc == 1 ? b[NC >= 2 ? j : 0] : c[NC >= 3 ? j : 0]);
    const uint32_t d = READ_IDS ? idv[READ_IDS ? j : 0] : pf(psm, key, wrow + j * 64);
    prt[j] = d;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; bit++) {
      const bool on = (d >> bit) & 1;
      const uint64_t bm = __ballot(on);
      peers &= on ? bm : ~bm;
    }
    const uint32_t r = (uint32_t)mbcnt(peers);
    uint32_t old = 0;
    if (valid && r == 0) {
      old = wcnt[w][d];
      wcnt[w][d] = old + (uint32_t)__popcll(peers);
    }
    old = (uint32_t)__shfl((int)old, valid ? __builtin_ctzll(peers) : 0, 64);
    rnk[j] = old + r;
  }
  __syncthreads();
  if (threadIdx.x < 256) {
    uint32_t acc = 0;
#pragma unroll
    for (int q = 0; q < SP_WAVES; q++) {
      uint32_t cnt = wcnt[q][threadIdx.x];
      wcnt[q][threadIdx.x] = acc;
      acc += cnt;
    }
    uint32_t inc = wave_iscan_u32(acc);
    if (lane == 63) s_wsum[w] = inc;
    dstart[threadIdx.x] = inc - acc;
  }
  __syncthreads();
  if (threadIdx.x < 256) {
    uint32_t wb = 0;
    for (int q = 0; q < w; q++) wb += s_wsum[q];
    uint32_t ds = dstart[threadIdx.x] + wb;
    dstart[threadIdx.x] = ds;
    gbase[threadIdx.x] = (int64_t)goff - (int64_t)ds;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SP_ITEMS; j++) {
    if (wrow + j * 64 >= n) continue;
    const uint32_t d = prt[j];
    const uint32_t p = dstart[d] + wcnt[w][d] + rnk[j];
    s0[p] = a[j];
    if (NC >= 2) s1[p] = b[j];
    if (NC >= 3) s2[p] = c[j];
    spart[p] = (uint8_t)d;
  }
  __syncthreads();
  const uint32_t len = (uint32_t)min<int64_t>(SP_TILE, n - tbase);
#pragma unroll
  for (int j = 0; j < SP_ITEMS; j++) {
    const uint32_t p = j * SP_WG + threadIdx.x;
    if (p < len) {
      const int64_t g = gbase[spart[p]] + p;
      o0[g] = s0[p];
      if (NC >= 2) o1[g] = s1[p];
      if (NC >= 3) o2[g] = s2[p];
    }
  }
}

} // namespace sq
