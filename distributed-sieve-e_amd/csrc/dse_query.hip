// dse_query.hip -- rank and select on a device-resident prime mask (gfx950):
// pi(x), the n-th entry, the entry after or before x, and membership, answered
// from the mask and its rank index without the mask leaving the device.
//
// The index is the scanned tile sums of the extractor (launch_primes_scan,
// dse_primes.hip): index[t] = entries in the tiles before t, index[tiles] = the
// total. A query then needs one tile of the mask, 2 KiB.
//
// query_kernel: one wave per query, workgroups of 4 waves, grid-stride over the
// queries. Everything a wave decides depends on the query alone, so its
// control flow is uniform and the wave primitives of dse_block.h apply.
//   rank    the tile of x's candidate: lane l holds the tile's words 4l .. 4l+3
//           (32 contiguous bytes; clipped word loads only in the tile that
//           holds the range's last word), popcounts what lies below the
//           candidate, wave_sum, + index[t];
//   select  the tile t with index[t] <= k < index[t + 1] by a 64-way search
//           (every lane probes one pivot, a ballot narrows the interval to a
//           64th), then popcount per lane, wave_scan, a ballot for the owning
//           lane, select in its words;
//   next    select(rank(x)); prev: select(rank(x - 1) - 1).
// query_test_kernel: one lane per query, one word load, no index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_block.h"
#include "dse_internal.h"
#include "dse_query_word.h"

namespace dse {
namespace {

constexpr uint32_t kQThreads = 256;
constexpr uint32_t kQWaves = kQThreads / 64;
constexpr uint32_t kQLaneWords = kMaskTileWords / 64;  // words of a tile per lane
static_assert(kQLaneWords == 4, "a lane holds 32 contiguous bytes of the tile");

struct QArgs {
  MaskRange r;
  const unsigned long long* index;  // [tiles + 1]
  uint64_t tiles;
  const uint64_t* q;
  uint64_t nq;
  uint64_t* out;
};

// this lane's words of tile t: 4 * lane .. 4 * lane + 3
struct LaneWords {
  uint64_t v[kQLaneWords];
  __device__ __forceinline__ uint64_t operator()(uint32_t i) const { return v[i]; }
};

__device__ __forceinline__ LaneWords load_lane_words(const QArgs& a, uint64_t t, uint32_t lane) {
  const uint64_t w0 = t * kMaskTileWords + lane * kQLaneWords;
  LaneWords lw;
  if ((t + 1) * kMaskTileWords < a.r.words) {  // the range's last word is in a later tile: nothing to clip
#pragma unroll
    for (uint32_t i = 0; i < kQLaneWords; ++i) lw.v[i] = a.r.mask[w0 + i];
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kQLaneWords; ++i) lw.v[i] = mask_word(a.r, w0 + i);
  }
  return lw;
}

// entries among the first m positions of the range, m <= nbits; the same in every lane
__device__ __forceinline__ uint64_t rank_lead(const QArgs& a, uint64_t m, uint32_t lane) {
  if (m >= a.r.nbits) return a.index[a.tiles];
  const uint64_t t = m / kMaskTileBits;
  const uint32_t p = (uint32_t)(m % kMaskTileBits);
  const LaneWords lw = load_lane_words(a, t, lane);
  const uint32_t c = query_rank_words<kQLaneWords>(lw, lane * kQLaneWords, p);
  return a.index[t] + wave_sum(c);
}

// the value of the entry of rank k, kQueryNone if k >= the total; the same in every lane
__device__ __forceinline__ uint64_t select_rank(const QArgs& a, uint64_t k, uint32_t lane) {
  if (k >= a.index[a.tiles]) return kQueryNone;
  // index[lo] <= k < index[hi] throughout; index[0] = 0 and index[tiles] > k
  uint64_t lo = 0, hi = a.tiles;
  while (hi - lo > 1) {
    const uint64_t step = (hi - lo + 63) / 64;
    const uint64_t pivot = lo + lane * step;  // lane 0 probes lo itself: at least one lane holds
    const bool le = pivot < hi && a.index[pivot] <= k;
    // the index is monotone: the lanes that hold are 0 .. c - 1
    const uint32_t c = (uint32_t)__popcll(__ballot(le));
    const uint64_t nlo = lo + (uint64_t)(c - 1) * step;
    hi = min(hi, nlo + step);
    lo = nlo;
  }
  const uint32_t r = (uint32_t)(k - a.index[lo]);  // below the tile's entries
  const LaneWords lw = load_lane_words(a, lo, lane);
  const uint32_t c = query_pop_words<kQLaneWords>(lw);
  const uint32_t s = wave_scan(c);
  const unsigned long long owns = __ballot(s > r);
  if (!owns) return kQueryNone;  // an index that is not this mask's
  const uint32_t owner = (uint32_t)__builtin_ctzll(owns);
  uint32_t pos = 0;
  if (lane == owner) pos = lane * kQLaneWords * 64 + query_select_words<kQLaneWords>(lw, r - (s - c));
  pos = __shfl(pos, owner);
  return query_value(a.r.g_start, lo * kMaskTileBits + pos);
}

template <uint32_t kKind>
__global__ __launch_bounds__(kQThreads) void query_kernel(QArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * kQWaves + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * kQWaves;
  for (uint64_t i = wave; i < a.nq; i += nwaves) {
    const uint64_t x = a.q[i];
    uint64_t ans;
    if (kKind == kQueryRank) {
      ans = rank_lead(a, query_lead(x, a.r.g_start, a.r.nbits), lane);
    } else if (kKind == kQuerySelect) {
      ans = select_rank(a, x, lane);
    } else if (kKind == kQueryNext) {
      ans = select_rank(a, rank_lead(a, query_lead(x, a.r.g_start, a.r.nbits), lane), lane);
    } else {  // kQueryPrev: the last entry among the values <= x - 1
      const uint64_t below = x ? rank_lead(a, query_lead(x - 1, a.r.g_start, a.r.nbits), lane) : 0ull;
      ans = below ? select_rank(a, below - 1, lane) : kQueryNone;
    }
    if (lane == 0) a.out[i] = ans;
  }
}

__global__ __launch_bounds__(kQThreads) void query_test_kernel(QArgs a) {
  const uint64_t n = (uint64_t)gridDim.x * kQThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kQThreads + threadIdx.x; i < a.nq; i += n) a.out[i] = query_test(a.r, a.q[i]);
}

}  // namespace

uint64_t query_index_words(uint64_t nbits) { return mask_tiles(nbits) + 1; }

uint32_t query_grid(uint32_t kind, uint64_t nq, int num_cus, uint32_t grid_cap) {
  const uint64_t per = kind == kQueryTest ? kQThreads : kQWaves;  // queries a workgroup takes at a time
  const uint64_t want = (nq + per - 1) / per;
  const uint64_t cap = grid_cap ? grid_cap : (uint64_t)kQueryGridPerCu * (uint64_t)(num_cus > 0 ? num_cus : 1);
  return (uint32_t)(want < cap ? want : cap);
}

hipError_t launch_query(uint32_t kind, uint64_t g_start, uint64_t nbits, const uint64_t* mask, const void* index,
                        const uint64_t* q, uint64_t nq, uint64_t* out, uint32_t grid, hipStream_t stream) {
  if (kind >= kQueryKinds) return hipErrorInvalidValue;
  if (!nq || !grid) return hipSuccess;
  const QArgs a{mask_range(mask, g_start, nbits), reinterpret_cast<const unsigned long long*>(index), mask_tiles(nbits), q,
                nq, out};
  const dim3 g(grid), b(kQThreads);
  switch (kind) {
    case kQueryRank: hipLaunchKernelGGL(query_kernel<kQueryRank>, g, b, 0, stream, a); break;
    case kQuerySelect: hipLaunchKernelGGL(query_kernel<kQuerySelect>, g, b, 0, stream, a); break;
    case kQueryNext: hipLaunchKernelGGL(query_kernel<kQueryNext>, g, b, 0, stream, a); break;
    case kQueryPrev: hipLaunchKernelGGL(query_kernel<kQueryPrev>, g, b, 0, stream, a); break;
    default: hipLaunchKernelGGL(query_test_kernel, g, b, 0, stream, a); break;
  }
  return hipGetLastError();
}

}  // namespace dse
