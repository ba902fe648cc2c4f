// dse_sums.hip -- power and reciprocal sums over the matches of a pattern in a
// device-resident prime mask (gfx950): the matches, the first and the last of
// them, the sum of their values and of the squares, and the fixed-point sum
// of floor(2^126 / member) over their required members, as one dse_sums
// (include/dse.h) in device memory. Every sum is an exact integer
// (dse_sums_word.h), so the grid cannot change a bit of the result.
//
// Two launches of the slab reduction (dse_slab.h) on the caller's stream; the
// launches are the only ordering and no workgroup waits on another:
//   sums_main_kernel<flags>  every workgroup walks its own contiguous run of
//                      tiles, one word of the visible candidates per thread and
//                      the low half of the word after it, both loaded a tile
//                      ahead, and makes the match word with dse_tuples_word.h.
//                      POWER: the word's matches, positions and squared positions
//                      from popcounts under fixed combs into register limbs with
//                      explicit carries; nothing per match.
//                      RECIP: the tile's matches are compacted into an LDS list
//                      (a workgroup scan of the popcounts; the list holds the
//                      all-ones tile), and the lanes take the list's (match,
//                      member) pairs in turn, one exact division each, into three
//                      register limbs.
//                      A kernel per flags value: a call pays for what it asks.
//                      The registers are reduced once, at the end of the run
//                      (slab_add_limbs), and the slab is written with plain
//                      stores: matches, first and last match, the limbs.
//   sums_close_kernel  one workgroup, a slab per thread: adds the limbs over the
//                      slabs, turns the position sums into sum1 and sum2 with the
//                      range's base value (sums_power_close) and writes the
//                      dse_sums.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_internal.h"
#include "dse_slab.h"
#include "dse_sums_word.h"

namespace dse {
namespace {

constexpr uint32_t kSmThreads = kMaskTileWords;  // one mask word per thread
constexpr uint32_t kSmWaves = kSmThreads / 64;
constexpr uint32_t kSmPerCu = 4;  // the RECIP kernels' list admits 4 workgroups per compute unit

// a workgroup's slab, in uint64 words
constexpr uint32_t kSlMatches = 0, kSlFirst = 1, kSlLast1 = 2, kSlP1 = 3, kSlP2 = 5, kSlRecip = 8, kSlabWords = 11;
// the half-limb sums in LDS: matches, p1, p2, recip
constexpr uint32_t kHfMatches = 0, kHfP1 = 2, kHfP2 = 6, kHfRecip = 12, kHalves = 18;
constexpr uint32_t kClThreads = kSlabCloseThreads;
static_assert(kSumsMaxGrid <= kClThreads, "the closing kernel takes one slab per thread");
static_assert(kMaskTileBits + kTuplesMaxAbove <= 65536, "a list entry is a tile position in 16 bits");

// dse_sums as uint64 words
constexpr uint32_t kOutGStart = 0, kOutNbits = 1, kOutRequire = 2, kOutForbid = 3, kOutAbove = 4, kOutFlags = 5,
                   kOutMatches = 6, kOutFirst = 7, kOutLast = 8, kOutSum1 = 9, kOutSum2 = 11, kOutRecip = 14;
static_assert(kOutRecip + 3 == kSumsWords, "dse_sums is kSumsWords words");

struct SmArgs {
  TupleSrc s;
  SlabRun run;
  uint32_t flags;
};

template <uint32_t kFlags>
__global__ __launch_bounds__(kSmThreads) void sums_main_kernel(SmArgs a, unsigned long long* __restrict__ slabs) {
  constexpr bool kPower = (kFlags & kSumsPower) != 0, kRecip = (kFlags & kSumsRecip) != 0;
  __shared__ uint16_t s_list[kRecip ? kMaskTileBits : 1];  // tile positions of the tile's matches, in order
  __shared__ uint8_t s_member[32];                         // the set bits of require, in order
  __shared__ uint32_t s_wave[2][kSmWaves];
  __shared__ unsigned long long s_half[kHalves];
  __shared__ unsigned long long s_first, s_last1;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;

  if (tid < kHalves) s_half[tid] = 0ull;
  if (tid == 0) {
    s_first = kSumsNone;
    s_last1 = 0ull;
  }
  const uint32_t members = stats_pop64(a.s.require);
  if (kRecip && tid == 0) {
    uint32_t k = 0;
    for (uint32_t r = a.s.require; r; r &= r - 1) s_member[k++] = (uint8_t)__builtin_ctz(r);
  }
  __syncthreads();

  SumsPower pw = {0ull, {0ull, 0ull}, {0ull, 0ull, 0ull}};
  uint64_t rc[3] = {0ull, 0ull, 0ull};
  uint64_t first = kSumsNone, last1 = 0;  // this thread's lowest match and its highest + 1, as positions
  const uint64_t B = 3ull + 2ull * a.s.r.g_start;

  uint64_t t0, t1;
  slab_tiles(a.run, t0, t1);
  // this thread's word of tile t of the visible candidates and the low half of the word after it
  auto load = [&](uint64_t t, uint64_t& x, uint32_t& nx) {
    const uint64_t wi = t * kMaskTileWords + tid;
    x = tuples_visible_word(a.s, wi);
    nx = (uint32_t)tuples_visible_word(a.s, wi + 1);
  };
  uint64_t x = 0, xn;
  uint32_t nx = 0, nxn;
  if (t0 < t1) load(t0, x, nx);
  for (uint64_t t = t0; t < t1; ++t) {
    load(t + 1, xn, nxn);  // a tile ahead; past the range these are zeros, and nothing is read
    const uint64_t wi = t * kMaskTileWords + tid;
    const uint64_t pos0 = wi * 64ull;
    const uint64_t m = tuples_word(a.s, wi, x, nx);
    if (m) {
      first = min(first, pos0 + stats_ctz64(m));
      last1 = pos0 + stats_msb64(m) + 1ull;  // a thread's words come in increasing order
    }
    if (kPower)
      sums_word_power(m, pos0, pw);
    else
      pw.n += stats_pop64(m);

    if (kRecip) {
      // the tile's matches into the list by rank; two sets of wave sums by tile parity, as the
      // list's own barriers order everything else
      const uint32_t c = stats_pop64(m);
      uint32_t total;
      uint32_t k = block_scan<kSmThreads>(c, s_wave[(uint32_t)(t - t0) & 1u], &total) - c;
      for (uint64_t it = m; it; it &= it - 1) s_list[k++] = (uint16_t)(tid * 64u + stats_ctz64(it));
      __syncthreads();
      // pair idx = member jm of match i, idx = jm total + i: one division per lane and step
      const uint64_t vt = B + 2ull * (t * (uint64_t)kMaskTileBits);
      const uint32_t work = total * members;
      uint32_t i = tid, jm = 0;
      for (uint32_t idx = tid; idx < work; idx += kSmThreads) {
        while (i >= total) {  // idx < work: ends with jm < members
          i -= total;
          ++jm;
        }
        uint64_t q[2];
        sums_recip(vt + 2ull * ((uint32_t)s_list[i] + (uint32_t)s_member[jm]), q);
        limbs_add(rc, q);
        i += kSmThreads;
      }
      __syncthreads();  // the list is free for the next tile
    }
    x = xn;
    nx = nxn;
  }

  // the registers, once per run
  {
    const uint64_t n1[1] = {pw.n};
    slab_add_limbs(n1, s_half + kHfMatches);
    if (kPower) {
      slab_add_limbs(pw.p1, s_half + kHfP1);
      slab_add_limbs(pw.p2, s_half + kHfP2);
    }
    if (kRecip) slab_add_limbs(rc, s_half + kHfRecip);
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) {
      first = min(first, (uint64_t)__shfl_xor((unsigned long long)first, o));
      last1 = max(last1, (uint64_t)__shfl_xor((unsigned long long)last1, o));
    }
    if (lane == 0 && first != kSumsNone) atomicMin(&s_first, (unsigned long long)first);
    if (lane == 0 && last1) atomicMax(&s_last1, (unsigned long long)last1);
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long* const sl = slabs + (uint64_t)blockIdx.x * kSlabWords;
    uint64_t n[1], p1[2], p2[3], r3[3];
    slab_fold_limbs(s_half + kHfMatches, n);
    slab_fold_limbs(s_half + kHfP1, p1);
    slab_fold_limbs(s_half + kHfP2, p2);
    slab_fold_limbs(s_half + kHfRecip, r3);
    sl[kSlMatches] = n[0];
    sl[kSlFirst] = s_first;
    sl[kSlLast1] = s_last1;
    sl[kSlP1] = p1[0];
    sl[kSlP1 + 1] = p1[1];
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
      sl[kSlP2 + k] = p2[k];
      sl[kSlRecip + k] = r3[k];
    }
  }
}

__global__ __launch_bounds__(kClThreads) void sums_close_kernel(SmArgs a, const unsigned long long* __restrict__ slabs,
                                                                uint32_t nslabs,
                                                                unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_half[kHalves];
  __shared__ unsigned long long s_first, s_last1;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  if (tid < kHalves) s_half[tid] = 0ull;
  if (tid == 0) {
    s_first = kSumsNone;
    s_last1 = 0ull;
  }
  __syncthreads();

  const bool have = tid < nslabs;
  const unsigned long long* const my = slabs + (uint64_t)(have ? tid : 0u) * kSlabWords;
  uint64_t n[1] = {0ull}, p1[2] = {0ull, 0ull}, p2[3] = {0ull, 0ull, 0ull}, r3[3] = {0ull, 0ull, 0ull};
  uint64_t first = kSumsNone, last1 = 0;
  if (have) {
    n[0] = my[kSlMatches];
    first = my[kSlFirst];
    last1 = my[kSlLast1];
    p1[0] = my[kSlP1];
    p1[1] = my[kSlP1 + 1];
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
      p2[k] = my[kSlP2 + k];
      r3[k] = my[kSlRecip + k];
    }
  }
  slab_add_limbs(n, s_half + kHfMatches);
  slab_add_limbs(p1, s_half + kHfP1);
  slab_add_limbs(p2, s_half + kHfP2);
  slab_add_limbs(r3, s_half + kHfRecip);
#pragma unroll
  for (uint32_t o = 32; o > 0; o >>= 1) {
    first = min(first, (uint64_t)__shfl_xor((unsigned long long)first, o));
    last1 = max(last1, (uint64_t)__shfl_xor((unsigned long long)last1, o));
  }
  if (lane == 0 && first != kSumsNone) atomicMin(&s_first, (unsigned long long)first);
  if (lane == 0 && last1) atomicMax(&s_last1, (unsigned long long)last1);
  __syncthreads();

  if (tid == 0) {
    SumsPower pw;
    uint64_t nn[1], rr[3], sum1[2] = {0ull, 0ull}, sum2[3] = {0ull, 0ull, 0ull};
    slab_fold_limbs(s_half + kHfMatches, nn);
    slab_fold_limbs(s_half + kHfP1, pw.p1);
    slab_fold_limbs(s_half + kHfP2, pw.p2);
    slab_fold_limbs(s_half + kHfRecip, rr);
    pw.n = nn[0];
    if (a.flags & kSumsPower) sums_power_close(pw, 3ull + 2ull * a.s.r.g_start, sum1, sum2);
    out[kOutGStart] = a.s.r.g_start;
    out[kOutNbits] = a.s.r.nbits;
    out[kOutRequire] = a.s.require;
    out[kOutForbid] = a.s.forbid;
    out[kOutAbove] = a.s.above_bits;
    out[kOutFlags] = a.flags;
    out[kOutMatches] = nn[0];
    out[kOutFirst] = s_first == kSumsNone ? kSumsNone : a.s.r.g_start + s_first;
    out[kOutLast] = s_last1 ? a.s.r.g_start + (s_last1 - 1) : kSumsNone;
    out[kOutSum1] = sum1[0];
    out[kOutSum1 + 1] = sum1[1];
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
      out[kOutSum2 + k] = sum2[k];
      out[kOutRecip + k] = rr[k];
    }
  }
}

}  // namespace

uint32_t sums_grid(uint64_t nbits, int num_cus, uint32_t grid_cap) {
  return slab_grid(nbits, kSmPerCu, num_cus, grid_cap, kSumsMaxGrid);
}

uint64_t sums_scratch_bytes(uint32_t grid) { return slab_bytes(grid, kSlabWords); }

hipError_t launch_sums(uint64_t g_start, uint64_t nbits, const uint64_t* mask, const TuplePattern& p, uint32_t flags,
                       uint64_t* out, void* slabs, uint32_t grid, hipStream_t stream) {
  if (grid > kSumsMaxGrid || (flags & ~(kSumsPower | kSumsRecip))) return hipErrorInvalidValue;
  if (!(p.require & 1u) || (p.require & p.forbid) || p.above_bits > kTuplesMaxAbove || p.above_shift > 63 ||
      (p.above_bits && !p.above))
    return hipErrorInvalidValue;
  SmArgs a;
  a.s = TupleSrc{mask_range(mask, g_start, nbits), p.above, p.above_shift, p.above_bits, p.require, p.forbid};
  a.flags = flags;
  if (!slab_run(nbits, grid, &a.run)) return hipErrorInvalidValue;
  void (*const main_kernel[4])(SmArgs, unsigned long long*) = {sums_main_kernel<0>, sums_main_kernel<1>,
                                                               sums_main_kernel<2>, sums_main_kernel<3>};
  return slab_launch(main_kernel[flags], sums_close_kernel, a, grid, kSmThreads, kSlabCloseBins, slabs, out, stream);
}

}  // namespace dse
