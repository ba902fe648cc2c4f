// dse_finish.hip -- finish (sieve.clj:82-108) on the device (gfx950).
//
// The reference turns a sieved chunk into primes{k}.txt with one thread; so
// does the host writer (dse_write_range_file). Here a device-resident prime
// mask becomes the file's text in HBM, so only text leaves the GPU. Three
// launches on the caller's stream, the ordered count / scan / write shape of
// the base-prime compaction (dse_base.hip):
//   finish_size_kernel  per tile of kMaskTileWords mask words: entries and the
//                       bytes of their printed values ("value bytes");
//   finish_scan_kernel  one workgroup: 64-bit exclusive scan of the tile pairs
//                       in place, and the call's totals;
//   finish_emit_kernel  per tile: its entries formatted into an LDS window and
//                       the window stored to global memory as dwords.
// The separators of an entry follow from its rank alone (fin_sep_bytes), so
// the one scan gives every tile its first rank R_t and its first byte
//   T_t = V_t + sep(R_t) - sep(first_rank),  V_t = value bytes before the tile.
// No workgroup waits on another: the launches are the only ordering.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_block.h"
#include "dse_finish_fmt.h"
#include "dse_internal.h"

namespace dse {
namespace {

constexpr uint32_t kFinThreads = kMaskTileWords;  // one mask word per thread
constexpr uint32_t kFinWaves = kFinThreads / 64;
// LDS window of a tile's text. A tile of a prime mask near 1e9 prints about
// 19 KB; an all-ones tile of 19-digit values prints 344 KB and takes 11 windows.
constexpr uint32_t kFinWindow = 32768;

struct FinArgs {
  MaskRange r;
  uint64_t first_rank;
  uint32_t flags;
};

// Word w of the range as the entries it prints: with the hack, bits 0..3 of
// word 0 are the four literal entries whatever the mask holds.
__device__ __forceinline__ uint64_t fin_load_word(const FinArgs& a, uint64_t w) {
  const uint64_t b = mask_word(a.r, w);
  return w == 0 && (a.flags & kFinishHack) ? b | 0xFull : b;
}

// value printed for bit b of word w
__device__ __forceinline__ uint64_t fin_value(const FinArgs& a, uint64_t w, uint32_t b) {
  if (w == 0 && b < 4 && (a.flags & kFinishHack)) return b == 0 ? 2ull : 2ull * b + 1ull;  // 2 3 5 7
  return 3ull + 2ull * (a.r.g_start + w * 64ull + b);
}

// entries and value bytes of one word, packed (entries << 32 | bytes): the
// length of a printed value is a step function of the value, so a word whose
// first and last candidates print equally long costs popcount * length; only
// a word that straddles a power of ten (or holds the literals) walks its bits.
__device__ __forceinline__ uint64_t fin_word_cost(const FinArgs& a, uint64_t w, uint64_t bits) {
  if (!bits) return 0ull;
  const bool dbl = a.flags & kFinishDoubles;
  const uint32_t c = __popcll(bits);
  const uint32_t l0 = fin_value_len(fin_value(a, w, 0), dbl), l1 = fin_value_len(fin_value(a, w, 63), dbl);
  uint32_t d;
  if (l0 == l1 && !(w == 0 && (a.flags & kFinishHack))) {
    d = c * l0;
  } else {
    d = 0;
    for (uint64_t x = bits; x; x &= x - 1) d += fin_value_len(fin_value(a, w, __ffsll((long long)x) - 1), dbl);
  }
  return ((uint64_t)c << 32) | d;
}

__global__ __launch_bounds__(kFinThreads) void finish_size_kernel(FinArgs a, unsigned long long* __restrict__ sums) {
  __shared__ uint64_t s_wave[kFinWaves];
  const uint64_t w = (uint64_t)blockIdx.x * kMaskTileWords + threadIdx.x;
  const uint64_t t = block_sum<kFinThreads>(fin_word_cost(a, w, fin_load_word(a, w)), s_wave);
  if (threadIdx.x == 0) {
    sums[2ull * blockIdx.x] = t >> 32;
    sums[2ull * blockIdx.x + 1] = t & 0xFFFFFFFFull;
  }
}

// exclusive scan of the (entries, value bytes) pairs in place; totals[0] =
// entries, totals[1] = text bytes of the slice, the closing "\n" of a partial
// last line included
__global__ __launch_bounds__(kSliceThreads) void finish_scan_kernel(unsigned long long* __restrict__ sums, uint32_t ntiles,
                                                           uint64_t first_rank, uint32_t flags,
                                                           unsigned long long* __restrict__ totals) {
  __shared__ uint64_t s_wave[2][kSliceThreads / 64];
  const ScanSlice<uint64_t> c = slice_scan(ntiles, s_wave[0], [&](uint32_t b) { return sums[2ull * b]; });
  const ScanSlice<uint64_t> d = slice_scan(ntiles, s_wave[1], [&](uint32_t b) { return sums[2ull * b + 1]; });
  uint64_t rc = c.start, rd = d.start;
  for (uint32_t b = c.b0; b < c.b1; ++b) {
    const uint64_t vc = sums[2ull * b], vd = sums[2ull * b + 1];
    sums[2ull * b] = rc;
    sums[2ull * b + 1] = rd;
    rc += vc;
    rd += vd;
  }
  if (threadIdx.x == 0) {
    const uint64_t C = c.total, D = d.total, end = first_rank + C;
    const uint64_t closing = ((flags & kFinishLast) && end % 10u) ? 1u : 0u;
    totals[0] = C;
    totals[1] = D + fin_sep_bytes(end) - fin_sep_bytes(first_rank) + closing;
  }
}

// LDS sink of one window: byte p of the tile's (dword-aligned) frame lands in
// the window when it lies in [w0, w0 + kFinWindow)
struct FinSink {
  char* s;
  uint32_t w0;
  __device__ __forceinline__ void operator()(uint32_t p, char ch) const {
    const uint32_t o = p - w0;
    if (o < kFinWindow) s[o] = ch;
  }
};

__global__ __launch_bounds__(kFinThreads) void finish_emit_kernel(FinArgs a,
                                                                  const unsigned long long* __restrict__ sums,
                                                                  const unsigned long long* __restrict__ totals,
                                                                  char* __restrict__ text, uint64_t text_cap) {
  __shared__ uint64_t s_wave[kFinWaves];
  __shared__ __attribute__((aligned(16))) char s_text[kFinWindow];
  const uint64_t total_bytes = totals[1];
  if (total_bytes > text_cap) return;  // the text does not fit: not one byte is written
  const uint32_t tid = threadIdx.x;
  const bool dbl = a.flags & kFinishDoubles;
  if (blockIdx.x == 0 && tid == 0 && (a.flags & kFinishLast) && (a.first_rank + totals[0]) % 10u)
    text[total_bytes - 1] = '\n';  // closes the file's partial last line
  if (a.r.words == 0) return;

  const uint64_t w = (uint64_t)blockIdx.x * kMaskTileWords + tid;
  uint64_t bits = fin_load_word(a, w);
  const uint64_t cost = fin_word_cost(a, w, bits);
  uint64_t tile;
  const uint64_t excl = block_scan<kFinThreads>(cost, s_wave, &tile) - cost;

  // the tile's first rank and first byte, and this word's
  const uint64_t R_t = a.first_rank + sums[2ull * blockIdx.x];
  const uint64_t sep_t = fin_sep_bytes(R_t);
  const uint64_t T_t = sums[2ull * blockIdx.x + 1] + sep_t - fin_sep_bytes(a.first_rank);
  const uint32_t tile_bytes = (uint32_t)((tile & 0xFFFFFFFFull) + fin_sep_bytes(R_t + (tile >> 32)) - sep_t);
  if (tile_bytes == 0) return;
  const uint64_t R_w = R_t + (excl >> 32);
  uint32_t r10 = (uint32_t)(R_w % 10u);
  // frame: byte x of the frame is address (tile start rounded down to a dword) + x,
  // so frame dwords are global dwords and the tile's text is [head, head + tile_bytes)
  char* const dst = text + T_t;
  const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
  char* const frame = dst - head;
  const uint32_t end = head + tile_bytes;
  uint32_t x = head + (uint32_t)((excl & 0xFFFFFFFFull) + fin_sep_bytes(R_w) - sep_t);

  for (uint32_t w0 = 0; w0 < end; w0 += kFinWindow) {
    const uint32_t w1 = w0 + kFinWindow;
    const FinSink sink{s_text, w0};
    // this word's entries that reach into the window; one that runs past its
    // end is printed again (its rest) in the next window
    while (bits && x < w1) {
      const uint32_t b = __ffsll((long long)bits) - 1;
      const uint32_t n = fin_format_entry(fin_value(a, w, b), dbl, r10, x, sink);
      if (x + n > w1) break;
      x += n;
      bits &= bits - 1;
      r10 = r10 == 9u ? 0u : r10 + 1u;
    }
    __syncthreads();
    // the window as coalesced dword stores; the dwords the tile shares with its
    // neighbours (unaligned head and tail) byte by byte, inside the tile only
    const uint32_t lim = min(w1, end);
    for (uint32_t p = w0 + 4u * tid; p < lim; p += 4u * kFinThreads) {
      if (p >= head && p + 4u <= end) {
        *reinterpret_cast<uint32_t*>(frame + p) = *reinterpret_cast<const uint32_t*>(s_text + (p - w0));
      } else {
        for (uint32_t j = 0; j < 4u; ++j)
          if (p + j >= head && p + j < end) frame[p + j] = s_text[p + j - w0];
      }
    }
    __syncthreads();
  }
}

}  // namespace

uint64_t finish_scratch_bytes(uint64_t nbits) {
  const uint64_t ntiles = mask_tiles(nbits);
  return (ntiles ? ntiles : 1) * 2 * sizeof(unsigned long long);
}

hipError_t launch_finish_text(uint32_t flags, uint64_t g_start, uint64_t nbits, const uint64_t* mask,
                              uint64_t first_rank, void* text, uint64_t text_cap, unsigned long long* totals,
                              void* tile_sums, hipStream_t stream) {
  const FinArgs a{mask_range(mask, g_start, nbits), first_rank, flags};
  if (mask_tiles(nbits) > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const uint32_t ntiles = (uint32_t)mask_tiles(nbits);
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(tile_sums);
  if (ntiles) hipLaunchKernelGGL(finish_size_kernel, dim3(ntiles), dim3(kFinThreads), 0, stream, a, sums);
  hipLaunchKernelGGL(finish_scan_kernel, dim3(1), dim3(kSliceThreads), 0, stream, sums, ntiles, first_rank, flags, totals);
  // an empty range still closes a partial line (block 0)
  hipLaunchKernelGGL(finish_emit_kernel, dim3(ntiles ? ntiles : 1), dim3(kFinThreads), 0, stream, a, sums, totals,
                     reinterpret_cast<char*>(text), text_cap);
  return hipGetLastError();
}

}  // namespace dse
