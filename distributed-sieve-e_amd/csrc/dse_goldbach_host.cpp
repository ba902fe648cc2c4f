// dse_goldbach_host.cpp -- minimal Goldbach partitions of a mask, the host side
// (include/dse.h): a device-resident mask and the candidates below it become one
// dse_goldbach on the device (dse_goldbach.hip), in the caller's device memory
// (dse_goldbach_dev_async) or on the host (dse_goldbach_range,
// dse_goldbach_resident); dse_goldbach_merge joins the results of adjacent ranges
// by host arithmetic, and dse_debug_goldbach_host runs the kernel's per-word
// bodies (dse_goldbach_word.h) on the host.
#include <algorithm>
#include <cstring>

#include "dse_goldbach_word.h"
#include "dse_host.h"

using namespace dse;

static_assert(sizeof(dse_goldbach) == 8 * DSE_GOLDBACH_WORDS, "dse_goldbach has no padding");
static_assert(DSE_GOLDBACH_WORDS == kGbWords && DSE_GOLDBACH_PRIMES == kGbPrimes && DSE_GOLDBACH_NONE == kGbNone,
              "the kernels write the struct of include/dse.h");

namespace {

// nprimes of a call -> the ranks it uses (0: all); DSE_EINVAL above DSE_GOLDBACH_PRIMES
int32_t gb_nprimes(uint32_t nprimes, uint32_t* n) {
  if (nprimes > DSE_GOLDBACH_PRIMES) return fail(DSE_EINVAL, "nprimes above 2048");
  *n = nprimes ? nprimes : DSE_GOLDBACH_PRIMES;
  return DSE_OK;
}

int32_t gb_check_below(const uint64_t* below, uint32_t below_shift, uint64_t below_bits, uint64_t g_start) {
  if (below_shift > 63) return fail(DSE_EINVAL, "below_shift above 63");
  if (below_bits > g_start) return fail(DSE_EINVAL, "below_bits reaches below candidate 0");
  if (below_bits && !below) return fail(DSE_EINVAL, "null below with below_bits > 0");
  if (reinterpret_cast<uintptr_t>(below) & 7u) return fail(DSE_EINVAL, "below is not 8-byte aligned");
  return DSE_OK;
}

// whole words of a `below` of `bits` candidates that starts `shift` bits into its first word
inline uint64_t below_words(uint32_t shift, uint64_t bits) { return (shift + bits + 63) / 64; }

void gb_empty(dse_goldbach* r, uint64_t g_start, uint64_t nbits, uint32_t n) {
  std::memset(r, 0, sizeof *r);
  r->g_start = g_start;
  r->nbits = nbits;
  r->nprimes = n;
  r->first_unresolved = r->max_rank = r->max_c = DSE_GOLDBACH_NONE;
}

}  // namespace

extern "C" uint64_t dse_goldbach_prime(uint32_t i) { return i < kGbPrimes ? 3ull + 2ull * kGbTable.h(i) : 0ull; }

extern "C" uint64_t dse_goldbach_reach(uint32_t nprimes) {
  if (nprimes > kGbPrimes) return 0;
  return kGbTable.h((nprimes ? nprimes : kGbPrimes) - 1);
}

extern "C" int32_t dse_goldbach_dev_async(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev,
                                          const uint64_t* below_dev, uint32_t below_shift, uint64_t below_bits,
                                          uint32_t nprimes, dse_goldbach* out_dev, void* stream) {
  int32_t rc;
  if ((rc = check_dev_args(ctx, nbits, mask_dev, out_dev, "out", true))) return rc;
  uint32_t n;
  if ((rc = gb_nprimes(nprimes, &n))) return rc;
  if ((rc = gb_check_below(below_dev, below_shift, below_bits, g_start))) return rc;
  if ((rc = check_mask_range("goldbach", g_start, nbits))) return rc;
  return unit_dev_async<kUnitGoldbach>(ctx, nbits, stream, [&](void* slabs, uint32_t grid, hipStream_t s) {
    return launch_goldbach(g_start, nbits, mask_dev, 0, below_dev, below_shift, below_bits, n,
                           reinterpret_cast<uint64_t*>(out_dev), slabs, grid, s);
  });
}

extern "C" int32_t dse_goldbach_range(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, uint32_t nprimes,
                                      dse_goldbach* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc;
  uint32_t n;
  if ((rc = gb_nprimes(nprimes, &n))) return rc;
  if ((rc = check_mask_range("goldbach", g_start, nbits))) return rc;
  // the extended range: what the small primes can reach below g_start is sieved with it
  const uint64_t reach = kGbTable.h(n - 1);
  const uint64_t ext = nbits ? std::min(g_start, reach) : 0;
  if ((rc = check_mask_range("goldbach", g_start - ext, nbits + ext))) return rc;
  // one scratch mask: `below` is its first ext bits, the range's own mask starts ext bits in
  return unit_range<kUnitGoldbach>(
      ctx, g_start - ext, nbits + ext, nbits,
      [&](const uint64_t* m, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) {
        return launch_goldbach(g_start, nbits, m + (ext >> 6), (uint32_t)(ext & 63), m, 0, ext, n, res, slabs, grid, s);
      },
      out);
}

extern "C" int32_t dse_goldbach_resident(dse_ctx* ctx, int32_t my_num, uint32_t nprimes, dse_goldbach* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc;
  uint32_t n;
  if ((rc = gb_nprimes(nprimes, &n))) return rc;
  int32_t k0, k1;
  if ((rc = resident_span(ctx, my_num, "goldbach", &k0, &k1))) return rc;
  const ResidentSet& r = ctx->resident;
  const uint64_t cs = (uint64_t)r.cs;
  // chunk k > 1 sees the last `reach` candidates of chunk k - 1
  const uint64_t reach = kGbTable.h(n - 1);
  if (k1 > 1 && cs < reach)
    return fail(DSE_EINVAL, "chunks of " + std::to_string(cs) + " candidates are shorter than the reach " +
                                std::to_string(reach) + " of " + std::to_string(n) + " primes: lower nprimes");
  const uint64_t off = cs - (k1 > 1 ? reach : 0);                          // the tail's first bit in a chunk's mask
  const uint32_t tail_shift = (uint32_t)(off & 63);
  const uint64_t tail_words = k1 > 1 ? below_words(tail_shift, reach) : 0;  // through the mask's last word
  const size_t nd = ctx->devs.size();
  return unit_resident<kUnitGoldbach>(
      ctx, k0, k1, nd > 1 ? tail_words : 0,  // behind the results: a neighbour's tail per chunk
      [&](DevState& d, int32_t k, uint64_t* copy, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) {
        const uint64_t* below = nullptr;
        uint64_t below_bits = 0;
        hipError_t e = hipSuccess;
        if (k > 1 && reach) {
          const DevState& sd = ctx->devs[(size_t)(k - 2) % nd];
          const uint64_t* const tail = r.masks[k - 2].as<uint64_t>() + (off >> 6);
          below_bits = reach;
          if (&sd == &d) {
            below = tail;  // the neighbour's mask is this device's: a pointer into it
          } else {
            // the neighbour's whole words into this device's scratch, on this device's stream: the
            // launch behind it is ordered by the stream, the scratch's next user by its event
            e = sd.device == d.device ? hipMemcpyAsync(copy, tail, tail_words * 8, hipMemcpyDeviceToDevice, s)
                                      : hipMemcpyPeerAsync(copy, d.device, tail, sd.device, tail_words * 8, s);
            below = copy;
          }
        }
        if (e == hipSuccess)
          e = launch_goldbach((uint64_t)(k - 1) * cs, cs, r.masks[k - 1].as<uint64_t>(), 0, below, tail_shift, below_bits,
                              n, res, slabs, grid, s);
        return e;
      },
      dse_goldbach_merge, out);
}

extern "C" int32_t dse_goldbach_merge(const dse_goldbach* a, const dse_goldbach* b, dse_goldbach* out) {
  if (!a || !b || !out) return fail(DSE_EINVAL, "null goldbach result");
  if (int32_t rc = check_merge_adjacent(a->g_start, a->nbits, b->g_start)) return rc;
  if (a->nprimes != b->nprimes || a->nprimes < 1 || a->nprimes > DSE_GOLDBACH_PRIMES)
    return fail(DSE_EINVAL, "the results are of different nprimes");
  if (int32_t rc = check_merge_end(b->g_start, b->nbits)) return rc;
  dse_goldbach r;  // out may alias a or b
  r.g_start = a->g_start;
  r.nbits = a->nbits + b->nbits;
  r.nprimes = a->nprimes;
  r.resolved = a->resolved + b->resolved;
  r.unresolved = a->unresolved + b->unresolved;
  r.first_unresolved = a->first_unresolved != DSE_GOLDBACH_NONE ? a->first_unresolved : b->first_unresolved;
  const bool take_b =
      b->max_rank != DSE_GOLDBACH_NONE && (a->max_rank == DSE_GOLDBACH_NONE || b->max_rank > a->max_rank);
  r.max_rank = take_b ? b->max_rank : a->max_rank;
  r.max_c = take_b ? b->max_c : a->max_c;
  for (uint32_t i = 0; i < DSE_GOLDBACH_PRIMES; ++i) r.hist[i] = a->hist[i] + b->hist[i];
  *out = r;
  return DSE_OK;
}

extern "C" int32_t dse_debug_goldbach_host(const uint64_t* mask, uint64_t g_start, uint64_t nbits, const uint64_t* below,
                                           uint32_t below_shift, uint64_t below_bits, uint32_t nprimes,
                                           dse_goldbach* out) {
  if (!out) return fail(DSE_EINVAL, "null out");
  if (nbits && !mask) return fail(DSE_EINVAL, "null mask");
  int32_t rc;
  uint32_t n;
  if ((rc = gb_nprimes(nprimes, &n))) return rc;
  if ((rc = gb_check_below(below, below_shift, below_bits, g_start))) return rc;
  if ((rc = check_mask_range("goldbach", g_start, nbits))) return rc;
  const GbSrc src{mask, below, nbits, below_bits, 0u, below_shift};
  dse_goldbach r;
  gb_empty(&r, g_start, nbits, n);
  // the main kernel's tile loop, one tile's line at a time
  std::vector<uint64_t> line(kGbLineWords + 1);
  const uint32_t* const l32 = reinterpret_cast<const uint32_t*>(line.data());
  auto ld = [&](uint32_t k) { return l32[k]; };
  uint64_t br = kGbNone, bc = kGbNone;
  for (uint64_t t = 0; t < mask_tiles(nbits); ++t) {
    for (uint32_t k = 0; k < kGbLineWords; ++k)
      line[k] = gb_bits64(src, ((int64_t)(t * kMaskTileWords) - (int64_t)kGbLowWords + (int64_t)k) * 64);
    for (uint32_t tid = 0; tid < kMaskTileWords; ++tid) {
      const uint64_t wi = t * kMaskTileWords + tid, pos0 = wi * 64;
      const uint32_t d0 = 2u * (kGbLowWords + tid);
      auto hit_at = [&](uint32_t i, uint64_t hit) {
        if (!hit) return;
        r.hist[i] += (uint64_t)__builtin_popcountll(hit);
        const uint64_t c = pos0 + (uint32_t)__builtin_ctzll(hit);
        if (gb_better(i, c, br, bc)) {
          br = i;
          bc = c;
        }
      };
      uint64_t U = gb_search_first<kGbRegRanks>(gb_evens(nbits, wi), n, d0, ld, hit_at);
      U = gb_search(U, kGbTable, kGbRegRanks, n, d0, ld, [](uint64_t u) { return u != 0; }, hit_at);
      if (U) {
        r.unresolved += (uint64_t)__builtin_popcountll(U);
        if (r.first_unresolved == DSE_GOLDBACH_NONE) r.first_unresolved = g_start + pos0 + (uint32_t)__builtin_ctzll(U);
      }
    }
  }
  // the closing kernel's scalar members
  r.resolved = nbits - r.unresolved;
  r.max_rank = br;
  if (br != kGbNone) r.max_c = g_start + bc;
  *out = r;
  return DSE_OK;
}
