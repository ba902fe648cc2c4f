// dse_stats_host.cpp -- statistics of a mask, the host side (include/dse.h): a
// device-resident mask becomes one dse_stats on the device (dse_stats.hip), in
// the caller's device memory (dse_stats_dev_async) or on the host
// (dse_stats_range, dse_stats_resident); dse_stats_merge joins the results of
// adjacent ranges by host arithmetic, and dse_debug_stats_host runs the
// kernels' per-word bodies (dse_stats_word.h) on the host.
#include <cstring>

#include "dse_host.h"
#include "dse_stats_word.h"

using namespace dse;

static_assert(sizeof(dse_stats) == 8 * DSE_STATS_WORDS, "dse_stats has no padding");
static_assert(DSE_STATS_WORDS == kStatsWords && DSE_STATS_GAP_BINS == kStatsBins && DSE_STATS_NONE == kStatsNone,
              "the kernels write the struct of include/dse.h");

namespace {

int32_t stats_check_patterns(const uint32_t* patterns, uint32_t npatterns) {
  if (npatterns > DSE_STATS_MAX_PATTERNS) return fail(DSE_EINVAL, "more than 8 patterns");
  if (npatterns && !patterns) return fail(DSE_EINVAL, "null patterns with a non-zero count");
  for (uint32_t p = 0; p < npatterns; ++p)
    if (!(patterns[p] & 1u)) return fail(DSE_EINVAL, "pattern " + std::to_string(p) + " has bit 0 clear");
  return DSE_OK;
}

// bit q of the 128 candidates around a seam: a's last 64 (its last at q = 63), then b's first 64
inline bool seam_bit(const dse_stats& a, const dse_stats& b, uint32_t q) {
  return q < 64 ? (a.tail >> q) & 1 : (b.head >> (q - 64)) & 1;
}

}  // namespace

extern "C" int32_t dse_stats_dev_async(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev,
                                       const uint32_t* patterns, uint32_t npatterns, dse_stats* stats_dev,
                                       void* stream) {
  int32_t rc;
  if ((rc = check_dev_args(ctx, nbits, mask_dev, stats_dev, "stats", false))) return rc;
  if ((rc = stats_check_patterns(patterns, npatterns))) return rc;
  if ((rc = check_mask_range("stats", g_start, nbits))) return rc;
  return unit_dev_async<kUnitStats>(ctx, nbits, stream, [&](void* slabs, uint32_t grid, hipStream_t s) {
    return launch_stats(g_start, nbits, mask_dev, patterns, npatterns, reinterpret_cast<uint64_t*>(stats_dev), slabs,
                        grid, s);
  });
}

extern "C" int32_t dse_stats_range(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint32_t* patterns,
                                   uint32_t npatterns, dse_stats* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc;
  if ((rc = stats_check_patterns(patterns, npatterns))) return rc;
  if ((rc = check_mask_range("stats", g_start, nbits))) return rc;
  return unit_range<kUnitStats>(
      ctx, g_start, nbits, nbits,
      [&](const uint64_t* mask, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) {
        return launch_stats(g_start, nbits, mask, patterns, npatterns, res, slabs, grid, s);
      },
      out);
}

extern "C" int32_t dse_stats_resident(dse_ctx* ctx, int32_t my_num, const uint32_t* patterns, uint32_t npatterns,
                                      dse_stats* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc;
  if ((rc = stats_check_patterns(patterns, npatterns))) return rc;
  int32_t k0, k1;
  if ((rc = resident_span(ctx, my_num, "stats", &k0, &k1))) return rc;
  const ResidentSet& r = ctx->resident;
  const uint64_t cs = (uint64_t)r.cs;
  return unit_resident<kUnitStats>(
      ctx, k0, k1, 0,
      [&](DevState&, int32_t k, uint64_t*, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) {
        return launch_stats((uint64_t)(k - 1) * cs, cs, r.masks[(size_t)k - 1].as<uint64_t>(), patterns, npatterns, res,
                            slabs, grid, s);
      },
      dse_stats_merge, out);
}

extern "C" int32_t dse_stats_merge(const dse_stats* a, const dse_stats* b, dse_stats* out) {
  if (!a || !b || !out) return fail(DSE_EINVAL, "null stats");
  if (int32_t rc = check_merge_adjacent(a->g_start, a->nbits, b->g_start)) return rc;
  if (a->npatterns != b->npatterns || a->npatterns > DSE_STATS_MAX_PATTERNS ||
      std::memcmp(a->pattern, b->pattern, sizeof a->pattern))
    return fail(DSE_EINVAL, "the pattern lists differ");
  if (int32_t rc = check_merge_end(b->g_start, b->nbits)) return rc;

  dse_stats r;
  std::memset(&r, 0, sizeof r);
  r.g_start = a->g_start;
  r.nbits = a->nbits + b->nbits;
  r.primes = a->primes + b->primes;
  r.first_g = a->first_g != DSE_STATS_NONE ? a->first_g : b->first_g;
  r.last_g = b->last_g != DSE_STATS_NONE ? b->last_g : a->last_g;
  r.head = a->nbits >= 64 ? a->head : a->head | (b->head << a->nbits);
  r.tail = b->nbits >= 64 ? b->tail : b->nbits == 0 ? a->tail : b->tail | (a->tail >> b->nbits);
  r.npatterns = a->npatterns;
  for (uint32_t p = 0; p < DSE_STATS_MAX_PATTERNS; ++p) {
    r.pattern[p] = a->pattern[p];
    uint64_t m = a->matches[p] + b->matches[p];
    const uint32_t pat = (uint32_t)a->pattern[p];
    if (p < a->npatterns && pat) {
      const uint32_t span = 32u - (uint32_t)__builtin_clz(pat);
      // a match that starts t places before the seam has its last member span - t - 1 places behind it
      for (uint32_t t = 1; t < span; ++t) {
        if (t > a->nbits || span - t > b->nbits) continue;
        bool all = true;
        for (uint32_t j = 0; j < span && all; ++j)
          if ((pat >> j) & 1u) all = seam_bit(*a, *b, 64 - t + j);
        m += all;
      }
    }
    r.matches[p] = m;
  }
  for (uint32_t d = 0; d < DSE_STATS_GAP_BINS; ++d) r.gaps[d] = a->gaps[d] + b->gaps[d];
  r.gap_overflow = a->gap_overflow + b->gap_overflow;
  r.max_gap = a->max_gap;
  r.max_gap_g = a->max_gap_g;
  if (a->last_g != DSE_STATS_NONE && b->first_g != DSE_STATS_NONE) {
    const uint64_t d = b->first_g - a->last_g;
    if (d < DSE_STATS_GAP_BINS)
      ++r.gaps[d];
    else
      ++r.gap_overflow;
    if (2 * d > r.max_gap) {
      r.max_gap = 2 * d;
      r.max_gap_g = a->last_g;
    }
  }
  if (b->max_gap > r.max_gap) {
    r.max_gap = b->max_gap;
    r.max_gap_g = b->max_gap_g;
  }
  *out = r;
  return DSE_OK;
}

extern "C" int32_t dse_debug_stats_host(const uint64_t* mask, uint64_t g_start, uint64_t nbits,
                                        const uint32_t* patterns, uint32_t npatterns, dse_stats* out) {
  if (!out) return fail(DSE_EINVAL, "null out");
  if (nbits && !mask) return fail(DSE_EINVAL, "null mask");
  int32_t rc;
  if ((rc = stats_check_patterns(patterns, npatterns))) return rc;
  if ((rc = check_mask_range("stats", g_start, nbits))) return rc;
  const MaskRange m = mask_range(mask, g_start, nbits);
  dse_stats r;
  std::memset(&r, 0, sizeof r);
  r.g_start = g_start;
  r.nbits = nbits;
  r.first_g = r.last_g = r.max_gap_g = DSE_STATS_NONE;
  r.npatterns = npatterns;
  for (uint32_t p = 0; p < npatterns; ++p) r.pattern[p] = patterns[p];
  uint64_t bd = 0, bi = kStatsNone, carry = 0;
  auto put = [&](uint64_t d, uint64_t i) {
    if (d < kStatsBins)
      ++r.gaps[d];
    else
      ++r.gap_overflow;
    if (stats_better(d, i, bd, bi)) {
      bd = d;
      bi = i;
    }
  };
  // the main kernel's tile loop, one word at a time: the scan's result is the loop's carry
  for (uint64_t wi = 0; wi < m.words; ++wi) {
    const uint64_t w = mask_word(m, wi);
    const uint32_t nx = (uint32_t)mask_word(m, wi + 1);
    const uint64_t pos0 = wi * 64;
    r.primes += stats_pop64(w);
    for (uint32_t p = 0; p < npatterns; ++p) r.matches[p] += stats_pattern_word(w, nx, patterns[p]);
    const uint64_t rem = stats_small_gaps(w, nx, r.gaps + 1);
    if (w) {
      const uint64_t f = pos0 + stats_ctz64(w);
      if (carry)
        stats_cross(f, carry, put);
      else
        r.first_g = g_start + f;
      stats_inword_large(w, rem, pos0, put);
      carry = pos0 + stats_msb64(w) + 1;
    }
  }
  if (bd == 0 && carry != 0)
    for (uint64_t wi = 0; wi < m.words; ++wi)
      stats_small_best(mask_word(m, wi), (uint32_t)mask_word(m, wi + 1), wi * 64, bd, bi);
  // the closing kernel's scalar members
  if (carry) r.last_g = g_start + (carry - 1);
  r.head = stats_bits64(m, 0);
  r.tail = nbits >= 64 ? stats_bits64(m, nbits - 64) : nbits == 0 ? 0ull : r.head << (64 - nbits);
  r.max_gap = 2 * bd;
  if (bd) r.max_gap_g = g_start + bi;
  *out = r;
  return DSE_OK;
}
