// dse_gaps_host.cpp -- where the prime gaps of a mask are, the host side
// (include/dse.h): a device-resident mask becomes one dse_gaps on the device
// (dse_gaps.hip), in the caller's device memory (dse_gaps_dev_async) or on the
// host (dse_gaps_range, dse_gaps_resident); dse_gaps_merge joins the results of
// adjacent ranges and dse_gaps_records reads the maximal gaps off a result, both
// by host arithmetic, and dse_debug_gaps_host runs the kernels' per-word bodies
// (dse_gaps_word.h) on the host.
#include <cstring>

#include "dse_gaps_word.h"
#include "dse_host.h"

using namespace dse;

static_assert(sizeof(dse_gaps) == 8 * DSE_GAPS_WORDS, "dse_gaps has no padding");
static_assert(DSE_GAPS_WORDS == kGapsWords && DSE_GAPS_BINS == kGapsBins && DSE_GAPS_NONE == kGapsNone,
              "the kernels write the struct of include/dse.h");

namespace {

void gaps_recount(dse_gaps* r) {
  r->found = 0;
  for (uint32_t d = 0; d < DSE_GAPS_BINS; ++d) r->found += r->first[d] != DSE_GAPS_NONE;
}

}  // namespace

extern "C" int32_t dse_gaps_dev_async(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev,
                                      dse_gaps* out_dev, void* stream) {
  int32_t rc;
  if ((rc = check_dev_args(ctx, nbits, mask_dev, out_dev, "out", false))) return rc;
  if ((rc = check_mask_range("gaps", g_start, nbits))) return rc;
  return unit_dev_async<kUnitGaps>(ctx, nbits, stream, [&](void* slabs, uint32_t grid, hipStream_t s) {
    return launch_gaps(g_start, nbits, mask_dev, reinterpret_cast<uint64_t*>(out_dev), slabs, grid, s);
  });
}

extern "C" int32_t dse_gaps_range(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, dse_gaps* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  if (int32_t rc = check_mask_range("gaps", g_start, nbits)) return rc;
  return unit_range<kUnitGaps>(
      ctx, g_start, nbits, nbits,
      [&](const uint64_t* mask, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) {
        return launch_gaps(g_start, nbits, mask, res, slabs, grid, s);
      },
      out);
}

extern "C" int32_t dse_gaps_resident(dse_ctx* ctx, int32_t my_num, dse_gaps* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc, k0, k1;
  if ((rc = resident_span(ctx, my_num, "gaps", &k0, &k1))) return rc;
  const ResidentSet& r = ctx->resident;
  const uint64_t cs = (uint64_t)r.cs;
  return unit_resident<kUnitGaps>(
      ctx, k0, k1, 0,
      [&](DevState&, int32_t k, uint64_t*, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) {
        return launch_gaps((uint64_t)(k - 1) * cs, cs, r.masks[(size_t)k - 1].as<uint64_t>(), res, slabs, grid, s);
      },
      dse_gaps_merge, out);
}

extern "C" int32_t dse_gaps_merge(const dse_gaps* a, const dse_gaps* b, dse_gaps* out) {
  if (!a || !b || !out) return fail(DSE_EINVAL, "null gaps");
  if (int32_t rc = check_merge_adjacent(a->g_start, a->nbits, b->g_start)) return rc;
  if (int32_t rc = check_merge_end(b->g_start, b->nbits)) return rc;

  // the seam's gap: s places at a's last prime, above every position of a and below every one of b
  const bool seam = a->last_g != DSE_GAPS_NONE && b->first_g != DSE_GAPS_NONE;
  const uint64_t s = seam ? b->first_g - a->last_g : 0;
  dse_gaps r;
  r.g_start = a->g_start;
  r.nbits = a->nbits + b->nbits;
  r.primes = a->primes + b->primes;
  r.first_g = a->first_g != DSE_GAPS_NONE ? a->first_g : b->first_g;
  r.last_g = b->last_g != DSE_GAPS_NONE ? b->last_g : a->last_g;
  for (uint32_t d = 0; d < DSE_GAPS_BINS; ++d)
    r.first[d] = a->first[d] != DSE_GAPS_NONE ? a->first[d] : seam && s == d ? a->last_g : b->first[d];
  r.overflow_g = a->overflow_g != DSE_GAPS_NONE  ? a->overflow_g
                 : seam && s >= DSE_GAPS_BINS ? a->last_g
                                              : b->overflow_g;
  r.max_gap = a->max_gap;
  r.max_gap_g = a->max_gap_g;
  if (seam && 2 * s > r.max_gap) {
    r.max_gap = 2 * s;
    r.max_gap_g = a->last_g;
  }
  if (b->max_gap > r.max_gap) {
    r.max_gap = b->max_gap;
    r.max_gap_g = b->max_gap_g;
  }
  gaps_recount(&r);
  *out = r;
  return DSE_OK;
}

extern "C" int32_t dse_gaps_records(const dse_gaps* g, uint32_t* d_out, uint32_t cap, uint32_t* count) {
  if (!g || !count) return fail(DSE_EINVAL, "null gaps or count");
  if (cap && !d_out) return fail(DSE_EINVAL, "null d_out with a capacity");
  // from the longest bin down: a bin is a record when it starts below every longer gap
  static_assert(DSE_GAPS_BINS <= 1024, "the records of one result fit the stack");
  uint32_t rec[DSE_GAPS_BINS], n = 0;
  uint64_t lowest = g->overflow_g;  // DSE_GAPS_NONE: above every position
  for (uint32_t d = DSE_GAPS_BINS - 1; d >= 1; --d) {
    const uint64_t f = g->first[d];
    if (f == DSE_GAPS_NONE) continue;
    if (f < lowest) {
      rec[n++] = d;
      lowest = f;
    }
  }
  for (uint32_t k = 0; k < n && k < cap; ++k) d_out[k] = rec[n - 1 - k];
  *count = n;
  return DSE_OK;
}

extern "C" int32_t dse_debug_gaps_host(const uint64_t* mask, uint64_t g_start, uint64_t nbits, dse_gaps* out) {
  if (!out) return fail(DSE_EINVAL, "null out");
  if (nbits && !mask) return fail(DSE_EINVAL, "null mask");
  int32_t rc;
  if ((rc = check_mask_range("gaps", g_start, nbits))) return rc;
  const MaskRange m = mask_range(mask, g_start, nbits);
  uint64_t tab[kGapsBins + 1];  // the main kernel's table: positions, [kGapsBins] the overflow bin
  for (uint32_t d = 0; d <= kGapsBins; ++d) tab[d] = kGapsNone;
  uint64_t primes = 0, first = kGapsNone, carry = 0, bd = 0, bi = kGapsNone;
  auto put = [&](uint64_t d, uint64_t i) {
    uint64_t& e = tab[d < kGapsBins ? d : kGapsBins];
    if (i < e) e = i;
    if (d >= kGapsBins && stats_better(d, i, bd, bi)) {
      bd = d;
      bi = i;
    }
  };
  // the main kernel's tile loop, one word at a time: the scan's result is the loop's carry, and
  // the settled bits are refreshed from the table at every tile, under that tile's floor
  const uint64_t ntiles = mask_tiles(nbits);
  for (uint64_t t = 0; t < ntiles; ++t) {
    const uint64_t floor = gaps_floor(t * (uint64_t)kMaskTileBits, carry);
    GapsSettled st = {0ull, 0ull};
    for (uint32_t d = 0; d < kGapsSettled; ++d)
      if (gaps_settled_bit(tab[d], floor)) (d < 64 ? st.lo : st.hi) |= 1ull << (d & 63);
    for (uint64_t wi = t * kMaskTileWords; wi < (t + 1) * kMaskTileWords && wi < m.words; ++wi) {
      const uint64_t w = mask_word(m, wi);
      const uint32_t nx = (uint32_t)mask_word(m, wi + 1);
      const uint64_t pos0 = wi * 64;
      primes += stats_pop64(w);
      const uint64_t rem = gaps_small(w, nx, pos0, st.lo, put);
      if (w) {
        const uint64_t f = pos0 + stats_ctz64(w);
        if (carry)
          gaps_cross(f, carry, st, put);
        else
          first = f;
        gaps_inword_large(w, rem, pos0, st, put);
        carry = pos0 + stats_msb64(w) + 1;
      }
    }
  }
  // the slab's maximal gap and the closing kernel's members
  for (uint32_t d = 0; d < kGapsBins; ++d)
    if (tab[d] != kGapsNone && stats_better(d, tab[d], bd, bi)) {
      bd = d;
      bi = tab[d];
    }
  dse_gaps r;
  r.g_start = g_start;
  r.nbits = nbits;
  r.primes = primes;
  r.first_g = first == kGapsNone ? DSE_GAPS_NONE : g_start + first;
  r.last_g = carry ? g_start + (carry - 1) : DSE_GAPS_NONE;
  r.max_gap = 2 * bd;
  r.max_gap_g = bd ? g_start + bi : DSE_GAPS_NONE;
  r.overflow_g = tab[kGapsBins] == kGapsNone ? DSE_GAPS_NONE : g_start + tab[kGapsBins];
  for (uint32_t d = 0; d < kGapsBins; ++d) r.first[d] = tab[d] == kGapsNone ? DSE_GAPS_NONE : g_start + tab[d];
  gaps_recount(&r);
  *out = r;
  return DSE_OK;
}
