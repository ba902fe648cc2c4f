// dse_sums_host.cpp -- power and reciprocal sums over the matches of a pattern, the
// host side (include/dse.h): a device-resident mask becomes one dse_sums on the
// device (dse_sums.hip), in the caller's device memory (dse_sums_dev_async) or on
// the host (dse_sums_range, dse_sums_resident); dse_sums_merge adds the results of
// adjacent ranges by host arithmetic, and dse_debug_sums_host runs the kernels'
// per-word and per-entry bodies (dse_sums_word.h) on the host.
#include <algorithm>

#include "dse_host.h"
#include "dse_sums_word.h"

using namespace dse;

static_assert(sizeof(dse_sums) == 8 * DSE_SUMS_WORDS, "dse_sums has no padding");
static_assert(DSE_SUMS_WORDS == kSumsWords && DSE_SUMS_NONE == kSumsNone && DSE_SUMS_POWER == kSumsPower &&
                  DSE_SUMS_RECIP == kSumsRecip && DSE_SUMS_RECIP_SHIFT == kSumsRecipShift,
              "the kernels write the struct of include/dse.h");

namespace {

int32_t sums_check(uint64_t require, uint64_t forbid, uint64_t flags) {
  if (require >> 32 || forbid >> 32) return fail(DSE_EINVAL, "a pattern has 32 bits");
  if (flags & ~(uint64_t)(DSE_SUMS_POWER | DSE_SUMS_RECIP)) return fail(DSE_EINVAL, "unknown flags");
  return tuples_check_pattern((uint32_t)require, (uint32_t)forbid);
}

}  // namespace

extern "C" int32_t dse_sums_dev_async(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev,
                                      uint32_t require, uint32_t forbid, const uint64_t* above_dev,
                                      uint32_t above_shift, uint32_t above_bits, uint32_t flags, dse_sums* out_dev,
                                      void* stream) {
  int32_t rc;
  if ((rc = check_dev_args(ctx, nbits, mask_dev, out_dev, "out", false))) return rc;
  if ((rc = sums_check(require, forbid, flags))) return rc;
  if ((rc = tuples_check_above(above_dev, above_shift, above_bits))) return rc;
  if ((rc = check_mask_range("sums", g_start, nbits))) return rc;
  if ((rc = check_odd_range(g_start, nbits + above_bits))) return rc;
  const TuplePattern p{require, forbid, above_dev, above_shift, above_bits};
  return unit_dev_async<kUnitSums>(ctx, nbits, stream, [&](void* slabs, uint32_t grid, hipStream_t s) {
    return launch_sums(g_start, nbits, mask_dev, p, flags, reinterpret_cast<uint64_t*>(out_dev), slabs, grid, s);
  });
}

extern "C" int32_t dse_sums_range(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, uint32_t require, uint32_t forbid,
                                  uint32_t flags, dse_sums* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc;
  if ((rc = sums_check(require, forbid, flags))) return rc;
  if ((rc = check_mask_range("sums", g_start, nbits))) return rc;
  // the candidates above the range are sieved with it, as dse_tuples_range does: up to 31 of them,
  // fewer where the sieve's last candidate (the odd index 2^61 - 2) ends them
  const uint64_t top = (1ull << 61) - 1, end = g_start + nbits;
  const uint64_t ext = nbits && end < top ? std::min<uint64_t>(kTuplesMaxAbove, top - end) : 0;
  return unit_range<kUnitSums>(
      ctx, g_start, nbits + ext, nbits,
      [&](const uint64_t* m, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) {
        const TuplePattern p{require, forbid, ext ? m + (nbits >> 6) : nullptr, (uint32_t)(nbits & 63), (uint32_t)ext};
        return launch_sums(g_start, nbits, m, p, flags, res, slabs, grid, s);
      },
      out);
}

extern "C" int32_t dse_sums_resident(dse_ctx* ctx, int32_t my_num, uint32_t require, uint32_t forbid, uint32_t flags,
                                     dse_sums* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc, k0, k1;
  if ((rc = sums_check(require, forbid, flags))) return rc;
  if ((rc = resident_span(ctx, my_num, "sums", &k0, &k1))) return rc;
  const ResidentSet& r = ctx->resident;
  const uint64_t cs = (uint64_t)r.cs;
  if (cs && (rc = resident_above_check(ctx, k0))) return rc;
  return unit_resident<kUnitSums>(
      ctx, k0, k1, 1,  // behind the results: a neighbour's head word per chunk
      [&](DevState& d, int32_t k, uint64_t* head, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) -> int32_t {
        TuplePattern p{require, forbid, nullptr, 0, 0};
        if (cs && k < r.P)
          if (int32_t ra = resident_above(ctx, d, k, head, &p)) return ra;
        const uint64_t* const mask = r.masks[(size_t)k - 1].as<uint64_t>();
        return launch_rc(kSlabUnits[kUnitSums],
                         launch_sums((uint64_t)(k - 1) * cs, cs, mask, p, flags, res, slabs, grid, s));
      },
      dse_sums_merge, out);
}

extern "C" int32_t dse_sums_merge(const dse_sums* a, const dse_sums* b, dse_sums* out) {
  if (!a || !b || !out) return fail(DSE_EINVAL, "null sums");
  if (int32_t rc = check_merge_adjacent(a->g_start, a->nbits, b->g_start)) return rc;
  if (a->require != b->require || a->forbid != b->forbid || a->flags != b->flags)
    return fail(DSE_EINVAL, "the sums are of different patterns or flags");
  if (int32_t rc = sums_check(a->require, a->forbid, a->flags)) return rc;
  // a must have seen across the seam: every candidate of b's that a span starting in a can reach
  const uint64_t span = tuples_span((uint32_t)a->require, (uint32_t)a->forbid);
  if (a->above_bits < std::min<uint64_t>(span - 1, b->nbits + b->above_bits))
    return fail(DSE_EINVAL, "the lower range saw too few candidates above it");
  if (int32_t rc = check_merge_end(b->g_start, b->nbits)) return rc;

  dse_sums r = *a;
  r.nbits = a->nbits + b->nbits;
  r.above_bits = b->above_bits;
  r.matches = a->matches + b->matches;
  r.first_g = a->first_g != DSE_SUMS_NONE ? a->first_g : b->first_g;
  r.last_g = b->last_g != DSE_SUMS_NONE ? b->last_g : a->last_g;
  limbs_add(r.sum1, b->sum1);
  limbs_add(r.sum2, b->sum2);
  limbs_add(r.recip, b->recip);
  *out = r;
  return DSE_OK;
}

extern "C" int32_t dse_debug_sums_host(const uint64_t* mask, uint64_t g_start, uint64_t nbits, uint32_t require,
                                       uint32_t forbid, const uint64_t* above, uint32_t above_shift,
                                       uint32_t above_bits, uint32_t flags, dse_sums* out) {
  if (!out) return fail(DSE_EINVAL, "null out");
  if (nbits && !mask) return fail(DSE_EINVAL, "null mask");
  int32_t rc;
  if ((rc = sums_check(require, forbid, flags))) return rc;
  if ((rc = tuples_check_above(above, above_shift, above_bits))) return rc;
  if ((rc = check_mask_range("sums", g_start, nbits))) return rc;
  if ((rc = check_odd_range(g_start, nbits + above_bits))) return rc;
  const TupleSrc s{mask_range(mask, g_start, nbits), above, above_shift, above_bits, require, forbid};
  const uint64_t B = 3 + 2 * g_start;
  // the main kernel's tile loop, one word at a time, into one set of its accumulators
  SumsPower pw = {0, {0, 0}, {0, 0, 0}};
  dse_sums r = {};
  r.g_start = g_start;
  r.nbits = nbits;
  r.require = require;
  r.forbid = forbid;
  r.above_bits = above_bits;
  r.flags = flags;
  r.first_g = r.last_g = DSE_SUMS_NONE;
  for (uint64_t wi = 0; wi < s.r.words; ++wi) {
    const uint64_t m = tuples_word(s, wi, tuples_visible_word(s, wi), (uint32_t)tuples_visible_word(s, wi + 1));
    if (!m) continue;
    const uint64_t pos0 = wi * 64;
    if (r.first_g == DSE_SUMS_NONE) r.first_g = g_start + pos0 + stats_ctz64(m);
    r.last_g = g_start + pos0 + stats_msb64(m);
    if (flags & DSE_SUMS_POWER)
      sums_word_power(m, pos0, pw);
    else
      pw.n += stats_pop64(m);
    if (flags & DSE_SUMS_RECIP)
      for (uint64_t it = m; it; it &= it - 1) sums_entry_recip(B + 2 * (pos0 + stats_ctz64(it)), require, r.recip);
  }
  r.matches = pw.n;
  if (flags & DSE_SUMS_POWER) sums_power_close(pw, B, r.sum1, r.sum2);
  *out = r;
  return DSE_OK;
}

extern "C" int32_t dse_debug_sums_recip(const uint64_t* v, uint64_t n, uint64_t* out) {
  if (n && (!v || !out)) return fail(DSE_EINVAL, "null v or out");
  for (uint64_t i = 0; i < n; ++i)
    if (v[i] < 3) return fail(DSE_ERANGE, "a divisor below 3");
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t q[2];
    sums_recip(v[i], q);
    out[2 * i] = q[0];
    out[2 * i + 1] = q[1];
  }
  return DSE_OK;
}
