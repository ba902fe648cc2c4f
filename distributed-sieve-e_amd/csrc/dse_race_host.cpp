// dse_race_host.cpp -- residue-class counts and prime races of a mask, the host side
// (include/dse.h): a device-resident mask becomes one dse_race on the device
// (dse_race.hip), in the caller's device memory (dse_race_dev_async) or on the host
// (dse_race_range, dse_race_resident); dse_race_merge joins the results of adjacent
// ranges by host arithmetic, and dse_debug_race_host runs the kernels' per-word
// bodies (dse_race_word.h) on the host.
#include <cstring>

#include "dse_host.h"
#include "dse_race_word.h"

using namespace dse;

static_assert(sizeof(dse_race) == 8 * DSE_RACE_WORDS, "dse_race has no padding");
static_assert(DSE_RACE_WORDS == kRaceWords && DSE_RACE_MAX_MODULUS == kRaceMaxModulus && DSE_RACE_NONE == kRaceNone,
              "the kernels write the struct of include/dse.h");

namespace {

constexpr int64_t kRaceDStartMax = 1ll << 45;

int32_t race_check(uint32_t q, uint32_t a, uint32_t b, int64_t d_start) {
  if (q < 3 || q > DSE_RACE_MAX_MODULUS) return fail(DSE_EINVAL, "q outside 3..64");
  if (a >= q || b >= q) return fail(DSE_EINVAL, "a or b is no residue mod q");
  if (a == b && d_start) return fail(DSE_EINVAL, "a == b (counts only) needs d_start 0");
  if (d_start > kRaceDStartMax || d_start < -kRaceDStartMax) return fail(DSE_ERANGE, "|d_start| above 2^45");
  return DSE_OK;
}

void race_empty(dse_race* r, uint64_t g_start, uint64_t nbits, uint32_t q, uint32_t a, uint32_t b, int64_t d_start) {
  std::memset(r, 0, sizeof *r);
  r->g_start = g_start;
  r->nbits = nbits;
  r->q = q;
  r->a = a;
  r->b = b;
  r->d_start = r->d_end = r->max_d = r->min_d = (uint64_t)d_start;
  r->first_a_ahead = r->first_b_ahead = r->max_g = r->min_g = DSE_RACE_NONE;
}

}  // namespace

extern "C" int32_t dse_race_dev_async(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev,
                                      uint32_t q, uint32_t a, uint32_t b, int64_t d_start, dse_race* out_dev,
                                      void* stream) {
  int32_t rc;
  if ((rc = check_dev_args(ctx, nbits, mask_dev, out_dev, "out", true))) return rc;
  if ((rc = race_check(q, a, b, d_start))) return rc;
  if ((rc = check_mask_range("race", g_start, nbits))) return rc;
  return unit_dev_async<kUnitRace>(ctx, nbits, stream, [&](void* slabs, uint32_t grid, hipStream_t s) {
    return launch_race(g_start, nbits, mask_dev, q, a, b, d_start, reinterpret_cast<uint64_t*>(out_dev), slabs, grid,
                       s);
  });
}

extern "C" int32_t dse_race_range(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, uint32_t q, uint32_t a, uint32_t b,
                                  int64_t d_start, dse_race* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc;
  if ((rc = race_check(q, a, b, d_start))) return rc;
  if ((rc = check_mask_range("race", g_start, nbits))) return rc;
  return unit_range<kUnitRace>(
      ctx, g_start, nbits, nbits,
      [&](const uint64_t* mask, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) {
        return launch_race(g_start, nbits, mask, q, a, b, d_start, res, slabs, grid, s);
      },
      out);
}

extern "C" int32_t dse_race_resident(dse_ctx* ctx, int32_t my_num, uint32_t q, uint32_t a, uint32_t b,
                                     int64_t d_start, dse_race* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc;
  if ((rc = race_check(q, a, b, d_start))) return rc;
  int32_t k0, k1;
  if ((rc = resident_span(ctx, my_num, "race", &k0, &k1))) return rc;
  const ResidentSet& r = ctx->resident;
  const uint64_t cs = (uint64_t)r.cs;
  const size_t n = (size_t)(k1 - k0 + 1);
  std::vector<int64_t> d_starts(n, d_start);
  std::vector<dse_race> parts;
  // one dse_race per chunk: chunk k with the classes (a, b2) from ds[k - k0]
  auto pass = [&](uint32_t b2, const std::vector<int64_t>& ds) {
    return unit_resident_parts<kUnitRace>(
        ctx, k0, k1, 0,
        [&](DevState&, int32_t k, uint64_t*, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) {
          return launch_race((uint64_t)(k - 1) * cs, cs, r.masks[(size_t)k - 1].as<uint64_t>(), q, a, b2,
                             ds[(size_t)(k - k0)], res, slabs, grid, s);
        },
        &parts);
  };
  if (n > 1 && a != b) {
    // chunk k + 1 starts from chunk k's d_end: the chunks' class counts first, on every device
    if ((rc = pass(a, std::vector<int64_t>(n, 0)))) return rc;
    for (size_t j = 1; j < n; ++j)
      d_starts[j] = d_starts[j - 1] + (int64_t)parts[j - 1].counts[a] - (int64_t)parts[j - 1].counts[b];
  }
  if ((rc = pass(b, d_starts))) return rc;
  return merge_parts(parts, dse_race_merge, out);
}

extern "C" int32_t dse_race_merge(const dse_race* a, const dse_race* b, dse_race* out) {
  if (!a || !b || !out) return fail(DSE_EINVAL, "null race result");
  if (int32_t rc = check_merge_adjacent(a->g_start, a->nbits, b->g_start)) return rc;
  if (a->q != b->q || a->a != b->a || a->b != b->b || a->q < 3 || a->q > DSE_RACE_MAX_MODULUS)
    return fail(DSE_EINVAL, "the results are of different races");
  if (b->d_start != a->d_end) return fail(DSE_EINVAL, "the second range does not start from the first one's d_end");
  if (int32_t rc = check_merge_end(b->g_start, b->nbits)) return rc;
  dse_race r = *a;  // out may alias a or b
  r.nbits = a->nbits + b->nbits;
  r.d_end = b->d_end;
  r.steps = a->steps + b->steps;
  r.a_ahead = a->a_ahead + b->a_ahead;
  r.b_ahead = a->b_ahead + b->b_ahead;
  r.ties = a->ties + b->ties;
  if (a->first_a_ahead == DSE_RACE_NONE) r.first_a_ahead = b->first_a_ahead;
  if (a->first_b_ahead == DSE_RACE_NONE) r.first_b_ahead = b->first_b_ahead;
  // a side without steps has no extremum of its own: its *_d only repeat its d_start
  if (b->steps && (!a->steps || (int64_t)b->max_d > (int64_t)a->max_d)) {
    r.max_d = b->max_d;
    r.max_g = b->max_g;
  }
  if (b->steps && (!a->steps || (int64_t)b->min_d < (int64_t)a->min_d)) {
    r.min_d = b->min_d;
    r.min_g = b->min_g;
  }
  for (uint32_t i = 0; i < DSE_RACE_MAX_MODULUS; ++i) r.counts[i] = a->counts[i] + b->counts[i];
  *out = r;
  return DSE_OK;
}

extern "C" int32_t dse_debug_race_host(const uint64_t* mask, uint64_t g_start, uint64_t nbits, uint32_t q, uint32_t a,
                                       uint32_t b, int64_t d_start, dse_race* out) {
  if (!out) return fail(DSE_EINVAL, "null out");
  if (nbits && !mask) return fail(DSE_EINVAL, "null mask");
  if (reinterpret_cast<uintptr_t>(mask) & 7u) return fail(DSE_EINVAL, "mask is not 8-byte aligned");
  int32_t rc;
  if ((rc = race_check(q, a, b, d_start))) return rc;
  if ((rc = check_mask_range("race", g_start, nbits))) return rc;
  const MaskRange mr = mask_range(mask, g_start, nbits);
  const uint32_t T = race_period(q), ca = race_class_pos(q, a), cb = race_class_pos(q, b);
  const uint64_t comb = race_comb(T);
  dse_race r;
  race_empty(&r, g_start, nbits, q, a, b, d_start);
  // the count kernel's loop, then the closing kernel's map from position classes to residues
  uint64_t cnt[kRaceMaxModulus] = {};
  uint32_t ph = (uint32_t)(g_start % T);
  for (uint64_t wi = 0; wi < mr.words; ++wi) {
    race_count_word<kRaceMaxModulus>(mask_word(mr, wi), comb, T, ph, cnt);
    ph = race_phase_add(ph, 64 % T, T);
  }
  for (uint32_t res = 0; res < q; ++res) {
    const uint32_t c = race_class_pos(q, res);
    r.counts[res] = c == kRaceNoClass ? 0 : cnt[c];
  }
  if (a != b) {
    // the main kernel's loop: the scan is the loop's carry
    RaceAcc acc;
    int64_t D = d_start;
    ph = (uint32_t)(g_start % T);
    for (uint64_t wi = 0; wi < mr.words; ++wi) {
      const uint64_t w = mask_word(mr, wi);
      const uint64_t A = w & race_class_mask(comb, T, ca, ph), B = w & race_class_mask(comb, T, cb, ph);
      ph = race_phase_add(ph, 64 % T, T);
      race_word(A, B, D, wi * 64, acc);
      D += (int64_t)__builtin_popcountll(A) - (int64_t)__builtin_popcountll(B);
    }
    // the closing kernel's scalar members
    r.steps = r.counts[a] + r.counts[b];
    r.d_end = (uint64_t)(d_start + (int64_t)r.counts[a] - (int64_t)r.counts[b]);
    r.a_ahead = acc.a_ahead;
    r.b_ahead = acc.b_ahead;
    r.ties = r.steps - acc.a_ahead - acc.b_ahead;
    if (acc.first_a != kRaceNone) r.first_a_ahead = g_start + acc.first_a;
    if (acc.first_b != kRaceNone) r.first_b_ahead = g_start + acc.first_b;
    if (acc.max_g != kRaceNone) {
      r.max_d = (uint64_t)acc.max_d;
      r.max_g = g_start + acc.max_g;
    }
    if (acc.min_g != kRaceNone) {
      r.min_d = (uint64_t)acc.min_d;
      r.min_g = g_start + acc.min_g;
    }
  }
  *out = r;
  return DSE_OK;
}
