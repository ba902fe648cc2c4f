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

// Acquire the device's slab scratch for `stream` with room for `nres` results
// behind the slabs of `grid` workgroups; *res = the first result's device address.
int32_t stats_acquire(DevState& d, uint32_t grid, uint32_t nres, hipStream_t stream, uint64_t** res) {
  StreamScratch& s = d.stats_scratch;
  const uint64_t slabs = stats_scratch_bytes(grid);
  const uint64_t need = slabs + (uint64_t)nres * sizeof(dse_stats);
  HIP_TRY(acquire_scratch_roomy(&s, need, stream));
  if (res) *res = reinterpret_cast<uint64_t*>(static_cast<char*>(s.buf.ptr) + slabs);
  return DSE_OK;
}

// The statistics of `n` ranges (g[i], nbits, masks[i]) of one device, launched one
// after another on d.stream into the scratch's result slots: nothing is waited for.
// The caller releases the scratch once it has copied the results out.
int32_t stats_enqueue(dse_ctx* ctx, DevState& d, const uint64_t* g, uint64_t nbits, uint64_t* const* masks, uint32_t n,
                      const uint32_t* patterns, uint32_t npatterns, uint64_t** res) {
  const uint32_t grid = stats_grid(nbits, d.num_cus, ctx->stats_grid);
  int32_t rc;
  if ((rc = stats_acquire(d, grid, n, d.stream, res))) return rc;
  hipError_t e = hipSuccess;
  for (uint32_t i = 0; i < n && e == hipSuccess; ++i)
    e = launch_stats(g[i], nbits, masks[i], patterns, npatterns, *res + (uint64_t)i * DSE_STATS_WORDS,
                     d.stats_scratch.buf.ptr, grid, d.stream);
  if (e != hipSuccess) {
    (void)release_scratch(&d.stats_scratch, d.stream);
    return fail(DSE_EHIP, std::string("stats launch failed: ") + hipGetErrorString(e));
  }
  return DSE_OK;
}

// the results of stats_enqueue to the host; drains d.stream and releases the scratch
int32_t stats_collect(DevState& d, const uint64_t* res, uint32_t n, dse_stats* out) {
  hipError_t e = hipMemcpyAsync(out, res, (uint64_t)n * sizeof(dse_stats), hipMemcpyDeviceToHost, d.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
  const hipError_t r = release_scratch(&d.stats_scratch, d.stream);
  if (e == hipSuccess) e = r;
  if (e != hipSuccess) return fail(DSE_EHIP, std::string("stats copy failed: ") + hipGetErrorString(e));
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
  if (!ctx || !stats_dev) return fail(DSE_EINVAL, "null ctx or stats");
  if (nbits && !mask_dev) return fail(DSE_EINVAL, "null mask");
  if (reinterpret_cast<uintptr_t>(stats_dev) & 7u) return fail(DSE_EINVAL, "stats_dev is not 8-byte aligned");
  int32_t rc;
  if ((rc = stats_check_patterns(patterns, npatterns))) return rc;
  if ((rc = check_mask_range("stats", g_start, nbits))) return rc;
  DevState& d = ctx->devs[0];
  HIP_TRY(hipSetDevice(d.device));
  hipStream_t s = (hipStream_t)stream;
  const uint32_t grid = stats_grid(nbits, d.num_cus, ctx->stats_grid);
  if ((rc = stats_acquire(d, grid, 0, s, nullptr))) return rc;
  const hipError_t e = launch_stats(g_start, nbits, mask_dev, patterns, npatterns,
                                    reinterpret_cast<uint64_t*>(stats_dev), d.stats_scratch.buf.ptr, grid, s);
  HIP_TRY(release_scratch(&d.stats_scratch, s));  // also after a failure: what was launched may read the scratch
  if (e != hipSuccess) return fail(DSE_EHIP, std::string("stats launch failed: ") + hipGetErrorString(e));
  return DSE_OK;
}

extern "C" int32_t dse_stats_range(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint32_t* patterns,
                                   uint32_t npatterns, dse_stats* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc;
  if ((rc = stats_check_patterns(patterns, npatterns))) return rc;
  if ((rc = check_mask_range("stats", g_start, nbits))) return rc;
  DevState& d = ctx->devs[0];
  if (nbits && (rc = sieve_range_host(ctx, d, g_start, nbits, nullptr, nullptr, true))) return rc;
  HIP_TRY(hipSetDevice(d.device));
  uint64_t* res;
  uint64_t* const mask = d.scratch_mask.as<uint64_t>();
  if ((rc = stats_enqueue(ctx, d, &g_start, nbits, &mask, 1, patterns, npatterns, &res))) return rc;
  dse_stats tmp;
  if ((rc = stats_collect(d, res, 1, &tmp))) return rc;
  *out = tmp;
  return DSE_OK;
}

extern "C" int32_t dse_stats_resident(dse_ctx* ctx, int32_t my_num, const uint32_t* patterns, uint32_t npatterns,
                                      dse_stats* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc;
  if ((rc = stats_check_patterns(patterns, npatterns))) return rc;
  const ResidentSet& r = ctx->resident;
  if (!r.valid || my_num < 0 || my_num > r.P)
    return fail(DSE_EINVAL, "chunk " + std::to_string(my_num) + " is not resident");
  const uint64_t cs = (uint64_t)r.cs;
  const int32_t k0 = my_num ? my_num : 1, k1 = my_num ? my_num : r.P;
  if ((rc = check_mask_range("stats", (uint64_t)(k1 - 1) * cs, cs))) return rc;

  // every device's chunks are enqueued on its stream before any result is waited for
  const size_t nd = ctx->devs.size();
  std::vector<std::vector<uint64_t>> g(nd);
  std::vector<std::vector<uint64_t*>> masks(nd);
  std::vector<std::vector<int32_t>> chunk(nd);
  for (int32_t k = k0; k <= k1; ++k) {
    const size_t i = (size_t)(k - 1) % nd;
    g[i].push_back((uint64_t)(k - 1) * cs);
    masks[i].push_back(r.masks[k - 1].as<uint64_t>());
    chunk[i].push_back(k);
  }
  std::vector<uint64_t*> res(nd, nullptr);
  std::vector<bool> queued(nd, false);
  rc = DSE_OK;
  for (size_t i = 0; i < nd && !rc; ++i) {
    if (g[i].empty()) continue;
    DevState& d = ctx->devs[i];
    if (hipSetDevice(d.device) != hipSuccess) {
      rc = fail(DSE_EHIP, "hipSetDevice failed");
      break;
    }
    rc = stats_enqueue(ctx, d, g[i].data(), cs, masks[i].data(), (uint32_t)g[i].size(), patterns, npatterns, &res[i]);
    queued[i] = !rc;
  }
  std::vector<dse_stats> parts((size_t)(k1 - k0 + 1));
  std::vector<dse_stats> got;
  for (size_t i = 0; i < nd; ++i) {  // collect what was enqueued, also after a failure: the scratch must be released
    if (!queued[i]) continue;
    DevState& d = ctx->devs[i];
    (void)hipSetDevice(d.device);
    got.resize(g[i].size());
    const int32_t r2 = stats_collect(d, res[i], (uint32_t)g[i].size(), got.data());
    if (r2 && !rc) rc = r2;
    if (!r2)
      for (size_t j = 0; j < got.size(); ++j) parts[(size_t)(chunk[i][j] - k0)] = got[j];
  }
  if (rc) return rc;
  dse_stats acc = parts[0];
  for (size_t j = 1; j < parts.size(); ++j)
    if ((rc = dse_stats_merge(&acc, &parts[j], &acc))) return rc;
  *out = acc;
  return DSE_OK;
}

extern "C" int32_t dse_stats_merge(const dse_stats* a, const dse_stats* b, dse_stats* out) {
  if (!a || !b || !out) return fail(DSE_EINVAL, "null stats");
  if (a->g_start + a->nbits != b->g_start || a->g_start > b->g_start)
    return fail(DSE_EINVAL, "the ranges are not adjacent");
  if (a->npatterns != b->npatterns || a->npatterns > DSE_STATS_MAX_PATTERNS ||
      std::memcmp(a->pattern, b->pattern, sizeof a->pattern))
    return fail(DSE_EINVAL, "the pattern lists differ");
  if (b->g_start > (1ull << 62) || b->nbits > (1ull << 62) - b->g_start)
    return fail(DSE_ERANGE, "merged range beyond 2^62");

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
