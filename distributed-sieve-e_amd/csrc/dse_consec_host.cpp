// dse_consec_host.cpp -- the residue pairs of consecutive primes of a mask, the host
// side (include/dse.h): a device-resident mask becomes one dse_consec on the device
// (dse_consec.hip), in the caller's device memory (dse_consec_dev_async) or on the
// host (dse_consec_range, dse_consec_resident); dse_consec_merge joins the results of
// adjacent ranges by host arithmetic, and dse_debug_consec_host runs the kernels'
// per-word bodies (dse_consec_word.h) on the host.
#include <cstring>

#include "dse_consec_word.h"
#include "dse_host.h"

using namespace dse;

static_assert(sizeof(dse_consec) == 8 * DSE_CONSEC_WORDS, "dse_consec has no padding");
static_assert(DSE_CONSEC_WORDS == kConsecWords && DSE_CONSEC_MAX_MODULUS == kConsecMaxModulus &&
                  DSE_CONSEC_MAX_MODULUS == kConsecStride && DSE_CONSEC_NONE == kConsecNone,
              "the kernels write the struct of include/dse.h");

namespace {

int32_t consec_check(uint32_t q) {
  if (q < 3 || q > DSE_CONSEC_MAX_MODULUS) return fail(DSE_EINVAL, "q outside 3..64");
  return DSE_OK;
}

hipError_t consec_launch(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint32_t q,
                         uint64_t* out, void* slabs, uint32_t grid, hipStream_t s) {
  return launch_consec(g_start, nbits, mask, q, out, slabs, grid, ctx->consec_flush_tiles, ctx->consec_body, s);
}

}  // namespace

extern "C" int32_t dse_consec_dev_async(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev,
                                        uint32_t q, dse_consec* out_dev, void* stream) {
  int32_t rc;
  if ((rc = check_dev_args(ctx, nbits, mask_dev, out_dev, "out", true))) return rc;
  if ((rc = consec_check(q))) return rc;
  if ((rc = check_mask_range("consec", g_start, nbits))) return rc;
  return unit_dev_async<kUnitConsec>(ctx, nbits, stream, [&](void* slabs, uint32_t grid, hipStream_t s) {
    return consec_launch(ctx, g_start, nbits, mask_dev, q, reinterpret_cast<uint64_t*>(out_dev), slabs, grid, s);
  });
}

extern "C" int32_t dse_consec_range(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, uint32_t q, dse_consec* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc;
  if ((rc = consec_check(q))) return rc;
  if ((rc = check_mask_range("consec", g_start, nbits))) return rc;
  return unit_range<kUnitConsec>(
      ctx, g_start, nbits, nbits,
      [&](const uint64_t* mask, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) {
        return consec_launch(ctx, g_start, nbits, mask, q, res, slabs, grid, s);
      },
      out);
}

extern "C" int32_t dse_consec_resident(dse_ctx* ctx, int32_t my_num, uint32_t q, dse_consec* out) {
  if (!ctx || !out) return fail(DSE_EINVAL, "null ctx or out");
  int32_t rc, k0, k1;
  if ((rc = consec_check(q))) return rc;
  if ((rc = resident_span(ctx, my_num, "consec", &k0, &k1))) return rc;
  const ResidentSet& r = ctx->resident;
  const uint64_t cs = (uint64_t)r.cs;
  return unit_resident<kUnitConsec>(
      ctx, k0, k1, 0,
      [&](DevState&, int32_t k, uint64_t*, uint64_t* res, void* slabs, uint32_t grid, hipStream_t s) {
        const uint64_t* const mask = r.masks[(size_t)k - 1].as<uint64_t>();
        return consec_launch(ctx, (uint64_t)(k - 1) * cs, cs, mask, q, res, slabs, grid, s);
      },
      dse_consec_merge, out);
}

extern "C" int32_t dse_consec_merge(const dse_consec* a, const dse_consec* b, dse_consec* out) {
  if (!a || !b || !out) return fail(DSE_EINVAL, "null consec result");
  if (int32_t rc = check_merge_adjacent(a->g_start, a->nbits, b->g_start)) return rc;
  if (a->q != b->q || a->q < 3 || a->q > DSE_CONSEC_MAX_MODULUS)
    return fail(DSE_EINVAL, "the results are of different moduli");
  if (int32_t rc = check_merge_end(b->g_start, b->nbits)) return rc;
  dse_consec r = *a;  // out may alias a or b
  r.nbits = a->nbits + b->nbits;
  r.primes = a->primes + b->primes;
  r.pairs = r.primes ? r.primes - 1 : 0;
  if (a->first_g == DSE_CONSEC_NONE) r.first_g = b->first_g;
  if (b->last_g != DSE_CONSEC_NONE) r.last_g = b->last_g;
  for (uint32_t i = 0; i < kConsecBins; ++i) r.counts[i] = a->counts[i] + b->counts[i];
  // the seam's pair: a's last entry and b's first, values 3 + 2 g below 2^63 + 3
  if (a->last_g != DSE_CONSEC_NONE && b->first_g != DSE_CONSEC_NONE) {
    const uint64_t q = a->q;
    r.counts[(3 + 2 * a->last_g) % q * DSE_CONSEC_MAX_MODULUS + (3 + 2 * b->first_g) % q] += 1;
  }
  *out = r;
  return DSE_OK;
}

extern "C" int32_t dse_debug_consec_host(const uint64_t* mask, uint64_t g_start, uint64_t nbits, uint32_t q,
                                         dse_consec* out) {
  if (!out) return fail(DSE_EINVAL, "null out");
  if (nbits && !mask) return fail(DSE_EINVAL, "null mask");
  if (reinterpret_cast<uintptr_t>(mask) & 7u) return fail(DSE_EINVAL, "mask is not 8-byte aligned");
  int32_t rc;
  if ((rc = consec_check(q))) return rc;
  if ((rc = check_mask_range("consec", g_start, nbits))) return rc;
  const MaskRange m = mask_range(mask, g_start, nbits);
  const uint32_t T = race_period(q), magic = consec_magic(T);
  const uint64_t comb = race_comb(T);
  // the main kernel's bins by position class; the bit-parallel body's counters stand apart, as its registers do
  uint64_t hist[kConsecBins] = {}, cnt[kConsecMaxModulus * kConsecMaxModulus] = {};
  uint64_t primes = 0, first = kConsecNone, carry = 0;
  uint32_t carry_cls = 0;
  // the main kernel's tile loop, one word at a time: the scan's result is the loop's carry
  const uint64_t ntiles = mask_tiles(nbits);
  uint32_t php = (uint32_t)(g_start % T);
  for (uint64_t t = 0; t < ntiles; ++t) {
    for (uint32_t tid = 0; tid < kMaskTileWords; ++tid) {
      const uint64_t wi = t * kMaskTileWords + tid;
      const uint64_t w = mask_word(m, wi);
      if (!w) continue;
      const uint32_t ph = consec_mod(php + tid * (64u % T), T, magic);
      primes += (uint64_t)__builtin_popcountll(w);
      if (T <= kConsecBitMaxT)
        consec_count_word<kConsecMaxModulus>(w, comb, T, ph, cnt);
      else
        consec_walk_word(w, T, magic, ph, [&](uint32_t c, uint32_t c2) { ++hist[c * kConsecStride + c2]; });
      const uint32_t f = (uint32_t)__builtin_ctzll(w);
      if (carry)
        ++hist[carry_cls * kConsecStride + consec_mod(ph + f, T, magic)];
      else
        first = wi * 64 + f;
      const uint32_t l1 = tid * 64u + (63u - (uint32_t)__builtin_clzll(w)) + 1u;  // tile position + 1 of the last prime
      carry = t * (uint64_t)kMaskTileBits + l1;
      carry_cls = consec_mod(php + l1 - 1u, T, magic);
    }
    php = race_phase_add(php, kMaskTileBits % T, T);
  }
  if (T <= kConsecBitMaxT)
    for (uint32_t c = 0; c < T; ++c)
      for (uint32_t c2 = 0; c2 < T; ++c2) hist[c * kConsecStride + c2] += cnt[c * kConsecMaxModulus + c2];
  // the closing kernel: position classes to residues, and the scalar members
  dse_consec r;
  std::memset(&r, 0, sizeof r);
  r.g_start = g_start;
  r.nbits = nbits;
  r.q = q;
  r.primes = primes;
  r.pairs = primes ? primes - 1 : 0;
  r.first_g = first == kConsecNone ? DSE_CONSEC_NONE : g_start + first;
  r.last_g = carry ? g_start + (carry - 1) : DSE_CONSEC_NONE;
  for (uint32_t a = 0; a < q; ++a) {
    const uint32_t c = race_class_pos(q, a);
    if (c == kRaceNoClass) continue;
    for (uint32_t b = 0; b < q; ++b) {
      const uint32_t c2 = race_class_pos(q, b);
      if (c2 != kRaceNoClass) r.counts[a * DSE_CONSEC_MAX_MODULUS + b] = hist[c * kConsecStride + c2];
    }
  }
  *out = r;
  return DSE_OK;
}
