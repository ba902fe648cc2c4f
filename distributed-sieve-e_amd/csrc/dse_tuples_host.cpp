// dse_tuples_host.cpp -- constellations as numbers, the host side (include/dse.h):
// the matches of a pattern in a device-resident mask become uint64 values on the
// device (dse_tuples.hip), in the caller's device buffer (dse_tuples_dev_async)
// or, through the slab pipeline of primes as numbers (rank_pipeline, rank_slabs),
// in a host buffer (dse_tuples_range, dse_tuples_resident);
// dse_debug_tuples_host runs the kernels' per-word body (dse_tuples_word.h) on
// the host.
#include <algorithm>

#include "dse_host.h"
#include "dse_primes_word.h"
#include "dse_tuples_word.h"

using namespace dse;

int32_t dse::tuples_check_pattern(uint32_t require, uint32_t forbid) {
  if (!(require & 1u)) return fail(DSE_EINVAL, "require has bit 0 clear");
  if (require & forbid) return fail(DSE_EINVAL, "require and forbid share a bit");
  return DSE_OK;
}

int32_t dse::tuples_check_above(const uint64_t* above, uint32_t above_shift, uint32_t above_bits) {
  if (above_bits > kTuplesMaxAbove) return fail(DSE_EINVAL, "above_bits above 31");
  if (above_shift > 63) return fail(DSE_EINVAL, "above_shift above 63");
  if (above_bits && !above) return fail(DSE_EINVAL, "null above with above_bits > 0");
  if (above_bits && (reinterpret_cast<uintptr_t>(above) & 7u)) return fail(DSE_EINVAL, "above is not 8-byte aligned");
  return DSE_OK;
}

int32_t dse::resident_above_check(dse_ctx* ctx, int32_t k0) {
  const ResidentSet& r = ctx->resident;
  if (k0 < r.P && (uint64_t)r.cs < kTuplesMaxAbove)
    return fail(DSE_EINVAL, "chunks of " + std::to_string(r.cs) + " candidates are shorter than the 31 a chunk sees of the next");
  return DSE_OK;
}

int32_t dse::resident_above(dse_ctx* ctx, DevState& d, int32_t k, uint64_t* head_slot, TuplePattern* p) {
  const ResidentSet& r = ctx->resident;
  const size_t nd = ctx->devs.size();
  const DevState& nd_dev = ctx->devs[(size_t)k % nd];
  const uint64_t* const head = r.masks[k].as<uint64_t>();
  p->above_shift = 0;
  p->above_bits = kTuplesMaxAbove;
  if (&nd_dev == &d) {
    p->above = head;  // the neighbour's mask is this device's: a pointer into it
  } else {
    // its first word into this device's scratch, on this device's stream
    HIP_TRY(nd_dev.device == d.device ? hipMemcpyAsync(head_slot, head, 8, hipMemcpyDeviceToDevice, d.stream)
                                      : hipMemcpyPeerAsync(head_slot, d.device, head, nd_dev.device, 8, d.stream));
    p->above = head_slot;
  }
  return DSE_OK;
}

namespace {

// the two launches on a mask that is ready in the stream's order
RankSource tuples_source(uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev, const TuplePattern& p) {
  return RankSource{
      nbits,
      [=](uint64_t first, uint64_t out_cap, unsigned long long* totals, void* sums, hipStream_t s) {
        return launch_tuples_scan(g_start, nbits, mask_dev, p, first, out_cap, totals, sums, s);
      },
      [=](uint64_t first, uint64_t* out, uint64_t out_cap, const void* sums, uint64_t t0, uint64_t tiles,
          hipStream_t s) {
        return launch_tuples_emit(g_start, nbits, mask_dev, p, first, out, out_cap, sums, t0, tiles, s);
      }};
}

}  // namespace

extern "C" int32_t dse_tuples_dev_async(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev,
                                        uint32_t require, uint32_t forbid, const uint64_t* above_dev,
                                        uint32_t above_shift, uint32_t above_bits, uint64_t first, uint64_t* out_dev,
                                        uint64_t out_cap, uint64_t* totals_dev, void* stream) {
  if (!ctx || !totals_dev) return fail(DSE_EINVAL, "null ctx or totals");
  if (nbits && !mask_dev) return fail(DSE_EINVAL, "null mask");
  int32_t rc;
  if ((rc = rank_check_out(out_dev, out_cap))) return rc;
  if (reinterpret_cast<uintptr_t>(out_dev) & 7u) return fail(DSE_EINVAL, "out_dev is not 8-byte aligned");
  if ((rc = tuples_check_pattern(require, forbid))) return rc;
  if ((rc = tuples_check_above(above_dev, above_shift, above_bits))) return rc;
  if ((rc = check_mask_range("tuples", g_start, nbits))) return rc;
  if ((rc = check_odd_range(g_start, nbits + above_bits))) return rc;
  DevState& d = ctx->devs[0];
  HIP_TRY(hipSetDevice(d.device));
  hipStream_t s = (hipStream_t)stream;
  const TuplePattern p{require, forbid, above_dev, above_shift, above_bits};
  return scratch_launch(d.primes_sums, primes_scratch_bytes(nbits), s, "tuples launch", [&](void* sums) {
    hipError_t e = launch_tuples_scan(g_start, nbits, mask_dev, p, first, out_cap,
                                      reinterpret_cast<unsigned long long*>(totals_dev), sums, s);
    if (e == hipSuccess)
      e = launch_tuples_emit(g_start, nbits, mask_dev, p, first, out_dev, out_cap, sums, 0, mask_tiles(nbits), s);
    return e;
  });
}

extern "C" int32_t dse_tuples_range(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, uint32_t require, uint32_t forbid,
                                    uint64_t first, uint64_t* out, uint64_t out_cap, uint64_t* total,
                                    uint64_t* written) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  int32_t rc;
  if ((rc = rank_check_out(out, out_cap))) return rc;
  if ((rc = tuples_check_pattern(require, forbid))) return rc;
  if ((rc = check_mask_range("tuples", g_start, nbits))) return rc;
  // the extended range: the candidates above the range are sieved with it, up to 31 of them; the
  // sieve's last candidate has the value 2^62 - 1, the odd index 2^61 - 2 (dse_sieve_odd_range's rule)
  const uint64_t top = (1ull << 61) - 1, end = g_start + nbits;
  const uint64_t ext = nbits && end < top ? std::min<uint64_t>(kTuplesMaxAbove, top - end) : 0;
  DevState& d = ctx->devs[0];
  if (nbits && (rc = sieve_range_host(ctx, d, g_start, nbits + ext, nullptr, nullptr, true))) return rc;
  HIP_TRY(hipSetDevice(d.device));
  // one scratch mask: the range's own mask, and `above` its bits from nbits on
  const uint64_t* const m = d.scratch_mask.as<uint64_t>();
  const TuplePattern p{require, forbid, ext ? m + (nbits >> 6) : nullptr, (uint32_t)(nbits & 63), (uint32_t)ext};
  return rank_pipeline(ctx, d, tuples_source(g_start, nbits, m, p), first, out, out_cap, total, written);
}

extern "C" int32_t dse_tuples_resident(dse_ctx* ctx, int32_t my_num, uint32_t require, uint32_t forbid, uint64_t first,
                                       uint64_t* out, uint64_t out_cap, uint64_t* total, uint64_t* written) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  int32_t rc;
  if ((rc = rank_check_out(out, out_cap))) return rc;
  if ((rc = tuples_check_pattern(require, forbid))) return rc;
  int32_t k0, k1;
  if ((rc = resident_span(ctx, my_num, "tuples", &k0, &k1))) return rc;
  if (total) *total = 0;
  if (written) *written = 0;
  const ResidentSet& r = ctx->resident;
  const uint64_t cs = (uint64_t)r.cs;
  if (!cs) return DSE_OK;
  // chunk k < P sees the first 31 candidates of chunk k + 1
  if ((rc = resident_above_check(ctx, k0))) return rc;

  const size_t nd = ctx->devs.size(), nc = (size_t)(k1 - k0 + 1);
  const uint64_t sum_bytes = primes_scratch_bytes(cs);
  std::vector<std::vector<int32_t>> chunks(nd);
  for (int32_t k = k0; k <= k1; ++k) chunks[(size_t)(k - 1) % nd].push_back(k);
  std::vector<char> acquired(nd, 0);
  std::vector<std::vector<unsigned long long>> dev_totals(nd);
  std::vector<RankSource> src(nc);
  std::vector<const void*> sums(nc);

  auto run = [&]() -> int32_t {
    // every chunk's size and scan launches, on its device's stream, before any is waited for. A
    // device's scratch: its chunks' tile sums | their totals | the head word of a neighbour's mask
    for (size_t i = 0; i < nd; ++i) {
      const uint32_t cnt = (uint32_t)chunks[i].size();
      if (!cnt) continue;
      DevState& d = ctx->devs[i];
      HIP_TRY(hipSetDevice(d.device));
      uint64_t *res, *heads;
      if (int32_t ra = result_acquire(d, d.primes_sums, cnt * sum_bytes, cnt, 2 * sizeof(uint64_t), cnt * 8ull, &res,
                                      &heads))
        return ra;
      acquired[i] = 1;
      for (uint32_t j = 0; j < cnt; ++j) {
        const int32_t k = chunks[i][j];
        TuplePattern p{require, forbid, nullptr, 0, 0};
        if (k < r.P)
          if (int32_t rv = resident_above(ctx, d, k, heads + j, &p)) return rv;
        const size_t c = (size_t)(k - k0);
        void* const s = static_cast<char*>(d.primes_sums.buf.ptr) + j * sum_bytes;
        src[c] = tuples_source((uint64_t)(k - 1) * cs, cs, r.masks[k - 1].as<uint64_t>(), p);
        sums[c] = s;
        HIP_TRY(src[c].scan(0, 0, reinterpret_cast<unsigned long long*>(res) + 2 * j, s, d.stream));
      }
      dev_totals[i].resize(2 * cnt);
      HIP_TRY(hipMemcpyAsync(dev_totals[i].data(), res, cnt * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
    }
    for (size_t i = 0; i < nd; ++i) {
      if (!acquired[i]) continue;
      HIP_TRY(hipSetDevice(ctx->devs[i].device));
      HIP_TRY(hipStreamSynchronize(ctx->devs[i].stream));
    }
    // the running totals cut the rank window per chunk
    std::vector<uint64_t> cnt_of(nc);
    for (size_t i = 0; i < nd; ++i)
      for (size_t j = 0; j < chunks[i].size(); ++j) cnt_of[(size_t)(chunks[i][j] - k0)] = dev_totals[i][2 * j];
    const uint64_t end = primes_window_end(first, out_cap);
    uint64_t before = 0, n_all = 0;
    for (size_t c = 0; c < nc; ++c) {
      const uint64_t lo = std::max(first, before), hi = std::min(end, before + cnt_of[c]);
      if (lo < hi) {
        DevState& d = ctx->devs[(size_t)(k0 + (int32_t)c - 1) % nd];
        HIP_TRY(hipSetDevice(d.device));
        if (int32_t rs = rank_slabs(ctx, d, src[c], sums[c], lo - before, hi - lo, out + (lo - first))) return rs;
        n_all += hi - lo;
      }
      before += cnt_of[c];
    }
    if (total) *total = before;
    if (written) *written = n_all;
    return DSE_OK;
  };
  rc = run();
  std::string msg = rc ? dse_last_error() : "";
  for (size_t i = 0; i < nd; ++i) {
    if (!acquired[i]) continue;
    DevState& d = ctx->devs[i];
    (void)hipSetDevice(d.device);
    if (rc) (void)hipStreamSynchronize(d.stream);  // dev_totals may still be a copy's target
    const hipError_t e = release_scratch(&d.primes_sums, d.stream);
    if (e != hipSuccess && !rc) {
      rc = DSE_EHIP;
      msg = std::string("release_scratch failed: ") + hipGetErrorString(e);
    }
  }
  return rc ? fail(rc, msg) : DSE_OK;
}

extern "C" int32_t dse_debug_tuples_host(const uint64_t* mask, uint64_t g_start, uint64_t nbits, uint32_t require,
                                         uint32_t forbid, const uint64_t* above, uint32_t above_shift,
                                         uint32_t above_bits, uint64_t first, uint64_t* out, uint64_t out_cap,
                                         uint64_t totals[2]) {
  if (!totals) return fail(DSE_EINVAL, "null totals");
  if (nbits && !mask) return fail(DSE_EINVAL, "null mask");
  int32_t rc;
  if ((rc = rank_check_out(out, out_cap))) return rc;
  if ((rc = tuples_check_pattern(require, forbid))) return rc;
  if ((rc = tuples_check_above(above, above_shift, above_bits))) return rc;
  if ((rc = check_mask_range("tuples", g_start, nbits))) return rc;
  if ((rc = check_odd_range(g_start, nbits + above_bits))) return rc;
  const TupleSrc s{mask_range(mask, g_start, nbits), above, above_shift, above_bits, require, forbid};
  const uint64_t end = primes_window_end(first, out_cap);
  // the kernels' tile bodies, one word at a time: the scan's result is the loop's running rank
  uint64_t rank = 0, n = 0;
  for (uint64_t wi = 0; wi < s.r.words; ++wi) {
    uint64_t bits = tuples_word(s, wi, tuples_visible_word(s, wi), (uint32_t)tuples_visible_word(s, wi + 1));
    uint64_t r0 = rank;
    rank += (uint64_t)__builtin_popcountll(bits);
    primes_word(bits, r0, g_start + wi * 64, first, end, [&](uint64_t rk, uint64_t v) {
      out[rk - first] = v;
      ++n;
    });
  }
  totals[0] = rank;
  totals[1] = n;
  return DSE_OK;
}
