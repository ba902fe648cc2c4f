// dse_primes_host.cpp -- primes as numbers, the host side (include/dse.h): a
// device-resident mask becomes uint64 prime values on the device
// (dse_primes.hip), in the caller's device buffer (dse_primes_dev_async) or, in
// slabs through pinned memory, in a host buffer (dse_primes_range,
// dse_primes_resident). The slab pipeline (rank_pipeline, rank_slabs) takes the
// two launches as a RankSource: dse_tuples_host.cpp runs it with its own.
#include <algorithm>
#include <cstring>

#include "dse_host.h"
#include "dse_primes_word.h"

using namespace dse;

namespace dse {

int32_t rank_check_out(const uint64_t* out, uint64_t out_cap) {
  if (out_cap && !out) return fail(DSE_EINVAL, "null out with a non-zero capacity");
  return DSE_OK;
}

int32_t rank_slabs(dse_ctx* ctx, DevState& d, const RankSource& src, const void* sums, uint64_t first, uint64_t n_out,
                   uint64_t* out) {
  if (!n_out) return DSE_OK;
  int32_t r;
  if ((r = ensure_slab_pipe(d, n_out > (1ull << 40) ? ~0ull : n_out * 8))) return r;
  SlabPipe& f = d.pipe;
  const uint64_t ntiles = mask_tiles(src.nbits);
  auto run = [&]() -> int32_t {
    std::vector<unsigned long long> hsums(ntiles + 1);
    HIP_TRY(hipMemcpyAsync(hsums.data(), sums, (ntiles + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));

    uint64_t slab = f.buf_bytes / 8;
    if (ctx->primes_slab_entries) slab = std::min(slab, ctx->primes_slab_entries);
    int prev_slot = -1;
    uint64_t prev_off = 0, prev_n = 0;
    auto take = [&](int slot, uint64_t off, uint64_t n) -> int32_t {  // once the slab's copy has run
      if (int32_t r2 = slab_wait(f, slot)) return r2;
      std::memcpy(out + off, f.hbuf[slot].ptr, n * 8);
      return DSE_OK;
    };
    int slot = 0;
    for (uint64_t off = 0; off < n_out; off += slab, slot ^= 1) {
      const uint64_t n = std::min(slab, n_out - off), ra = first + off, rb = ra + n;
      // tiles [t0, t1): the last tile that starts at or below rank ra, up to the first that starts at or above rb
      const uint64_t t0 = (uint64_t)(std::upper_bound(hsums.begin(), hsums.begin() + ntiles, ra) - hsums.begin()) - 1;
      const uint64_t t1 = (uint64_t)(std::lower_bound(hsums.begin(), hsums.begin() + ntiles, rb) - hsums.begin());
      if ((r = slab_reuse(f, slot, d.stream))) return r;
      HIP_TRY(src.emit(ra, f.dbuf[slot].as<uint64_t>(), n, sums, t0, t1 - t0, d.stream));
      if ((r = slab_send(f, slot, n * 8, d.stream))) return r;
      if (prev_slot >= 0 && (r = take(prev_slot, prev_off, prev_n))) return r;
      prev_slot = slot;
      prev_off = off;
      prev_n = n;
    }
    return take(prev_slot, prev_off, prev_n);
  };
  r = run();
  if (r) slab_drain(f, d.stream);
  return r;
}

int32_t rank_pipeline(dse_ctx* ctx, DevState& d, const RankSource& src, uint64_t first, uint64_t* out,
                      uint64_t out_cap, uint64_t* total, uint64_t* written) {
  if (total) *total = 0;
  if (written) *written = 0;
  if (!src.nbits) return DSE_OK;
  int32_t rc;
  const uint64_t want = out_cap > (1ull << 40) ? ~0ull : out_cap * 8;
  if ((rc = ensure_slab_pipe(d, want))) return rc;
  SlabPipe& f = d.pipe;
  bool acquired = false;

  auto run = [&]() -> int32_t {
    HIP_TRY(acquire_scratch_roomy(&d.primes_sums, primes_scratch_bytes(src.nbits), d.stream));
    acquired = true;
    void* const sums = d.primes_sums.buf.ptr;
    HIP_TRY(src.scan(first, out_cap, f.dtotals, sums, d.stream));
    HIP_TRY(hipMemcpyAsync(f.htotals, f.dtotals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    const uint64_t cnt = f.htotals[0], n_out = f.htotals[1];
    if (total) *total = cnt;
    if (int32_t r = rank_slabs(ctx, d, src, sums, first, n_out, out)) return r;
    if (written) *written = n_out;
    return DSE_OK;
  };
  rc = run();
  if (acquired) {
    const hipError_t e = release_scratch(&d.primes_sums, d.stream);
    if (e != hipSuccess && !rc) rc = fail(DSE_EHIP, std::string("release_scratch failed: ") + hipGetErrorString(e));
  }
  if (rc) slab_drain(f, d.stream);
  return rc;
}

}  // namespace dse

namespace {

// the extractor's two launches on a mask that is ready in the stream's order
RankSource primes_source(uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev) {
  return RankSource{
      nbits,
      [=](uint64_t first, uint64_t out_cap, unsigned long long* totals, void* sums, hipStream_t s) {
        return launch_primes_scan(g_start, nbits, mask_dev, first, out_cap, totals, sums, s);
      },
      [=](uint64_t first, uint64_t* out, uint64_t out_cap, const void* sums, uint64_t t0, uint64_t tiles,
          hipStream_t s) {
        return launch_primes_emit(g_start, nbits, mask_dev, first, out, out_cap, sums, t0, tiles, s);
      }};
}

}  // namespace

extern "C" int32_t dse_primes_dev_async(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev,
                                        uint64_t first, uint64_t* out_dev, uint64_t out_cap, uint64_t* totals_dev,
                                        void* stream) {
  if (!ctx || !totals_dev) return fail(DSE_EINVAL, "null ctx or totals");
  if (nbits && !mask_dev) return fail(DSE_EINVAL, "null mask");
  int32_t rc = rank_check_out(out_dev, out_cap);
  if (rc) return rc;
  if (reinterpret_cast<uintptr_t>(out_dev) & 7u) return fail(DSE_EINVAL, "out_dev is not 8-byte aligned");
  if ((rc = check_mask_range("primes", g_start, nbits))) return rc;
  DevState& d = ctx->devs[0];
  HIP_TRY(hipSetDevice(d.device));
  hipStream_t s = (hipStream_t)stream;
  return scratch_launch(d.primes_sums, primes_scratch_bytes(nbits), s, "primes launch", [&](void* sums) {
    hipError_t e = launch_primes_scan(g_start, nbits, mask_dev, first, out_cap,
                                      reinterpret_cast<unsigned long long*>(totals_dev), sums, s);
    if (e == hipSuccess)
      e = launch_primes_emit(g_start, nbits, mask_dev, first, out_dev, out_cap, sums, 0, mask_tiles(nbits), s);
    return e;
  });
}

extern "C" int32_t dse_primes_range(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, uint64_t first, uint64_t* out,
                                    uint64_t out_cap, uint64_t* total, uint64_t* written) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  int32_t rc = rank_check_out(out, out_cap);
  if (rc) return rc;
  if ((rc = check_mask_range("primes", g_start, nbits))) return rc;
  DevState& d = ctx->devs[0];
  if (nbits && (rc = sieve_range_host(ctx, d, g_start, nbits, nullptr, nullptr, true))) return rc;
  return rank_pipeline(ctx, d, primes_source(g_start, nbits, d.scratch_mask.as<uint64_t>()), first, out, out_cap, total,
                       written);
}

extern "C" int32_t dse_primes_resident(dse_ctx* ctx, int32_t my_num, uint64_t first, uint64_t* out,
                                       uint64_t out_cap, uint64_t* total, uint64_t* written) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  int32_t rc = rank_check_out(out, out_cap);
  if (rc) return rc;
  DevState* d;
  uint64_t* mask;
  if ((rc = find_resident(ctx, my_num, &d, &mask))) return rc;
  const uint64_t cs = (uint64_t)ctx->resident.cs;
  const uint64_t g_start = (uint64_t)(my_num - 1) * cs;
  if ((rc = check_mask_range("primes", g_start, cs))) return rc;
  HIP_TRY(hipSetDevice(d->device));
  return rank_pipeline(ctx, *d, primes_source(g_start, cs, mask), first, out, out_cap, total, written);
}

extern "C" int32_t dse_debug_primes_word(uint64_t word, uint64_t g_word_start, uint64_t rank0, uint64_t first,
                                         uint64_t cap, uint64_t out[64]) {
  if (!out) return fail(DSE_EINVAL, "null out");
  if (g_word_start > (1ull << 62) - 64 || rank0 > (1ull << 62))
    return fail(DSE_ERANGE, "word or rank beyond 2^62");
  uint32_t n = 0;
  uint64_t bits = word, rank = rank0;
  primes_word(bits, rank, g_word_start, first, primes_window_end(first, cap), [&](uint64_t, uint64_t v) { out[n++] = v; });
  return (int32_t)n;
}
