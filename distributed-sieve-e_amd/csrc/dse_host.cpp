// dse_host.cpp -- C-ABI host layer of libdse.so (include/dse.h): contexts,
// chunk geometry, the base table and its sharing, collectives, the sieve entry
// points, debug options and stats, and what the other host units share (range
// and residency checks, scratch growth, the result scratch and per-device fan-out
// of resident chunks, the two-slot slab pipe). The finish side is
// dse_finish_host.cpp, primes as numbers dse_primes_host.cpp, statistics
// dse_stats_host.cpp, rank and select dse_query_host.cpp, Goldbach dse_goldbach_host.cpp,
// residue classes and races dse_race_host.cpp.
//
// Replaces the reference's orchestration of the hot path:
//   spread-work (sieve.clj:15-34)            -> dse_spread_work (exact int64)
//   gen-table + sieve-e (sieve.clj:9-172)    -> dse_sieve_chunk / dse_sieve_all
//   per-prime [mi ps p] relay through the
//     lead (sieve.clj:139, core.clj:118-134) -> one RCCL broadcast of base primes
//   (no result gather in the reference)      -> RCCL all-reduce of counts
//   finish (sieve.clj:82-108)                -> dse_write_primes_file (host), or
//                                               dse_finish_resident_file / dse_finish_range_file
//                                               (text formatted on the device, dse_finish.hip)
#include <algorithm>
#include <cmath>
#include <cstring>

#include "dse_expand_bits.h"
#include "dse_finish_fmt.h"
#include "dse_host.h"

namespace {
thread_local std::string g_err;
thread_local int32_t g_code = DSE_OK;
}  // namespace

namespace dse {

int32_t fail(int32_t code, const std::string& msg) {
  g_err = msg;
  g_code = code;
  return code;
}

hipError_t free_buf(Buf* b) {
  if (!b->ptr) return hipSuccess;
  const hipError_t e = b->pinned ? hipHostFree(b->ptr) : hipFree(b->ptr);
  if (e != hipSuccess) return e;
  b->ptr = nullptr;
  b->bytes = 0;
  return hipSuccess;
}

hipError_t grow_buf(Buf* b, uint64_t bytes) {
  if (b->bytes >= bytes) return hipSuccess;
  hipError_t e = free_buf(b);
  if (e == hipSuccess)
    e = b->pinned ? hipHostMalloc(&b->ptr, bytes, hipHostMallocDefault) : hipMalloc(&b->ptr, bytes);
  if (e == hipSuccess) b->bytes = bytes;
  return e;
}

hipError_t acquire_scratch(StreamScratch* s, uint64_t bytes, hipStream_t stream) {
  hipError_t e;
  if (!s->done && (e = hipEventCreateWithFlags(&s->done, hipEventDisableTiming)) != hipSuccess) return e;
  if (s->buf.bytes < bytes) {  // the old buffer is freed: wait for its last user on the host
    if (s->used && (e = hipEventSynchronize(s->done)) != hipSuccess) return e;
    s->used = false;
    return grow_buf(&s->buf, bytes);
  }
  return s->used ? hipStreamWaitEvent(stream, s->done, 0) : hipSuccess;
}

hipError_t acquire_scratch_roomy(StreamScratch* s, uint64_t need, hipStream_t stream) {
  return acquire_scratch(s, s->buf.bytes >= need ? need : std::max<uint64_t>(need + need / 2, 1ull << 16), stream);
}

hipError_t release_scratch(StreamScratch* s, hipStream_t stream) {
  const hipError_t e = hipEventRecord(s->done, stream);
  if (e == hipSuccess) s->used = true;
  return e;
}

hipError_t free_scratch(StreamScratch* s) {
  const hipError_t e = s->used ? hipEventSynchronize(s->done) : hipSuccess;  // the last user may still read it
  const hipError_t f = free_buf(&s->buf);
  const hipError_t g = s->done ? hipEventDestroy(s->done) : hipSuccess;
  s->done = nullptr;
  s->used = false;
  return e != hipSuccess ? e : f != hipSuccess ? f : g;
}

int32_t chunk_geometry(int64_t n, int32_t P, int64_t* cs, int64_t* nums_out) {
  if (P < 1) return fail(DSE_EINVAL, "num-comps must be >= 1");
  if (n < 0) return fail(DSE_EINVAL, "n must be >= 0");
  const int64_t nums = n >= 1 ? (n - 1) / 2 : 0;
  *cs = nums / P;
  if (nums_out) *nums_out = nums;
  return DSE_OK;
}

int32_t check_odd_range(uint64_t g_start, uint64_t nbits) {
  if (g_start > (1ull << 62) || nbits > (1ull << 62) - g_start)
    return fail(DSE_ERANGE, "odd-index range beyond 2^62");
  return DSE_OK;
}

int32_t check_mask_range(const char* what, uint64_t g_start, uint64_t nbits) {
  if (int32_t rc = check_odd_range(g_start, nbits)) return rc;
  if (nbits > (1ull << 44)) return fail(DSE_ERANGE, std::string(what) + " range above 2^44 candidates in one call");
  return DSE_OK;
}

int32_t check_resident(dse_ctx* ctx, int32_t my_num, bool one_chunk) {
  const ResidentSet& r = ctx->resident;
  if (!r.valid || my_num < 0 || my_num > r.P || (one_chunk && !my_num))
    return fail(DSE_EINVAL, "chunk " + std::to_string(my_num) + " is not resident");
  return DSE_OK;
}

int32_t find_resident(dse_ctx* ctx, int32_t my_num, DevState** d, uint64_t** mask) {
  if (int32_t rc = check_resident(ctx, my_num, true)) return rc;
  *d = &ctx->devs[(size_t)(my_num - 1) % ctx->devs.size()];
  *mask = ctx->resident.masks[my_num - 1].as<uint64_t>();
  return DSE_OK;
}

int32_t resident_span(dse_ctx* ctx, int32_t my_num, const char* what, int32_t* k0, int32_t* k1) {
  if (int32_t rc = check_resident(ctx, my_num, false)) return rc;
  const ResidentSet& r = ctx->resident;
  *k0 = my_num ? my_num : 1;
  *k1 = my_num ? my_num : r.P;
  return check_mask_range(what, (uint64_t)(*k1 - 1) * (uint64_t)r.cs, (uint64_t)r.cs);
}

int32_t result_acquire(DevState& d, StreamScratch& s, uint64_t slab_bytes, uint32_t nres, uint64_t res_bytes,
                       uint64_t extra_bytes, uint64_t** res, uint64_t** extra) {
  HIP_TRY(acquire_scratch_roomy(&s, slab_bytes + nres * res_bytes + extra_bytes, d.stream));
  char* const p = static_cast<char*>(s.buf.ptr) + slab_bytes;
  *res = reinterpret_cast<uint64_t*>(p);
  if (extra) *extra = reinterpret_cast<uint64_t*>(p + nres * res_bytes);
  return DSE_OK;
}

int32_t result_collect(DevState& d, StreamScratch& s, const char* what, const uint64_t* res, uint64_t n, void* out) {
  hipError_t e = hipMemcpyAsync(out, res, n, hipMemcpyDeviceToHost, d.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
  const hipError_t r = release_scratch(&s, d.stream);
  if (e == hipSuccess) e = r;
  if (e != hipSuccess) return fail(DSE_EHIP, std::string(what) + " copy failed: " + hipGetErrorString(e));
  return DSE_OK;
}

int32_t launch_rc(const SlabUnitDesc& u, hipError_t e) {
  if (e != hipSuccess) return fail(DSE_EHIP, std::string(u.name) + " launch failed: " + hipGetErrorString(e));
  return DSE_OK;
}

int32_t check_dev_args(const dse_ctx* ctx, uint64_t nbits, const void* mask_dev, const void* out_dev, const char* out,
                       bool mask_aligned) {
  if (!ctx || !out_dev) return fail(DSE_EINVAL, std::string("null ctx or ") + out);
  if (nbits && !mask_dev) return fail(DSE_EINVAL, "null mask");
  if (reinterpret_cast<uintptr_t>(out_dev) & 7u)
    return fail(DSE_EINVAL, std::string(out) + "_dev is not 8-byte aligned");
  if (mask_aligned && (reinterpret_cast<uintptr_t>(mask_dev) & 7u))
    return fail(DSE_EINVAL, "mask_dev is not 8-byte aligned");
  return DSE_OK;
}

int32_t check_merge_adjacent(uint64_t a_g, uint64_t a_nbits, uint64_t b_g) {
  if (a_g + a_nbits != b_g || a_g > b_g) return fail(DSE_EINVAL, "the ranges are not adjacent");
  return DSE_OK;
}

int32_t check_merge_end(uint64_t b_g, uint64_t b_nbits) {
  if (b_g > (1ull << 62) || b_nbits > (1ull << 62) - b_g) return fail(DSE_ERANGE, "merged range beyond 2^62");
  return DSE_OK;
}

int32_t resident_fanout(dse_ctx* ctx, int32_t k0, int32_t k1, const FanEnqueue& enqueue, const FanCollect& collect) {
  const size_t nd = ctx->devs.size();
  std::vector<std::vector<int32_t>> chunks(nd);
  for (int32_t k = k0; k <= k1; ++k) chunks[(size_t)(k - 1) % nd].push_back(k);
  // every device's launches are enqueued on its stream before any result is waited for
  std::vector<char> acquired(nd, 0);
  int32_t rc = DSE_OK;
  for (size_t i = 0; i < nd && !rc; ++i) {
    if (chunks[i].empty()) continue;
    DevState& d = ctx->devs[i];
    bool a = false;
    rc = hipSetDevice(d.device) == hipSuccess ? enqueue(i, d, chunks[i], &a) : fail(DSE_EHIP, "hipSetDevice failed");
    acquired[i] = a;
  }
  std::string msg = rc ? g_err : std::string();
  for (size_t i = 0; i < nd; ++i) {  // collect what was enqueued, also after a failure: the scratch must be released
    if (!acquired[i]) continue;
    DevState& d = ctx->devs[i];
    (void)hipSetDevice(d.device);
    const int32_t r = collect(i, d, chunks[i]);
    if (r && !rc) {
      rc = r;
      msg = g_err;
    }
  }
  return rc ? fail(rc, msg) : DSE_OK;  // the first failure, whatever a collect behind it said
}

int32_t ensure_slab_pipe(DevState& d, uint64_t want) {
  SlabPipe& p = d.pipe;
  if (!p.copy) HIP_TRY(hipStreamCreateWithFlags(&p.copy, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) {
    if (!p.ready_ev[i]) HIP_TRY(hipEventCreateWithFlags(&p.ready_ev[i], hipEventDisableTiming));
    if (!p.copy_ev[i]) HIP_TRY(hipEventCreateWithFlags(&p.copy_ev[i], hipEventDisableTiming));
    p.pending[i] = false;  // every earlier call has drained both streams before it returned
  }
  if (!p.dtotals) HIP_TRY(hipMalloc(&p.dtotals, 4 * sizeof(unsigned long long)));
  if (!p.htotals) HIP_TRY(hipHostMalloc(&p.htotals, 4 * sizeof(unsigned long long), hipHostMallocDefault));
  want = std::min(std::max(want, kSlabBufMin), kSlabBufMax);
  if (p.buf_bytes >= want) return DSE_OK;
  p.buf_bytes = 0;
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(grow_buf(&p.dbuf[i], want));
    HIP_TRY(grow_buf(&p.hbuf[i], want));
  }
  p.buf_bytes = want;
  return DSE_OK;
}

int32_t slab_reuse(SlabPipe& p, int s, hipStream_t producer) {
  if (p.pending[s]) HIP_TRY(hipStreamWaitEvent(producer, p.copy_ev[s], 0));
  return DSE_OK;
}

int32_t slab_send(SlabPipe& p, int s, uint64_t bytes, hipStream_t producer) {
  HIP_TRY(hipEventRecord(p.ready_ev[s], producer));
  HIP_TRY(hipStreamWaitEvent(p.copy, p.ready_ev[s], 0));
  if (bytes) HIP_TRY(hipMemcpyAsync(p.hbuf[s].ptr, p.dbuf[s].ptr, bytes, hipMemcpyDeviceToHost, p.copy));
  HIP_TRY(hipEventRecord(p.copy_ev[s], p.copy));
  p.pending[s] = true;
  return DSE_OK;
}

int32_t slab_wait(SlabPipe& p, int s) {
  HIP_TRY(hipEventSynchronize(p.copy_ev[s]));
  p.pending[s] = false;
  return DSE_OK;
}

void slab_drain(SlabPipe& p, hipStream_t producer) {
  (void)hipStreamSynchronize(producer);
  if (p.copy) (void)hipStreamSynchronize(p.copy);
}

void free_slab_pipe(SlabPipe& p) {
  if (p.copy) (void)hipStreamSynchronize(p.copy);
  for (int i = 0; i < 2; ++i) {
    (void)free_buf(&p.dbuf[i]);
    (void)free_buf(&p.hbuf[i]);
    if (p.ready_ev[i]) (void)hipEventDestroy(p.ready_ev[i]);
    if (p.copy_ev[i]) (void)hipEventDestroy(p.copy_ev[i]);
  }
  if (p.dtotals) (void)hipFree(p.dtotals);
  if (p.htotals) (void)hipHostFree(p.htotals);
  if (p.copy) (void)hipStreamDestroy(p.copy);
  p = SlabPipe();
}

}  // namespace dse

using namespace dse;

namespace {

// Upper bound on the number of odd primes <= x (Rosser-Schoenfeld
// pi(x) < 1.25506 x / ln x for x > 1), padded.
uint32_t prime_cap(uint64_t x) {
  if (x < 100) return 64;
  double b = 1.25506 * (double)x / std::log((double)x);
  return (uint32_t)b + 64;
}

int32_t build_table(DevState& d, uint64_t limit) {
  if (limit > kBigBaseLimitMax)
    return fail(DSE_ERANGE, "base-prime limit " + std::to_string(limit) + " above the supported " +
                                std::to_string(kBigBaseLimitMax));
  HIP_TRY(grow_buf(&d.table, dse_base_table_bytes(limit)));
  HIP_TRY(launch_base_primes_big(limit, d.table.ptr, prime_cap(limit), d.num_cus, d.stream));
  return DSE_OK;
}

// Enqueue a copy of the sticky bucket-overflow flag on d.stream (before the
// caller's stream sync); check_flag after the sync reports and clears it.
// d.stream first waits for the last bucketed pass on the context's scratch,
// whatever stream it ran on (an async pass on a user stream may still be
// running: its overflow must neither be reported as this call's nor be
// cleared before it is written).
int32_t fetch_flag(DevState& d, uint32_t* h) {
  *h = 0;
  if (!d.scratch.flag) return DSE_OK;
  if (d.scratch.used) HIP_TRY(hipStreamWaitEvent(d.stream, d.scratch.done, 0));
  HIP_TRY(hipMemcpyAsync(h, d.scratch.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
  return DSE_OK;
}

int32_t check_flag(DevState& d, uint32_t h) {
  if (!h) return DSE_OK;
  HIP_TRY(hipMemsetAsync(d.scratch.flag, 0, sizeof(uint32_t), d.stream));
  HIP_TRY(hipStreamSynchronize(d.stream));
  return fail(DSE_EINTERNAL, "bucketed pass exceeded its entry capacity on device " + std::to_string(d.device) +
                                 "; the count and mask of this call are not valid");
}

// One device (the current one): fetch the flag, drain d.stream, check the flag.
int32_t sync_and_check(DevState& d) {
  int32_t rc;
  uint32_t hf;
  if ((rc = fetch_flag(d, &hf))) return rc;
  HIP_TRY(hipStreamSynchronize(d.stream));
  return check_flag(d, hf);
}

// Prologue of the multi-device calls: on every device a table buffer for
// `limit` and `nc` counts, zeroed on its stream.
int32_t prepare_devices(dse_ctx* ctx, uint64_t limit, uint64_t nc) {
  for (DevState& d : ctx->devs) {
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(grow_buf(&d.table, dse_base_table_bytes(limit)));
    HIP_TRY(grow_buf(&d.counts, nc * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(d.counts.ptr, 0, nc * sizeof(unsigned long long), d.stream));
  }
  return DSE_OK;
}

int32_t allreduce_counts(dse_ctx* ctx, uint64_t n);

// Epilogue of the multi-device calls: all-reduce the `nc` counts, copy device
// 0's to h, then every device's overflow flag: all fetched and every stream
// drained before the first is checked.
int32_t collect_counts(dse_ctx* ctx, uint64_t nc, unsigned long long* h) {
  int32_t rc;
  if ((rc = allreduce_counts(ctx, nc))) return rc;
  DevState& r = ctx->devs[0];
  HIP_TRY(hipSetDevice(r.device));
  HIP_TRY(hipMemcpyAsync(h, r.counts.ptr, nc * sizeof(unsigned long long), hipMemcpyDeviceToHost, r.stream));
  std::vector<uint32_t> hf(ctx->devs.size());
  for (size_t i = 0; i < hf.size(); ++i) {
    HIP_TRY(hipSetDevice(ctx->devs[i].device));
    if ((rc = fetch_flag(ctx->devs[i], &hf[i]))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->devs[i].stream));
  }
  for (size_t i = 0; i < hf.size(); ++i) {
    HIP_TRY(hipSetDevice(ctx->devs[i].device));
    if ((rc = check_flag(ctx->devs[i], hf[i]))) return rc;
  }
  return DSE_OK;
}

int32_t free_resident(dse_ctx* ctx) {
  ResidentSet& r = ctx->resident;
  r.valid = false;
  for (size_t k = 0; k < r.masks.size(); ++k) {
    HIP_TRY(hipSetDevice(ctx->devs[k % ctx->devs.size()].device));
    HIP_TRY(free_buf(&r.masks[k]));
    if (k < r.index.size()) HIP_TRY(free_buf(&r.index[k]));  // every query call has drained its stream
  }
  r.masks.clear();
  r.index.clear();
  r.indexed.clear();
  return DSE_OK;
}

// The resident set of (n, P): kept when the last successful call was for the
// same (n, P) (the same chunk map and mask sizes), otherwise replaced. Valid
// only once every mask is allocated; a failure leaves no masks behind.
int32_t ensure_resident(dse_ctx* ctx, int64_t n, int32_t P, int64_t cs) {
  ResidentSet& r = ctx->resident;
  if (r.valid && r.n == n && r.P == P) return DSE_OK;
  int32_t rc;
  if ((rc = free_resident(ctx))) return rc;
  r.n = n;
  r.P = P;
  r.cs = cs;
  r.words = ((uint64_t)cs + 63) / 64;
  r.masks.assign((size_t)P, Buf());
  r.index.assign((size_t)P, Buf());
  r.indexed.assign((size_t)P, 0);
  r.total.assign((size_t)P, 0);
  r.first.assign((size_t)P, DSE_QUERY_NONE);
  r.last.assign((size_t)P, DSE_QUERY_NONE);
  for (int32_t k = 0; k < P; ++k) {
    hipError_t e = hipSetDevice(ctx->devs[(size_t)k % ctx->devs.size()].device);
    if (e == hipSuccess) e = grow_buf(&r.masks[k], r.words * 8);
    if (e != hipSuccess) {
      (void)free_resident(ctx);
      return fail(DSE_EHIP, std::string("hipMalloc of a resident mask failed: ") + hipGetErrorString(e));
    }
  }
  r.valid = true;
  return DSE_OK;
}

int32_t init_dev(DevState& d, int device) {
  d.device = device;
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  d.num_cus = prop.multiProcessorCount;
  HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
  return DSE_OK;
}

// Start of a context constructor: clear the thread's error, count the visible devices.
int visible_devices() {
  g_err.clear();
  g_code = DSE_OK;
  return dse_device_count();
}

// A context of n DevStates on devices first, first + 1, ...; logical: all on
// `first`, with the events of the copy collectives. Null (the error set, the
// context destroyed) when a device cannot be set up.
dse_ctx* make_ctx(int n, int first, bool logical) {
  dse_ctx* ctx = new dse_ctx();
  ctx->logical = logical;
  ctx->devs.resize(n);
  bool ok = true;
  for (int i = 0; i < n && ok; ++i) {
    DevState& d = ctx->devs[i];
    ok = init_dev(d, logical ? first : first + i) == DSE_OK &&
         (!logical || hipEventCreateWithFlags(&d.xev, hipEventDisableTiming) == hipSuccess);
  }
  ok = ok && (!logical || hipEventCreateWithFlags(&ctx->lg_done, hipEventDisableTiming) == hipSuccess);
  if (ok) return ctx;
  if (!g_code) fail(DSE_EHIP, "event creation failed");
  dse_destroy(ctx);
  return nullptr;
}

// Base primes once, on device 0, then an RCCL broadcast of the primes (the
// table's header + p[]) to the other devices, which derive their Barrett
// factors and wheel offsets locally: the reference's prime broadcast
// (sieve.clj:139, core.clj:94-95,126) done once. Every device's table buffer
// must already hold dse_base_table_bytes(limit) bytes.
// A table whose primes exceed the broadcast cap (dse_base_table_broadcast_bytes:
// the window's 203 MB) is built on every device instead, each on its own
// stream: 0.2 ms of local work against 0.7-2 ms of broadcast (DESIGN.md
// section 5). The test option table_broadcast_max_bytes moves the cap.
int32_t share_table(dse_ctx* ctx, uint64_t limit) {
  int32_t rc;
  const int nd = (int)ctx->devs.size();
  const uint64_t pbytes = dse_base_table_prime_bytes(limit);
  const uint64_t cap = ctx->opts.table_bcast_max ? ctx->opts.table_bcast_max : DSE_TABLE_BROADCAST_MAX_BYTES;
  if ((nd > 1 || ctx->rccl_single) && pbytes > cap) {
    for (int i = 0; i < nd; ++i) {
      HIP_TRY(hipSetDevice(ctx->devs[i].device));
      if ((rc = build_table(ctx->devs[i], limit))) return rc;
    }
    ctx->table_local_builds += nd;
    return DSE_OK;
  }
  HIP_TRY(hipSetDevice(ctx->devs[0].device));
  if ((rc = build_table(ctx->devs[0], limit))) return rc;
  if (nd == 1 && !ctx->rccl_single) return DSE_OK;
  if (ctx->logical) {  // the broadcast as copies from device 0's table, each on its device's stream
    DevState& r = ctx->devs[0];
    HIP_TRY(hipEventRecord(r.xev, r.stream));
    for (int i = 1; i < nd; ++i) {
      DevState& d = ctx->devs[i];
      HIP_TRY(hipStreamWaitEvent(d.stream, r.xev, 0));
      HIP_TRY(hipMemcpyAsync(d.table.ptr, r.table.ptr, pbytes, hipMemcpyDeviceToDevice, d.stream));
      HIP_TRY(launch_wheel_offsets(d.table.ptr, d.num_cus, d.stream, prime_cap(limit)));
    }
    return DSE_OK;
  }
  NCCL_TRY(ncclGroupStart());
  for (int i = 0; i < nd; ++i) {
    DevState& d = ctx->devs[i];
    NCCL_TRY(ncclBroadcast(ctx->devs[0].table.ptr, d.table.ptr, pbytes, ncclUint8, 0, ctx->comms[i], d.stream));
  }
  NCCL_TRY(ncclGroupEnd());
  ctx->rccl_calls += nd;
  for (int i = 1; i < nd; ++i) {
    DevState& d = ctx->devs[i];
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(launch_wheel_offsets(d.table.ptr, d.num_cus, d.stream, prime_cap(limit)));
  }
  return DSE_OK;
}

// Sum `n` uint64 counts over the devices with an RCCL all-reduce (in place).
int32_t allreduce_counts(dse_ctx* ctx, uint64_t n) {
  if (ctx->devs.size() < 2 && !ctx->rccl_single) return DSE_OK;
  const size_t row = n * sizeof(unsigned long long);
  if (ctx->logical) {  // gather + sum on device 0's stream, then every device copies the sum back
    const uint32_t nd = (uint32_t)ctx->devs.size();
    DevState& r = ctx->devs[0];
    HIP_TRY(hipSetDevice(r.device));
    // every earlier call has drained the streams that used the two buffers
    HIP_TRY(grow_buf(&ctx->lg_stage, nd * row));
    HIP_TRY(grow_buf(&ctx->lg_sum, row));
    unsigned long long* stage = ctx->lg_stage.as<unsigned long long>();
    for (uint32_t i = 0; i < nd; ++i) {
      DevState& d = ctx->devs[i];
      if (i) {
        HIP_TRY(hipEventRecord(d.xev, d.stream));
        HIP_TRY(hipStreamWaitEvent(r.stream, d.xev, 0));
      }
      HIP_TRY(hipMemcpyAsync(stage + i * n, d.counts.ptr, row, hipMemcpyDeviceToDevice, r.stream));
    }
    HIP_TRY(launch_sum_rows(stage, nd, (uint32_t)n, ctx->lg_sum.as<unsigned long long>(), r.stream));
    HIP_TRY(hipEventRecord(ctx->lg_done, r.stream));
    for (uint32_t i = 0; i < nd; ++i) {
      DevState& d = ctx->devs[i];
      if (i) HIP_TRY(hipStreamWaitEvent(d.stream, ctx->lg_done, 0));
      HIP_TRY(hipMemcpyAsync(d.counts.ptr, ctx->lg_sum.ptr, row, hipMemcpyDeviceToDevice, d.stream));
    }
    return DSE_OK;
  }
  NCCL_TRY(ncclGroupStart());
  for (size_t i = 0; i < ctx->devs.size(); ++i) {
    DevState& d = ctx->devs[i];
    NCCL_TRY(ncclAllReduce(d.counts.ptr, d.counts.ptr, n, ncclUint64, ncclSum, ctx->comms[i], d.stream));
  }
  NCCL_TRY(ncclGroupEnd());
  ctx->rccl_calls += (int64_t)ctx->devs.size();
  return DSE_OK;
}

// what dse_base_primes_dev_async and dse_base_table_finish_dev_async refuse
int32_t check_table_args(dse_ctx* ctx, uint64_t limit, void* table_dev, uint64_t table_bytes) {
  if (!ctx || !table_dev) return fail(DSE_EINVAL, "null ctx or table");
  if (table_bytes < dse_base_table_bytes(limit)) return fail(DSE_EINVAL, "table buffer too small");
  if (limit > kBigBaseLimitMax) return fail(DSE_ERANGE, "base-prime limit above the supported maximum");
  return DSE_OK;
}

// The plain numeric knobs of dse_debug_set_option: a value outside [min, max]
// is refused with "<name> <bad>".
template <uint32_t SieveOpts::*F>
void set_opt32(dse_ctx* c, int64_t v) {
  c->opts.*F = (uint32_t)v;
}
constexpr int64_t kU32Max = 0xFFFFFFFFll, kI64Max = INT64_MAX;
const struct {
  const char* name;
  int64_t min, max;
  const char* bad;
  void (*set)(dse_ctx*, int64_t);
} kNumOpts[] = {
    {"bucket_pass_segments", 0, kU32Max, "out of range", set_opt32<&SieveOpts::bucket_pass_segs>},
    {"bucket_split_log2", 0, 63, "out of range", set_opt32<&SieveOpts::bucket_split_log2>},
    {"wheel_geometry", 0, 2, "must be 0, 1 or 2", set_opt32<&SieveOpts::wheel_geometry>},
    {"bucket_k0_divisor", 0, kU32Max, "out of range", set_opt32<&SieveOpts::bucket_k0_div>},
    {"scratch_poison", 0, 1, "must be 0 or 1", set_opt32<&SieveOpts::scratch_poison>},
    {"bucket_cap_divisor", 0, kU32Max, "out of range", set_opt32<&SieveOpts::bucket_cap_div>},
    {"table_broadcast_max_bytes", 0, kI64Max, "must be >= 0",
     [](dse_ctx* c, int64_t v) { c->opts.table_bcast_max = (uint64_t)v; }},
    {"finish_slab_words", 0, kI64Max, "must be >= 0",
     [](dse_ctx* c, int64_t v) { c->finish_slab_words = (uint64_t)v; }},
    {"primes_slab_entries", 0, kI64Max, "must be >= 0",
     [](dse_ctx* c, int64_t v) { c->primes_slab_entries = (uint64_t)v; }},
    {"query_grid", 0, (int64_t)kQueryMaxGrid, "out of range", [](dse_ctx* c, int64_t v) { c->query_grid = (uint32_t)v; }},
    {"consec_flush_tiles", 0, (int64_t)kConsecFlushTiles, "out of range",
     [](dse_ctx* c, int64_t v) { c->consec_flush_tiles = (uint32_t)v; }},
    {"consec_body", 0, 2, "must be 0, 1 or 2", [](dse_ctx* c, int64_t v) { c->consec_body = (uint32_t)v; }},
};

}  // namespace

int32_t dse::sieve_range_host(dse_ctx* ctx, DevState& d, uint64_t g0, uint64_t nbits, uint64_t* mask_or_null,
                              uint64_t* count, bool keep_dev) {
  int32_t rc;
  HIP_TRY(hipSetDevice(d.device));
  const uint64_t words = (nbits + 63) / 64;
  ctx->plan = PlanStats();
  if ((rc = build_table(d, dse_base_limit_for_range(g0, nbits)))) return rc;
  HIP_TRY(grow_buf(&d.counts, sizeof(unsigned long long)));
  const bool dev_mask = mask_or_null || keep_dev;
  // every earlier call that used the mask has drained d.stream
  if (dev_mask) HIP_TRY(grow_buf(&d.scratch_mask, words * 8));
  unsigned long long* counts = d.counts.as<unsigned long long>();
  HIP_TRY(hipMemsetAsync(counts, 0, sizeof(unsigned long long), d.stream));
  HIP_TRY(launch_sieve_range(d.table.ptr, g0, nbits, dev_mask ? d.scratch_mask.as<uint32_t>() : nullptr, counts,
                             d.num_cus, d.stream, &d.scratch, &ctx->opts, &ctx->plan));
  unsigned long long c = 0;
  HIP_TRY(hipMemcpyAsync(&c, counts, sizeof(c), hipMemcpyDeviceToHost, d.stream));
  if (mask_or_null && words)
    HIP_TRY(hipMemcpyAsync(mask_or_null, d.scratch_mask.ptr, words * 8, hipMemcpyDeviceToHost, d.stream));
  if ((rc = sync_and_check(d))) return rc;
  if (count) *count = c;
  return DSE_OK;
}

extern "C" {

const char* dse_version(void) { return "dse 0.1 gfx950"; }

const char* dse_last_error(void) { return g_err.c_str(); }

int32_t dse_last_status(void) { return g_code; }

int32_t dse_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

dse_ctx* dse_init(int32_t num_gpus) {
  const int avail = visible_devices();
  if (avail < 1) {
    fail(DSE_EHIP, "no HIP device visible");
    return nullptr;
  }
  if (num_gpus <= 0) num_gpus = avail;
  if (num_gpus > avail) {
    fail(DSE_EINVAL, "asked for " + std::to_string(num_gpus) + " GPUs, " + std::to_string(avail) + " visible");
    return nullptr;
  }
  dse_ctx* ctx = make_ctx(num_gpus, 0, false);
  if (ctx && num_gpus > 1) {
    ctx->comms.resize(num_gpus);
    std::vector<int> ids(num_gpus);
    for (int i = 0; i < num_gpus; ++i) ids[i] = i;
    ncclResult_t r = ncclCommInitAll(ctx->comms.data(), num_gpus, ids.data());
    if (r != ncclSuccess) {
      fail(DSE_ENCCL, std::string("ncclCommInitAll: ") + ncclGetErrorString(r));
      ctx->comms.clear();
      dse_destroy(ctx);
      return nullptr;
    }
  }
  return ctx;
}

dse_ctx* dse_init_device(int32_t device) {
  const int avail = visible_devices();
  if (device < 0 || device >= avail) {
    fail(DSE_EINVAL, "device " + std::to_string(device) + " not visible");
    return nullptr;
  }
  return make_ctx(1, device, false);
}

dse_ctx* dse_debug_init_logical(int32_t num_logical) {
  if (visible_devices() < 1) {
    fail(DSE_EHIP, "no HIP device visible");
    return nullptr;
  }
  if (num_logical < 1 || num_logical > 64) {
    fail(DSE_EINVAL, "num_logical must be in 1..64");
    return nullptr;
  }
  return make_ctx(num_logical, 0, true);
}

void dse_destroy(dse_ctx* ctx) {
  if (!ctx) return;
  for (auto& c : ctx->comms) ncclCommDestroy(c);
  (void)free_resident(ctx);
  if (ctx->logical && !ctx->devs.empty()) {
    (void)hipSetDevice(ctx->devs[0].device);
    (void)free_buf(&ctx->lg_stage);
    (void)free_buf(&ctx->lg_sum);
    if (ctx->lg_done) (void)hipEventDestroy(ctx->lg_done);
  }
  for (auto& d : ctx->devs) {
    (void)hipSetDevice(d.device);
    (void)free_buf(&d.table);
    (void)free_buf(&d.counts);
    (void)free_buf(&d.scratch_mask);
    (void)free_scratch(&d.scratch);
    if (d.scratch.flag) (void)hipFree(d.scratch.flag);
    free_slab_pipe(d.pipe);
    (void)free_scratch(&d.finish_sums);
    (void)free_scratch(&d.primes_sums);
    (void)free_scratch(&d.query_scratch);
    for (StreamScratch& s : d.unit_scratch) (void)free_scratch(&s);
    if (d.xev) (void)hipEventDestroy(d.xev);
    if (d.stream) (void)hipStreamDestroy(d.stream);
  }
  delete ctx;
}

int32_t dse_ctx_num_devices(const dse_ctx* ctx) { return ctx ? (int32_t)ctx->devs.size() : 0; }

int32_t dse_spread_work(int64_t n, int32_t P, int64_t* lo_hi, int64_t* cs) {
  int64_t c;
  int32_t rc = chunk_geometry(n, P, &c);
  if (rc) return rc;
  if (cs) *cs = c;
  if (lo_hi)
    for (int32_t k = 1; k <= P; ++k) {
      lo_hi[2 * (k - 1)] = 3 + 2 * (int64_t)(k - 1) * c;
      lo_hi[2 * (k - 1) + 1] = 3 + 2 * (int64_t)k * c;
    }
  return DSE_OK;
}

int32_t dse_tail_range(int64_t n, int32_t P, uint64_t* g_start, uint64_t* nbits) {
  int64_t cs, nums;
  int32_t rc = chunk_geometry(n, P, &cs, &nums);
  if (rc) return rc;
  if (g_start) *g_start = (uint64_t)(P * cs);
  if (nbits) *nbits = (uint64_t)(nums - P * cs);
  return DSE_OK;
}

uint64_t dse_base_table_bytes(uint64_t limit) { return table_bytes_for_cap(prime_cap(limit)); }

uint64_t dse_base_limit_max(void) { return kBigBaseLimitMax; }

uint64_t dse_base_limit_for_range(uint64_t g_start, uint64_t nbits) {
  if (nbits == 0) return 0;
  const uint64_t vmax = 3 + 2 * (g_start + nbits - 1);
  return isqrt64(vmax);
}

int32_t dse_base_primes_dev_async(dse_ctx* ctx, uint64_t limit, void* table_dev, uint64_t table_bytes,
                                  void* stream) {
  int32_t rc = check_table_args(ctx, limit, table_dev, table_bytes);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->devs[0].device));
  HIP_TRY(launch_base_primes_big(limit, table_dev, prime_cap(limit), ctx->devs[0].num_cus, (hipStream_t)stream));
  return DSE_OK;
}

uint64_t dse_base_table_prime_bytes(uint64_t limit) { return 16ull + 4ull * prime_cap(limit); }

uint64_t dse_base_table_broadcast_bytes(uint64_t limit) {
  const uint64_t pbytes = dse_base_table_prime_bytes(limit);
  return pbytes <= DSE_TABLE_BROADCAST_MAX_BYTES ? pbytes : 0;
}

int32_t dse_base_table_finish_dev_async(dse_ctx* ctx, uint64_t limit, void* table_dev, uint64_t table_bytes,
                                        void* stream) {
  int32_t rc = check_table_args(ctx, limit, table_dev, table_bytes);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->devs[0].device));
  HIP_TRY(launch_wheel_offsets(table_dev, ctx->devs[0].num_cus, (hipStream_t)stream, prime_cap(limit)));
  return DSE_OK;
}

int32_t dse_sieve_range_dev_async(dse_ctx* ctx, const void* table_dev, uint64_t g_start, uint64_t nbits,
                                  uint64_t* mask_dev, uint64_t* count_dev, void* stream) {
  if (!ctx || !table_dev || !count_dev) return fail(DSE_EINVAL, "null ctx, table or count");
  int32_t rc = check_odd_range(g_start, nbits);
  if (rc) return rc;
  ctx->plan = PlanStats();
  HIP_TRY(hipSetDevice(ctx->devs[0].device));
  HIP_TRY(launch_sieve_range(table_dev, g_start, nbits, reinterpret_cast<uint32_t*>(mask_dev),
                             reinterpret_cast<unsigned long long*>(count_dev), ctx->devs[0].num_cus,
                             (hipStream_t)stream, &ctx->devs[0].scratch, &ctx->opts, &ctx->plan));
  return DSE_OK;
}

int32_t dse_sieve_odd_range(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, uint64_t* mask_or_null,
                            uint64_t* count) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  int32_t rc = check_odd_range(g_start, nbits);
  if (rc) return rc;
  return sieve_range_host(ctx, ctx->devs[0], g_start, nbits, mask_or_null, count);
}

int32_t dse_sieve_chunk(dse_ctx* ctx, int64_t n, int32_t P, int32_t my_num, uint64_t* mask_or_null,
                        uint64_t* count) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  int64_t cs;
  int32_t rc = chunk_geometry(n, P, &cs);
  if (rc) return rc;
  if (my_num < 1 || my_num > P) return fail(DSE_EINVAL, "my_num outside 1..P");
  if (cs < 1) return fail(DSE_EINVAL, "empty chunk (find-first-prime would throw)");
  DevState& d = ctx->devs[(my_num - 1) % ctx->devs.size()];
  return sieve_range_host(ctx, d, (uint64_t)(my_num - 1) * (uint64_t)cs, (uint64_t)cs, mask_or_null, count);
}

int32_t dse_sieve_all(dse_ctx* ctx, int64_t n, int32_t P, uint64_t* per_chunk_counts, uint64_t* pi_ref,
                      uint64_t* pi_full) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  int64_t cs;
  int32_t rc = chunk_geometry(n, P, &cs);
  if (rc) return rc;
  if (cs < 1) return fail(DSE_EINVAL, "empty chunk (find-first-prime would throw)");
  uint64_t tail_g, tail_n;
  dse_tail_range(n, P, &tail_g, &tail_n);
  const int nd = (int)ctx->devs.size();
  // every chunk and the tail are covered by the primes <= sqrt(largest odd <= n)
  const uint64_t limit = dse_base_limit_for_range(0, (uint64_t)P * (uint64_t)cs + tail_n);
  const uint64_t nc = (uint64_t)P + 1;  // per-chunk counts + tail
  ctx->plan = PlanStats();

  // resident masks: one device buffer per chunk, on its device
  if ((rc = ensure_resident(ctx, n, P, cs))) return rc;
  if ((rc = prepare_devices(ctx, limit, nc))) return rc;
  if ((rc = share_table(ctx, limit))) return rc;

  // each device sieves its chunks; the last device also sieves the tail.
  // All of a device's ranges go to one launch_sieve_ranges call: its chunks
  // (and the tail) share persistent launches of the wheel kernel, so no
  // chunk's partial last round leaves the CUs idle and no host launch sits
  // between chunks.
  for (int i = 0; i < nd; ++i) {
    DevState& d = ctx->devs[i];
    HIP_TRY(hipSetDevice(d.device));
    unsigned long long* counts = d.counts.as<unsigned long long>();
    std::vector<RangeSpec> rs;
    for (int32_t k = i; k < P; k += nd)
      rs.push_back({(uint64_t)k * (uint64_t)cs, (uint64_t)cs, ctx->resident.masks[k].as<uint32_t>(),
                    counts + k});
    if (i == nd - 1 && tail_n) rs.push_back({tail_g, tail_n, nullptr, counts + P});
    HIP_TRY(launch_sieve_ranges(d.table.ptr, rs.data(), rs.size(), d.num_cus, d.stream, &d.scratch, &ctx->opts,
                                &ctx->plan));
  }

  // counts: RCCL all-reduce (each slot is non-zero on exactly one device)
  std::vector<unsigned long long> h(nc);
  if ((rc = collect_counts(ctx, nc, h.data()))) return rc;
  uint64_t sum = 0;
  for (int32_t k = 0; k < P; ++k) {
    if (per_chunk_counts) per_chunk_counts[k] = h[k];
    sum += h[k];
  }
  if (pi_ref) *pi_ref = 1 + sum;
  if (pi_full) *pi_full = 1 + sum + h[P];
  return DSE_OK;
}

int32_t dse_copy_chunk_mask(dse_ctx* ctx, int32_t my_num, uint64_t* mask) {
  if (!ctx || !mask) return fail(DSE_EINVAL, "null ctx or mask");
  DevState* d;
  uint64_t* dev_mask;
  int32_t rc = find_resident(ctx, my_num, &d, &dev_mask);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipMemcpyAsync(mask, dev_mask, ctx->resident.words * 8, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return DSE_OK;
}

int32_t dse_sieve_window(dse_ctx* ctx, uint64_t lo, uint64_t hi, uint64_t* count) {
  if (!ctx || !count) return fail(DSE_EINVAL, "null ctx or count");
  *count = 0;
  uint64_t a = lo < 3 ? 3 : lo;
  if (!(a & 1)) ++a;
  if (hi < a) return DSE_OK;
  const uint64_t b = (hi & 1) ? hi : hi - 1;
  const uint64_t g0 = (a - 3) / 2, nb = (b - a) / 2 + 1;
  const uint64_t limit = dse_base_limit_for_range(g0, nb);
  if (limit > kBigBaseLimitMax)
    return fail(DSE_ERANGE, "window needs base primes up to " + std::to_string(limit) +
                                "; the device base-prime build supports " + std::to_string(kBigBaseLimitMax));
  const int nd = (int)ctx->devs.size();
  int32_t rc;
  ctx->plan = PlanStats();
  if ((rc = prepare_devices(ctx, limit, 1))) return rc;
  // one table, built on device 0 and RCCL-broadcast (as dse_sieve_all)
  if ((rc = share_table(ctx, limit))) return rc;
  // contiguous slices of the window, one per device
  const uint64_t part = (nb + nd - 1) / nd;
  for (int i = 0; i < nd; ++i) {
    DevState& d = ctx->devs[i];
    HIP_TRY(hipSetDevice(d.device));
    const uint64_t s = std::min<uint64_t>(nb, part * i), e = std::min<uint64_t>(nb, part * (i + 1));
    if (e > s)
      HIP_TRY(launch_sieve_range(d.table.ptr, g0 + s, e - s, nullptr, d.counts.as<unsigned long long>(), d.num_cus,
                                 d.stream, &d.scratch, &ctx->opts, &ctx->plan));
  }
  unsigned long long c = 0;
  if ((rc = collect_counts(ctx, 1, &c))) return rc;
  *count = c;
  return DSE_OK;
}

int32_t dse_device_status(dse_ctx* ctx) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  int32_t rc;
  for (auto& d : ctx->devs) {
    if (!d.scratch.flag) continue;
    HIP_TRY(hipSetDevice(d.device));
    if (d.scratch.used) HIP_TRY(hipEventSynchronize(d.scratch.done));
    if ((rc = sync_and_check(d))) return rc;
  }
  return DSE_OK;
}

int32_t dse_debug_set_option(dse_ctx* ctx, const char* name, int64_t value) {
  if (!ctx || !name) return fail(DSE_EINVAL, "null ctx or option name");
  const std::string n(name);
  for (const auto& o : kNumOpts)
    if (n == o.name) {
      if (value < o.min || value > o.max) return fail(DSE_EINVAL, n + " " + o.bad);
      o.set(ctx, value);
      return DSE_OK;
    }
  for (uint32_t u = 0; u < kNumSlabUnits; ++u)  // "<unit>_grid"
    if (n == std::string(kSlabUnits[u].name) + "_grid") {
      if (value < 0 || value > (int64_t)kSlabUnits[u].max_grid) return fail(DSE_EINVAL, n + " out of range");
      ctx->grid_cap[u] = (uint32_t)value;
      return DSE_OK;
    }
  if (n == "bucket_lo_log2") {
    // primes above 2^value are bucketed; those up to it go to the wheel kernel's
    // L units, which hold primes <= kWheelMaxPrime only: a larger value would
    // leave (kWheelMaxPrime, 2^value] in neither place
    if (value != 0 && (value < 17 || value > DSE_WHEEL_MAX_LOG))
      return fail(DSE_EINVAL, "bucket_lo_log2 must be 0 or 17.." + std::to_string(DSE_WHEEL_MAX_LOG));
    ctx->opts.bucket_lo_log2 = (uint32_t)value;
    return DSE_OK;
  }
  if (n == "rccl_single") {
    if (value < 0 || value > 1) return fail(DSE_EINVAL, "rccl_single must be 0 or 1");
    if (ctx->logical || ctx->devs.size() != 1)
      return fail(DSE_EINVAL, "rccl_single needs a one-device context (dse_init(1) or dse_init_device)");
    if (value == 1 && ctx->comms.empty()) {
      int dev = ctx->devs[0].device;
      HIP_TRY(hipSetDevice(dev));
      ncclComm_t c;
      NCCL_TRY(ncclCommInitAll(&c, 1, &dev));
      ctx->comms.push_back(c);
    } else if (value == 0 && !ctx->comms.empty()) {
      HIP_TRY(hipSetDevice(ctx->devs[0].device));
      HIP_TRY(hipStreamSynchronize(ctx->devs[0].stream));
      NCCL_TRY(ncclCommDestroy(ctx->comms[0]));
      ctx->comms.clear();
    }
    ctx->rccl_single = value == 1;
    return DSE_OK;
  }
  return fail(DSE_EINVAL, "unknown option " + n);
}

int32_t dse_debug_get_stat(dse_ctx* ctx, const char* name, int64_t* value) {
  if (!ctx || !name || !value) return fail(DSE_EINVAL, "null ctx, stat name or value");
  const std::string n(name);
  if (n == "rccl_calls") {
    *value = ctx->rccl_calls;
  } else if (n == "table_local_builds") {
    *value = ctx->table_local_builds;
  } else if (n == "rccl_comms") {
    *value = (int64_t)ctx->comms.size();
  } else if (n == "rccl_ranks") {  // ranks of the context's communicators, as RCCL reports them
    int c = 0;
    if (!ctx->comms.empty()) NCCL_TRY(ncclCommCount(ctx->comms[0], &c));
    *value = c;
  } else if (n == "plan_wheel_launches") {
    *value = (int64_t)ctx->plan.wheel_launches;
  } else if (n == "plan_full_segments") {
    *value = (int64_t)ctx->plan.full_segments;
  } else if (n == "plan_half_segments") {
    *value = (int64_t)ctx->plan.half_segments;
  } else if (n == "plan_max_rounds") {
    *value = (int64_t)ctx->plan.max_rounds;
  } else if (n == "plan_bucket_passes") {
    *value = (int64_t)ctx->plan.bucket_passes;
  } else if (n == "plan_bucket_max_pass_segments") {
    *value = (int64_t)ctx->plan.bucket_max_pass_segments;
  } else if (n == "plan_bucket_max_lds_bytes") {
    *value = (int64_t)ctx->plan.bucket_max_lds_bytes;
  } else if (n == "primes_tile_bits") {
    *value = (int64_t)kMaskTileBits;
  } else if (n == "stats_tile_bits") {
    *value = (int64_t)kMaskTileBits;
  } else if (n == "gaps_tile_bits") {
    *value = (int64_t)kMaskTileBits;
  } else if (n == "sums_tile_bits") {
    *value = (int64_t)kMaskTileBits;
  } else if (n == "query_index_builds") {
    *value = ctx->query_index_builds;
  } else if (n == "wheel_ta") {
    *value = (int64_t)wheel_consts().ta;
  } else if (n == "wheel_tb1") {
    *value = (int64_t)wheel_consts().tb1;
  } else if (n == "wheel_tb") {
    *value = (int64_t)wheel_consts().tb;
  } else if (n == "wheel_max_prime") {
    *value = (int64_t)wheel_consts().max_prime;
  } else if (n == "wheel_log_kp") {
    *value = (int64_t)wheel_consts().log_kp;
  } else {
    return fail(DSE_EINVAL, "unknown stat " + n);
  }
  return DSE_OK;
}

int32_t dse_debug_expand_block(int32_t variant, const uint32_t planes[8], uint32_t out[15]) {
  if (!planes || !out) return fail(DSE_EINVAL, "null planes or out");
  uint32_t p[8], o[15];
  std::memcpy(p, planes, sizeof p);
  if (!expand_block_variant(variant, p, o)) return fail(DSE_EINVAL, "expand variant outside 0..14");
  std::memcpy(out, o, sizeof o);
  return DSE_OK;
}

int32_t dse_debug_finish_format(uint64_t v, uint32_t flags, char out[32]) {
  if (!out) return fail(DSE_EINVAL, "null out");
  if (flags & ~DSE_FINISH_DOUBLES) return fail(DSE_EINVAL, "only DSE_FINISH_DOUBLES applies to one value");
  return (int32_t)fin_format_value(v, flags & DSE_FINISH_DOUBLES, 0u, [&](uint32_t p, char c) { out[p] = c; });
}

int32_t dse_debug_wheel_arith_dev(dse_ctx* ctx, uint32_t op, const uint64_t* x_dev, const uint64_t* y_dev, uint64_t n,
                                  uint64_t* out_dev, void* stream) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  if (op >= kArithOps) return fail(DSE_EINVAL, "unknown wheel arithmetic op");
  static_assert(kArithKbModF32 == DSE_ARITH_KBMOD_F32 && kArithKbModF38 == DSE_ARITH_KBMOD_F38 &&
                    kArithKbModBarrett == DSE_ARITH_KBMOD_BARRETT && kArithModBarrett == DSE_ARITH_MOD_BARRETT &&
                    kArithBarrettFactor == DSE_ARITH_BARRETT_FACTOR && kArithDivSmall == DSE_ARITH_DIV_SMALL &&
                    kArithDivCeilSmall == DSE_ARITH_DIV_CEIL_SMALL && kArithMulmodSmall == DSE_ARITH_MULMOD_SMALL &&
                    kArithPlaneFirst == DSE_ARITH_PLANE_FIRST && kArithFirstAtOrAfter == DSE_ARITH_FIRST_AT_OR_AFTER &&
                    kArithOps == DSE_ARITH_FIRST_AT_OR_AFTER + 1,
                "include/dse.h DSE_ARITH_* are the probe's ops");
  if (n > 0 && (!x_dev || !y_dev || !out_dev)) return fail(DSE_EINVAL, "null x_dev, y_dev or out_dev");
  if ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(y_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 7u)
    return fail(DSE_EINVAL, "x_dev, y_dev or out_dev is not 8-byte aligned");
  if (n == 0) return DSE_OK;
  HIP_TRY(hipSetDevice(ctx->devs[0].device));
  HIP_TRY(launch_arith_probe(op, x_dev, y_dev, n, out_dev, ctx->devs[0].num_cus, (hipStream_t)stream));
  return DSE_OK;
}

}  // extern "C"
