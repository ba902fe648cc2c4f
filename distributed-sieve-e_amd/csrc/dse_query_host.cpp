// dse_query_host.cpp -- rank and select, the host side (include/dse.h): queries
// about single values or ranks of a device-resident mask (dse_query.hip), on
// the caller's device memory (dse_query_index_dev_async, dse_query_dev_async),
// on a range sieved for the call (dse_query_range) or on the chunks the last
// dse_sieve_all left resident (dse_query_resident), whose rank indices live as
// long as the masks; dse_debug_query_host runs the kernel's per-word and
// per-tile bodies (dse_query_word.h) on the host.
#include <algorithm>

#include "dse_host.h"
#include "dse_query_word.h"

using namespace dse;

static_assert(DSE_QUERY_NONE == kQueryNone && DSE_QUERY_RANK == kQueryRank && DSE_QUERY_SELECT == kQuerySelect &&
                  DSE_QUERY_NEXT == kQueryNext && DSE_QUERY_PREV == kQueryPrev && DSE_QUERY_TEST == kQueryTest,
              "the kernels answer the kinds of include/dse.h");

namespace {

constexpr uint64_t kQueryMaxBatch = 1ull << 40;  // queries of one call: their bytes stay far below 2^64

// the index's words and, behind them, the two totals the scan launch writes
uint64_t index_bytes(uint64_t nbits) { return (query_index_words(nbits) + 2) * sizeof(uint64_t); }

int32_t query_check(const char* what, uint32_t kind, const void* q, uint64_t nq, const void* out) {
  if (kind >= kQueryKinds) return fail(DSE_EINVAL, std::string(what) + ": unknown query kind " + std::to_string(kind));
  if (nq && (!q || !out)) return fail(DSE_EINVAL, std::string(what) + ": null queries or answers with nq > 0");
  return DSE_OK;
}

hipError_t build_index(uint64_t g_start, uint64_t nbits, const uint64_t* mask, void* index, hipStream_t stream) {
  unsigned long long* const w = static_cast<unsigned long long*>(index);
  return launch_primes_scan(g_start, nbits, mask, 0, 0, w + query_index_words(nbits), w, stream);
}

int32_t hip_or_nomem(hipError_t e, const char* what) {
  if (e == hipSuccess) return DSE_OK;
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    return fail(DSE_ENOMEM, std::string(what) + ": out of device memory");
  }
  return fail(DSE_EHIP, std::string(what) + " failed: " + hipGetErrorString(e));
}

// One batch of queries for one mask: q -> device -> launch -> a, on the stream.
struct Batch {
  int32_t chunk = 0;  // 1-based
  const uint64_t* q = nullptr;
  uint64_t* a = nullptr;
  uint64_t n = 0;
};

// Enqueue a batch at `dev` (16 n bytes of device memory): nothing is waited for.
hipError_t enqueue_batch(dse_ctx* ctx, DevState& d, uint32_t kind, uint64_t g_start, uint64_t nbits, const uint64_t* mask,
                         const void* index, const Batch& b, char* dev, hipStream_t stream) {
  uint64_t* const dq = reinterpret_cast<uint64_t*>(dev);
  uint64_t* const da = dq + b.n;
  hipError_t e = hipMemcpyAsync(dq, b.q, b.n * 8, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
    e = launch_query(kind, g_start, nbits, mask, index, dq, b.n, da, query_grid(kind, b.n, d.num_cus, ctx->query_grid),
                     stream);
  if (e == hipSuccess) e = hipMemcpyAsync(b.a, da, b.n * 8, hipMemcpyDeviceToHost, stream);
  return e;
}

// Chunks k0 .. k1 of the resident set get their rank index, total, first and last entry, each on
// its own device and stream: every build is enqueued before any is waited for.
int32_t ensure_indices(dse_ctx* ctx, int32_t k0, int32_t k1) {
  ResidentSet& r = ctx->resident;
  const uint64_t cs = (uint64_t)r.cs, words = query_index_words(cs);
  std::vector<int32_t> todo;
  for (int32_t k = k0; k <= k1; ++k)
    if (!r.indexed[(size_t)k - 1]) todo.push_back(k);
  if (todo.empty()) return DSE_OK;
  auto dev_of = [&](int32_t k) -> DevState& { return ctx->devs[(size_t)(k - 1) % ctx->devs.size()]; };
  auto drain = [&]() -> hipError_t {
    hipError_t e = hipSuccess;
    for (int32_t k : todo) {
      hipError_t s = hipSetDevice(dev_of(k).device);
      if (s == hipSuccess) s = hipStreamSynchronize(dev_of(k).stream);
      if (e == hipSuccess) e = s;
    }
    return e;
  };
  std::vector<uint64_t> fq(2 * todo.size()), fa(2 * todo.size());
  auto run = [&]() -> int32_t {
    int32_t rc;
    for (int32_t k : todo) {
      DevState& d = dev_of(k);
      Buf& ib = r.index[(size_t)k - 1];
      HIP_TRY(hipSetDevice(d.device));
      if ((rc = hip_or_nomem(grow_buf(&ib, index_bytes(cs) + 4 * sizeof(uint64_t)), "hipMalloc of a rank index")))
        return rc;
      HIP_TRY(build_index((uint64_t)(k - 1) * cs, cs, r.masks[(size_t)k - 1].as<uint64_t>(), ib.ptr, d.stream));
      ++ctx->query_index_builds;
      HIP_TRY(hipMemcpyAsync(&r.total[(size_t)k - 1], ib.as<uint64_t>() + (words - 1), sizeof(uint64_t),
                             hipMemcpyDeviceToHost, d.stream));
    }
    HIP_TRY(drain());
    for (size_t j = 0; j < todo.size(); ++j) {
      const int32_t k = todo[j];
      DevState& d = dev_of(k);
      const uint64_t tot = r.total[(size_t)k - 1];
      fq[2 * j] = 0;
      fq[2 * j + 1] = tot ? tot - 1 : kQueryNone;
      Batch b;
      b.chunk = k;
      b.q = &fq[2 * j];
      b.a = &fa[2 * j];
      b.n = 2;
      HIP_TRY(hipSetDevice(d.device));
      HIP_TRY(enqueue_batch(ctx, d, kQuerySelect, (uint64_t)(k - 1) * cs, cs, r.masks[(size_t)k - 1].as<uint64_t>(),
                            r.index[(size_t)k - 1].ptr, b, r.index[(size_t)k - 1].as<char>() + index_bytes(cs), d.stream));
    }
    HIP_TRY(drain());
    for (size_t j = 0; j < todo.size(); ++j) {
      const size_t i = (size_t)todo[j] - 1;
      r.first[i] = fa[2 * j];
      r.last[i] = fa[2 * j + 1];
      r.indexed[i] = 1;
    }
    return DSE_OK;
  };
  const int32_t rc = run();
  if (rc) (void)drain();  // nothing in flight reads this call's memory
  return rc;
}

// The batches of the resident chunks k0 .. k1, each on its chunk's device and stream (resident_fanout).
// Returns with every stream drained, also after a failure: what was enqueued reads the caller's memory.
int32_t run_batches(dse_ctx* ctx, uint32_t kind, int32_t k0, int32_t k1, const std::vector<Batch>& batches) {
  const ResidentSet& r = ctx->resident;
  const uint64_t cs = (uint64_t)r.cs;
  const size_t nd = ctx->devs.size();
  return resident_fanout(
      ctx, k0, k1,
      [&](size_t i, DevState& d, const std::vector<int32_t>&, bool* acquired) -> int32_t {
        uint64_t bytes = 0;
        for (const Batch& b : batches)
          if ((size_t)(b.chunk - 1) % nd == i) bytes += 16 * b.n;
        if (!bytes) return DSE_OK;
        if (int32_t rc = hip_or_nomem(acquire_scratch_roomy(&d.query_scratch, bytes, d.stream),
                                      "hipMalloc of the query buffers"))
          return rc;
        *acquired = true;
        char* dev = d.query_scratch.buf.as<char>();
        for (const Batch& b : batches) {
          if ((size_t)(b.chunk - 1) % nd != i || !b.n) continue;
          const size_t c = (size_t)b.chunk - 1;
          const uint64_t* const mask = r.masks[c].as<uint64_t>();
          const hipError_t e = enqueue_batch(ctx, d, kind, (uint64_t)c * cs, cs, mask, r.index[c].ptr, b, dev, d.stream);
          if (e != hipSuccess) return fail(DSE_EHIP, std::string("query launch failed: ") + hipGetErrorString(e));
          dev += 16 * b.n;
        }
        return DSE_OK;
      },
      [](size_t, DevState& d, const std::vector<int32_t>&) -> int32_t {
        hipError_t e = hipStreamSynchronize(d.stream);
        const hipError_t e2 = release_scratch(&d.query_scratch, d.stream);
        if (e == hipSuccess) e = e2;
        if (e != hipSuccess) return fail(DSE_EHIP, std::string("query copy failed: ") + hipGetErrorString(e));
        return DSE_OK;
      });
}

}  // namespace

extern "C" uint64_t dse_query_index_bytes(uint64_t nbits) { return index_bytes(nbits); }

extern "C" int32_t dse_query_index_dev_async(dse_ctx* ctx, uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev,
                                             uint64_t* index_dev, uint64_t index_bytes_, void* stream) {
  if (!ctx || !index_dev) return fail(DSE_EINVAL, "null ctx or index");
  if (nbits && !mask_dev) return fail(DSE_EINVAL, "null mask");
  if (reinterpret_cast<uintptr_t>(index_dev) & 7u) return fail(DSE_EINVAL, "index_dev is not 8-byte aligned");
  int32_t rc;
  if ((rc = check_mask_range("query", g_start, nbits))) return rc;
  if (index_bytes_ < index_bytes(nbits)) return fail(DSE_EINVAL, "index buffer too small");
  HIP_TRY(hipSetDevice(ctx->devs[0].device));
  const hipError_t e = build_index(g_start, nbits, mask_dev, index_dev, (hipStream_t)stream);
  if (e != hipSuccess) return fail(DSE_EHIP, std::string("index launch failed: ") + hipGetErrorString(e));
  return DSE_OK;
}

extern "C" int32_t dse_query_dev_async(dse_ctx* ctx, uint32_t kind, uint64_t g_start, uint64_t nbits,
                                       const uint64_t* mask_dev, const uint64_t* index_dev, const uint64_t* q_dev,
                                       uint64_t nq, uint64_t* out_dev, void* stream) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  int32_t rc;
  if ((rc = query_check("dse_query_dev_async", kind, q_dev, nq, out_dev))) return rc;
  if (nbits && !mask_dev) return fail(DSE_EINVAL, "null mask");
  if (kind != kQueryTest && !index_dev) return fail(DSE_EINVAL, "null index for a kind that needs it");
  if ((reinterpret_cast<uintptr_t>(index_dev) | reinterpret_cast<uintptr_t>(q_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 7u)
    return fail(DSE_EINVAL, "index_dev, q_dev or out_dev is not 8-byte aligned");
  if ((rc = check_mask_range("query", g_start, nbits))) return rc;
  if (!nq) return DSE_OK;
  DevState& d = ctx->devs[0];
  HIP_TRY(hipSetDevice(d.device));
  const hipError_t e = launch_query(kind, g_start, nbits, mask_dev, index_dev, q_dev, nq, out_dev,
                                    query_grid(kind, nq, d.num_cus, ctx->query_grid), (hipStream_t)stream);
  if (e != hipSuccess) return fail(DSE_EHIP, std::string("query launch failed: ") + hipGetErrorString(e));
  return DSE_OK;
}

extern "C" int32_t dse_query_range(dse_ctx* ctx, uint32_t kind, uint64_t g_start, uint64_t nbits, const uint64_t* q,
                                   uint64_t nq, uint64_t* out) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  int32_t rc;
  if ((rc = query_check("dse_query_range", kind, q, nq, out))) return rc;
  if ((rc = check_mask_range("query", g_start, nbits))) return rc;
  if (nq > kQueryMaxBatch) return fail(DSE_ENOMEM, "more than 2^40 queries in one call");
  DevState& d = ctx->devs[0];
  if (nbits && (rc = sieve_range_host(ctx, d, g_start, nbits, nullptr, nullptr, true))) return rc;
  if (!nq) return DSE_OK;
  HIP_TRY(hipSetDevice(d.device));
  const uint64_t ib = index_bytes(nbits);
  if ((rc = hip_or_nomem(acquire_scratch_roomy(&d.query_scratch, ib + 16 * nq, d.stream), "hipMalloc of the query buffers")))
    return rc;
  char* const base = d.query_scratch.buf.as<char>();
  const uint64_t* const mask = d.scratch_mask.as<uint64_t>();
  hipError_t e = kind == kQueryTest ? hipSuccess : build_index(g_start, nbits, mask, base, d.stream);
  Batch b;
  b.q = q;
  b.a = out;
  b.n = nq;
  if (e == hipSuccess) e = enqueue_batch(ctx, d, kind, g_start, nbits, mask, base, b, base + ib, d.stream);
  const hipError_t e1 = hipStreamSynchronize(d.stream);  // also after a failure: a copy may read the caller's memory
  const hipError_t e2 = release_scratch(&d.query_scratch, d.stream);
  if (e == hipSuccess) e = e1 != hipSuccess ? e1 : e2;
  if (e != hipSuccess) return fail(DSE_EHIP, std::string("query failed: ") + hipGetErrorString(e));
  return DSE_OK;
}

extern "C" int32_t dse_query_resident(dse_ctx* ctx, int32_t my_num, uint32_t kind, const uint64_t* q, uint64_t nq,
                                      uint64_t* out) {
  if (!ctx) return fail(DSE_EINVAL, "null ctx");
  int32_t rc;
  if ((rc = query_check("dse_query_resident", kind, q, nq, out))) return rc;
  // the two halves of resident_span, the batch's bound between them: which error wins stays as it was
  if ((rc = check_resident(ctx, my_num, false))) return rc;
  if (nq > kQueryMaxBatch) return fail(DSE_ENOMEM, "more than 2^40 queries in one call");
  ResidentSet& r = ctx->resident;
  const uint64_t cs = (uint64_t)r.cs, P = (uint64_t)r.P;
  if (my_num == 0 && P == 1) my_num = 1;  // one chunk is the whole range
  int32_t k0, k1;
  if ((rc = resident_span(ctx, my_num, "query", &k0, &k1))) return rc;
  if (!nq) return DSE_OK;
  if (kind != kQueryTest && (rc = ensure_indices(ctx, k0, k1))) return rc;

  if (my_num) {
    Batch b;
    b.chunk = my_num;
    b.q = q;
    b.a = out;
    b.n = nq;
    return run_batches(ctx, kind, k0, k1, {b});
  }

  // All chunks as one range: every query goes to the chunk that holds its candidate (its rank,
  // for SELECT), and the answer is completed from the chunks' totals, first and last entries.
  std::vector<uint64_t> before(P + 1, 0);  // entries in the chunks before chunk j + 1
  if (kind != kQueryTest)
    for (uint64_t j = 0; j < P; ++j) before[j + 1] = before[j] + r.total[j];
  const uint64_t all = P * cs;
  std::vector<std::vector<uint64_t>> cq(P), ca(P), where(P);
  std::vector<uint64_t> none;  // SELECT past the total: answered here
  for (uint64_t i = 0; i < nq; ++i) {
    uint64_t x = q[i], j;
    if (kind == kQuerySelect) {
      if (x >= before[P]) {
        none.push_back(i);
        continue;
      }
      j = (uint64_t)(std::upper_bound(before.begin(), before.end(), x) - before.begin()) - 1;
      x -= before[j];
    } else if (kind == kQueryPrev) {
      // the last candidate below x, if any, is at position lead(x - 1) - 1
      const uint64_t m = x ? query_lead(x - 1, 0, all) : 0;
      j = m ? std::min((m - 1) / cs, P - 1) : 0;
    } else if (kind == kQueryTest) {
      // x's own candidate; a value that is nobody's candidate gets its 0 from any chunk
      j = x >= 3 ? std::min((x - 3) / 2 / cs, P - 1) : 0;
    } else {
      // the first candidate above x is at position lead(x): the chunks before it hold values <= x only
      j = std::min(query_lead(x, 0, all) / cs, P - 1);
    }
    cq[j].push_back(x);
    where[j].push_back(i);
  }
  std::vector<Batch> batches;
  for (uint64_t j = 0; j < P; ++j) {
    if (cq[j].empty()) continue;
    ca[j].resize(cq[j].size());
    Batch b;
    b.chunk = (int32_t)j + 1;
    b.q = cq[j].data();
    b.a = ca[j].data();
    b.n = cq[j].size();
    batches.push_back(b);
  }
  if ((rc = run_batches(ctx, kind, k0, k1, batches))) return rc;
  for (uint64_t j = 0; j < P; ++j) {
    // what a NEXT or PREV that finds nothing in chunk j + 1 takes from the non-empty chunk after or before it
    uint64_t hop = kQueryNone;
    if (kind == kQueryNext)
      for (uint64_t n = j + 1; n < P && hop == kQueryNone; ++n) hop = r.first[n];
    if (kind == kQueryPrev)
      for (uint64_t n = j; n-- > 0 && hop == kQueryNone;) hop = r.last[n];
    for (size_t i = 0; i < ca[j].size(); ++i) {
      uint64_t a = ca[j][i];
      if (kind == kQueryRank) a += before[j];
      if ((kind == kQueryNext || kind == kQueryPrev) && a == kQueryNone) a = hop;
      out[where[j][i]] = a;
    }
  }
  for (uint64_t i : none) out[i] = kQueryNone;
  return DSE_OK;
}

extern "C" int32_t dse_debug_query_host(const uint64_t* mask, uint64_t g_start, uint64_t nbits, uint32_t kind,
                                        const uint64_t* q, uint64_t nq, uint64_t* out) {
  int32_t rc;
  if ((rc = query_check("dse_debug_query_host", kind, q, nq, out))) return rc;
  if (nbits && !mask) return fail(DSE_EINVAL, "null mask");
  if ((rc = check_mask_range("query", g_start, nbits))) return rc;
  const MaskRange m = mask_range(mask, g_start, nbits);
  const uint64_t tiles = mask_tiles(nbits);
  auto tile_word = [&](uint64_t t) { return [&m, t](uint32_t i) { return mask_word(m, t * kMaskTileWords + i); }; };
  // the index, as the size and scan launches leave it
  std::vector<uint64_t> index(tiles + 1, 0);
  for (uint64_t t = 0; t < tiles; ++t) index[t + 1] = index[t] + query_pop_words<kMaskTileWords>(tile_word(t));
  auto rank_lead = [&](uint64_t lead) -> uint64_t {
    if (lead >= nbits) return index[tiles];
    const uint64_t t = lead / kMaskTileBits;
    return index[t] + query_rank_words<kMaskTileWords>(tile_word(t), 0, (uint32_t)(lead % kMaskTileBits));
  };
  auto select_rank = [&](uint64_t k) -> uint64_t {
    if (k >= index[tiles]) return kQueryNone;
    const uint64_t t = (uint64_t)(std::upper_bound(index.begin(), index.begin() + tiles, k) - index.begin()) - 1;
    const uint32_t pos = query_select_words<kMaskTileWords>(tile_word(t), (uint32_t)(k - index[t]));
    return query_value(g_start, t * kMaskTileBits + pos);
  };
  for (uint64_t i = 0; i < nq; ++i) {
    const uint64_t x = q[i];
    switch (kind) {
      case kQueryRank: out[i] = rank_lead(query_lead(x, g_start, nbits)); break;
      case kQuerySelect: out[i] = select_rank(x); break;
      case kQueryNext: out[i] = select_rank(rank_lead(query_lead(x, g_start, nbits))); break;
      case kQueryPrev: {
        const uint64_t below = x ? rank_lead(query_lead(x - 1, g_start, nbits)) : 0ull;
        out[i] = below ? select_rank(below - 1) : kQueryNone;
        break;
      }
      default: out[i] = query_test(m, x); break;
    }
  }
  return DSE_OK;
}
