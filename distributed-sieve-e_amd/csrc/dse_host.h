// dse_host.h -- shared by the units of the C-ABI host layer. Not installed;
// include/dse.h is the ABI.
//   dse_host.cpp           contexts, tables, collectives, sieve entry points
//   dse_finish_host.cpp    the primes{k}.txt writers
//   dse_primes_host.cpp    primes as numbers
//   dse_tuples_host.cpp    constellations as numbers
//   dse_query_host.cpp     rank and select
//   dse_stats_host.cpp     statistics of a mask
//   dse_goldbach_host.cpp  minimal Goldbach partitions
//   dse_race_host.cpp      residue classes and races
//   dse_gaps_host.cpp      where the gaps are
//   dse_sums_host.cpp      power and reciprocal sums
//   dse_consec_host.cpp    residue pairs of consecutive primes
// Here: contexts and device state, the slab pipe and the rank pipeline of the
// units that bring values to the host, and for the last six, the slab units
// (dse_slab.h: a mask becomes one small struct), their table and the three
// drivers of their entry points.
#pragma once
#include <rccl/rccl.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/dse.h"
#include "dse_internal.h"

#pragma GCC visibility push(hidden)  // private to the host layer: libdse.so's exports stay as they are
namespace dse {

// Sets the calling thread's dse_last_error / dse_last_status; returns `code`.
int32_t fail(int32_t code, const std::string& msg);

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return dse::fail(DSE_EHIP, std::string(#expr " failed: ") + hipGetErrorString(e_));      \
  } while (0)

#define NCCL_TRY(expr)                                                                         \
  do {                                                                                         \
    ncclResult_t r_ = (expr);                                                                  \
    if (r_ != ncclSuccess)                                                                     \
      return dse::fail(DSE_ENCCL, std::string(#expr " failed: ") + ncclGetErrorString(r_));    \
  } while (0)

// The slab units: six passes that turn a mask into one small struct through the
// slab reduction of dse_slab.h. One row each: the name of its messages and of
// its test option "<name>_grid", its grid and scratch rules (dse_internal.h),
// the largest grid and the uint64 words of its result.
enum SlabUnit : uint32_t { kUnitStats, kUnitGoldbach, kUnitRace, kUnitGaps, kUnitSums, kUnitConsec, kNumSlabUnits };
struct SlabUnitDesc {
  const char* name;
  uint32_t (*grid)(uint64_t nbits, int num_cus, uint32_t grid_cap);
  uint64_t (*scratch_bytes)(uint32_t grid);
  uint32_t max_grid;
  uint32_t words;
};
inline constexpr SlabUnitDesc kSlabUnits[kNumSlabUnits] = {
    {"stats", stats_grid, stats_scratch_bytes, kStatsMaxGrid, DSE_STATS_WORDS},
    {"goldbach", goldbach_grid, goldbach_scratch_bytes, kGbMaxGrid, DSE_GOLDBACH_WORDS},
    {"race", race_grid, race_scratch_bytes, kRaceMaxGrid, DSE_RACE_WORDS},
    {"gaps", gaps_grid, gaps_scratch_bytes, kGapsMaxGrid, DSE_GAPS_WORDS},
    {"sums", sums_grid, sums_scratch_bytes, kSumsMaxGrid, DSE_SUMS_WORDS},
    {"consec", consec_grid, consec_scratch_bytes, kConsecMaxGrid, DSE_CONSEC_WORDS},
};

// The two-slot slab pipe of the blocking entry points that bring a device
// result to the host in slabs (finish text, prime values): slab i + 1 is
// produced on the device's stream into slot (i + 1) & 1 while slab i is copied
// to pinned memory on the copy stream and slab i - 1 is consumed by the
// calling thread. Two device and two pinned buffers of `buf_bytes` each (1 MiB
// to 64 MiB, grown on demand) and the events that order them, which only the
// slab_* operations below touch. A call that uses the pipe drains both streams
// before it returns.
constexpr uint64_t kSlabBufMax = 64ull << 20;  // 4 buffers: 256 MiB per device in all
constexpr uint64_t kSlabBufMin = 1ull << 20;
struct SlabPipe {
  Buf dbuf[2];
  Buf hbuf[2] = {{nullptr, 0, true}, {nullptr, 0, true}};
  uint64_t buf_bytes = 0;                 // all four buffers hold this much
  unsigned long long* dtotals = nullptr;  // device [2][2]: a producer's totals, per slot
  unsigned long long* htotals = nullptr;  // pinned [2][2]
  hipStream_t copy = nullptr;             // the slabs' D2H copies
  hipEvent_t ready_ev[2] = {nullptr, nullptr};  // slot produced (producing stream)
  hipEvent_t copy_ev[2] = {nullptr, nullptr};   // slot copied (copy stream)
  bool pending[2] = {false, false};             // copy_ev recorded and not yet waited for on the host
};

struct DevState {
  int device = 0;
  int num_cus = 0;
  hipStream_t stream = nullptr;
  Buf table;
  Buf counts;                // device scratch (unsigned long long)
  Buf scratch_mask;          // for dse_sieve_chunk
  Scratch scratch;           // bucketed-pass scratch (high-offset ranges)
  SlabPipe pipe;             // slabs to the host: finish text, prime and constellation values
  // tile-sum scratch of the three launches of the device finish (dse_finish.hip)
  StreamScratch finish_sums;
  // the same of primes and constellations as numbers (dse_primes.hip,
  // dse_tuples.hip), and dse_tuples_resident's totals and head words
  StreamScratch primes_sums;
  // rank and select (dse_query.hip): queries and answers on their way,
  // dse_query_range's index
  StreamScratch query_scratch;
  // one per slab unit, so that the units stay independent of each other on
  // different streams: the workgroups' slabs, results on their way to the host
  // and what a chunk sees of its neighbour (Goldbach: a tail, sums: a head word)
  StreamScratch unit_scratch[kNumSlabUnits];
  hipEvent_t xev = nullptr;  // logical devices: this device's side of a collective
};

// The chunk masks dse_sieve_all keeps on the devices, with the call they were
// sieved for: chunk k's mask is masks[k - 1], on device (k - 1) mod #devices.
// `valid` only after every mask of that call was allocated; a failed
// allocation frees them all.
struct ResidentSet {
  bool valid = false;
  int64_t n = 0;
  int32_t P = 0;
  int64_t cs = 0;                // candidates per chunk
  uint64_t words = 0;            // uint64 words per mask
  std::vector<Buf> masks;        // [P], of `words` uint64 each
  // Rank and select (dse_query_host.cpp): chunk k's rank index, built on its device at the first
  // query that needs it and freed with the masks. Behind the index's words and the scan's two
  // totals the buffer holds the two queries and two answers that fetched `first` and `last`.
  std::vector<Buf> index;        // [P]
  std::vector<char> indexed;     // [P]: index, total, first and last are this mask's
  std::vector<uint64_t> total;   // [P]: entries of the chunk
  std::vector<uint64_t> first;   // [P]: value of its first entry, DSE_QUERY_NONE for an empty chunk
  std::vector<uint64_t> last;    // [P]: of its last
};

}  // namespace dse

struct dse_ctx {
  std::vector<dse::DevState> devs;
  std::vector<ncclComm_t> comms;
  dse::ResidentSet resident;
  dse::SieveOpts opts;  // test-only knobs (dse_debug_set_option)
  // test-only knobs of the units (dse_debug_set_option); 0 leaves each alone
  uint64_t finish_slab_words = 0;    // caps a finish slab at that many mask words
  uint64_t primes_slab_entries = 0;  // caps a slab of dse_primes_range / _resident at that many values
  uint32_t query_grid = 0;           // caps the workgroups of a query launch
  uint32_t grid_cap[dse::kNumSlabUnits] = {};  // "<unit>_grid": caps the workgroups of that slab unit's launch
  uint32_t consec_flush_tiles = 0;   // the tiles after which a consec workgroup empties its 32-bit counters
  uint32_t consec_body = 0;          // 1 / 2 force the bit-parallel / per-entry body of the consec main kernel
  int64_t query_index_builds = 0;  // rank indices built for resident chunks (dse_debug_get_stat)
  // dse_debug_init_logical: every DevState on device 0, the collectives
  // replaced by copies (xfer_table / allreduce_counts); on device 0:
  bool logical = false;
  // dse_debug_set_option("rccl_single"): a one-device context with a 1-rank
  // RCCL communicator, so share_table / allreduce_counts issue the real
  // grouped ncclBroadcast / ncclAllReduce on a one-GPU box.
  bool rccl_single = false;
  int64_t rccl_calls = 0;          // collectives RCCL accepted (dse_debug_get_stat)
  int64_t table_local_builds = 0;  // tables built per device instead of broadcast (share_table)
  dse::PlanStats plan;             // what the last sieving entry point launched (dse_debug_get_stat "plan_*")
  dse::Buf lg_stage;               // gathered counts [devs][n]
  dse::Buf lg_sum;                 // their sum [n]
  hipEvent_t lg_done = nullptr;    // the sum on device 0's stream
};

namespace dse {

// cs = candidates per chunk of (n, P); nums = the odd candidates 3..n
int32_t chunk_geometry(int64_t n, int32_t P, int64_t* cs, int64_t* nums = nullptr);
int32_t check_odd_range(uint64_t g_start, uint64_t nbits);
// check_odd_range, and at most 2^44 candidates: what every consumer of a resident mask refuses
// ("<what> range above 2^44 candidates in one call")
int32_t check_mask_range(const char* what, uint64_t g_start, uint64_t nbits);
// keep_dev: sieve into d.scratch_mask even without a host mask (dse_finish_range_file)
int32_t sieve_range_host(dse_ctx* ctx, DevState& d, uint64_t g0, uint64_t nbits, uint64_t* mask_or_null,
                         uint64_t* count, bool keep_dev = false);
// DSE_EINVAL, naming my_num, unless it is a resident chunk or, without one_chunk, 0 for all of them.
int32_t check_resident(dse_ctx* ctx, int32_t my_num, bool one_chunk);
// The device and mask of resident chunk my_num (check_resident for one chunk).
int32_t find_resident(dse_ctx* ctx, int32_t my_num, DevState** d, uint64_t** mask);
// check_resident, my_num's chunks k0 .. k1 (itself, or all for 0), check_mask_range(what) of the last.
int32_t resident_span(dse_ctx* ctx, int32_t my_num, const char* what, int32_t* k0, int32_t* k1);

// A *_dev_async entry point's launches around a scratch: acquire `s` for `stream`, launch(its
// address), release also after a failure (what was launched may read it); "<what> failed: ...".
template <typename Launch>
int32_t scratch_launch(StreamScratch& s, uint64_t bytes, hipStream_t stream, const char* what, Launch&& launch) {
  HIP_TRY(acquire_scratch_roomy(&s, bytes, stream));
  const hipError_t e = launch(s.buf.ptr);
  HIP_TRY(release_scratch(&s, stream));
  if (e != hipSuccess) return fail(DSE_EHIP, std::string(what) + " failed: " + hipGetErrorString(e));
  return DSE_OK;
}

// Results on their way to the host through a scratch laid out as slabs (dse_slab.h) | nres results
// of res_bytes | extra_bytes of the unit's own: result_acquire acquires it for d.stream and gives
// the two addresses behind the slabs; result_collect copies n bytes from res to `out` on d.stream,
// drains the stream and releases, also after an error ("<what> copy failed: ...").
int32_t result_acquire(DevState& d, StreamScratch& s, uint64_t slab_bytes, uint32_t nres, uint64_t res_bytes,
                       uint64_t extra_bytes, uint64_t** res, uint64_t** extra);
int32_t result_collect(DevState& d, StreamScratch& s, const char* what, const uint64_t* res, uint64_t n, void* out);

// The per-device fan-out over the resident chunks k0 .. k1. For every device that holds some:
// hipSetDevice and enqueue(device index, DevState, its chunks, &acquired), which acquires a scratch
// (and says so) and launches on d.stream without waiting. Then for every device that acquired,
// also after a failure: hipSetDevice and collect(...), which waits and releases. The first error.
using FanEnqueue = std::function<int32_t(size_t, DevState&, const std::vector<int32_t>&, bool*)>;
using FanCollect = std::function<int32_t(size_t, DevState&, const std::vector<int32_t>&)>;
int32_t resident_fanout(dse_ctx* ctx, int32_t k0, int32_t k1, const FanEnqueue& enqueue, const FanCollect& collect);

// The drivers of the slab units' entry points (U: the unit, R: its struct of include/dse.h). Each
// entry point checks its own arguments first, in its own order; a launch callable hands the
// addresses and the grid it is given to the unit's launch_* and returns its hipError_t, which a
// driver reports as "<unit> launch failed: ..." (launch_rc), or an int32_t it has reported itself.
int32_t launch_rc(const SlabUnitDesc& u, hipError_t e);
inline int32_t launch_rc(const SlabUnitDesc&, int32_t rc) { return rc; }
// The pointer checks at the head of a *_dev_async entry point: "null ctx or <out>", "null mask",
// "<out>_dev is not 8-byte aligned" and, for the units that refuse one, a misaligned mask_dev.
int32_t check_dev_args(const dse_ctx* ctx, uint64_t nbits, const void* mask_dev, const void* out_dev, const char* out,
                       bool mask_aligned);
// The range checks every dse_*_merge shares: "the ranges are not adjacent" (DSE_EINVAL) opens it,
// "merged range beyond 2^62" (DSE_ERANGE) follows the unit's own checks of the pair.
int32_t check_merge_adjacent(uint64_t a_g, uint64_t a_nbits, uint64_t b_g);
int32_t check_merge_end(uint64_t b_g, uint64_t b_nbits);

// *_dev_async: launch(slabs, grid, stream) on device 0 around the unit's scratch (scratch_launch).
template <SlabUnit U, typename Launch>
int32_t unit_dev_async(dse_ctx* ctx, uint64_t nbits, void* stream, Launch&& launch) {
  constexpr const SlabUnitDesc& u = kSlabUnits[U];
  DevState& d = ctx->devs[0];
  HIP_TRY(hipSetDevice(d.device));
  hipStream_t s = (hipStream_t)stream;
  const uint32_t grid = u.grid(nbits, d.num_cus, ctx->grid_cap[U]);
  return scratch_launch(d.unit_scratch[U], u.scratch_bytes(grid), s, (std::string(u.name) + " launch").c_str(),
                        [&](void* slabs) { return launch(slabs, grid, s); });
}

// *_range: the candidates [sieve_g, sieve_g + sieve_bits) are sieved into device 0's scratch mask
// (the unit's nbits of them and what it sees beside them; nothing for an empty range), then
// launch(that mask, result, slabs, grid, stream) and the result to *out. The scratch is released
// after a failed launch too; *out is written only on success.
template <SlabUnit U, typename R, typename Launch>
int32_t unit_range(dse_ctx* ctx, uint64_t sieve_g, uint64_t sieve_bits, uint64_t nbits, Launch&& launch, R* out) {
  constexpr const SlabUnitDesc& u = kSlabUnits[U];
  static_assert(sizeof(R) == 8 * u.words, "R is the unit's struct");
  DevState& d = ctx->devs[0];
  StreamScratch& s = d.unit_scratch[U];
  int32_t rc;
  if (nbits && (rc = sieve_range_host(ctx, d, sieve_g, sieve_bits, nullptr, nullptr, true))) return rc;
  HIP_TRY(hipSetDevice(d.device));
  const uint32_t grid = u.grid(nbits, d.num_cus, ctx->grid_cap[U]);
  uint64_t* res;
  if ((rc = result_acquire(d, s, u.scratch_bytes(grid), 1, sizeof(R), 0, &res, nullptr))) return rc;
  if ((rc = launch_rc(u, launch(d.scratch_mask.as<uint64_t>(), res, s.buf.ptr, grid, d.stream)))) {
    (void)release_scratch(&s, d.stream);
    return rc;
  }
  R tmp;
  if ((rc = result_collect(d, s, u.name, res, sizeof tmp, &tmp))) return rc;
  *out = tmp;
  return DSE_OK;
}

// *_resident, the parts: one R per resident chunk k0 .. k1 into (*parts)[k - k0]. On every device
// that holds some (resident_fanout), behind the slabs one R per chunk and extra_words uint64 per
// chunk of the unit's own, then chunk(d, k, extra, result, slabs, grid, stream) for each of its
// chunks k in order, until one fails: it may copy a neighbour's words into `extra` on the stream
// and launches on chunk k's mask. Every device's launches are enqueued before any result is waited for.
template <SlabUnit U, typename R, typename Chunk>
int32_t unit_resident_parts(dse_ctx* ctx, int32_t k0, int32_t k1, uint64_t extra_words, Chunk&& chunk,
                            std::vector<R>* parts) {
  constexpr const SlabUnitDesc& u = kSlabUnits[U];
  static_assert(sizeof(R) == 8 * u.words, "R is the unit's struct");
  const uint64_t cs = (uint64_t)ctx->resident.cs;
  parts->clear();
  parts->resize((size_t)(k1 - k0 + 1));
  std::vector<uint64_t*> res(ctx->devs.size(), nullptr);
  std::vector<R> got;
  return resident_fanout(
      ctx, k0, k1,
      [&](size_t i, DevState& d, const std::vector<int32_t>& chunks, bool* acquired) -> int32_t {
        const uint32_t n = (uint32_t)chunks.size(), grid = u.grid(cs, d.num_cus, ctx->grid_cap[U]);
        StreamScratch& s = d.unit_scratch[U];
        uint64_t* extra;
        int32_t rc = result_acquire(d, s, u.scratch_bytes(grid), n, sizeof(R), n * extra_words * 8, &res[i], &extra);
        if (rc) return rc;
        *acquired = true;
        for (uint32_t j = 0; j < n && !rc; ++j)
          rc = launch_rc(u, chunk(d, chunks[j], extra + j * extra_words, res[i] + (uint64_t)j * u.words, s.buf.ptr,
                                  grid, d.stream));
        return rc;
      },
      [&](size_t i, DevState& d, const std::vector<int32_t>& chunks) {
        got.resize(chunks.size());
        const int32_t rc = result_collect(d, d.unit_scratch[U], u.name, res[i], chunks.size() * sizeof(R), got.data());
        if (!rc)
          for (size_t j = 0; j < got.size(); ++j) (*parts)[(size_t)(chunks[j] - k0)] = got[j];
        return rc;
      });
}

// The parts (at least one), folded into *out in chunk order by the unit's merge.
template <typename R>
int32_t merge_parts(const std::vector<R>& parts, int32_t (*merge)(const R*, const R*, R*), R* out) {
  R acc = parts[0];
  for (size_t j = 1; j < parts.size(); ++j)
    if (int32_t rc = merge(&acc, &parts[j], &acc)) return rc;
  *out = acc;
  return DSE_OK;
}

// *_resident: unit_resident_parts, then merge_parts.
template <SlabUnit U, typename R, typename Chunk>
int32_t unit_resident(dse_ctx* ctx, int32_t k0, int32_t k1, uint64_t extra_words, Chunk&& chunk,
                      int32_t (*merge)(const R*, const R*, R*), R* out) {
  std::vector<R> parts;
  if (int32_t rc = unit_resident_parts<U>(ctx, k0, k1, extra_words, chunk, &parts)) return rc;
  return merge_parts(parts, merge, out);
}

// The pattern and `above` rules of the units that match a pattern against the visible candidates
// (dse_tuples_host.cpp, dse_sums_host.cpp): DSE_EINVAL as dse_tuples_dev_async documents them.
int32_t tuples_check_pattern(uint32_t require, uint32_t forbid);
int32_t tuples_check_above(const uint64_t* above, uint32_t above_shift, uint32_t above_bits);
// Resident chunk k < P sees the first 31 candidates of chunk k + 1 as p's `above`: a pointer into
// that mask when both are on device d, otherwise its first word copied to head_slot (device memory
// of d's) on d.stream. resident_above_check: DSE_EINVAL for chunks shorter than that when a chunk
// from k0 on has a successor. (dse_tuples_host.cpp)
int32_t resident_above_check(dse_ctx* ctx, int32_t k0);
int32_t resident_above(dse_ctx* ctx, DevState& d, int32_t k, uint64_t* head_slot, TuplePattern* p);

// The slab pipe (d.pipe; dse_host.cpp), the device current. ensure_slab_pipe: its stream, events,
// totals and four buffers of min(max(want, 1 MiB), 64 MiB) bytes each, no slot pending.
int32_t ensure_slab_pipe(DevState& d, uint64_t want);
void free_slab_pipe(SlabPipe& p);
// Slot s may be overwritten by work enqueued on `producer` from here on.
int32_t slab_reuse(SlabPipe& p, int s, hipStream_t producer);
// What `producer` has enqueued so far fills slot s: its first `bytes` bytes go to the slot's
// pinned buffer on the copy stream.
int32_t slab_send(SlabPipe& p, int s, uint64_t bytes, hipStream_t producer);
// Blocks until the bytes of slab_send(s) are in the slot's pinned buffer.
int32_t slab_wait(SlabPipe& p, int s);
// After an error: leaves nothing in flight on the buffers.
void slab_drain(SlabPipe& p, hipStream_t producer);

// The slab pipeline of the compactions by rank window (dse_primes_host.cpp), shared by primes as
// numbers and constellations as numbers. A RankSource is a unit's two launches over a device mask of
// nbits candidates that is ready in the stream's order:
//   scan(first, out_cap, totals, tile_sums, stream)              launch_primes_scan's contract,
//   emit(first, out, out_cap, tile_sums, tile0, tiles, stream)   launch_primes_emit's.
// rank_pipeline: mask -> out. The scan runs once on d.stream into d.primes_sums; rank_slabs brings
// the n_out values of ranks [first, first + n_out) of a scanned tile_sums to `out`: the sums are
// copied to the host, and every slab of at most `slab` ranks (the pipe's buffers, or the test option
// primes_slab_entries) is emitted over the tiles that hold its ranks (the sums are monotone: two
// binary searches). Slab i + 1 is emitted on d.stream while slab i's values are copied on the copy
// stream and slab i - 1 is copied into the caller's memory by this thread. The device is current.
struct RankSource {
  uint64_t nbits;
  std::function<hipError_t(uint64_t, uint64_t, unsigned long long*, void*, hipStream_t)> scan;
  std::function<hipError_t(uint64_t, uint64_t*, uint64_t, const void*, uint64_t, uint64_t, hipStream_t)> emit;
};
// DSE_EINVAL for a null `out` with a capacity (out may be null for a count)
int32_t rank_check_out(const uint64_t* out, uint64_t out_cap);
int32_t rank_pipeline(dse_ctx* ctx, DevState& d, const RankSource& src, uint64_t first, uint64_t* out,
                      uint64_t out_cap, uint64_t* total, uint64_t* written);
int32_t rank_slabs(dse_ctx* ctx, DevState& d, const RankSource& src, const void* sums, uint64_t first, uint64_t n_out,
                   uint64_t* out);

}  // namespace dse
#pragma GCC visibility pop
