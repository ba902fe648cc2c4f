/*
 * dse.h -- C ABI of the MI355X-native chunked odd-only sieve (libdse.so).
 *
 * This is the drop-in boundary for the hot path of dpbriggs/Distributed-Sieve-e:
 * the reference's lead/follower entry points (core.clj:136-205) call
 * spread-work / gen-table / sieve-e / finish (sieve.clj:9-172); here those
 * calls become the functions below, which launch hand-written gfx950 HIP
 * kernels. Each declaration names the reference interface it replaces.
 *
 * Conventions
 *  - Every function returns DSE_OK (0) or a negative DSE_E* status; the
 *    message of the last failure on the calling thread is dse_last_error().
 *  - Host output buffers are caller-allocated (ctypes / JNA Memory / FFM
 *    MemorySegment). The library never retains caller pointers.
 *  - Device buffers are owned by the dse_ctx, except in the *_dev entry
 *    points, which take caller-owned device pointers (e.g. torch tensors).
 *  - Calls are blocking (like sieve-e on the caller's main thread,
 *    core.clj:163,196) unless the name ends in _async.
 *  - Chunk semantics are the reference's exactly: cs = floor(floor((n-1)/2)/P),
 *    chunk k (1-based) holds the odd values [3+2(k-1)cs, 3+2k*cs); the
 *    floor((n-1)/2) - P*cs highest odd candidates are dropped (sieve.clj:21-34).
 *  - Mask layout: little-endian uint64 words, bit j of chunk k = 1 iff the
 *    value 3+2((k-1)cs+j) is prime (= element j non-zero before finish);
 *    bits past cs in the last word are 0.
 *  - Supported range: every value 3+2g of a sieved range must be below 2^62,
 *    i.e. the range's last odd index is at most 2^61 - 2 (value 2^62 - 1), so
 *    that the base primes stop at 2^31 - 1 (dse_base_limit_max). Two checks
 *    enforce it, both DSE_ERANGE: the entry points that take an odd-index range
 *    first refuse g_start + nbits > 2^62 (a bound on the INDEX, which keeps
 *    3+2g inside 64 bits; it alone would admit values up to 2^63), then any
 *    range whose largest value is 2^62 + 1 or more is refused because it needs
 *    a base-prime limit of 2^31 or more (dse_sieve_odd_range, dse_sieve_chunk,
 *    dse_sieve_all, dse_sieve_window, dse_finish_range_file,
 *    dse_base_primes_dev_async). dse_sieve_range_dev_async checks only the
 *    index bound: its caller's table fixes the limit.
 */
#ifndef DSE_H
#define DSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSE_OK 0
#define DSE_EINVAL -1   /* bad argument (P < 1, cs < 4 where finish needs it, ...) */
#define DSE_EHIP -2     /* HIP runtime error */
#define DSE_ENCCL -3    /* RCCL error */
#define DSE_ENOMEM -4   /* host or device allocation failed */
#define DSE_EIO -5      /* file I/O */
#define DSE_ERANGE -6   /* input outside the supported range */
#define DSE_EINTERNAL -7 /* device-side invariant broken (bucket capacity overflow); result not valid */

typedef struct dse_ctx dse_ctx;

/* Library version string, e.g. "dse 0.1 gfx950". */
const char *dse_version(void);

/* Message of the last failed call on this thread ("" if none). */
const char *dse_last_error(void);

/* DSE_E* status of the last failed call on this thread (DSE_OK if none); for
 * the entry points that return a pointer (dse_init, dse_init_device). */
int32_t dse_last_status(void);

/* Number of visible HIP devices (0 if none). */
int32_t dse_device_count(void);

/* One process driving num_gpus devices 0..num_gpus-1 (0 = all visible), with
 * one RCCL communicator over them when num_gpus > 1. Replaces the lead's
 * socket server + client wait (core.clj:76-116, 141-147). NULL on failure. */
dse_ctx *dse_init(int32_t num_gpus);

/* One context bound to a single device, for one-process-per-GPU ranks that
 * bring their own communicator (torch.distributed / RCCL). Replaces the
 * follower's connect (core.clj:13-31, 186). NULL on failure. */
dse_ctx *dse_init_device(int32_t device);

void dse_destroy(dse_ctx *ctx);

/* Number of devices the context drives. */
int32_t dse_ctx_num_devices(const dse_ctx *ctx);

/* sieve.clj:15-34 spread-work, in exact int64: lo_hi[2(k-1)], lo_hi[2(k-1)+1]
 * = bounds of chunk k (caller allocates 2*P entries; may be NULL); *cs = chunk
 * size in odd candidates. */
int32_t dse_spread_work(int64_t n, int32_t P, int64_t *lo_hi, int64_t *cs);

/* Odd indices [*g_start, *g_start + *nbits) that spread-work drops
 * (values 3+2P*cs .. n); *nbits <= P-1. */
int32_t dse_tail_range(int64_t n, int32_t P, uint64_t *g_start, uint64_t *nbits);

/* gen-table + sieve-e for ONE chunk (sieve.clj:9-13, 118-172; core.clj:152,
 * 163, 192, 196): sieve chunk my_num of the (n, P) run on the context's
 * device ((my_num-1) mod num_devices). mask_or_null: host buffer of
 * ceil(cs/64) uint64 words, or NULL for count only. *count = primes in the
 * chunk (odd values only; the "2" that finish injects is not counted). */
int32_t dse_sieve_chunk(dse_ctx *ctx, int64_t n, int32_t P, int32_t my_num,
                        uint64_t *mask_or_null, uint64_t *count);

/* gen-table + sieve-e for an arbitrary odd-index range (a chunk given by its
 * bounds [lo, hi): g_start = (lo-3)/2, nbits = (hi-lo)/2), on the context's
 * first device. mask_or_null: ceil(nbits/64) words; *count = primes. */
int32_t dse_sieve_odd_range(dse_ctx *ctx, uint64_t g_start, uint64_t nbits,
                            uint64_t *mask_or_null, uint64_t *count);

/* The whole lead/follower run (core.clj:136-205) on the context's devices:
 * base primes <= sqrt(max value) computed once on device 0 and broadcast with
 * RCCL (replaces the per-prime [mi ps p] relay, sieve.clj:139 /
 * core.clj:118-134), chunk k sieved on device (k-1) mod num_devices with its
 * mask left resident in that device's HBM, the dropped tail sieved on the last
 * device, counts combined with an RCCL all-reduce.
 * per_chunk_counts: P entries (may be NULL). *pi_ref = 1 + sum(counts) (what
 * the reference's files hold); *pi_full = pi_ref + primes in the tail = pi(n).
 * Either pi pointer may be NULL. */
int32_t dse_sieve_all(dse_ctx *ctx, int64_t n, int32_t P, uint64_t *per_chunk_counts,
                      uint64_t *pi_ref, uint64_t *pi_full);

/* Copy chunk my_num's mask kept resident by the last dse_sieve_all into a host
 * buffer of ceil(cs/64) words. DSE_EINVAL if that chunk is not resident. */
int32_t dse_copy_chunk_mask(dse_ctx *ctx, int32_t my_num, uint64_t *mask);

/* Sieve the odd values in [lo, hi] (any 64-bit window, lo,hi odd or even;
 * "segment-only" mode outside the reference's chunk semantics). Counts
 * primes in [max(lo,3), hi] among odd values. With several devices: the base
 * primes are built on device 0 and RCCL-broadcast (as in dse_sieve_all), each
 * device sieves one contiguous slice, the counts are RCCL all-reduced. */
int32_t dse_sieve_window(dse_ctx *ctx, uint64_t lo, uint64_t hi, uint64_t *count);

/* sieve.clj:82-108 finish: write chunk my_num's primes to path, byte-exact
 * with the reference's file: chunk 1 values printed as Java Doubles ("2.0",
 * "1.0000019E7") with the 2/3/5/7 hack, others as Longs; 10 per line,
 * ", "-separated, LF-terminated lines. mask: ceil(cs/64) words. Needs cs >= 4. */
int32_t dse_write_primes_file(const char *path, int32_t my_num, int64_t n, int32_t P,
                              const uint64_t *mask);

/* finish for a chunk given by its odd-index range: same format as
 * dse_write_primes_file; my_num == 1 selects the Double printing + hack. */
int32_t dse_write_range_file(const char *path, int32_t my_num, uint64_t g_start, uint64_t nbits,
                             const uint64_t *mask);

/* ---- Device-resident entry points (one-process-per-GPU ranks) ---------- */

/* Bytes of a base-prime table able to hold every odd prime <= limit. */
uint64_t dse_base_table_bytes(uint64_t limit);

/* Largest base-prime limit the device kernel supports. */
uint64_t dse_base_limit_max(void);

/* isqrt of the largest value in odd-index range [g_start, g_start+nbits):
 * the base-prime limit that range needs. */
uint64_t dse_base_limit_for_range(uint64_t g_start, uint64_t nbits);

/* Build the table of odd primes <= limit into caller-owned device memory
 * table_dev (dse_base_table_bytes(limit) bytes) on stream (hipStream_t, NULL
 * = default). Asynchronous. The table is plain bytes: ranks may broadcast it
 * with any collective (RCCL) before sieving. */
int32_t dse_base_primes_dev_async(dse_ctx *ctx, uint64_t limit, void *table_dev,
                                  uint64_t table_bytes, void *stream);

/* Bytes at the start of a base-prime table that hold the primes themselves
 * (header + p[]). Ranks broadcast only these (the reference's prime
 * broadcast, sieve.clj:139 / core.clj:126) and complete the rest locally with
 * dse_base_table_finish_dev_async. */
uint64_t dse_base_table_prime_bytes(uint64_t limit);

/* How ranks should share the base table for `limit`: the bytes to broadcast
 * from rank 0 (dse_base_table_prime_bytes(limit)), or 0 when every rank should
 * build its own table with dse_base_primes_dev_async instead. The primes are
 * broadcast (as the reference broadcasts them, sieve.clj:139) while they fit
 * in DSE_TABLE_BROADCAST_MAX_BYTES; a larger table (the 1e18 window's 50.8 M
 * primes, 203 MB) is rebuilt on every device, which takes less time than
 * moving it. dse_sieve_all / dse_sieve_window follow
 * the same rule. */
#define DSE_TABLE_BROADCAST_MAX_BYTES (8ull << 20)
uint64_t dse_base_table_broadcast_bytes(uint64_t limit);

/* Complete a table of odd primes <= limit whose first
 * dse_base_table_prime_bytes(limit) bytes are in place (e.g. received by
 * broadcast): Barrett factors and mod-30 wheel offsets, on this context's
 * device. Asynchronous on stream. */
int32_t dse_base_table_finish_dev_async(dse_ctx *ctx, uint64_t limit, void *table_dev,
                                        uint64_t table_bytes, void *stream);

/* Sieve odd indices [g_start, g_start+nbits) with a base table on the device:
 * mask_dev (ceil(nbits/64) uint64 words, or NULL) receives the prime bits,
 * *count_dev (device uint64) is INCREMENTED by the prime count (zero it
 * first). Asynchronous on stream. A device-side failure (DSE_EINTERNAL: a
 * bucket pass over its entry capacity, a rigorous bound, so never expected)
 * sets bit 63 of *count_dev and is reported by dse_device_status.
 * Nothing outside [mask_dev, mask_dev + ceil(nbits/64)) is written, and the
 * last word's bits past nbits are stored as 0. nbits = 0 returns DSE_OK and
 * launches nothing: neither the mask nor *count_dev is touched. The table
 * must hold every odd prime <= dse_base_limit_for_range(g_start, nbits); a
 * larger table serves as well. */
int32_t dse_sieve_range_dev_async(dse_ctx *ctx, const void *table_dev, uint64_t g_start,
                                  uint64_t nbits, uint64_t *mask_dev, uint64_t *count_dev,
                                  void *stream);

/* Wait for the context's last bucketed pass, then read and clear its
 * device-side error flag: DSE_OK, or DSE_EINTERNAL if any pass since the last
 * check overflowed. The blocking entry points check it themselves. */
int32_t dse_device_status(dse_ctx *ctx);

/* ---- finish on the device ---------------------------------------------- */

/* sieve.clj:82-108 finish with the mask staying in device memory: the mask is
 * turned into the file's text on the GPU (same bytes as dse_write_range_file)
 * and only text crosses to the host. */
#define DSE_FINISH_DOUBLES 1u  /* Double.toString printing (chunk 1) */
#define DSE_FINISH_HACK    2u  /* ranks 0..3 are 2 3 5 7, bits 0..3 ignored; needs nbits >= 4 */
#define DSE_FINISH_LAST    4u  /* this slice ends the file: close a partial last line */

/* Rigorous upper bound on the text bytes of `count` entries of the range (host arithmetic only). */
uint64_t dse_finish_text_bound(uint64_t g_start, uint64_t nbits, uint64_t count, uint32_t flags);

/* Format the set bits of mask_dev (range [g_start, g_start+nbits)) as the slice of a finish file
 * whose first entry has rank first_rank. totals_dev[0] = entries, totals_dev[1] = text bytes
 * needed (always written). Text is written to text_dev only if it fits text_cap; otherwise not one
 * byte of text_dev is touched. Asynchronous on stream. Bits past nbits in the last word are
 * ignored. With DSE_FINISH_HACK the slice's first four entries are 2 3 5 7. DSE_ERANGE for a range
 * beyond 2^62, more than 2^44 candidates in one call, or DSE_FINISH_DOUBLES with a value >= 2^53. */
int32_t dse_finish_text_dev_async(dse_ctx *ctx, uint32_t flags, uint64_t g_start, uint64_t nbits,
                                  const uint64_t *mask_dev, uint64_t first_rank,
                                  void *text_dev, uint64_t text_cap, uint64_t *totals_dev, void *stream);

/* finish for chunk my_num kept resident by the last dse_sieve_all: same bytes as
 * dse_copy_chunk_mask + dse_write_primes_file, without the mask leaving the device. The text is
 * formatted in slabs of whole mask words through two device and two pinned host buffers (256 MiB
 * per device in all, kept until dse_destroy): a slab is formatted while the one before it is
 * copied to the host and the one before that is written to the file. */
int32_t dse_finish_resident_file(dse_ctx *ctx, const char *path, int32_t my_num);

/* gen-table + sieve-e + finish for an odd-index range with no host mask:
 * same bytes as dse_sieve_odd_range + dse_write_range_file; *count may be NULL. */
int32_t dse_finish_range_file(dse_ctx *ctx, const char *path, int32_t my_num,
                              uint64_t g_start, uint64_t nbits, uint64_t *count);

/* ---- primes as numbers --------------------------------------------------- */

/* The set bits of a device-resident mask as little-endian uint64 prime values
 * 3 + 2(g_start + bit index), in increasing order, extracted on the GPU. The
 * entries of a range are ranked 0, 1, 2, ... in that order; a call returns the
 * rank window [first, first + out_cap), so a large range can be paged through
 * a small buffer and a count costs no output at all. Bits past nbits in the
 * last word are ignored. DSE_ERANGE for a range beyond 2^62 or more than 2^44
 * candidates in one call. */

/* Async on stream. totals_dev[0] = set bits of the range (always written);
 * totals_dev[1] = elements written = min(out_cap, max(0, total - first)).
 * out_dev[i] = value of the entry of rank first + i. Nothing outside
 * [out_dev, out_dev + totals_dev[1]) is touched; out_dev may be NULL when
 * out_cap == 0 (count only). out_dev must be 8-byte aligned. DSE_EINVAL for a
 * null ctx or totals, a null mask with nbits > 0, a null out_dev with
 * out_cap > 0, or a misaligned out_dev. */
int32_t dse_primes_dev_async(dse_ctx *ctx, uint64_t g_start, uint64_t nbits,
                             const uint64_t *mask_dev, uint64_t first,
                             uint64_t *out_dev, uint64_t out_cap,
                             uint64_t *totals_dev, void *stream);

/* gen-table + sieve-e + extraction of an odd-index range, on the first device; host buffer.
 * *total = primes of the range, *written = values stored to out (either may be NULL); the range
 * rules of dse_sieve_odd_range apply. The values cross to the host in slabs through the two device
 * and two pinned host buffers of the device finish (dse_finish_resident_file): a slab is extracted
 * while the one before it is copied to the host and the one before that is copied into out. */
int32_t dse_primes_range(dse_ctx *ctx, uint64_t g_start, uint64_t nbits, uint64_t first,
                         uint64_t *out, uint64_t out_cap, uint64_t *total, uint64_t *written);

/* The same for chunk my_num left resident by the last dse_sieve_all; DSE_EINVAL if not resident. */
int32_t dse_primes_resident(dse_ctx *ctx, int32_t my_num, uint64_t first,
                            uint64_t *out, uint64_t out_cap, uint64_t *total, uint64_t *written);

/* ---- statistics of a mask ------------------------------------------------- */

/* Constellation counts and prime-gap statistics of a device-resident mask, computed on the GPU in
 * one read of the mask; only the dse_stats crosses to the host. All statistics are over the odd
 * primes of the mask (candidate g is the value 3 + 2g): the prime 2 is in no mask and the gap 2 -> 3
 * is never counted.
 *
 * Pattern: a uint32 with bit 0 set. Bit j set means the candidate j places above must be prime too
 * (the value p + 2j); its span is its bit length (at most 32: differences up to 62). A pattern
 * matches at g when every required candidate g + j is prime, and a match is counted for a range when
 * ALL its members lie inside the range; matches across range ends are counted only by
 * dse_stats_merge. Twins are 0b11, triplets 0b1011 (p, p+2, p+6) and 0b1101 (p, p+4, p+6),
 * quadruplets 0b11011, quintuplets 0b1011011 and 0b1101101, sextuplets 0b101101101 (primesieve's
 * conventions: (3,5) and (5,7) are twins, (3,5,7) matches no triplet pattern). The pattern 1 counts
 * the primes.
 *
 * Gap: the difference of two consecutive primes that both lie in the range. gaps[d] = number of
 * gaps equal to 2d, d < DSE_STATS_GAP_BINS; larger gaps are counted in gap_overflow (synthetic masks
 * only: every prime gap below 2^64 is under 1600). max_gap is exact whatever its size, max_gap_g the
 * odd index of the lower prime of the FIRST such gap; with fewer than two primes max_gap = 0 and
 * max_gap_g = DSE_STATS_NONE.
 *
 * Every member is a uint64_t and there is no padding: bindings may treat a dse_stats as an array of
 * DSE_STATS_WORDS uint64 words. head and tail make two adjacent results mergeable by host
 * arithmetic alone: the candidates either side of a seam are a.tail (last candidate at bit 63)
 * followed by b.head (first candidate at bit 0), a 128-bit window with the seam in the middle. */
#define DSE_STATS_MAX_PATTERNS 8
#define DSE_STATS_GAP_BINS 1024
#define DSE_STATS_NONE UINT64_MAX
#define DSE_STATS_WORDS (27 + DSE_STATS_GAP_BINS)
typedef struct dse_stats {
  uint64_t g_start, nbits;      /* the range the numbers are of */
  uint64_t primes;              /* set bits */
  uint64_t first_g, last_g;     /* odd index of the first / last prime, DSE_STATS_NONE if none */
  uint64_t head;                /* bit i = candidate g_start + i, i < min(64, nbits); other bits 0 */
  uint64_t tail;                /* bit 63 - i = candidate g_start + nbits - 1 - i, i < min(64, nbits); other bits 0 */
  uint64_t npatterns, pattern[DSE_STATS_MAX_PATTERNS], matches[DSE_STATS_MAX_PATTERNS]; /* unused slots 0 */
  uint64_t max_gap, max_gap_g, gap_overflow;
  uint64_t gaps[DSE_STATS_GAP_BINS]; /* gaps[0] stays 0 */
} dse_stats;

/* Async on stream, on a caller-owned device mask. patterns is a host array of npatterns values,
 * passed by value into the launch and never retained. stats_dev: sizeof(dse_stats) bytes of device
 * memory, 8-byte aligned; every member is written and nothing outside it is touched. Bits past
 * nbits in the last word are ignored; nbits = 0 writes the empty result. DSE_EINVAL for a null ctx
 * or stats_dev, a null mask with nbits > 0, a misaligned stats_dev, npatterns > 8, null patterns
 * with npatterns > 0, or a pattern that is 0 or has bit 0 clear. DSE_ERANGE for a range beyond 2^62
 * or more than 2^44 candidates in one call. */
int32_t dse_stats_dev_async(dse_ctx *ctx, uint64_t g_start, uint64_t nbits,
                            const uint64_t *mask_dev, const uint32_t *patterns, uint32_t npatterns,
                            dse_stats *stats_dev, void *stream);

/* gen-table + sieve-e + statistics of an odd-index range, on the first device; host result. The
 * range rules of dse_sieve_odd_range apply. */
int32_t dse_stats_range(dse_ctx *ctx, uint64_t g_start, uint64_t nbits,
                        const uint32_t *patterns, uint32_t npatterns, dse_stats *out);

/* The statistics of chunk my_num left resident by the last dse_sieve_all; my_num = 0: of all P
 * chunks, that is of [3, 3 + 2 P cs), the candidates the reference's files hold. For all chunks,
 * every chunk's launches are enqueued on its own device's stream before any is waited for, and the
 * P results are merged on the host in chunk order. DSE_EINVAL if the chunk is not resident. */
int32_t dse_stats_resident(dse_ctx *ctx, int32_t my_num,
                           const uint32_t *patterns, uint32_t npatterns, dse_stats *out);

/* The statistics of the union of two adjacent ranges, by host arithmetic only; out may alias a or
 * b. Needs a->g_start + a->nbits == b->g_start and equal pattern lists (else DSE_EINVAL; out is not
 * touched); a union that ends above 2^62 gives DSE_ERANGE. Counts and histograms add; the matches
 * that straddle the seam are counted from a->tail and b->head; the seam's gap is added when both
 * sides hold a prime; the maximal gap is taken over a, the seam, then b, keeping the first strictly
 * greatest; head and tail of the union are rebuilt (either side may be shorter than 64 candidates,
 * or empty). */
int32_t dse_stats_merge(const dse_stats *a, const dse_stats *b, dse_stats *out);

/* ---- rank and select ------------------------------------------------------ */

/* Questions about single values or ranks, answered on the GPU from a device-resident mask and its
 * rank index; a query reads one tile of the mask (2 KiB) and only the answers cross to the host.
 * All semantics are over the mask's entries: an entry is a set bit, its value 3 + 2(g_start + bit
 * index); the entries are ranked 0, 1, 2, ... in increasing order, the ranks of dse_primes_*. The
 * prime 2 is in no mask. Every x in 0 .. UINT64_MAX is legal for every kind: even, below 3, below
 * or above the range. */
#define DSE_QUERY_NONE   UINT64_MAX
#define DSE_QUERY_RANK   0u  /* in: value x  -> entries with value <= x (0 below the range, the total at or above its end) */
#define DSE_QUERY_SELECT 1u  /* in: rank k   -> value of the entry of rank k, DSE_QUERY_NONE if k >= total */
#define DSE_QUERY_NEXT   2u  /* in: value x  -> smallest entry value > x, DSE_QUERY_NONE if none */
#define DSE_QUERY_PREV   3u  /* in: value x  -> largest entry value < x, DSE_QUERY_NONE if none */
#define DSE_QUERY_TEST   4u  /* in: value x  -> 1 if x is an entry's value, else 0 (even x, x < 3, x outside the range: 0) */

/* Bytes of the rank index of a range of nbits candidates (host arithmetic only). */
uint64_t dse_query_index_bytes(uint64_t nbits);

/* Build the index of a caller-owned device mask into caller-owned device memory, async on stream:
 * index_dev[t], t = 0 .. tiles (tiles = ceil(nbits / 16384)), is the number of entries in the
 * tiles before t, so index_dev[tiles] is the total. What lies behind those words, up to
 * dse_query_index_bytes(nbits), is the library's. Bits past nbits in the last word are ignored.
 * DSE_EINVAL for a null ctx or index, a null mask with nbits > 0, a misaligned index (8 bytes), or
 * index_bytes below dse_query_index_bytes(nbits). DSE_ERANGE for a range beyond 2^62 or more than
 * 2^44 candidates in one call. */
int32_t dse_query_index_dev_async(dse_ctx *ctx, uint64_t g_start, uint64_t nbits,
                                  const uint64_t *mask_dev, uint64_t *index_dev, uint64_t index_bytes,
                                  void *stream);

/* out_dev[i] = the answer of `kind` to q_dev[i], i < nq, async on stream; index_dev as built by
 * dse_query_index_dev_async for the same range and mask. Queries come in any order, duplicates
 * allowed. Nothing outside [out_dev, out_dev + nq) is written; nq = 0 launches nothing. Bits past
 * nbits in the last word are ignored; nbits = 0 is legal (rank 0, everything else
 * DSE_QUERY_NONE or 0). DSE_QUERY_TEST reads no index: index_dev may be NULL for it. DSE_EINVAL
 * for a null ctx, an unknown kind, null q_dev or out_dev with nq > 0, a null mask with nbits > 0,
 * a null index for a kind that needs it, or a pointer that is not 8-byte aligned. DSE_ERANGE as
 * above. */
int32_t dse_query_dev_async(dse_ctx *ctx, uint32_t kind, uint64_t g_start, uint64_t nbits,
                            const uint64_t *mask_dev, const uint64_t *index_dev,
                            const uint64_t *q_dev, uint64_t nq, uint64_t *out_dev, void *stream);

/* gen-table + sieve-e + index + queries of an odd-index range, on the first device; host arrays.
 * The range rules of dse_sieve_odd_range apply. DSE_ENOMEM when the device buffers for nq queries
 * and answers cannot be had. */
int32_t dse_query_range(dse_ctx *ctx, uint32_t kind, uint64_t g_start, uint64_t nbits,
                        const uint64_t *q, uint64_t nq, uint64_t *out);

/* Queries against chunk my_num left resident by the last dse_sieve_all; my_num = 0: against all P
 * chunks as the one range [3, 3 + 2 P cs) (dse_stats_resident's convention; the dropped tail is in
 * no mask and in no answer). A chunk's index is built on its own device and stream by the first
 * call that needs it and kept until dse_sieve_all replaces the masks or dse_destroy. For all
 * chunks the host routes each query to the chunk that holds its candidate (its rank, for
 * DSE_QUERY_SELECT), enqueues every chunk's batch on its device's stream before it waits for any,
 * and completes the answers from the chunks' totals and first and last entries. DSE_EINVAL if the
 * chunk is not resident. */
int32_t dse_query_resident(dse_ctx *ctx, int32_t my_num, uint32_t kind,
                           const uint64_t *q, uint64_t nq, uint64_t *out);

/* ---- additive questions ---------------------------------------------------- */

/* Minimal Goldbach partitions, computed on the GPU from a device-resident mask; only the
 * dse_goldbach crosses to the host.
 *
 * Evens. The even of candidate index c is e(c) = 6 + 2c = 3 + (3 + 2c), so a range [g_start,
 * g_start + nbits) owns exactly nbits evens, adjacent ranges own adjacent evens, and [0, n) owns
 * 6, 8, ..., 4 + 2n. The even 4 = 2 + 2 belongs to no range, as the prime 2 is in no mask.
 *
 * Small primes. P_i is the i-th odd prime (P_0 = 3) and h_i = (P_i - 3) / 2. A call uses the first
 * nprimes of the DSE_GOLDBACH_PRIMES = 2048 (P_2047 = 17881, h_2047 = 8939); nprimes is 1..2048,
 * and 0 means 2048. Its reach is h_(nprimes - 1): dse_goldbach_reach.
 *
 * Partition. e(c) - P_i = 3 + 2 (c - h_i), so partition i of e(c) holds iff candidate c - h_i is a
 * visible entry (a set bit). The range's own candidates are visible, and so are the `below`
 * candidates [g_start - below_bits, g_start) the caller supplies; anything lower, or below
 * candidate 0, is not an entry. The minimal rank of e(c) is the smallest i < nprimes whose
 * partition holds; with none, e(c) is unresolved. When all candidates down to 0 are visible the
 * minimal p is automatically <= q.
 *
 * Every member is a uint64_t and there is no padding: bindings may treat a dse_goldbach as an array
 * of DSE_GOLDBACH_WORDS uint64 words. */
#define DSE_GOLDBACH_PRIMES 2048
#define DSE_GOLDBACH_NONE UINT64_MAX
#define DSE_GOLDBACH_WORDS (8 + DSE_GOLDBACH_PRIMES)
typedef struct dse_goldbach {
  uint64_t g_start, nbits;      /* the range the numbers are of */
  uint64_t nprimes;             /* small primes used, 1..2048 */
  uint64_t resolved, unresolved; /* resolved + unresolved == nbits */
  uint64_t first_unresolved;    /* lowest global index c of an unresolved even, DSE_GOLDBACH_NONE if none */
  uint64_t max_rank;            /* largest minimal rank over the resolved evens, DSE_GOLDBACH_NONE if none */
  uint64_t max_c;               /* lowest global index c whose even attains it, DSE_GOLDBACH_NONE if none */
  uint64_t hist[DSE_GOLDBACH_PRIMES]; /* hist[i] = evens whose minimal rank is i; slots >= nprimes are 0 */
} dse_goldbach;

/* P_i, the i-th odd prime (P_0 = 3); 0 for i >= DSE_GOLDBACH_PRIMES. */
uint64_t dse_goldbach_prime(uint32_t i);

/* h of the last of the first nprimes small primes (0 means 2048): how far below its own candidate
 * an even's partitions look. Host arithmetic only; 0 for nprimes above 2048. */
uint64_t dse_goldbach_reach(uint32_t nprimes);

/* Async on stream, on a caller-owned device mask (bit c = candidate g_start + c). Candidate
 * g_start - below_bits + j, j < below_bits, is bit below_shift + j of the bit string at below_dev:
 * below_shift < 64, below_bits <= g_start, below_dev 8-byte aligned, NULL allowed when below_bits =
 * 0. So `below` may be a pointer into a larger mask, with no copy. Only the whole words that cover
 * those bits are read, and only the last dse_goldbach_reach(nprimes) of the bits can matter. Every
 * member of *out_dev (sizeof(dse_goldbach) bytes of device memory, 8-byte aligned) is written and
 * nothing outside it is touched. Bits past nbits in the last mask word are ignored; nbits = 0
 * writes the empty result. DSE_EINVAL for a null ctx or out_dev, a null mask with nbits > 0, a
 * misaligned mask_dev, below_dev or out_dev, nprimes > 2048, below_shift > 63, below_bits >
 * g_start, or a null below_dev with below_bits > 0. DSE_ERANGE for a range beyond 2^62 or more than
 * 2^44 candidates in one call. */
int32_t dse_goldbach_dev_async(dse_ctx *ctx, uint64_t g_start, uint64_t nbits,
                               const uint64_t *mask_dev, const uint64_t *below_dev,
                               uint32_t below_shift, uint64_t below_bits, uint32_t nprimes,
                               dse_goldbach *out_dev, void *stream);

/* gen-table + sieve-e + minimal partitions of an odd-index range, on the first device; host
 * result. The range is sieved together with the min(g_start, reach) candidates below it, which the
 * kernel sees as `below` (a pointer and a shift into the same scratch mask): every even of the
 * range gets its true minimal partition. The range rules of dse_sieve_odd_range apply. */
int32_t dse_goldbach_range(dse_ctx *ctx, uint64_t g_start, uint64_t nbits, uint32_t nprimes,
                           dse_goldbach *out);

/* The same for chunk my_num left resident by the last dse_sieve_all; my_num = 0: for all P chunks,
 * that is for [3, 3 + 2 P cs) (dse_stats_resident's convention). Chunk k > 1 sees the tail of chunk
 * k - 1 as its `below`: a pointer into that mask when both are on one device, otherwise a copy of
 * those whole words into this device's scratch. Every device's launches are enqueued on its own
 * stream before any is waited for, and the results are merged on the host in chunk order.
 * DSE_EINVAL if the chunk is not resident, and when a chunk that needs a `below` is shorter than
 * dse_goldbach_reach(nprimes) (the message says so: lower nprimes). */
int32_t dse_goldbach_resident(dse_ctx *ctx, int32_t my_num, uint32_t nprimes, dse_goldbach *out);

/* The result of the union of two adjacent ranges, by host arithmetic only; out may alias a or b.
 * Needs a->g_start + a->nbits == b->g_start and equal nprimes (else DSE_EINVAL; out is not
 * touched); a union that ends above 2^62 gives DSE_ERANGE. Counts and the histogram add; the
 * maximum keeps the first strictly greatest; first_unresolved is a's if a has one, otherwise b's.
 * Each side must have been computed with the candidates below it visible (b's `below` = a's tail). */
int32_t dse_goldbach_merge(const dse_goldbach *a, const dse_goldbach *b, dse_goldbach *out);

/* ---- residue classes and races ---------------------------------------------- */

/* pi(x; q, r) for every class r mod q, and the race between two classes (Chebyshev's bias),
 * computed on the GPU from a device-resident mask; only the dse_race crosses to the host.
 *
 * Entries. An entry is a set bit of the mask; its value is v = 3 + 2 (g_start + bit index). The
 * prime 2 is in no mask: a race from 3 on that involves its class (2 mod q, q odd) counts it by
 * starting from d_start = -1 or +1.
 *
 * Modulus. 3 <= q <= DSE_RACE_MAX_MODULUS = 64.
 *
 * Class counts. counts[r], r < q, is the number of entries with v mod q == r; slots r >= q are 0. A
 * prime that divides q is counted in its own class like any other: 3 is in class 3 mod 4, and in
 * class 0 mod 3.
 *
 * Race. For residues a != b (both < q) a step is an entry whose value is = a or = b (mod q). D
 * starts at the caller's d_start (an int64) and goes +1 at every a-step and -1 at every b-step, in
 * increasing order of value. Every race number is about the value of D after a step of the range:
 * steps is their number; a_ahead, b_ahead and ties count the steps after which D > 0, D < 0 and
 * D == 0 (they sum to steps); first_a_ahead and first_b_ahead are the global candidate index g of
 * the first step after which D > 0 and D < 0, DSE_RACE_NONE if there is none; max_d is the largest
 * D after a step and max_g the g of the first step that attains it, min_d and min_g likewise; with
 * no step in the range max_d = min_d = d_start and max_g = min_g = DSE_RACE_NONE; d_end is D after
 * the last step (d_start if there is none). A class that holds no odd candidate (q = 4, a = 2) is
 * legal and never steps.
 *
 * Counts only. a == b means no race: it requires d_start == 0 (else DSE_EINVAL), only counts[] is
 * computed, steps, a_ahead, b_ahead, ties, max_d, min_d and d_end are 0, the four positions are
 * DSE_RACE_NONE, and the race pass is not launched.
 *
 * d_start, d_end, max_d and min_d hold an int64 in two's complement. Every member is a uint64_t and
 * there is no padding: bindings may treat a dse_race as an array of DSE_RACE_WORDS uint64 words. */
#define DSE_RACE_MAX_MODULUS 64
#define DSE_RACE_NONE UINT64_MAX
#define DSE_RACE_WORDS (17 + DSE_RACE_MAX_MODULUS)
typedef struct dse_race {
  uint64_t g_start, nbits;             /* the range the numbers are of */
  uint64_t q, a, b;
  uint64_t d_start, d_end;             /* int64, two's complement */
  uint64_t steps, a_ahead, b_ahead, ties;
  uint64_t first_a_ahead, first_b_ahead;
  uint64_t max_d, max_g, min_d, min_g; /* *_d int64 */
  uint64_t counts[DSE_RACE_MAX_MODULUS];
} dse_race;

/* Async on stream, on a caller-owned device mask (bit c = candidate g_start + c). Every member of
 * *out_dev (sizeof(dse_race) bytes of device memory, 8-byte aligned) is written and nothing
 * outside it is touched. Bits past nbits in the last mask word are ignored; nbits = 0 writes the
 * empty result. DSE_EINVAL for a null ctx or out_dev, a null mask with nbits > 0, a misaligned
 * mask_dev or out_dev, q outside 3..64, a or b >= q, or a == b with d_start != 0. DSE_ERANGE for
 * |d_start| > 2^45, a range beyond 2^62 or more than 2^44 candidates in one call. */
int32_t dse_race_dev_async(dse_ctx *ctx, uint64_t g_start, uint64_t nbits, const uint64_t *mask_dev,
                           uint32_t q, uint32_t a, uint32_t b, int64_t d_start, dse_race *out_dev,
                           void *stream);

/* gen-table + sieve-e + the race of an odd-index range, on the first device; host result. The
 * range rules of dse_sieve_odd_range apply. */
int32_t dse_race_range(dse_ctx *ctx, uint64_t g_start, uint64_t nbits, uint32_t q, uint32_t a,
                       uint32_t b, int64_t d_start, dse_race *out);

/* The same for chunk my_num left resident by the last dse_sieve_all; my_num = 0: for all P chunks
 * as the one range [3, 3 + 2 P cs) (dse_stats_resident's convention). Chunk k + 1 starts from chunk
 * k's d_end, so for several chunks with a != b the chunks' class counts are taken first, on every
 * device and enqueued before any is waited for; the host forms the running d_start of every chunk,
 * then every chunk's race is enqueued and the results are merged in chunk order. DSE_EINVAL if the
 * chunk is not resident. */
int32_t dse_race_resident(dse_ctx *ctx, int32_t my_num, uint32_t q, uint32_t a, uint32_t b,
                          int64_t d_start, dse_race *out);

/* The result of the union of two adjacent ranges, by host arithmetic only; out may alias a or b.
 * Needs a->g_start + a->nbits == b->g_start, equal q, a and b, and b->d_start == a->d_end (else
 * DSE_EINVAL; out is not touched); a union that ends above 2^62 gives DSE_ERANGE. Counts and the
 * four step counters add; first_* is a's if a has one, otherwise b's; the maximum keeps the first
 * strictly greatest and the minimum the first strictly smallest, and a side with steps == 0 takes
 * no part in either. */
int32_t dse_race_merge(const dse_race *a, const dse_race *b, dse_race *out);

/* ---- constellations as numbers ----------------------------------------------- */

/* Where the matches of a pattern are: the positions of a device-resident mask at which a pattern
 * matches, as little-endian uint64 values, in increasing order, extracted on the GPU. The counting
 * half is dse_stats' matches[] and gaps[].
 *
 * Pattern. Two uint32: `require`, with bit 0 set as a dse_stats pattern has, and `forbid`, with
 * require & forbid == 0. Bit j of require: the candidate j places above must be an entry; bit j of
 * forbid: it must not be. The span is the bit length of require | forbid (<= 32). forbid = 0 gives
 * exactly the dse_stats patterns; require = 1 | 1 << d with forbid = the bits 1 .. d - 1 lists the
 * consecutive primes exactly 2d apart, d <= 31.
 *
 * Visible candidates. The range's own nbits candidates, followed by above_bits <= 31 candidates of
 * the caller's: the bits of the bit string at `above` from bit above_shift < 64 on (the way
 * dse_goldbach_dev_async takes `below`). `above` is 8-byte aligned, may be NULL when above_bits == 0
 * and may point into a larger mask: only the whole words that cover the bits are read.
 *
 * Match. Position i < nbits matches when i + span <= nbits + above_bits, every required candidate is
 * a visible entry and every forbidden one is visible and not an entry. A match belongs to the range
 * that holds its lowest member, so adjacent ranges that each see the next one's head as `above` list
 * every match of their union exactly once, in order. With forbid = 0 and above_bits = 0 this is
 * dse_stats' rule "all members inside the range".
 *
 * Output. The matches are ranked 0, 1, ... in increasing position; the value of a match is
 * 3 + 2 (g_start + i), its lowest member. A call returns the rank window [first, first + out_cap)
 * as dse_primes_* do, so a count costs no output. */

/* Async on stream. totals_dev[0] = matches of the range (always written); totals_dev[1] = elements
 * written = min(out_cap, max(0, matches - first)); out_dev[i] = value of the match of rank
 * first + i. Nothing outside [out_dev, out_dev + totals_dev[1]) is touched; out_dev may be NULL when
 * out_cap == 0 (count only) and must be 8-byte aligned. Bits past nbits in the last mask word are
 * ignored; nbits = 0 writes totals 0, 0. DSE_EINVAL for a null ctx or totals, a null mask with
 * nbits > 0, a null out_dev with out_cap > 0, a misaligned out_dev, require with bit 0 clear,
 * require & forbid != 0, above_bits > 31, above_shift > 63, or a null or misaligned above_dev with
 * above_bits > 0. DSE_ERANGE for visible candidates beyond 2^62 or more than 2^44 candidates in
 * one call. */
int32_t dse_tuples_dev_async(dse_ctx *ctx, uint64_t g_start, uint64_t nbits,
                             const uint64_t *mask_dev, uint32_t require, uint32_t forbid,
                             const uint64_t *above_dev, uint32_t above_shift, uint32_t above_bits,
                             uint64_t first, uint64_t *out_dev, uint64_t out_cap,
                             uint64_t *totals_dev, void *stream);

/* gen-table + sieve-e + the matches of an odd-index range, on the first device; host buffer. The
 * range is sieved together with the candidates above it in one scratch mask (31 of them, fewer where
 * the 2^62 bound ends them), which are its `above`. *total = matches of the range, *written = values
 * stored to out (either may be NULL); the values cross to the host through dse_primes_range's slab
 * pipeline. */
int32_t dse_tuples_range(dse_ctx *ctx, uint64_t g_start, uint64_t nbits, uint32_t require,
                         uint32_t forbid, uint64_t first, uint64_t *out, uint64_t out_cap,
                         uint64_t *total, uint64_t *written);

/* The same for chunk my_num left resident by the last dse_sieve_all; my_num = 0: for all P chunks
 * as the one range [3, 3 + 2 P cs) (dse_stats_resident's convention). Chunk k < P sees the first 31
 * candidates of chunk k + 1 (a pointer into that mask when both are on one device, otherwise that
 * one word copied); chunk P has no `above`: the dropped tail is in no mask. Every chunk's size and
 * scan launches are enqueued on its device's stream before any is waited for; the host forms the
 * running totals, cuts the rank window per chunk, and each chunk's slice goes through the slab
 * pipeline to its offset in out. DSE_EINVAL if the chunk is not resident, or for chunks of fewer
 * than 31 candidates when a chunk with a successor is asked for. */
int32_t dse_tuples_resident(dse_ctx *ctx, int32_t my_num, uint32_t require, uint32_t forbid,
                            uint64_t first, uint64_t *out, uint64_t out_cap, uint64_t *total,
                            uint64_t *written);

/* ---- where the gaps are ----------------------------------------------------- */

/* The first occurrence of every prime gap of a device-resident mask (A000230) and, from it, the
 * maximal or record gaps (A002386, A005250), computed on the GPU in one read of the mask; only the
 * dse_gaps crosses to the host. Candidates, entries, values and g are dse_stats': candidate g is the
 * value 3 + 2g, an entry is a set bit. A gap is the difference of two consecutive entries that both
 * lie in the range: it has d places (the difference of the candidate indices) and the value 2d, and
 * its position is the global candidate index g of its lower prime. The prime 2 is in no mask and the
 * gap 2 -> 3 is never seen.
 *
 * first[d] = position of the first gap of exactly d places, d < DSE_GAPS_BINS, DSE_GAPS_NONE where
 * the range has none; first[0] is always DSE_GAPS_NONE. found counts the bins that are not NONE.
 * Gaps of DSE_GAPS_BINS places and more (synthetic masks only: every prime gap below 2^64 is under
 * 1600) have one bin, overflow_g, the position of the first of them. max_gap and max_gap_g are
 * exactly dse_stats' members: max_gap is exact whatever its size, max_gap_g the position of the
 * FIRST such gap; with fewer than two primes max_gap = 0 and max_gap_g = DSE_GAPS_NONE.
 *
 * Every member is a uint64_t and there is no padding: bindings may treat a dse_gaps as an array of
 * DSE_GAPS_WORDS uint64 words. */
#define DSE_GAPS_BINS 1024
#define DSE_GAPS_NONE UINT64_MAX
#define DSE_GAPS_WORDS (9 + DSE_GAPS_BINS)
typedef struct dse_gaps {
  uint64_t g_start, nbits;     /* the range the numbers are of */
  uint64_t primes;             /* set bits */
  uint64_t first_g, last_g;    /* first / last entry, DSE_GAPS_NONE if none */
  uint64_t found;              /* bins d < DSE_GAPS_BINS with first[d] != NONE */
  uint64_t max_gap, max_gap_g; /* exactly dse_stats' members: 2d of the longest gap, g of the FIRST such; 0 / NONE */
  uint64_t overflow_g;         /* g of the first gap of >= DSE_GAPS_BINS places (synthetic masks only), NONE */
  uint64_t first[DSE_GAPS_BINS]; /* first[d] = g of the lower prime of the first gap of exactly d places; NONE if there is none; first[0] is always NONE */
} dse_gaps;

/* Async on stream, on a caller-owned device mask. out_dev: sizeof(dse_gaps) bytes of device memory,
 * 8-byte aligned; every member is written and nothing outside it is touched. Bits past nbits in the
 * last word are ignored; nbits = 0 writes the empty result. DSE_EINVAL for a null ctx or out_dev, a
 * null mask with nbits > 0 or a misaligned out_dev. DSE_ERANGE for a range beyond 2^62 or more than
 * 2^44 candidates in one call. */
int32_t dse_gaps_dev_async(dse_ctx *ctx, uint64_t g_start, uint64_t nbits,
                           const uint64_t *mask_dev, dse_gaps *out_dev, void *stream);

/* gen-table + sieve-e + the table of an odd-index range, on the first device; host result. The
 * range rules of dse_sieve_odd_range apply. */
int32_t dse_gaps_range(dse_ctx *ctx, uint64_t g_start, uint64_t nbits, dse_gaps *out);

/* The table of chunk my_num left resident by the last dse_sieve_all; my_num = 0: of all P chunks,
 * that is of [3, 3 + 2 P cs) (dse_stats_resident's convention). For all chunks, every chunk's
 * launches are enqueued on its own device's stream before any is waited for, and the P results are
 * merged on the host in chunk order: the merge rebuilds a seam's gap from the two sides' last and
 * first entry, so no chunk sees its neighbour. DSE_EINVAL if the chunk is not resident. */
int32_t dse_gaps_resident(dse_ctx *ctx, int32_t my_num, dse_gaps *out);

/* The table of the union of two adjacent ranges, by host arithmetic only; out may alias a or b.
 * Needs a->g_start + a->nbits == b->g_start (else DSE_EINVAL; out is not touched); a union that ends
 * above 2^62 gives DSE_ERANGE. primes adds; first_g / last_g come from whichever side has them. With
 * an entry on both sides the seam's gap has s = b->first_g - a->last_g places at position a->last_g,
 * which lies above every position of a and below every one of b: first[d] is a's if set, else the
 * seam's if d == s, else b's; overflow_g is decided the same way, the seam counting when s >=
 * DSE_GAPS_BINS. The maximal gap is taken over a, the seam, then b, keeping the first strictly
 * greatest; found is recounted. The merge is associative, with empty and prime-less pieces on
 * either side. */
int32_t dse_gaps_merge(const dse_gaps *a, const dse_gaps *b, dse_gaps *out);

/* The maximal gaps of the range, by host arithmetic: bin d (1 <= d < DSE_GAPS_BINS) is a record when
 * first[d] != NONE and no longer gap starts lower, in a higher bin or at overflow_g. *count = their
 * number; their d go to d_out in increasing order, up to cap of them. d_out may be NULL with cap = 0.
 * DSE_EINVAL for a null g or count, or a null d_out with cap > 0. */
int32_t dse_gaps_records(const dse_gaps *g, uint32_t *d_out, uint32_t cap, uint32_t *count);

/* ---- power and reciprocal sums ----------------------------------------------- */

/* Sums over the matches of a pattern in a device-resident mask, computed on the GPU in one read of
 * the mask; only the dse_sums crosses to the host: the sum of the primes (A046731 less the prime 2),
 * of their squares, of their reciprocals (Mertens), and Brun-type sums over constellations such as
 * B2 = sum of 1/p + 1/(p + 2) over the twins. Candidates, entries, values and g are dse_stats'. The
 * pattern (require, forbid), the visible candidates (above / above_shift / above_bits <= 31) and
 * the match rule are exactly dse_tuples': a match belongs to the range that holds its lowest member,
 * so adjacent ranges that each see the next one's head count every match of their union once.
 * require = 1, forbid = 0 sums over the primes, require = 3 over the twins, require = 1 | 1 << d with
 * forbid = the bits 1 .. d - 1 over the consecutive primes exactly 2d apart.
 *
 * The value of a match at position i is v = 3 + 2 (g_start + i), its lowest member, as dse_tuples
 * reports it. Every sum is an exact integer in little-endian uint64 limbs, so a result does not
 * depend on the order of the additions and dse_sums_merge is plain addition:
 *   sum1  = sum of v, sum2 = sum of v^2 (flag DSE_SUMS_POWER, else 0);
 *   recip = sum over the matches, over every set bit j of require, of floor(2^126 / (v + 2j))
 *           (flag DSE_SUMS_RECIP, else 0): the fixed-point sum of the reciprocals of all required
 *           members, the convention of Brun-type constants: 1/5 counts in (3, 5) and in (5, 7).
 *           With require = 1 it is the sum of floor(2^126 / p).
 * matches, first_g and last_g are always written.
 *
 * Bounds. v >= 3, so a term is below 2^125. The sum of 1/v over all odd v < 2^62 is under 23, which
 * with 32 members gives recip < 23 * 32 * 2^126 < 2^141. The sieve's values are below 2^62 and there
 * are fewer than 2^61 of them, so sum1 < 2^123 and sum2 < 2^61 * 2^124 = 2^185. A caller's mask may
 * reach the odd-index bound 2^62 (values below 2^63 + 2, 2^62 candidates): then sum1 < 2^126,
 * sum2 < 2^189 and the reciprocals still sum to less than 24. No limb can overflow, even after
 * merging the whole accepted range. Every floor loses less than 1, so the true sum of the
 * reciprocals lies in [recip / 2^126, (recip + matches * popcount(require)) / 2^126].
 *
 * Every member is a uint64_t and there is no padding: bindings may treat a dse_sums as an array of
 * DSE_SUMS_WORDS uint64 words. */
#define DSE_SUMS_POWER 1u /* sum1, sum2 */
#define DSE_SUMS_RECIP 2u /* recip */
#define DSE_SUMS_NONE UINT64_MAX
#define DSE_SUMS_RECIP_SHIFT 126
#define DSE_SUMS_WORDS 17
typedef struct dse_sums {
  uint64_t g_start, nbits;                     /* the range the numbers are of */
  uint64_t require, forbid, above_bits, flags; /* what the numbers are of */
  uint64_t matches;                            /* always */
  uint64_t first_g, last_g; /* g of the lowest / highest match, DSE_SUMS_NONE if none; always */
  uint64_t sum1[2];         /* sum of v,   128 bits, little-endian limbs; 0 without POWER */
  uint64_t sum2[3];         /* sum of v^2, 192 bits;                     0 without POWER */
  uint64_t recip[3]; /* sum over matches, over every set bit j of require, of floor(2^126 / (v + 2j)), 192 bits; 0 without RECIP */
} dse_sums;

/* Async on stream, on a caller-owned device mask. out_dev: sizeof(dse_sums) bytes of device memory,
 * 8-byte aligned; every member is written and nothing outside it is touched. flags: any of
 * DSE_SUMS_POWER | DSE_SUMS_RECIP; 0 gives the count and the positions only. Bits past nbits in the
 * last mask word are ignored; nbits = 0 writes the empty result (0 matches, NONE, zero sums).
 * DSE_EINVAL for a null ctx or out_dev, a null mask with nbits > 0, a misaligned out_dev, flags with
 * unknown bits, require with bit 0 clear, require & forbid != 0, above_bits > 31, above_shift > 63,
 * or a null or misaligned above_dev with above_bits > 0. DSE_ERANGE for visible candidates beyond
 * 2^62 or more than 2^44 candidates in one call. */
int32_t dse_sums_dev_async(dse_ctx *ctx, uint64_t g_start, uint64_t nbits, const uint64_t *mask_dev,
                           uint32_t require, uint32_t forbid, const uint64_t *above_dev,
                           uint32_t above_shift, uint32_t above_bits, uint32_t flags,
                           dse_sums *out_dev, void *stream);

/* gen-table + sieve-e + the sums of an odd-index range, on the first device; host result. The range
 * is sieved together with the candidates above it in one scratch mask (31 of them, fewer where the
 * 2^62 bound ends them), which are its `above`, as dse_tuples_range does. */
int32_t dse_sums_range(dse_ctx *ctx, uint64_t g_start, uint64_t nbits, uint32_t require,
                       uint32_t forbid, uint32_t flags, dse_sums *out);

/* The sums of chunk my_num left resident by the last dse_sieve_all; my_num = 0: of all P chunks, that
 * is of [3, 3 + 2 P cs) (dse_stats_resident's convention). Chunk k < P sees the first 31 candidates
 * of chunk k + 1 exactly as dse_tuples_resident arranges it; chunk P has no `above`. For all chunks,
 * every chunk's launches are enqueued on its own device's stream before any is waited for, and the
 * P results are merged on the host in chunk order. DSE_EINVAL if the chunk is not resident, or for
 * chunks of fewer than 31 candidates when a chunk with a successor is asked for. */
int32_t dse_sums_resident(dse_ctx *ctx, int32_t my_num, uint32_t require, uint32_t forbid,
                          uint32_t flags, dse_sums *out);

/* The sums of the union of two adjacent ranges, by host arithmetic only; out may alias a or b. Needs
 * a->g_start + a->nbits == b->g_start, equal require, forbid and flags, and a->above_bits >=
 * min(span - 1, b->nbits + b->above_bits): a must have seen across the seam (else DSE_EINVAL; out is
 * not touched). A union that ends above 2^62 gives DSE_ERANGE. matches and the sums add with
 * carries; first_g / last_g come from whichever side has them; out->above_bits = b->above_bits. The
 * merge is associative, with empty pieces on either side. */
int32_t dse_sums_merge(const dse_sums *a, const dse_sums *b, dse_sums *out);

/* ---- residue pairs of consecutive primes -------------------------------------- */

/* The joint distribution of the classes mod q of consecutive primes of a device-resident mask, the
 * q x q matrix N(a, b) = #{consecutive primes p < p' of the range : p = a, p' = b (mod q)} of Lemke
 * Oliver and Soundararajan's "Unexpected biases in the distribution of consecutive primes" (2016),
 * computed on the GPU in one read of the mask; only the dse_consec crosses to the host. Candidates,
 * entries, values and g are dse_stats': candidate g is the value 3 + 2g, an entry is a set bit. The
 * modulus is 3 <= q <= DSE_CONSEC_MAX_MODULUS, as dse_race's.
 *
 * A pair is two consecutive entries that both lie in the range (dse_gaps' rule for a gap).
 * counts[a * 64 + b] = number of pairs whose lower value is = a and whose upper value is = b (mod q).
 * Slots with a >= q or b >= q are 0, and so are the rows and columns of the residues that hold no
 * odd candidate (q even, r even). A prime that divides q sits in its own class like any other: for
 * q = 3 from g = 0 the pair (3, 5) is counts[0 * 64 + 2] = 1. The prime 2 is in no mask and the pair
 * (2, 3) is never seen. pairs = primes - 1 (0 with fewer than two primes) = the sum of counts[]; the
 * row sums of counts[] are dse_race's counts[] less the last entry, the column sums less the first.
 *
 * Every member is a uint64_t and there is no padding: bindings may treat a dse_consec as an array of
 * DSE_CONSEC_WORDS uint64 words. */
#define DSE_CONSEC_MAX_MODULUS 64
#define DSE_CONSEC_NONE UINT64_MAX
#define DSE_CONSEC_WORDS (7 + DSE_CONSEC_MAX_MODULUS * DSE_CONSEC_MAX_MODULUS)
typedef struct dse_consec {
  uint64_t g_start, nbits;   /* the range the numbers are of */
  uint64_t q;
  uint64_t primes;           /* set bits */
  uint64_t pairs;            /* primes - 1, or 0 with fewer than two primes; == sum of counts[] */
  uint64_t first_g, last_g;  /* first / last entry, DSE_CONSEC_NONE if none (dse_gaps' members) */
  uint64_t counts[DSE_CONSEC_MAX_MODULUS * DSE_CONSEC_MAX_MODULUS]; /* counts[a * 64 + b] */
} dse_consec;

/* Async on stream, on a caller-owned device mask. out_dev: sizeof(dse_consec) bytes of device
 * memory, 8-byte aligned; every member is written and nothing outside it is touched. Bits past nbits
 * in the last word are ignored; nbits = 0 writes the empty result. DSE_EINVAL for a null ctx or
 * out_dev, a null mask with nbits > 0, a misaligned out_dev or mask_dev, or q outside 3..64.
 * DSE_ERANGE for a range beyond 2^62 or more than 2^44 candidates in one call. */
int32_t dse_consec_dev_async(dse_ctx *ctx, uint64_t g_start, uint64_t nbits,
                             const uint64_t *mask_dev, uint32_t q, dse_consec *out_dev,
                             void *stream);

/* gen-table + sieve-e + the matrix of an odd-index range, on the first device; host result. The
 * range rules of dse_sieve_odd_range apply. */
int32_t dse_consec_range(dse_ctx *ctx, uint64_t g_start, uint64_t nbits, uint32_t q,
                         dse_consec *out);

/* The matrix of chunk my_num left resident by the last dse_sieve_all; my_num = 0: of all P chunks,
 * that is of [3, 3 + 2 P cs) (dse_stats_resident's convention). For all chunks, every chunk's
 * launches are enqueued on its own device's stream before any is waited for, and the P results are
 * merged on the host in chunk order: the merge rebuilds a seam's pair from the two sides' last and
 * first entry, so no chunk sees its neighbour. DSE_EINVAL if the chunk is not resident. */
int32_t dse_consec_resident(dse_ctx *ctx, int32_t my_num, uint32_t q, dse_consec *out);

/* The matrix of the union of two adjacent ranges, by host arithmetic only; out may alias a or b.
 * Needs a->g_start + a->nbits == b->g_start and a->q == b->q in 3..64 (else DSE_EINVAL; out is not
 * touched); a union that ends above 2^62 gives DSE_ERANGE. counts and primes add; first_g / last_g
 * come from whichever side has them. With an entry on both sides the seam's pair
 * ((3 + 2 a->last_g) mod q, (3 + 2 b->first_g) mod q) is counted once; pairs is recomputed. The
 * merge is associative, with empty and prime-less pieces on either side. */
int32_t dse_consec_merge(const dse_consec *a, const dse_consec *b, dse_consec *out);

/* ---- Test-only ---------------------------------------------------------- */

/* Set a test-only option of this context (the production library reads no
 * environment variable; defaults are the production configuration):
 *   "bucket_pass_segments" = k > 0: bucketed passes of at most k segments
 *   (covers the multi-pass path on small windows); 0 = default.
 *   "bucket_split_log2" = k in 0..63: bucketed primes <= 2^k take the
 *   one-level fill, larger ones the two-level staged fill; 0 = the default
 *   split (2^28).
 *   "wheel_geometry" = 0 (default): a range's last partial round of full
 *   segments is sieved as half-size segments when that is faster; 1: full
 *   segments only; 2: half-size segments only (covers that kernel in tests).
 *   "bucket_cap_divisor" = d >= 0: divide each pass's bucket entry capacities
 *   by d (> 1), forcing the overflow path (DSE_EINTERNAL); 0 or 1 = default.
 *   "bucket_k0_divisor" = d >= 0: divide the band-0 region capacity by d
 *   (> 1), so hits go through the spill list (results unchanged); 0 or 1 =
 *   default.
 *   "scratch_poison" = 1: fill the bucket scratch with 0xFF bytes before
 *   every bucketed pass (stale contents: results unchanged, and an overflowed
 *   pass still reads only what it wrote); 0 = default.
 *   "bucket_lo_log2" = k in 17..20 (at most the build's wheel limit, 2^20 in
 *   production): a range that needs the bucketed pass (sqrt of its largest
 *   value above 2^20) buckets every prime above 2^k instead of the production
 *   threshold; 0 = default.
 *   "table_broadcast_max_bytes" = b > 0: dse_sieve_all / dse_sieve_window
 *   broadcast the table's primes while they take at most b bytes and build
 *   the table on every device above that; 0 = default
 *   (DSE_TABLE_BROADCAST_MAX_BYTES).
 *   "rccl_single" = 1: give a one-device context (dse_init(1) or
 *   dse_init_device) a 1-rank RCCL communicator (ncclCommInitAll), so
 *   dse_sieve_all / dse_sieve_window issue the same grouped ncclBroadcast of
 *   the primes and ncclAllReduce of the counts as an 8-GPU context instead of
 *   skipping them (the RCCL path exercised on a one-GPU box); 0 = default (no
 *   communicator, no collective for one device).
 *   "finish_slab_words" = k > 0: dse_finish_resident_file / dse_finish_range_file
 *   format slabs of at most k mask words (slab seams on tiny inputs); 0 = default.
 *   "primes_slab_entries" = k > 0: dse_primes_range / dse_primes_resident move
 *   slabs of at most k values (slab seams on tiny inputs); 0 = default.
 *   "stats_grid" = k in 1..1024: the dse_stats_* launches use at most k
 *   workgroups, so one workgroup walks several tiles and the closing launch
 *   sums several slabs on tiny inputs; 0 = default (3 per compute unit).
 *   "query_grid" = k in 1..1024: the dse_query_* launches use at most k
 *   workgroups, so a wave takes several queries on tiny inputs; 0 = default
 *   (8 per compute unit).
 *   "goldbach_grid" = k in 1..1024: the dse_goldbach_* launches use at most k
 *   workgroups, so one workgroup walks several tiles and the closing launch
 *   sums several slabs on tiny inputs; 0 = default (one resident round).
 *   "race_grid" = k in 1..1024: the dse_race_* launches use at most k
 *   workgroups, so one workgroup walks several tiles, a workgroup's D starts
 *   from the slabs before its own and the closing launch reduces several slabs
 *   on tiny inputs; 0 = default (one resident round).
 *   "gaps_grid" = k in 1..1024: the dse_gaps_* launches use at most k
 *   workgroups, so one workgroup walks several tiles and the closing launch
 *   reduces several slabs on tiny inputs; 0 = default (one resident round).
 *   "sums_grid" = k in 1..1024: the dse_sums_* launches use at most k
 *   workgroups, so one workgroup walks several tiles and the closing launch
 *   adds several slabs on tiny inputs; 0 = default (one resident round).
 *   "consec_grid" = k in 1..1024: the dse_consec_* launches use at most k
 *   workgroups, so one workgroup walks several tiles and the closing launch
 *   sums several slabs and counts their seams' pairs on tiny inputs; 0 =
 *   default (one resident round).
 *   "consec_flush_tiles" = k in 1..262143: a workgroup of the dse_consec_*
 *   main kernel empties its 32-bit counters into its slab's 64-bit bins every
 *   k tiles, so tiny inputs run the flush; 0 = default (262143 tiles: a bin
 *   grows by at most 64 pairs per word and tile).
 *   "consec_body" = 1: the in-word pairs are counted by the bit-parallel body
 *   whenever it is built for the period (T <= 6); 2: by the per-entry body for
 *   every period; 0 = default (the measured threshold). The results are the
 *   same; the bench tool's A/B.
 * DSE_EINVAL for an unknown name or a value out of range. */
int32_t dse_debug_set_option(dse_ctx *ctx, const char *name, int64_t value);

/* Read a test-only statistic of this context into *value:
 *   "rccl_calls": RCCL collectives (one per device and call) accepted so far;
 *   "rccl_comms": communicators the context holds;
 *   "rccl_ranks": ranks of its communicator as ncclCommCount reports (0: none);
 *   "table_local_builds": base tables built on a device of their own instead
 *   of broadcast (one per device and call);
 *   "primes_tile_bits": candidates per tile of the dse_primes_* kernels;
 *   "stats_tile_bits": candidates per tile of the dse_stats_* kernels;
 *   "gaps_tile_bits": candidates per tile of the dse_gaps_* main kernel;
 *   "sums_tile_bits": candidates per tile of the dse_sums_* main kernels;
 *   "query_index_builds": rank indices dse_query_resident has built for
 *   resident chunks so far (one per chunk and dse_sieve_all that replaced the
 *   masks);
 *   "wheel_ta", "wheel_tb1", "wheel_tb": the wheel kernel's unit thresholds as
 *   built (a prime p > 79 is marked by an A unit up to wheel_ta, a B1 unit up
 *   to wheel_tb1, a B2 unit up to wheel_tb, an L unit above);
 *   "wheel_max_prime": the largest prime the wheel kernel marks itself (the
 *   table's m[], a[] and pl[] are filled up to it; larger primes are bucketed);
 *   "wheel_log_kp": log2 of the periods of 30 integers in a full segment.
 * The "plan_*" names describe what the context's most recent sieving entry
 * point (dse_sieve_odd_range, dse_sieve_chunk, dse_sieve_all, dse_sieve_window,
 * dse_sieve_range_dev_async, and the calls that sieve a range before they
 * finish, extract or count it) launched to sieve its ranges: host-side
 * counters, cleared when the entry point begins, summed over the context's
 * devices (the two maxima: taken over them). The launches that build a base
 * table are not counted. A test that is about later rounds, the full / half
 * split or several super-buckets asserts them, so that it fails when its
 * shape stops producing what it is about (another CU count, other cost
 * constants):
 *   "plan_wheel_launches": launches of the wheel kernel (the batches of 9
 *   ranges of a pooled launch and the bucketed passes count one each);
 *   "plan_full_segments": full-size segments launched without bucket units;
 *   "plan_half_segments": half-size segments launched;
 *   "plan_max_rounds": the largest ceil(segments / workgroups) of a wheel
 *   launch, workgroups = min(segments, CUs): above 1, workgroups carried
 *   state from one segment to their next;
 *   "plan_bucket_passes": bucketed passes;
 *   "plan_bucket_max_pass_segments": the largest of them, in segments;
 *   "plan_bucket_max_lds_bytes": the largest dynamic LDS size a pass gave to
 *   its fill-and-stage launch, in bytes (above 65,536 the launch needs the
 *   kernel's opt-in to more dynamic LDS: passes of more than 7,936 segments
 *   with band-1 primes).
 * DSE_EINVAL for an unknown name. */
int32_t dse_debug_get_stat(dse_ctx *ctx, const char *name, int64_t *value);

/* A context of num_logical devices that all run on device 0 (each its own
 * stream, table, counts, masks and scratch; a device's chunks are pooled into
 * one persistent launch, as on a real device), so the multi-device
 * code of dse_sieve_all / dse_sieve_window -- chunk map, table completion on
 * the non-root devices, tail on the last device, flag checks -- runs on a
 * one-GPU box. Only the two RCCL collectives are replaced: the broadcast of
 * the primes by a device-to-device copy from device 0's table, the count
 * all-reduce by a gather + sum on device 0 and a copy back, each ordered
 * with events exactly where the RCCL calls would run. Test-only; NULL on
 * failure (dse_last_status). */
dse_ctx *dse_debug_init_logical(int32_t num_logical);

/* The wheel kernel's block transform of its expand phase, run on the host
 * (no device call): planes[i] = plane i's word of one image block (bit k set:
 * the candidate of period k is composite), variant = (V0 mod 30) / 2 of the
 * range. Writes the block's 15 output words: bit 15k + slot_i is set exactly
 * when bit k of planes[i] is clear, slot_i being the i-th smallest of
 * ((r - 1)/2 - variant) mod 15 over the residues r coprime to 30. Test-only;
 * DSE_EINVAL for a variant outside 0..14 or a null pointer. */
int32_t dse_debug_expand_block(int32_t variant, const uint32_t planes[8], uint32_t out[15]);

/* The finish kernels' own per-value formatter, run on the host (no device
 * call): prints v into out as a Long, or with DSE_FINISH_DOUBLES as
 * Double.toString prints it (v < 2^53), and returns the length (no
 * terminator; at most 24 bytes). Test-only; DSE_EINVAL (negative) for a null
 * pointer or a flag other than DSE_FINISH_DOUBLES. */
int32_t dse_debug_finish_format(uint64_t v, uint32_t flags, char out[32]);

/* The dse_primes_* emit kernel's own per-word body, run on the host (no device
 * call): word's set bits are entries of ranks rank0, rank0 + 1, ... in
 * increasing bit order, bit b having the value 3 + 2(g_word_start + b). The
 * values of the entries whose rank lies in [first, first + cap) are written to
 * out[0], out[1], ... in that order; returns how many (0..64). Test-only;
 * negative: DSE_EINVAL for a null pointer, DSE_ERANGE for g_word_start + 64 or
 * rank0 above 2^62. */
int32_t dse_debug_primes_word(uint64_t word, uint64_t g_word_start, uint64_t rank0, uint64_t first,
                              uint64_t cap, uint64_t out[64]);

/* The dse_stats_* kernels' own per-word bodies, run on the host in a plain loop
 * over the words of a host mask (no device call): the same result as
 * dse_stats_dev_async on the same bits. Test-only; DSE_EINVAL / DSE_ERANGE as
 * dse_stats_dev_async for the mask, the patterns and the range. */
int32_t dse_debug_stats_host(const uint64_t *mask, uint64_t g_start, uint64_t nbits,
                             const uint32_t *patterns, uint32_t npatterns, dse_stats *out);

/* The dse_query_* kernel's own per-word and per-tile bodies, run on the host over
 * a host mask (no device call): the same answers as dse_query_index_dev_async +
 * dse_query_dev_async on the same bits. Test-only; DSE_EINVAL / DSE_ERANGE as
 * dse_query_dev_async for the kind, the pointers and the range. */
int32_t dse_debug_query_host(const uint64_t *mask, uint64_t g_start, uint64_t nbits, uint32_t kind,
                             const uint64_t *q, uint64_t nq, uint64_t *out);

/* The dse_goldbach_* kernel's own per-word bodies, run on the host in a plain loop
 * over the tiles and words of a host mask and a host `below` (no device call): the
 * same result as dse_goldbach_dev_async on the same bits. Test-only; DSE_EINVAL /
 * DSE_ERANGE as dse_goldbach_dev_async for the pointers, nprimes, `below` and the
 * range. */
int32_t dse_debug_goldbach_host(const uint64_t *mask, uint64_t g_start, uint64_t nbits,
                                const uint64_t *below, uint32_t below_shift, uint64_t below_bits,
                                uint32_t nprimes, dse_goldbach *out);

/* The dse_race_* kernels' own per-word bodies, run on the host in a plain loop over
 * the words of a host mask (no device call): the same result as dse_race_dev_async
 * on the same bits. Test-only; DSE_EINVAL / DSE_ERANGE as dse_race_dev_async for
 * the pointers, q, a, b, d_start and the range. */
int32_t dse_debug_race_host(const uint64_t *mask, uint64_t g_start, uint64_t nbits, uint32_t q,
                            uint32_t a, uint32_t b, int64_t d_start, dse_race *out);

/* The dse_gaps_* kernels' own per-word bodies, run on the host in a plain loop over
 * the tiles and words of a host mask (no device call), the settled bins refreshed
 * per tile as the main kernel does: the same result as dse_gaps_dev_async on the
 * same bits. Test-only; DSE_EINVAL / DSE_ERANGE as dse_gaps_dev_async for the
 * pointers and the range. */
int32_t dse_debug_gaps_host(const uint64_t *mask, uint64_t g_start, uint64_t nbits, dse_gaps *out);

/* The dse_consec_* kernels' own per-word bodies, run on the host in a plain loop over
 * the tiles and words of a host mask (no device call), the in-word pairs by the body
 * the launch would take for q: the same result as dse_consec_dev_async on the same
 * bits. Test-only; DSE_EINVAL / DSE_ERANGE as dse_consec_dev_async for the pointers,
 * q and the range. */
int32_t dse_debug_consec_host(const uint64_t *mask, uint64_t g_start, uint64_t nbits, uint32_t q,
                              dse_consec *out);

/* The dse_sums_* kernels' own per-word and per-entry bodies, run on the host in a plain loop over
 * the words of a host mask and a host `above` (no device call), the device's division routine
 * included (not the compiler's 128-bit divide): the same result as dse_sums_dev_async on the same
 * bits. Test-only; DSE_EINVAL / DSE_ERANGE as dse_sums_dev_async for the pointers, the pattern,
 * `above`, the flags and the range. */
int32_t dse_debug_sums_host(const uint64_t *mask, uint64_t g_start, uint64_t nbits, uint32_t require,
                            uint32_t forbid, const uint64_t *above, uint32_t above_shift,
                            uint32_t above_bits, uint32_t flags, dse_sums *out);

/* That division routine alone, on the host: out[2i], out[2i + 1] = the low and high word of
 * floor(2^126 / v[i]), i < n, for any v[i] >= 3. Test-only; DSE_EINVAL for a null pointer with
 * n > 0, DSE_ERANGE for a v[i] below 3 (nothing is written). */
int32_t dse_debug_sums_recip(const uint64_t *v, uint64_t n, uint64_t *out);

/* The dse_tuples_* kernels' own per-word body, run on the host in a plain loop over
 * the words of a host mask and a host `above` (no device call): the same totals and
 * values as dse_tuples_dev_async on the same bits. Test-only; DSE_EINVAL /
 * DSE_ERANGE as dse_tuples_dev_async for the pointers, the pattern, `above` and the
 * range. */
int32_t dse_debug_tuples_host(const uint64_t *mask, uint64_t g_start, uint64_t nbits,
                              uint32_t require, uint32_t forbid, const uint64_t *above,
                              uint32_t above_shift, uint32_t above_bits, uint64_t first,
                              uint64_t *out, uint64_t out_cap, uint64_t totals[2]);

/* The wheel kernel's integer helpers, run elementwise on the device by the
 * functions the kernels themselves call: out_dev[i] = op(x_dev[i], y_dev[i])
 * for i < n, enqueued on `stream`; y is always the modulus p, and the float
 * reciprocal the helpers take is formed from p as the kernel's units form it.
 * With TB = "wheel_tb" and PMAX = "wheel_max_prime" of dse_debug_get_stat, the
 * ops and their domains (outside a domain the result is unspecified; the call
 * reads and writes only the n words of each array whatever they hold):
 *   KBMOD_F32      x mod p by one float quotient: x < 2^32 (the low 32 bits of
 *                  x are reduced whatever the rest holds), TB < p <= PMAX;
 *   KBMOD_F38      x mod p as the launches without bucketed primes reduce it
 *                  (one float quotient below 2^32, two above): x < 2^38,
 *                  TB < p <= PMAX;
 *   KBMOD_BARRETT  x mod p as the bucketed launches reduce it (the two above,
 *                  the 64-bit Barrett reduction from 2^38 on): x < 2^63,
 *                  TB < p <= PMAX;
 *   MOD_BARRETT    x mod p by the Barrett reduction: x < 2^63, 2 <= p < 2^32;
 *   BARRETT_FACTOR floor((2^64 - 1) / p), the factor the two ops above compute
 *                  for themselves: 2 <= p < 2^32 (x is read and ignored);
 *   DIV_SMALL      floor(x / p), DIV_CEIL_SMALL ceil(x / p): x < 2^24,
 *                  7 <= p <= TB;
 *   MULMOD_SMALL   a b mod p, x = a | b << 32: a, b < p, 7 <= p <= TB;
 *   PLANE_FIRST    the smallest k >= 0 with p | Xs + rho + 30k, x = Xs | rho << 32:
 *                  Xs < p, rho < 30, 7 <= p <= TB coprime to 30;
 *   FIRST_AT_OR_AFTER the smallest k >= start with k = kp (mod p),
 *                  x = kp | start << 32: kp < p, start < 2^23, 7 <= p <= TB.
 * A y below 2 or above 2^32 - 1 gives 0 for every op. Test-only; n = 0 launches
 * nothing. DSE_EINVAL for a null ctx, an unknown op, a null pointer with n > 0
 * or a pointer that is not 8-byte aligned. */
#define DSE_ARITH_KBMOD_F32 0u
#define DSE_ARITH_KBMOD_F38 1u
#define DSE_ARITH_KBMOD_BARRETT 2u
#define DSE_ARITH_MOD_BARRETT 3u
#define DSE_ARITH_BARRETT_FACTOR 4u
#define DSE_ARITH_DIV_SMALL 5u
#define DSE_ARITH_DIV_CEIL_SMALL 6u
#define DSE_ARITH_MULMOD_SMALL 7u
#define DSE_ARITH_PLANE_FIRST 8u
#define DSE_ARITH_FIRST_AT_OR_AFTER 9u
int32_t dse_debug_wheel_arith_dev(dse_ctx *ctx, uint32_t op, const uint64_t *x_dev, const uint64_t *y_dev,
                                  uint64_t n, uint64_t *out_dev, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DSE_H */
