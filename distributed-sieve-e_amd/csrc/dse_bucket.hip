// dse_bucket.hip -- the bucketed pass of the wheel sieve: its kernels, their
// capacity bounds, the scratch buffer's lifetime and the pass planner
// (launch_bucketed). It shares the segment geometry, WheelArgs and the entry
// format with the wheel kernel (dse_wheel_geometry.h, dse_wheel_args.h) and
// runs that kernel over each pass through launch_wheel_bucketed
// (dse_wheel.hip).
#include "dse_block.h"
#include "dse_wheel_args.h"

namespace dse {
namespace {

static_assert(kWheelLogKP == 17, "bucketed passes feed the full geometry's kernel");

// ---------------------------------------------------------------------------
// Bucketed pass of the ranges whose sqrt(max value) exceeds kWheelMaxPrime
// (high-offset windows) for their primes above 2^kBucketLoLog (or the
// bucket_lo_log2 option): such a prime hits a 3.9 M-integer segment about
// 2^20 / p times (at most twice), so instead of
// visiting every (prime, segment) pair the kernels below walk each prime's
// multiples p*m, gcd(m, 30) = 1, across the whole range once and file every
// hit under its segment (bucket_entry). Band 0 (one level): each fill
// workgroup files its hits into per-(segment, workgroup) regions of a fixed
// capacity, overflow into a spill list. Band 1 (two levels): two identical
// walks, count (LDS per-segment counters -> per-workgroup column) and stage
// (regions from the scanned columns), then a sort by segment. The wheel
// kernel ORs its segment's band-0 regions, band-1 list and spilled hits.
// ---------------------------------------------------------------------------
constexpr uint32_t kBucketThreads = 256;
#ifndef DSE_BK_SEGS
#define DSE_BK_SEGS 8192
#endif
#ifndef DSE_BK_GRID1
#define DSE_BK_GRID1 4096
#endif
// Two bands of bucketed primes: band 0 (p <= split, kBucketGrid workgroups)
// is filled one level, band 1 (p > split, kBucketGrid1 workgroups) staged in
// two levels; the count kernel's columns are band 1's workgroups.
constexpr uint32_t kBucketGrid = DSE_BK_GRID;
constexpr uint32_t kBucketGrid1 = DSE_BK_GRID1;
constexpr uint32_t kBucketCols = kBucketGrid1;
static_assert(kBucketCols % 64 == 0, "column scan: whole lanes");
#ifndef DSE_BK_SPLIT_LOG
#define DSE_BK_SPLIT_LOG 28
#endif
constexpr uint32_t kBucketSplitLog = DSE_BK_SPLIT_LOG;  // production split: primes <= 2^28 one-level
// bucketed ranges bucket the primes above 2^kBucketLoLog (<= kWheelMaxPrime;
// profiles/r05/window_bucket_lo.txt)
constexpr uint32_t kBucketLoLog = 19;
static_assert((1ull << kBucketLoLog) <= kWheelMaxPrime && kBucketLoLog >= 17, "bucket threshold");
constexpr uint32_t kBucketMaxSegs = DSE_BK_SEGS; // segments per pass (LDS counters)
constexpr uint32_t kCoprime30 = (1u << 1) | (1u << 7) | (1u << 11) | (1u << 13) | (1u << 17) | (1u << 19) |
                                (1u << 23) | (1u << 29);
// gap from R30[w] to the next coprime residue: 6 4 2 4 2 4 6 2 (3 bits each)
constexpr uint32_t kGap30 = 6u | (4u << 3) | (2u << 6) | (4u << 9) | (2u << 12) | (4u << 15) | (6u << 18) | (2u << 21);

struct BucketArgs {
  uint64_t V0;         // v_start - 1 of the pass
  uint64_t span;       // integers covered by the pass: nseg * kWheelSpan
  uint64_t plane_lut;  // plane of relative residue rho (odd) in bits [3(rho >> 1), +3)
  uint32_t nseg;       // segments in the pass (<= kBucketMaxSegs)
  uint64_t vmax;       // largest value of the pass (primes with p^2 > vmax have no hits)
  uint64_t split;      // band 0: 2^kBucketLoLog < p <= split, band 1: p > split
};

// Band-0 output of a pass (bucket_fill_wg).
struct BandZero {
  uint32_t* reg0;                  // [kBucketGrid][nseg][k0] regions
  uint32_t* n0;                    // [nseg][kBucketGrid] region fills
  unsigned long long* spill;       // segment << 32 | entry
  uint32_t* nspill;                // spill list length
  uint32_t k0;                     // region capacity
  uint64_t spill_cap;              // spill list capacity (rigorous)
  uint32_t* flag;                  // scratch flag[0] (sticky overflow) ...
  unsigned long long* count;       // ... and bit 63 of the count, if the spill list overflows
};

// First index in [lo, hi) where the ascending table P has P[i] > bound (hi
// if none), by one wave: 64 pivots per step (a step's loads are independent,
// so a 50 M-prime table takes 4 dependent loads instead of 26).
__device__ uint32_t wave_upper_bound(const uint32_t* __restrict__ P, uint32_t lo, uint32_t hi, uint64_t bound,
                                     bool squared) {
  const uint32_t lane = threadIdx.x & 63;
  auto le = [&](uint32_t i) { const uint64_t p = P[i]; return (squared ? p * p : p) <= bound; };
  while (hi - lo > 64) {
    const uint32_t step = (hi - lo + 63) / 64, i = lo + lane * step;
    const uint32_t c = (uint32_t)__popcll(__ballot(i < hi && le(i)));  // pivots at or below the bound
    if (c == 0) return lo;
    const uint32_t nhi = min(hi, lo + c * step);  // the answer is in (pivot c-1, pivot c]
    lo += (c - 1) * step + 1;
    hi = nhi;
  }
  return lo + (uint32_t)__popcll(__ballot(lo + lane < hi && le(lo + lane)));
}

// range[0] = first table index with p > lo_p (the pass's bucket threshold),
// range[1] = first with p^2 > vmax, range[2] = first with p > split (clamped
// to [range[0], range[1]]). One wave.
__global__ __launch_bounds__(64) void bucket_range_kernel(const void* __restrict__ table, uint64_t lo_p, uint64_t vmax,
                                                          uint64_t split, uint32_t* __restrict__ range,
                                                          uint32_t* __restrict__ nspill) {
  const TableHeader* th = reinterpret_cast<const TableHeader*>(table);
  const uint32_t np = th->count == 0xFFFFFFFFu ? 0u : th->count;
  const uint32_t* P = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(table) + 16);
  const uint32_t i_lo = wave_upper_bound(P, 0, np, lo_p, false);
  const uint32_t i_hi = max(i_lo, wave_upper_bound(P, i_lo, np, vmax, true));
  const uint32_t i_sp = wave_upper_bound(P, i_lo, i_hi, split, false);
  if (threadIdx.x == 0) {
    range[0] = i_lo;
    range[1] = i_hi;
    range[2] = i_sp;
    *nspill = 0;  // the band-0 spill list of this pass
  }
}

// First coprime-to-30 multiple of p at or above max(V0 + 1, p^2): its offset
// o from V0 and 3 * (index of the multiplier mod 30 in R30).
__device__ __forceinline__ uint64_t bucket_first(uint32_t p, const BucketArgs& ba, uint32_t& w3) {
  const uint64_t p2 = (uint64_t)p * p;
  const uint64_t vlo = max(ba.V0 + 1, p2);
  // floor(vlo / p) from a double quotient: vlo < 2^62 rounds by < 2^9 and
  // p > 2^17, so the estimate is within 1 of the truth; corrected exactly
  uint64_t q = (uint64_t)((double)vlo / (double)p);
  int64_t rs = (int64_t)(vlo - q * p);
  while (rs < 0) { rs += p; --q; }
  while (rs >= (int64_t)p) { rs -= p; ++q; }
  const uint64_t r = (uint64_t)rs;
  const uint64_t m0 = q + (r != 0);
  const uint32_t r30 = (uint32_t)(m0 % 30);
  const uint32_t d = __builtin_ctz(kCoprime30 >> r30);
  w3 = 3 * __popc(kCoprime30 & ((1u << (r30 + d)) - 1));
  return (uint64_t)p * (m0 + d) - ba.V0;
}

// The hit at offset o (< span): its segment s and entry = the LDS word index
// of (period k, plane) in the wheel kernel's image << 5 | k & 31, i.e. the
// address and bit the wheel kernel ORs, decoded here where the walk has VALU
// to spare (the fill kernels are bound by their stores), not in the wheel
// kernel (mark_entry). Word index = 8 * block + plane < 2^15, so an entry is
// < 2^20.
__device__ __forceinline__ uint32_t bucket_entry(uint64_t o, const BucketArgs& ba, uint32_t& s) {
  s = ((uint32_t)(o >> kWheelLogKP)) / 30u;  // o < 2^34
  const uint32_t u = (uint32_t)(o - (uint64_t)s * kWheelSpan);
  const uint32_t k = u / 30u, rho = u - 30u * k;
  const uint32_t pl = (uint32_t)(ba.plane_lut >> (3 * (rho >> 1))) & 7u;
  const uint32_t word = ((k >> 5) << 3) | pl;  // block k >> 5, plane pl
  return (word << 5) | (k & 31u);
}

// Grid-strided walk (workgroup b of its band) over this thread's bucketed
// primes [i_lo, i_hi): each prime is loaded one prime ahead, so the load's
// latency hides behind the previous prime's walk (loaded on demand, a
// thread's ~200 primes were a chain of dependent global loads: ~0.7 ms per
// walk at the 1e18 window).
template <typename Walk>
__device__ __forceinline__ void for_bucket_primes(const uint32_t* __restrict__ P, uint32_t i_lo, uint32_t i_hi,
                                                  uint32_t b, uint32_t stride, Walk walk) {
  uint32_t i = i_lo + b * kBucketThreads + threadIdx.x;
  if (i >= i_hi) return;
  uint32_t pn = P[i];
  for (;;) {
    const uint32_t p = pn;
    i += stride;
    const bool more = i < i_hi;
    if (more) pn = P[i];
    walk(p);
    if (!more) break;
  }
}

// Walk the coprime-to-30 multiples of p inside [V0 + 1, V0 + span), from p^2 on.
template <typename Emit>
__device__ __forceinline__ void bucket_walk(uint32_t p, const BucketArgs& ba, Emit emit) {
  uint32_t w3;
  uint64_t o = bucket_first(p, ba, w3);
  while (o < ba.span) {
    uint32_t s;
    const uint32_t e = bucket_entry(o, ba, s);
    emit(s, e);
    o += (uint64_t)p * ((kGap30 >> w3) & 7u);
    w3 = w3 == 21 ? 0u : w3 + 3;
  }
}

__global__ __launch_bounds__(kBucketThreads) void bucket_count_kernel(const void* __restrict__ table, BucketArgs ba,
                                                                    const uint32_t* __restrict__ range,
                                                                    uint32_t* __restrict__ cols) {
  extern __shared__ uint32_t cnt[];  // [nseg]
  const uint32_t* P = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(table) + 16);
  for (uint32_t j = threadIdx.x; j < ba.nseg; j += kBucketThreads) cnt[j] = 0;
  __syncthreads();
  // band-1 workgroup x: column x
  for_bucket_primes(P, range[2], range[1], blockIdx.x, kBucketGrid1 * kBucketThreads, [&](uint32_t p) {
    bucket_walk(p, ba, [&](uint32_t sg, uint32_t) { atomicAdd(&cnt[sg], 1u); });
  });
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < ba.nseg; j += kBucketThreads) cols[(uint64_t)j * kBucketCols + blockIdx.x] = cnt[j];
}

// per segment (one wave each): exclusive scan of its row over the virtual
// workgroups, in place; total -> tot[s]
__global__ __launch_bounds__(256) void bucket_colscan_kernel(uint32_t* __restrict__ cols, uint32_t nseg,
                                                             uint32_t* __restrict__ tot) {
  constexpr uint32_t kPer = kBucketCols / 64;
  const uint32_t sg = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (sg >= nseg) return;
  uint32_t* c = cols + (uint64_t)sg * kBucketCols + lane * kPer;
  uint32_t v[kPer], sum = 0;
#pragma unroll
  for (uint32_t t = 0; t < kPer; ++t) sum += (v[t] = c[t]);
  uint32_t x = sum;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) tot[sg] = x;
  x -= sum;
#pragma unroll
  for (uint32_t t = 0; t < kPer; ++t) {
    c[t] = x;
    x += v[t];
  }
}

// exclusive scan of the segment totals -> start[0..nseg]. A total above the
// entry capacity (a rigorous bound, so never expected) sets *flag: the fill,
// stage and sort kernels of the pass then skip (the fill only zeroing its
// band-0 region fills), every segment's list is left empty (start[] all 0,
// n0[] all 0) and the pass's count gets bit 63 set, so neither an
// out-of-bounds store nor a silently wrong count can result; the host entry
// points report it as DSE_EINTERNAL (dse_device_status).
__global__ __launch_bounds__(kSliceThreads) void bucket_startscan_kernel(const uint32_t* __restrict__ tot, uint32_t nseg,
                                                                uint32_t* __restrict__ start, uint64_t cap,
                                                                uint32_t* __restrict__ flag,
                                                                unsigned long long* __restrict__ count) {
  __shared__ uint32_t s_wave[kSliceThreads / 64];
  const ScanSlice<uint32_t> s = slice_scan(nseg, s_wave, [&](uint32_t b) { return tot[b]; });
  const bool over = s.total > cap;  // every thread sees the same total
  uint32_t run = s.start;
  for (uint32_t b = s.b0; b < s.b1; ++b) {
    const uint32_t t = tot[b];
    start[b] = over ? 0u : run;
    run += t;
  }
  if (threadIdx.x == 0) {
    start[nseg] = over ? 0u : s.total;
    if (over) {
      flag[1] = 1u;  // this pass (read by the kernels below)
      flag[0] = 1u;  // sticky, cleared by dse_device_status
      atomicOr(count, 1ull << 63);
    } else {
      flag[1] = 0u;
    }
  }
}

#ifndef DSE_BK_CHUNK
#define DSE_BK_CHUNK 16  // band-0 fill walks chunks of this many segments (first group of kFillRG rounds) ...
#endif
#ifndef DSE_BK_CHUNK_GROW
#define DSE_BK_CHUNK_GROW 1  // ... doubled for each later group, up to 8x (profiles/r06/window_fill_chunks.txt)
#endif
#ifndef DSE_BK_FILL_RG
#define DSE_BK_FILL_RG 16
#endif
constexpr uint32_t kFillRG = DSE_BK_FILL_RG;  // stride rounds of primes walked together

// Band 0, one-level fill: every hit is one dword store at its slot. Workgroup
// b owns region (s, b) of every segment s: k0 slots at reg0 + (b nseg + s) k0
// (a workgroup's regions are contiguous, so a slot is a 32-bit offset from
// one scalar base), slot = an LDS cursor per segment. No count pass: k0
// bounds the region's expected fill by many standard deviations (bucket_k0),
// and a hit past it goes to the spill list (a global atomic; the list's
// capacity is a rigorous bound on the band's hits), so nothing is dropped
// whatever k0 is. At the end the region fills go to n0[s kBucketGrid + b]
// (capped at k0).
//
// The walk is issue-bound (profiles/r06/window_fill_knockouts.txt: without
// its atomics and stores it still takes 2/3 of the fill's time), so a hit
// costs as few VALU as the walk allows: a prime's state is its period index
// k = o / 30 from V0 (32 bits: a pass spans < 2^30 periods) and its wheel
// step w, kept as w4 = 4 w; everything that depends on the step comes from
// 4-bit fields at bit 4 w (v_bfe reads only the low 5 bits of the offset, so
// w4 just counts up): the gap, the carry of the residue, and the plane. With
// p = 30 pq + pm and residue rho_w of step w, the next hit is
// k + pq gap_w + (rho_w + pm gap_w) / 30; bucket_fill_start builds the carry
// and plane fields once per prime (eight residues from the first hit's).
constexpr uint64_t kFillMaxSplit = 30ull << 24;  // band-0 primes p < 30 * 2^24: p / 30 < 2^24 (v_mul_u32_u24)
static_assert((1ull << kBucketSplitLog) <= kFillMaxSplit, "production split");
constexpr uint32_t kGap30x4 = 6u | (4u << 4) | (2u << 8) | (4u << 12) | (2u << 16) | (4u << 20) | (6u << 24) | (2u << 28);

struct FillWalk {
  uint32_t k;       // period index of the next hit from V0 (~0u: none left in the pass)
  uint32_t w4;      // 4 * wheel step (mod 32 as used)
  uint32_t pq;      // p / 30
  uint32_t carry;   // 4-bit fields: (rho_w + pm gap_w) / 30
  uint32_t plane;   // 4-bit fields: plane of rho_w
};

__device__ __forceinline__ FillWalk bucket_fill_start(uint32_t p, const BucketArgs& ba) {
  uint32_t w3;
  const uint64_t o = bucket_first(p, ba, w3);
  FillWalk f{~0u, 0u, p / 30u, 0u, 0u};
  if (o >= ba.span) return f;
  const uint32_t kq = (uint32_t)(o / 30u);  // o < span + 6 p < 2^36: kq < 2^31
  uint32_t rho = (uint32_t)(o - 30ull * kq);
  const uint32_t w0 = w3 / 3u, pm = p - 30u * f.pq;
  f.k = kq;
  f.w4 = 4u * w0;
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t w = (w0 + j) & 7u, gap = (kGap30x4 >> (4u * w)) & 15u;
    const uint32_t t = rho + pm * gap;  // < 30 + 29 * 6
    const uint32_t c = t / 30u;
    f.carry |= c << (4u * w);
    f.plane |= ((uint32_t)(ba.plane_lut >> (3u * (rho >> 1))) & 7u) << (4u * w);
    rho = t - 30u * c;
  }
  return f;
}

// (band-0 workgroup b; cur: nseg words of LDS)
__device__ __forceinline__ void bucket_fill_wg(uint32_t* cur, uint32_t b, const void* __restrict__ table,
                                               const BucketArgs& ba, const uint32_t* __restrict__ range,
                                               const BandZero& bz) {
  const uint32_t* P = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(table) + 16);
  const uint32_t i_lo = range[0], i_hi = range[2];
  for (uint32_t j = threadIdx.x; j < ba.nseg; j += kBucketThreads) cur[j] = 0;
  __syncthreads();
  char* const reg_b = reinterpret_cast<char*>(bz.reg0 + (uint64_t)b * ba.nseg * bz.k0);  // this workgroup's regions
  const uint32_t k0 = bz.k0;
  // slot pos of region (sg, b), or the spill list past its capacity
  auto put = [&](uint32_t sg, uint32_t pos, uint32_t e) {
    if (pos < k0) {
      *reinterpret_cast<uint32_t*>(reg_b + 4u * (__umul24(sg, k0) + pos)) = e;  // < 2^32: per-workgroup regions
    } else {
      const uint32_t j = atomicAdd(bz.nspill, 1u);
      if (j < bz.spill_cap) {
        bz.spill[j] = (unsigned long long)sg << 32 | e;
      } else {  // only with a test-shrunk capacity (bucket_cap_divisor): fail loudly
        bz.flag[0] = 1u;
        atomicOr(bz.count, 1ull << 63);
      }
    }
  };
  auto emit = [&](uint32_t sg, uint32_t e) {
#if defined(DSE_BK_FILL_KO) && DSE_BK_FILL_KO == 3  // profiling knockout: the walk alone
    asm volatile("" ::"v"(e), "v"(sg));
    return;
#endif
    const uint32_t pos = atomicAdd(&cur[sg], 1u);
#if defined(DSE_BK_FILL_KO) && DSE_BK_FILL_KO == 1  // profiling knockout: no global store
    asm volatile("" ::"v"(e), "v"(pos));
    return;
#elif defined(DSE_BK_FILL_KO) && DSE_BK_FILL_KO == 2  // profiling knockout: one coalesced line per store
    bz.reg0[(uint64_t)b * kBucketThreads + threadIdx.x] = e + pos;
    return;
#endif
    put(sg, pos, e);
  };
  // Segment-ordered walk: a thread walks its primes of kFillRG stride rounds
  // together, chunk by chunk of DSE_BK_CHUNK segments, so region (s, b) gets
  // its hits within one chunk's time (while its lines are still in the L2)
  // instead of over the whole walk. Snake order: odd rounds of the stride
  // take their block in reverse thread order, so the thread with one round's
  // smallest prime (the most hits, ~1/p) gets the next round's largest (in
  // plain order the threads holding a band's smallest primes walk up to
  // ~1.7x the mean).
  constexpr uint32_t stride = kBucketGrid * kBucketThreads;
  constexpr uint32_t kKPMask = (1u << kWheelLogKP) - 1;
  const uint32_t j = b * kBucketThreads + threadIdx.x;
  const uint32_t jr = stride - 1 - j;
  const uint32_t kspan = ba.nseg << kWheelLogKP;  // periods of the pass (< 2^30)
  for (uint64_t r0 = 0; i_lo + r0 * stride < i_hi; r0 += kFillRG) {
    FillWalk f[kFillRG];
#pragma unroll
    for (uint32_t r = 0; r < kFillRG; ++r) {
      const uint64_t i = i_lo + (r0 + r) * stride + (((r0 + r) & 1) ? jr : j);
      f[r] = FillWalk{~0u, 0u, 0u, 0u, 0u};
      if (i < i_hi) f[r] = bucket_fill_start(P[i], ba);
    }
    // later groups walk larger primes (fewer hits per chunk: lanes idle in
    // the divergent walk) at larger chunks
    const uint32_t cseg = DSE_BK_CHUNK << min(3u, (uint32_t)(r0 / kFillRG) * DSE_BK_CHUNK_GROW);
    for (uint32_t end = cseg;; end += cseg) {
      const uint32_t klim = min(end << kWheelLogKP, kspan);
      bool left = false;
#pragma unroll
      for (uint32_t r = 0; r < kFillRG; ++r) {
        while (f[r].k < klim) {
          const uint32_t k = f[r].k, w4 = f[r].w4;
          const uint32_t pl = __builtin_amdgcn_ubfe(f[r].plane, w4, 4);
          const uint32_t gap = __builtin_amdgcn_ubfe(kGap30x4, w4, 4);
          const uint32_t c = __builtin_amdgcn_ubfe(f[r].carry, w4, 4);
          // entry (bucket_entry): LDS word (block << 3 | plane) << 5 | bit
          emit(k >> kWheelLogKP, ((k & kKPMask & ~31u) << 3) | (pl << 5) | (k & 31u));
          f[r].k = k + __umul24(f[r].pq, gap) + c;  // pq < 2^24
          f[r].w4 = w4 + 4u;
        }
        left |= f[r].k < kspan;
      }
      if (!left) break;
    }
  }
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < ba.nseg; j += kBucketThreads) bz.n0[(uint64_t)j * kBucketGrid + b] = min(cur[j], bz.k0);
}

// Band 1, two-level fill: every global store is a run of consecutive dwords.
//
// Level 1 (bucket_stage_kernel) files each hit under its super-bucket of
// kSupSegs consecutive segments, key = (segment mod kSupSegs) << 20 | entry.
// Each wave stages kStageCap keys per super-bucket in LDS (a slot per lane
// from an LDS atomic) and writes a full stage as one 256 B run into its
// workgroup's region of that super-bucket; the region of (band-1 workgroup g,
// super-bucket S) starts at
//   start[S kSupSegs] + sum over S's segments s of cols[s][g]
// (cols = per-segment exclusive scans over the virtual workgroups), so the
// temporary array holds each super-bucket where its band-1 entries will end
// up. A lane whose stage is full keeps its hit and retries after the flush.
// Lanes move on to their next prime independently, its (p, m) loaded one
// prime ahead (a wave-synchronous walk that waited on that load at every
// prime change was latency-bound).
//
// Level 2 (bucket_sort_kernel): job (S, group of kSortGroup band-1
// workgroups) reads its contiguous slice of super-bucket S, whose per-segment
// counts are known (cols again), and counting-sorts tiles of kSortTile keys by
// segment in LDS, the next tile's keys loaded while the current one sorts;
// each segment's run of a tile is stored contiguously at its cursor, which
// starts at start[s] + cols[s][first workgroup of the group].
constexpr uint32_t kSupLog = 7;
constexpr uint32_t kSupSegs = 1u << kSupLog;       // segments per super-bucket
constexpr uint32_t kStageCap = 64;                 // keys per (wave, super-bucket) stage: one 256 B run
static_assert(kKeyShift + kSupLog <= 32, "bucket key layout (kKeyShift: dse_wheel_geometry.h)");
#ifndef DSE_BK_SORT_GROUP
#define DSE_BK_SORT_GROUP 64
#endif
constexpr uint32_t kSortGroup = DSE_BK_SORT_GROUP;  // band-1 workgroups per level-2 job
#ifndef DSE_BK_SORT_TILE
#define DSE_BK_SORT_TILE 8192
#endif
constexpr uint32_t kSortTile = DSE_BK_SORT_TILE;   // keys per LDS counting sort
#ifndef DSE_BK_SORT_THREADS
#define DSE_BK_SORT_THREADS 1024
#endif
constexpr uint32_t kSortThreads = DSE_BK_SORT_THREADS;
static_assert(kSortTile % kSortThreads == 0 && kSortThreads >= kSupSegs, "sort tile");
static_assert(kBucketGrid1 % kSortGroup == 0, "sort groups");

__host__ __device__ constexpr uint32_t stage_lds_words(uint32_t nsup) {
  return nsup + (kBucketThreads / 64) * nsup * (kStageCap + 1);
}

// (band-1 workgroup b; sm: stage_lds_words(nsup) words of LDS)
__device__ __forceinline__ void bucket_stage_wg(uint32_t* sm, uint32_t b, const void* __restrict__ table,
                                                const BucketArgs& ba, const uint32_t* __restrict__ range,
                                                const uint32_t* __restrict__ cols, const uint32_t* __restrict__ start,
                                                uint32_t* __restrict__ tmp, uint32_t nsup) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t i_hi = range[1];
  constexpr uint32_t stride = kBucketGrid1 * kBucketThreads;
  uint32_t i = range[2] + b * kBucketThreads + tid;  // index of the prefetched prime
  if (__syncthreads_or(i < i_hi) == 0) return;
  uint32_t* cur = sm;                                          // [nsup] region cursors of this workgroup
  uint32_t* scnt = sm + nsup + wave * nsup * (kStageCap + 1);  // [nsup] this wave's stage fills
  uint32_t* stage = scnt + nsup;                               // [nsup][kStageCap]
  for (uint32_t S = tid; S < nsup; S += kBucketThreads) cur[S] = start[S << kSupLog];
  for (uint32_t S = lane; S < nsup; S += 64) scnt[S] = 0;
  __syncthreads();
  for (uint32_t s = tid; s < ba.nseg; s += kBucketThreads)
    atomicAdd(&cur[s >> kSupLog], cols[(uint64_t)s * kBucketCols + b]);
  __syncthreads();

  const uint32_t* P = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(table) + 16);
  uint32_t pn = i < i_hi ? P[i] : 0u;
  uint32_t p = 0, w3 = 0;
  uint64_t o = ba.span;
  // next prime of this lane with a hit in the pass (o >= span: none left)
  auto next_prime = [&]() {
    while (i < i_hi) {
      p = pn;
      i += stride;
      if (i < i_hi) pn = P[i];
      o = bucket_first(p, ba, w3);
      if (o < ba.span) return;
    }
    o = ba.span;
  };
  next_prime();
  while (__ballot(o < ba.span)) {
    uint32_t S = 0, pos = kStageCap;
    if (o < ba.span) {
      uint32_t s;
      const uint32_t e = bucket_entry(o, ba, s);
      S = s >> kSupLog;
      pos = atomicAdd(&scnt[S], 1u);
      if (pos < kStageCap) stage[S * kStageCap + pos] = ((s & (kSupSegs - 1)) << kKeyShift) | e;
    }
    // stages that just filled: exactly one lane took their last slot and reserves the run
    const bool filled = pos == kStageCap - 1;
    uint32_t g = 0;
    if (filled) g = atomicAdd(&cur[S], kStageCap);
    uint64_t full = __ballot(filled);
    __builtin_amdgcn_wave_barrier();
    while (full) {
      const uint32_t l = (uint32_t)__builtin_ctzll(full);
      full &= full - 1;
      const uint32_t Sf = (uint32_t)__builtin_amdgcn_readlane((int)S, (int)l);
      const uint32_t gf = (uint32_t)__builtin_amdgcn_readlane((int)g, (int)l);
      tmp[gf + lane] = stage[Sf * kStageCap + lane];
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) scnt[Sf] = 0;  // lanes that overshot the full stage retry next step
      __builtin_amdgcn_wave_barrier();
    }
    if (pos < kStageCap) {  // placed: advance to the next hit (or prime)
      o += (uint64_t)p * ((kGap30 >> w3) & 7u);
      w3 = w3 == 21 ? 0u : w3 + 3;
      if (o >= ba.span) next_prime();
    }
  }
  // partial stages
  for (uint32_t S = 0; S < nsup; ++S) {
    const uint32_t n = scnt[S];
    if (n == 0) continue;
    uint32_t g = 0;
    if (lane == 0) g = atomicAdd(&cur[S], n);
    g = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
    if (lane < n) tmp[g + lane] = stage[S * kStageCap + lane];
  }
}

// Band-0 fill and band-1 stage in one launch: workgroups [0, nfill) fill,
// the rest stage, so the request-bound scattered stores of the one and the
// latency-bound staging of the other share the CUs (and neither pays a tail).
__global__ __launch_bounds__(kBucketThreads) void bucket_fill_stage_kernel(
    const void* __restrict__ table, BucketArgs ba, const uint32_t* __restrict__ range,
    const uint32_t* __restrict__ cols, const uint32_t* __restrict__ start, BandZero bz,
    uint32_t* __restrict__ tmp, uint32_t nsup, uint32_t nfill, const uint32_t* __restrict__ flag) {
  extern __shared__ uint32_t sm[];
  const uint32_t x = blockIdx.x;
  if (flag[1]) {  // capacity overflow (bucket_startscan_kernel): no hits, but every band-0 region empty
    if (x < nfill)
      for (uint32_t j = threadIdx.x; j < ba.nseg; j += kBucketThreads) bz.n0[(uint64_t)j * kBucketGrid + x] = 0;
    return;
  }
#if defined(DSE_BK_FILL_KO) && DSE_BK_FILL_KO == 4  // profiling knockout: band-0 fill only
  if (x >= nfill) return;
#elif defined(DSE_BK_FILL_KO) && DSE_BK_FILL_KO == 5  // profiling knockout: band-1 staging only
  if (x < nfill) return;
#endif
  if (x < nfill)
    bucket_fill_wg(sm, x, table, ba, range, bz);
  else
    bucket_stage_wg(sm, x - nfill, table, ba, range, cols, start, tmp, nsup);
}

__global__ __launch_bounds__(kSortThreads) void bucket_sort_kernel(BucketArgs ba, const uint32_t* __restrict__ cols,
                                                                   const uint32_t* __restrict__ start,
                                                                   const uint32_t* __restrict__ tmp,
                                                                   uint32_t* __restrict__ entries,
                                                                   const uint32_t* __restrict__ flag) {
  if (flag[1]) return;  // capacity overflow (bucket_startscan_kernel)
#if defined(DSE_BK_FILL_KO) && DSE_BK_FILL_KO == 4  // profiling knockout: nothing staged to sort
  return;
#endif
  constexpr uint32_t kPer = kSortTile / kSortThreads;
  constexpr uint32_t kPerLane = kSupSegs / 64;  // scan: segment counts per lane of wave 0
  __shared__ uint32_t sorted[kSortTile];
  __shared__ uint32_t hist[kSupSegs], off[kSupSegs], curs[kSupSegs];
  __shared__ uint32_t rb[2];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  constexpr uint32_t ngroups = kBucketGrid1 / kSortGroup;
  const uint32_t S = blockIdx.x / ngroups, g0 = (blockIdx.x % ngroups) * kSortGroup,
                 g1 = g0 + kSortGroup;
  const uint32_t s0 = S << kSupLog;
  if (tid < 2) rb[tid] = 0;
  if (tid < kSupSegs) hist[tid] = 0;
  __syncthreads();
  if (tid < kSupSegs) {
    const uint32_t s = s0 + tid;
    uint32_t c0 = 0, c1 = 0;
    if (s < ba.nseg) {
      c0 = cols[(uint64_t)s * kBucketCols + g0];
      c1 = g1 < kBucketCols ? cols[(uint64_t)s * kBucketCols + g1] : start[s + 1] - start[s];
      curs[tid] = start[s] + c0;
    }
    atomicAdd(&rb[0], c0);
    atomicAdd(&rb[1], c1);
  }
  __syncthreads();
  const uint32_t r0 = start[s0] + rb[0], r1 = start[s0] + rb[1];
  uint32_t nxt[kPer];
  auto load_tile = [&](uint32_t base) {
    const uint32_t n = min(kSortTile, r1 - base);
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q) {
      const uint32_t j = q * kSortThreads + tid;
      nxt[q] = j < n ? __builtin_nontemporal_load(tmp + base + j) : 0u;
    }
  };
  if (r0 < r1) load_tile(r0);
  for (uint32_t base = r0; base < r1; base += kSortTile) {
    const uint32_t n = min(kSortTile, r1 - base);
    uint32_t key[kPer], rk[kPer];
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q) key[q] = nxt[q];
    if (base + kSortTile < r1) load_tile(base + kSortTile);
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q)
      rk[q] = q * kSortThreads + tid < n ? atomicAdd(&hist[key[q] >> kKeyShift], 1u) : 0u;
    __syncthreads();
    if (tid < 64) {  // exclusive scan of the segment counts (one wave, kPerLane each)
      uint32_t c[kPerLane], sum = 0;
#pragma unroll
      for (uint32_t t = 0; t < kPerLane; ++t) sum += (c[t] = hist[lane * kPerLane + t]);
      uint32_t x = sum;
#pragma unroll
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
      }
      x -= sum;
#pragma unroll
      for (uint32_t t = 0; t < kPerLane; ++t) {
        off[lane * kPerLane + t] = x;
        x += c[t];
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q)
      if (q * kSortThreads + tid < n) sorted[off[key[q] >> kKeyShift] + rk[q]] = key[q];
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q) {
      const uint32_t j = q * kSortThreads + tid;
      if (j < n) {
        const uint32_t v = sorted[j], k = v >> kKeyShift;
        entries[curs[k] + j - off[k]] = v & ((1u << kKeyShift) - 1);
      }
    }
    __syncthreads();
    if (tid < kSupSegs) {
      curs[tid] += hist[tid];
      hist[tid] = 0;
    }
    __syncthreads();
  }
}

// Rigorous bound on the bucket entries of a pass spanning `span` integers with
// primes in (a, b]: each prime has <= 8 span / (30 p) + 8 coprime multiples;
// sum 1/p <= ln(ln b / ln a) + 1/ln^2 a and pi(b) <= 1.25506 b / ln b.
uint64_t bucket_cap(uint64_t span, double a, double b) {
  if (b <= a) return 64;
  const double la = __builtin_log(a), lb = __builtin_log(b);
  const double s = __builtin_log(lb / la) + 1.0 / (la * la);
  return (uint64_t)(8.0 * (double)span / 30.0 * s + 8.0 * 1.25506 * b / lb) + 1024;
}

// Band-0 region capacity k0 (bucket_fill_wg). A region collects the hits in one
// segment of one fill workgroup's primes: 256 per stride round r, all >= the
// round's first prime p(r), so its mean is at most lambda = (8 W / 30) sum_r
// 256 / p(r) (p(r) from the table index i_lo + r S: p_n >= n (ln n + ln ln n
// - 1), Dusart), and its variance at most lambda plus ~4 per prime below the
// segment span W: such a prime (2^19 < p < W, all in round 0) hits each of
// the 8 planes floor or ceil of KP / p times, a deviation of variance <= 1/4
// per plane, 2 per prime (4 taken). k0 = lambda + 10 sigma + 64:
// a region past it is a >10-sigma event, and even then its hits are spilled,
// not lost.
uint32_t bucket_k0(uint32_t i_lo, double a, double b) {
  if (b <= a) return 0;
  const double S = (double)kBucketGrid * kBucketThreads;
  const double n_band = 1.25506 * b / __builtin_log(b) - (double)i_lo;  // >= the band's primes
  const double mu = 8.0 * (double)kWheelSpan / 30.0;
  double lam = 0;
  for (double r = 0; r * S < n_band; r += 1) {
    const double n = (double)i_lo + r * S + 2;  // 1-based index of the round's first prime (2 is p_1)
    const double pl = std::max(a, n * (__builtin_log(n) + __builtin_log(__builtin_log(n)) - 1.0));
    lam += mu * kBucketThreads / pl;
  }
  const double var = lam + 4.0 * kBucketThreads;
  const uint64_t k0 = (uint64_t)(lam + 10.0 * __builtin_sqrt(var) + 64.0);
  return (uint32_t)((k0 + 15) & ~15ull);
}

constexpr uint64_t kBucketMaxEntries = 1ull << 31;  // 8 GB of band-1 entries per pass
constexpr uint64_t kBucketMaxRegionBytes = 24ull << 30;  // band-0 regions per pass

// The context's scratch at `bytes` for a pass on `stream` (acquire_scratch:
// ordered after the previous pass whatever stream that ran on), with its
// overflow flag, created and zeroed on first use.
hipError_t ensure_scratch(Scratch* sc, uint64_t bytes, hipStream_t stream, char** out) {
  hipError_t e;
  if (!sc->flag) {
    if ((e = hipMalloc(&sc->flag, 2 * sizeof(uint32_t))) != hipSuccess) return e;
    if ((e = hipMemsetAsync(sc->flag, 0, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;
  }
  if ((e = acquire_scratch(sc, bytes, stream)) != hipSuccess) return e;
  *out = sc->buf.as<char>();
  return hipSuccess;
}

}  // namespace

// A range whose primes reach above kWheelMaxPrime: bucketed passes.
// tests/max_pass_ref.py (planned_passes) restates the pass planning, bucket_cap, bucket_k0 and the
// scratch layout below for the tests of the largest passes: change them together.
hipError_t launch_bucketed(const void* table, uint64_t g_start, uint64_t nbits, uint32_t* out,
                           unsigned long long* count, int num_cus, hipStream_t stream, Scratch* scratch,
                           const SieveOpts* opts, PlanStats* plan) {
  const uint64_t vmax = 3 + 2 * (g_start + nbits - 1);
  const uint64_t root = isqrt64(vmax);
  uint64_t plane_lut;
  if (!scratch) return hipErrorInvalidValue;
  // primes above kWheelMaxPrime: passes of <= kBucketMaxSegs segments, each
  // with its own bucket build, then the wheel kernel over the pass
  const uint64_t total_seg = (nbits + kWheelOutBits - 1) / kWheelOutBits;
  uint64_t max_segs = kBucketMaxSegs;
  if (opts && opts->bucket_pass_segs >= 1 && opts->bucket_pass_segs < max_segs) max_segs = opts->bucket_pass_segs;
  // band 0 stops below 30 * 2^24 whatever the option (its walk's 24-bit step product, bucket_fill_wg)
  const uint64_t split =
      std::min<uint64_t>(1ull << (opts && opts->bucket_split_log2 ? opts->bucket_split_log2 : kBucketSplitLog), kFillMaxSplit);
  // primes above lo_p are bucketed: below kWheelMaxPrime for a range that is
  // bucketed anyway (a prime that hits a segment about once is cheaper as a
  // bucket entry than as 8 plane slots of an L unit; window: 2^19 -2%)
  const uint64_t lo_p = 1ull << (opts && opts->bucket_lo_log2 ? opts->bucket_lo_log2 : kBucketLoLog);
  const uint32_t cap_div = opts && opts->bucket_cap_div > 1 ? opts->bucket_cap_div : 1;  // test-only: overflow
  const uint32_t k0_div = opts && opts->bucket_k0_div > 1 ? opts->bucket_k0_div : 1;     // test-only: spills
  const double a0 = (double)lo_p, b0 = std::min((double)split, (double)root);  // band 0: (a0, b0]
  for (uint64_t s0 = 0; s0 < total_seg;) {
    uint64_t ns = std::min<uint64_t>(max_segs, total_seg - s0);
    RangeSpec piece{g_start + s0 * kWheelOutBits, kWheelOutBits, nullptr, count};
    WheelArgs wa = make_wheel_args(&piece, 1, &plane_lut, lo_p);  // (wa.nthr)
    const uint32_t k0_full = bucket_k0(wa.nthr[4], a0, b0);
    while (ns > 1 && (bucket_cap(ns * kWheelSpan, (double)split, (double)root) > kBucketMaxEntries ||
                      4ull * ns * kBucketGrid * k0_full > kBucketMaxRegionBytes))
      ns /= 2;
    const uint64_t g0 = g_start + s0 * kWheelOutBits;
    const uint64_t nb = std::min<uint64_t>(nbits - s0 * kWheelOutBits, ns * kWheelOutBits);
    const uint64_t vmax_p = 3 + 2 * (g0 + nb - 1);
    piece = {g0, nb, out ? out + s0 * (kWheelOutBits / 32) : nullptr, count};
    wa = make_wheel_args(&piece, 1, &plane_lut, lo_p);
    if (wa.nseg != ns) return hipErrorInvalidValue;  // the band-0 region layout's nseg (wheel side: wa.nseg)
    BucketArgs ba{};
    ba.V0 = wa.r[0].V0;
    ba.span = ns * kWheelSpan;
    ba.plane_lut = plane_lut;
    ba.nseg = (uint32_t)ns;
    ba.vmax = vmax_p;
    ba.split = split;
    const uint64_t root_p = isqrt64(vmax_p);
    const bool band0 = split > lo_p, band1 = split < root_p;
    // band 1: rigorous entry capacity (its keys, then its sorted entries);
    // band 0: regions of k0 slots per (segment, fill workgroup), the spill
    // list's capacity a rigorous bound on the band's hits
    const uint64_t cap = (band1 ? bucket_cap(ba.span, (double)split, (double)root_p) : 64) / cap_div;
    const uint32_t k0 = band0 ? std::max<uint32_t>(1, k0_full / k0_div / cap_div) : 0;
    const uint64_t spill_cap = band0 ? bucket_cap(ba.span, a0, std::min((double)split, (double)root_p)) / cap_div : 0;
    // scratch: [range 3, nspill][cols grid1*ns][tot ns][start ns+1][entries cap][band-1 keys cap]
    //          [band-0 regions ns*grid*k0][band-0 fills ns*grid][spill list (8 B) spill_cap]
    auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
    const uint64_t o_cols = 256, o_tot = o_cols + 4ull * kBucketCols * ns, o_start = o_tot + 4 * ns + 256,
                   o_ent = al(o_start + 4 * (ns + 1)), o_tmp = al(o_ent + 4 * cap),
                   o_reg = al(band1 ? o_tmp + 4 * cap : o_tmp), o_n0 = al(o_reg + 4ull * ns * kBucketGrid * k0),
                   o_spill = al(o_n0 + (band0 ? 4ull * ns * kBucketGrid : 0)), bytes = o_spill + 8 * spill_cap;
    char* sc = nullptr;
    hipError_t e = ensure_scratch(scratch, bytes, stream, &sc);
    if (e != hipSuccess) return e;
    // from here on kernels may read the scratch: every exit records `done`
    // (a later grow frees the buffer only after it)
    auto fail_pass = [&](hipError_t err) {
      (void)release_scratch(scratch, stream);
      return err;
    };
    if (opts && opts->scratch_poison && (e = hipMemsetAsync(sc, 0xFF, bytes, stream)) != hipSuccess)
      return fail_pass(e);  // test-only: stale scratch contents
    uint32_t* range = reinterpret_cast<uint32_t*>(sc);
    uint32_t* cols = reinterpret_cast<uint32_t*>(sc + o_cols);
    uint32_t* tot = reinterpret_cast<uint32_t*>(sc + o_tot);
    uint32_t* start = reinterpret_cast<uint32_t*>(sc + o_start);
    uint32_t* ent = reinterpret_cast<uint32_t*>(sc + o_ent);
    uint32_t* tmp = reinterpret_cast<uint32_t*>(sc + o_tmp);
    BandZero bz{};
    bz.reg0 = reinterpret_cast<uint32_t*>(sc + o_reg);
    bz.n0 = reinterpret_cast<uint32_t*>(sc + o_n0);
    bz.spill = reinterpret_cast<unsigned long long*>(sc + o_spill);
    bz.nspill = range + 3;
    bz.k0 = k0;
    bz.spill_cap = spill_cap;
    bz.flag = scratch->flag;
    bz.count = count;
    hipLaunchKernelGGL(bucket_range_kernel, dim3(1), dim3(64), 0, stream, table, lo_p, vmax_p, ba.split, range,
                       bz.nspill);
    hipLaunchKernelGGL(bucket_count_kernel, dim3(kBucketGrid1), dim3(kBucketThreads), 4 * (uint32_t)ns, stream, table,
                       ba, range, cols);
    hipLaunchKernelGGL(bucket_colscan_kernel, dim3((uint32_t)((ns + 3) / 4)), dim3(256), 0, stream, cols,
                       (uint32_t)ns, tot);
    hipLaunchKernelGGL(bucket_startscan_kernel, dim3(1), dim3(kSliceThreads), 0, stream, tot, (uint32_t)ns, start, cap,
                       scratch->flag, count);
    const uint32_t nsup = (uint32_t)((ns + kSupSegs - 1) >> kSupLog);
    const uint32_t nfill = band0 ? kBucketGrid : 0;
    const uint32_t lds_bytes = std::max(band0 ? 4 * (uint32_t)ns : 0u, band1 ? 4 * stage_lds_words(nsup) : 0u);
    if (lds_bytes > 65536 &&
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&bucket_fill_stage_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes)) != hipSuccess)
      return fail_pass(e);
    hipLaunchKernelGGL(bucket_fill_stage_kernel, dim3(nfill + (band1 ? kBucketGrid1 : 0)), dim3(kBucketThreads),
                       lds_bytes, stream, table, ba, range, cols, start, bz, tmp, nsup, nfill, scratch->flag);
    // defensive (no refusal has been seen: the runtime launches 66,816 bytes of LDS even
    // without the opt-in): had this launch failed, the sort would run over unwritten keys
    if ((e = hipGetLastError()) != hipSuccess) return fail_pass(e);
    if (band1) {
      hipLaunchKernelGGL(bucket_sort_kernel, dim3(nsup * (kBucketGrid1 / kSortGroup)), dim3(kSortThreads), 0,
                         stream, ba, cols, start, tmp, ent, scratch->flag);
    }
    if ((e = hipGetLastError()) != hipSuccess) return fail_pass(e);
    wa.bk_entries = ent;
    wa.bk_start = start;
    wa.bk_reg0 = bz.reg0;
    wa.bk_n0 = bz.n0;
    wa.bk_spill = bz.spill;
    wa.bk_nspill = bz.nspill;
    wa.bk_spill_cap = spill_cap;
    wa.bk_k0 = k0;
    // always the instantiation with bucket units: wa.bk_start points into the scratch, never null
    if ((e = launch_wheel_bucketed(table, wa, num_cus, stream)) != hipSuccess) return fail_pass(e);
    if ((e = release_scratch(scratch, stream)) != hipSuccess) return e;
    if (plan) {
      plan->add_wheel_launch(wa.nseg, wheel_grid(wa.nseg, num_cus));
      ++plan->bucket_passes;
      plan->bucket_max_pass_segments = std::max(plan->bucket_max_pass_segments, ns);
      plan->bucket_max_lds_bytes = std::max<uint64_t>(plan->bucket_max_lds_bytes, lds_bytes);
    }
    s0 += ns;
  }
  return hipSuccess;
}

}  // namespace dse
