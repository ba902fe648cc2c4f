// dse_wheel.hip -- the wheel sieve's host dispatch (launch_sieve_ranges: which
// ranges pool into persistent launches, which geometry their tail takes,
// which go through bucketed passes), the table kernel (wheel_offsets_kernel)
// and the wheel kernel's instantiation for bucketed passes.
//
// The kernel body -- wheel_segments_kernel with mark_segment, expand_segment
// and init_segment, the A, B1, B2 and L units and the mark helpers -- is in
// dse_wheel_kernel.h; the segment geometry and WheelArgs in
// dse_wheel_geometry.h, make_wheel_args in dse_wheel_args.h; the bucketed
// pass (fill, stage and sort kernels, scratch, launch_bucketed) in
// dse_bucket.hip. dse_wheel_plain.hip and dse_wheel_half.hip instantiate the
// kernel without bucket units, for the full and the half-size geometry.
#include "dse_wheel_args.h"
#include "dse_wheel_kernel.h"

namespace dse {
namespace {

// m[i] = floor((2^64-1)/p) (barrett_factor, dse_wheel_kernel.h) and the rotated wheel-offset row of every table
// prime: a[8i + ((j - i) & 7)] = first k >= 0 with p | R30[j] + 30k (p >= 7).
__global__ void wheel_offsets_kernel(void* __restrict__ table) {
  const TableHeader* h = reinterpret_cast<const TableHeader*>(table);
  const uint32_t n = h->count == 0xFFFFFFFFu ? 0u : h->count;
  const uint32_t* P = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(table) + 16);
  uint64_t* M = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(table) + table_m_offset(h->cap));
  uint32_t* A = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(table) + table_a_offset(h->cap));
  uint32_t* PL = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(table) + table_l_offset(h->cap));
  static_assert(kWheelLogKP == 17, "pl[0] is the full geometry's, pl[1] the half geometry's");
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t p = P[i];
    if (p > kWheelMaxPrime) break;  // bucketed primes (P ascends: all later ones too): the walks divide in double precision
    // the plans of the prime's set of 64 in the L list (unit_L), per geometry
    uint32_t plan0 = 0, plan1 = 0;
    if (i >= kL0) {
      const uint32_t s0 = i - (i - kL0) % 64;
      // pmax is the set's last prime in the table, but the kernel's L list may
      // end before the set does (i_big: the primes above wa.nthr[4] are
      // bucketed or absent), so a plan must stay valid for every pmax' <=
      // pmax. It does: pmax enters l_plan only through n_min = floor(KP /
      // pmax), which a larger pmax only lowers, and a lower n_min is a shorter
      // unconditional run, or the choice of n_all, which covers every lane.
      const uint32_t pmin = P[s0], pmax = P[min(s0 + 63, n - 1)];
      plan0 = l_plan(pmin, pmax, 1u << 17);
      plan1 = l_plan(pmin, pmax, 1u << 16);
    }
    PL[i] = p | plan0 << 20;
    PL[h->cap + i] = p | plan1 << 20;
    const uint64_t m = barrett_factor(p);
    M[i] = m;
    if (p < 7) {
#pragma unroll
      for (int j = 0; j < 8; ++j) A[8ull * i + j] = 0;
      continue;
    }
    const uint64_t inv = inv30_of(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t t = kR30[j] % p;
      const uint32_t u = t ? p - t : 0u;
      A[8ull * i + ((j - i) & 7)] = mod_barrett((uint64_t)u * inv, p, m);  // row rotated by i & 7
    }
  }
}

}  // namespace

hipError_t launch_wheel_offsets(void* table, int num_cus, hipStream_t stream, uint64_t n_hint) {
  // rows, factors and plans only for the primes <= kWheelMaxPrime (82,025 below 2^20): the kernel stops
  // at the first bucketed prime, so a window's 50.8 M-prime table needs no larger grid (the grid-stride
  // loop covers every index whatever the grid)
  n_hint = std::min<uint64_t>(n_hint, 1u << 17);
  const uint64_t grid = std::max<uint64_t>(4 * (uint64_t)num_cus, std::min<uint64_t>(n_hint / 1024 + 1, 1u << 16));
  hipLaunchKernelGGL(wheel_offsets_kernel, dim3((uint32_t)grid), dim3(256), 0, stream, table);
  return hipGetLastError();
}

// The wheel kernel over a bucketed pass (launch_bucketed, dse_bucket.hip): the
// instantiation with bucket units, built with iterative-ILP (Makefile).
hipError_t launch_wheel_bucketed(const void* table, const WheelArgs& wa, int num_cus, hipStream_t stream) {
  return launch_wheel<true>(table, wa, num_cus, stream);
}

namespace {

// Time of a half-size segment (dse_wheel_half.hip) relative to a full one,
// and of a launch relative to a round of full segments
// (profiles/r03/geometry_ab.txt).
#ifndef DSE_HALF_SEG_COST
#define DSE_HALF_SEG_COST 0.68
#endif
#ifndef DSE_LAUNCH_COST
#define DSE_LAUNCH_COST 0.1
#endif
constexpr double kHalfSegCost = DSE_HALF_SEG_COST, kLaunchCost = DSE_LAUNCH_COST;

// The ranges without bucketed primes, pooled: one persistent launch (per
// kMaxRanges ranges) over all their segments. Segments go to the num_cus
// workgroups in rounds; a last, partial round of full segments leaves CUs
// idle for a whole segment time, so the segments past the last full round
// go to the half-size geometry instead when that finishes sooner: (their
// half segments / num_cus rounds) x kHalfSegCost plus the second launch.
hipError_t launch_pooled(const void* table, const RangeSpec* rs, size_t n, int num_cus, hipStream_t stream,
                         const SieveOpts* opts, PlanStats* plan) {
  if (n == 0) return hipSuccess;
  const uint32_t geo = opts ? opts->wheel_geometry : 0;  // 0 auto, 1 full only, 2 half only
  constexpr uint64_t kHalfBits = kWheelOutBits / 2;
  const uint64_t G = (uint64_t)num_cus;
  uint64_t S = 0;
  for (size_t i = 0; i < n; ++i) S += (rs[i].nbits + kWheelOutBits - 1) / kWheelOutBits;
  uint64_t F = geo == 2 ? 0 : geo == 1 ? S : (S / G) * G;  // segments of the full geometry
  // split the list after its first F full segments
  std::vector<RangeSpec> full, half;
  uint64_t left = F;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t ns = (rs[i].nbits + kWheelOutBits - 1) / kWheelOutBits;
    const uint64_t take = std::min(ns, left);
    left -= take;
    const uint64_t fb = std::min(rs[i].nbits, take * kWheelOutBits);
    if (fb) full.push_back({rs[i].g_start, fb, rs[i].out, rs[i].count});
    if (fb < rs[i].nbits)
      half.push_back({rs[i].g_start + fb, rs[i].nbits - fb, rs[i].out ? rs[i].out + fb / 32 : nullptr,
                      rs[i].count});
  }
  if (geo == 0 && !half.empty()) {
    uint64_t nhalf = 0;
    for (const auto& h : half) nhalf += (h.nbits + kHalfBits - 1) / kHalfBits;
    if (kHalfSegCost * (double)((nhalf + G - 1) / G) + (F ? kLaunchCost : 0.0) >= 1.0) {
      half.clear();  // the whole list in the full geometry
      full.assign(rs, rs + n);
    }
  }
  hipError_t e = launch_wheel_batches(launch_wheel_plain, table, full.data(), full.size(), num_cus, stream, plan,
                                      &PlanStats::full_segments);
  if (e != hipSuccess) return e;
  return half.empty() ? hipSuccess
                      : launch_wheel_ranges_half(table, half.data(), half.size(), num_cus, stream, plan);
}

}  // namespace

hipError_t launch_sieve_ranges(const void* table, const RangeSpec* rs, size_t n, int num_cus, hipStream_t stream,
                               Scratch* scratch, const SieveOpts* opts, PlanStats* plan) {
  // ranges of up to 2^30 segments (the launch's 32-bit segment indices)
  constexpr uint64_t kMaxBits = (1ull << 30) * kWheelOutBits;
  std::vector<RangeSpec> pooled;
  for (size_t i = 0; i < n; ++i) {
    for (uint64_t b = 0; b < rs[i].nbits; b += kMaxBits) {
      const RangeSpec piece{rs[i].g_start + b, std::min(kMaxBits, rs[i].nbits - b),
                            rs[i].out ? rs[i].out + b / 32 : nullptr, rs[i].count};
      if (isqrt64(3 + 2 * (piece.g_start + piece.nbits - 1)) <= kWheelMaxPrime) {
        pooled.push_back(piece);
      } else {
        const hipError_t e = launch_bucketed(table, piece.g_start, piece.nbits, piece.out, piece.count, num_cus,
                                             stream, scratch, opts, plan);
        if (e != hipSuccess) return e;
      }
    }
  }
  return launch_pooled(table, pooled.data(), pooled.size(), num_cus, stream, opts, plan);
}

hipError_t launch_sieve_range(const void* table, uint64_t g_start, uint64_t nbits, uint32_t* out,
                              unsigned long long* count, int num_cus, hipStream_t stream, Scratch* scratch,
                              const SieveOpts* opts, PlanStats* plan) {
  const RangeSpec rs{g_start, nbits, out, count};
  return launch_sieve_ranges(table, &rs, 1, num_cus, stream, scratch, opts, plan);
}

}  // namespace dse
