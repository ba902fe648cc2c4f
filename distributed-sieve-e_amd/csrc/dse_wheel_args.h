// dse_wheel_args.h -- host side of a wheel launch: WheelArgs built from the
// caller's ranges for the including unit's geometry. For the units that
// build launches (dse_wheel.hip, dse_wheel_half.hip, dse_bucket.hip); internal
// linkage throughout, as the half unit compiles it with other constants.
#pragma once
#include <algorithm>
#include <vector>

#include "dse_wheel_geometry.h"

namespace dse {
namespace {

// One range's geometry (shared by the wheel kernel and the bucket walks):
// the planes of V0 mod 30, the small-prime fixes, the init offsets.
// *plane_lut: plane of relative residue rho in bits [3 (rho >> 1), +3).
WheelRange make_wheel_range(const RangeSpec& rs, uint64_t* plane_lut) {
  WheelRange w{};
  const uint64_t v_start = 3 + 2 * rs.g_start;
  w.V0 = v_start - 1;
  w.nbits = rs.nbits;
  w.KB0 = w.V0 / 30;
  w.out = rs.out;
  w.count = rs.count;
  const uint32_t v0m = (uint32_t)(w.V0 % 30);
  w.variant = v0m / 2;  // V0 is even
  uint32_t n = 0;
  *plane_lut = 0;
  for (uint32_t rho = 1; rho < 30; rho += 2) {
    const uint32_t r = (v0m + rho) % 30;
    if (r % 3 == 0 || r % 5 == 0) continue;
    uint32_t iota = 0;
    while (kR30[iota] != r) ++iota;
    w.rho_pack |= (uint64_t)rho << (5 * n);
    w.pl_pack |= n << (3 * iota);
    if (v0m + rho >= 30) w.e_iota |= 1u << iota;
    *plane_lut |= (uint64_t)n << (3 * (rho >> 1));
    ++n;
  }
  // primes 3..79 inside the range: the wheel drops 3 and 5, the patterns mark 7..79 themselves
  constexpr uint32_t small[] = {3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79};
  static_assert(small[sizeof(small) / sizeof(small[0]) - 1] == kQMax && (kQMax - 3) / 2 < 64, "fix covers 3..kQMax");
  for (uint32_t v : small)
    if (v >= v_start && (v - v_start) / 2 < rs.nbits) w.fix |= 1ull << ((v - v_start) / 2);
  for (int g = 0; g < kNG; ++g) w.v0g[g] = (uint16_t)(w.V0 % gmod(g));
  return w;
}

// A launch over the ranges rs[0..n) (1 <= n <= kMaxRanges, each < 2^31
// segments in all), their segments in order; thresholds: odd primes up to
// kQMax, TA, TB1, TB and wheel_max (<= kWheelMaxPrime: the primes above it are
// bucketed or absent).
WheelArgs make_wheel_args(const RangeSpec* rs, uint32_t n, uint64_t* plane_lut,
                          uint64_t wheel_max = kWheelMaxPrime) {
  static const std::vector<uint32_t> odd_primes = [] {  // odd primes <= kWheelMaxPrime (sieved once)
    std::vector<uint8_t> comp(kWheelMaxPrime / 2 + 1, 0);  // comp[i]: 2i + 1 composite
    for (uint64_t i = 1; (2 * i + 1) * (2 * i + 1) <= kWheelMaxPrime; ++i)
      if (!comp[i])
        for (uint64_t j = ((2 * i + 1) * (2 * i + 1)) / 2; j <= kWheelMaxPrime / 2; j += 2 * i + 1) comp[j] = 1;
    std::vector<uint32_t> v;
    for (uint64_t i = 1; 2 * i + 1 <= kWheelMaxPrime; ++i)
      if (!comp[i]) v.push_back((uint32_t)(2 * i + 1));
    return v;
  }();
  const uint64_t lim[5] = {kQMax, TA, TB1, TB, std::min<uint64_t>(wheel_max, kWheelMaxPrime)};
  WheelArgs wa{};
  for (int t = 0; t < 5; ++t)
    wa.nthr[t] = (uint32_t)(std::upper_bound(odd_primes.begin(), odd_primes.end(), lim[t]) - odd_primes.begin());
  uint64_t seg = 0, lut = 0;
  for (uint32_t i = 0; i < n; ++i) {
    WheelRange& r = wa.r[i];
    r = make_wheel_range(rs[i], i ? &lut : plane_lut);
    r.seg0 = (uint32_t)seg;
    const uint64_t nseg_r = (rs[i].nbits + kWheelOutBits - 1) / kWheelOutBits;
    seg += nseg_r;
    // piece j = segments [j << lsh, (j + 1) << lsh): the odd primes with p^2
    // below the end of its last segment (the kernel's live test is p^2 < Vend)
    r.lsh = 0;
    while (nseg_r > 0 && ((nseg_r - 1) >> r.lsh) >= kLPieces) ++r.lsh;
    for (uint32_t j = 0; j < kLPieces; ++j) {
      const uint64_t last = nseg_r == 0 ? 0 : std::min<uint64_t>(((uint64_t)(j + 1) << r.lsh) - 1, nseg_r - 1);
      const uint64_t vend = r.V0 + (last + 1) * (uint64_t)kWheelSpan;
      r.lcap[j] = (uint32_t)(std::upper_bound(odd_primes.begin(), odd_primes.end(), isqrt64(vend - 1)) -
                             odd_primes.begin());
      if (r.lcap[j] == odd_primes.size()) r.lcap[j] = ~0u;  // past kWheelMaxPrime: no bound
    }
  }
  wa.nranges = n;
  wa.nseg = (uint32_t)seg;
  // (Non-temporal mask stores paid 5% at 1e12 only while segments claimed the
  // dead large units past their live primes; with lcap they do not:
  // profiles/r05/ab_nt_store_policy.txt, ab_nmin_and_nt_recheck.txt)
  return wa;
}

// Launches over rs[0..n), kMaxRanges ranges at a time, built for this unit's
// geometry (make_wheel_args): launch(table, wa, num_cus, stream) must launch
// a kernel of the same one (launch_wheel_plain from dse_wheel.hip,
// launch_wheel<false> in dse_wheel_half.hip). plan (may be null) counts the
// launches, and their segments in plan->*segs.
template <typename Launch>
hipError_t launch_wheel_batches(Launch launch, const void* table, const RangeSpec* rs, size_t n, int num_cus,
                                hipStream_t stream, PlanStats* plan, uint64_t PlanStats::*segs) {
  for (size_t i = 0; i < n; i += kMaxRanges) {
    uint64_t plane_lut;
    const WheelArgs wa = make_wheel_args(rs + i, (uint32_t)std::min<size_t>(kMaxRanges, n - i), &plane_lut);
    const hipError_t e = launch(table, wa, num_cus, stream);
    if (e != hipSuccess) return e;
    if (plan && wa.nseg) {
      plan->add_wheel_launch(wa.nseg, wheel_grid(wa.nseg, num_cus));
      plan->*segs += wa.nseg;
    }
  }
  return hipSuccess;
}

}  // namespace
}  // namespace dse
