// dse_wheel_half.hip -- the wheel kernel again with half-size segments (2^16
// periods per plane, a 64 KiB LDS image) for the tails of ranges
// (launch_wheel_ranges_half, dse_internal.h): a range's last partial round of
// full segments is sieved as twice as many half segments, so more CUs share
// it. Same kernel header as the other units; only the geometry differs, so
// nothing of it may leave this unit (internal linkage throughout).
#define DSE_WHEEL_LOG_KP 16
#include "dse_wheel_args.h"
#include "dse_wheel_kernel.h"

namespace dse {

// The tail of a launch whose last round of full segments would leave most
// CUs idle (launch_pooled, dse_wheel.hip). Primes <= kWheelMaxPrime only.
hipError_t launch_wheel_ranges_half(const void* table, const RangeSpec* rs, size_t n, int num_cus,
                                    hipStream_t stream, PlanStats* plan) {
  return launch_wheel_batches(launch_wheel<false>, table, rs, n, num_cus, stream, plan, &PlanStats::half_segments);
}

}  // namespace dse
