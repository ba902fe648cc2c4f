// dse_wheel_plain.hip -- the wheel kernel's instantiation for ranges without
// bucketed primes (N up to 1.1e12, the headline configs), in a translation unit
// of its own so it has its own compile flags (Makefile, PLAIN_FLAGS: iterative
// ILP like the bucket instantiation since round 6; the default machine
// scheduler won in round 3) and its unit loop carries no bucket code.
#include "dse_wheel_kernel.h"

namespace dse {

hipError_t launch_wheel_plain(const void* table, const WheelArgs& wa, int num_cus, hipStream_t stream) {
  return launch_wheel<false>(table, wa, num_cus, stream);
}

}  // namespace dse
