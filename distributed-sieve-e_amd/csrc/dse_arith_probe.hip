// dse_arith_probe.hip -- the wheel kernel's integer helpers, run elementwise on
// the device for the tests (dse_debug_wheel_arith_dev, include/dse.h): Kb mod p
// of the L units in its three regimes (kb_mod_p_f32, kb_mod_p<false>,
// kb_mod_p<true>), mod_barrett, barrett_factor, and the small-prime helpers
// of the A, B1 and B2 units (div_small, div_ceil_small, mulmod_small,
// plane_first, first_at_or_after). Every op calls the function of
// dse_wheel_kernel.h that the kernels call, with invp = fast_rcp((float)p)
// formed as the units form it; nothing is restated here. Built with the wheel
// units' flags and the full geometry, whose unit thresholds wheel_consts()
// reports (dse_debug_get_stat "wheel_*").
#include "dse_wheel_kernel.h"

namespace dse {
namespace {

__device__ __forceinline__ uint64_t arith_op(uint32_t op, uint64_t x, uint32_t p) {
  const float invp = fast_rcp((float)p);
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  switch (op) {
    case kArithKbModF32: return kb_mod_p_f32(lo, p, invp);
    case kArithKbModF38: return kb_mod_p<false>(x, p, invp, 0ull);
    case kArithKbModBarrett: return kb_mod_p<true>(x, p, invp, barrett_factor(p));
    case kArithModBarrett: return mod_barrett(x, p, barrett_factor(p));
    case kArithBarrettFactor: return barrett_factor(p);
    case kArithDivSmall: return div_small(lo, p, invp);
    case kArithDivCeilSmall: return div_ceil_small(lo, p, invp);
    case kArithMulmodSmall: return mulmod_small(lo, hi, p, invp);
    case kArithPlaneFirst: {
      // the staged word of a mid prime and its two halves, as the kernel packs
      // and the A, B1 and B2 units unpack them
      const uint32_t pi = p | ((uint32_t)inv30_of(p) << 16);
      return plane_first(lo, hi, pi & 0xFFFFu, pi >> 16, fast_rcp((float)(pi & 0xFFFFu)));
    }
    case kArithFirstAtOrAfter: return first_at_or_after(lo, hi, p, invp);
    default: return 0;
  }
}

__global__ void arith_probe_kernel(uint32_t op, const uint64_t* __restrict__ x, const uint64_t* __restrict__ y,
                                   uint64_t n, uint64_t* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t yi = y[i];
    // p < 2 or p >= 2^32 is outside every op's domain (barrett_factor's
    // correction loops need p >= 2): 0, without running the op
    out[i] = yi < 2 || (yi >> 32) ? 0ull : arith_op(op, x[i], (uint32_t)yi);
  }
}

}  // namespace

WheelConsts wheel_consts() { return {TA, TB1, TB, (uint32_t)kWheelLogKP, kWheelMaxPrime}; }

hipError_t launch_arith_probe(uint32_t op, const uint64_t* x, const uint64_t* y, uint64_t n, uint64_t* out,
                              int num_cus, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint64_t grid = std::min<uint64_t>((n + 255) / 256, 8ull * (uint64_t)num_cus);
  hipLaunchKernelGGL(arith_probe_kernel, dim3((uint32_t)grid), dim3(256), 0, stream, op, x, y, n, out);
  return hipGetLastError();
}

}  // namespace dse
