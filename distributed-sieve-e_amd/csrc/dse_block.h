// dse_block.h -- wave and workgroup primitives of the gfx950 kernels (device
// only): sums and inclusive scans by shuffles inside a wave of 64, the waves'
// totals through one LDS word per wave, one barrier; the best of a pair under
// a caller's order (block_best, two barriers).
//
// s_wave arguments are kThreads / 64 elements of LDS. A primitive writes them
// before its barrier and reads them behind it, so a second call on the same
// array needs a barrier of the caller's in between.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dse {

struct ScanAdd {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const {
    return a + b;
  }
};
struct ScanMax {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const {
    return a > b ? a : b;
  }
};

// the wave's sum, in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (uint32_t o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// inclusive scan over the wave's lanes
template <typename T, typename Op = ScanAdd>
__device__ __forceinline__ T wave_scan(T v, Op op = Op()) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(v, o);
    if (lane >= o) v = op(v, y);
  }
  return v;
}

// inclusive scan (sum) of one value per thread over the workgroup; *total = the
// workgroup's sum, in every thread
template <uint32_t kThreads, typename T>
__device__ __forceinline__ T block_scan(T v, T* s_wave, T* total) {
  static_assert(kThreads % 64 == 0, "whole waves");
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const T x = wave_scan(v);
  if (lane == 63) s_wave[wave] = x;
  __syncthreads();
  T base = 0, sum = 0;
#pragma unroll
  for (uint32_t i = 0; i < kThreads / 64; ++i) {
    const T t = s_wave[i];
    if (i < wave) base += t;
    sum += t;
  }
  *total = sum;
  return x + base;
}

// the workgroup's sum, in every thread
template <uint32_t kThreads, typename T>
__device__ __forceinline__ T block_sum(T v, T* s_wave) {
  static_assert(kThreads % 64 == 0, "whole waves");
  v = wave_sum(v);
  if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  T sum = 0;
#pragma unroll
  for (uint32_t i = 0; i < kThreads / 64; ++i) sum += s_wave[i];
  return sum;
}

// The workgroup's best pair (a, b), in every thread: better(a', b', a, b) says whether (a', b')
// comes before (a, b). s_a, s_b: kWaves elements of LDS each. Two barriers, the first before the
// arrays are written (their last readers), so a second call needs no barrier in between.
template <uint32_t kWaves, typename Better>
__device__ __forceinline__ void block_best(uint64_t& a, uint64_t& b, unsigned long long* s_a, unsigned long long* s_b,
                                           Better better) {
  for (uint32_t o = 32; o > 0; o >>= 1) {
    const uint64_t oa = (uint64_t)__shfl_xor((unsigned long long)a, o);
    const uint64_t ob = (uint64_t)__shfl_xor((unsigned long long)b, o);
    if (better(oa, ob, a, b)) {
      a = oa;
      b = ob;
    }
  }
  __syncthreads();
  if ((threadIdx.x & 63u) == 0) {
    s_a[threadIdx.x >> 6] = a;
    s_b[threadIdx.x >> 6] = b;
  }
  __syncthreads();
  a = s_a[0];
  b = s_b[0];
  for (uint32_t i = 1; i < kWaves; ++i)
    if (better(s_a[i], s_b[i], a, b)) {
      a = s_a[i];
      b = s_b[i];
    }
}

// The single-workgroup scan over n values (tile or segment sums) by one
// workgroup of kSliceThreads threads: a thread owns the contiguous slice
// [b0, b1) of ceil(n / kSliceThreads) values, both ends clamped to n (empty
// behind the last value). slice_scan sums the slice through load(b) and scans
// the slice sums: `start` is the sum of everything before b0 (the exclusive
// scan's value at b0), `total` the sum of all n values, the same in every
// thread. The caller walks [b0, b1) once more to write its results back.
constexpr uint32_t kSliceThreads = 1024;

template <typename T>
struct ScanSlice {
  uint32_t b0, b1;
  T start, total;
};

template <typename T, typename Load>
__device__ __forceinline__ ScanSlice<T> slice_scan(uint32_t n, T* s_wave, Load&& load) {
  const uint32_t per = (n + kSliceThreads - 1) / kSliceThreads;
  ScanSlice<T> s;
  s.b0 = min(n, threadIdx.x * per);
  s.b1 = min(n, s.b0 + per);
  T sum = 0;
  for (uint32_t b = s.b0; b < s.b1; ++b) sum += load(b);
  s.start = block_scan<kSliceThreads>(sum, s_wave, &s.total) - sum;
  return s;
}

}  // namespace dse
