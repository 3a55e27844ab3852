// reduce.hpp -- wave and workgroup reductions of doubles shared by the kernels.
//
// One fixed order everywhere: __shfl_down with offsets 32, 16, ..., 1 inside a wave, then the waves' results in wave
// index order.  The sums that depend on it (ICP's moments, the centroid chunks, the robust range) are deterministic run
// to run; min / max do not depend on it.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = fmin(v, __shfl_down(v, d, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = fmax(v, __shfl_down(v, d, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// how value k of a fold combines
struct FoldSum {
  __device__ static double wave(int, double v) { return wave_sum(v); }
  __device__ static double op(int, double a, double b) { return a + b; }
};
// bounding box: [0, 3) min, [3, 6) max, [6] sum (the non-finite count)
struct FoldBox {
  __device__ static double wave(int k, double v) { return k < 3 ? wave_min(v) : k < 6 ? wave_max(v) : wave_sum(v); }
  __device__ static double op(int k, double a, double b) { return k < 3 ? fmin(a, b) : k < 6 ? fmax(a, b) : a + b; }
};

// Workgroup fold of N values per thread (TB threads, all of them call it): thread k < N writes result k to out[k].
template <int TB, int N, class F>
__device__ __forceinline__ void block_fold(const double (&v)[N], F, double* __restrict__ out) {
  __shared__ double sm[TB / 64][N];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const double r = F::wave(k, v[k]);
    if (lane == 0) sm[w][k] = r;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double r = sm[0][threadIdx.x];
#pragma unroll
    for (int j = 1; j < TB / 64; j++) r = F::op(threadIdx.x, r, sm[j][threadIdx.x]);
    out[threadIdx.x] = r;
  }
}

// The same fold of sums when the caller knows, wave by wave, whether any lane of the wave added a term (`wave_has_terms` is
// wave-uniform).  A wave whose lanes all hold the +0.0 they started from sums to +0.0 through the shuffle tree, so it writes
// +0.0 without the shuffles: the same bits as block_fold with FoldSum.  With clusters far smaller than a workgroup most waves
// are such waves, and the shuffles are what a fold costs.
template <int TB, int N>
__device__ __forceinline__ void block_fold_sum_sparse(const double (&v)[N], bool wave_has_terms, double* __restrict__ out) {
  __shared__ double sm[TB / 64][N];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (wave_has_terms) {
#pragma unroll
    for (int k = 0; k < N; k++) {
      const double r = wave_sum(v[k]);
      if (lane == 0) sm[w][k] = r;
    }
  } else if (lane < N) {
    sm[w][lane] = 0.0;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double r = sm[0][threadIdx.x];
#pragma unroll
    for (int j = 1; j < TB / 64; j++) r = r + sm[j][threadIdx.x];
    out[threadIdx.x] = r;
  }
}
