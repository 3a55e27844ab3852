// radix_pick.hpp -- the pick step of an 8-bit radix select run by a workgroup of 256 threads, one thread per bin: the
// trimmed ICP's select (icp.hip) and the per-cluster quantiles (cluster_quant.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wave.hpp"

// Thread t holds the count c of bin t; rank r, 1 <= r <= the total: the bin g with below(g) < r <= below(g) + c(g) and
// the rank left in it, to every thread.  sh: 8 words of LDS, free again on return.
__device__ __forceinline__ void vcp_radix_pick(uint32_t c, uint32_t r, uint32_t* sh, uint32_t& g, uint32_t& left) {
  const int lane = threadIdx.x & 63;
  uint32_t inc = wave_incl<WaveAdd>(c, lane);
  const int w = threadIdx.x >> 6;
  if (threadIdx.x == 0) {
    sh[4] = 0;
    sh[5] = 1;
  }
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  for (int u = 0; u < w; u++) inc += sh[u];
  const uint32_t exc = inc - c;
  if (exc < r && r <= inc) {
    sh[4] = threadIdx.x;
    sh[5] = r - exc;
  }
  __syncthreads();
  g = sh[4];
  left = sh[5];
  __syncthreads();
}
