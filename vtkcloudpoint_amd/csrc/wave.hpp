// wave.hpp -- the integer and predicate idioms of a wave (64 lanes) and of a workgroup of whole waves, shared by the
// kernels: scan, all-reduce, count and append.  (reduce.hpp holds the double reductions, whose order is pinned.)
//
// Device only, no __shared__ of its own: a workgroup form takes the caller's LDS words (one per wave unless it says
// otherwise) and holds exactly one __syncthreads(), which every thread of the workgroup must reach.  The words are free
// again after the caller's next barrier.  Workgroups are one-dimensional; lane = threadIdx.x & 63, w = threadIdx.x >> 6.
// Sums are modulo 2^32 (2^64 for the 64-bit all-reduce).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

struct WaveAdd {
  template <class T>
  __device__ __forceinline__ static T op(T a, T b) { return a + b; }
};
struct WaveMin {
  template <class T>
  __device__ __forceinline__ static T op(T a, T b) { return min(a, b); }
};
struct WaveMax {
  template <class T>
  __device__ __forceinline__ static T op(T a, T b) { return max(a, b); }
};
struct WaveOr {
  template <class T>
  __device__ __forceinline__ static T op(T a, T b) { return a | b; }
};

// ---- scan ---------------------------------------------------------------------------------------------------------
// Inclusive scan (Op: WaveAdd or WaveMax) over every group of W consecutive lanes; lane = the lane's index in its group.
// (The shuffles span the wave: what a lane reads from below its group, lane >= d discards.)
template <class Op, int W = 64>
__device__ __forceinline__ uint32_t wave_incl(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < W; d <<= 1) {
    const uint32_t t = __shfl_up(v, d, 64);
    if (lane >= d) v = Op::op(v, t);
  }
  return v;
}

// the value of the lane before (lane 0: its own)
__device__ __forceinline__ uint32_t wave_prev(uint32_t v) { return __shfl_up(v, 1, 64); }

// Exclusive add-scan over the workgroup, in thread order: base + the sum of v over the threads before this one.  wsum:
// one word per wave.
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t* wsum, uint32_t base = 0) {
  const int lane = threadIdx.x & 63;
  const uint32_t inc = wave_incl<WaveAdd>(v, lane);
  const int w = threadIdx.x >> 6;
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t pre = base + inc - v;
  for (int k = 0; k < w; k++) pre += wsum[k];
  return pre;
}
// ... and the workgroup's total, to every thread (TB threads)
template <int TB>
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t* wsum, uint32_t& total) {
  const int lane = threadIdx.x & 63;
  const uint32_t inc = wave_incl<WaveAdd>(v, lane);
  const int w = threadIdx.x >> 6;
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t pre = inc - v, tot = 0;
  for (int k = 0; k < TB / 64; k++) {
    if (k < w) pre += wsum[k];
    tot += wsum[k];
  }
  total = tot;
  return pre;
}

// ---- all-reduce ---------------------------------------------------------------------------------------------------
// Op (WaveAdd, WaveMin, WaveMax, WaveOr) over the wave's 64 values, to every lane: an xor butterfly, offsets 32 ... 1.
// T: a 32- or 64-bit integer.
template <class Op, class T>
__device__ __forceinline__ T wave_all(T v) {
  static_assert(std::is_integral<T>::value && (sizeof(T) == 4 || sizeof(T) == 8), "wave_all: a 32- or 64-bit integer");
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = Op::op(v, __shfl_xor(v, d, 64));
  return v;
}

// ---- count --------------------------------------------------------------------------------------------------------
// the lanes of the wave that hold pred, to every lane
__device__ __forceinline__ uint32_t wave_count(bool pred) { return (uint32_t)__popcll(__ballot(pred)); }

// The threads of the workgroup (TB of them) that hold pred: true in thread 0, which alone gets the count.
template <int TB>
__device__ __forceinline__ bool block_count(bool pred, uint32_t* wc, uint32_t& total) {
  const uint32_t c = wave_count(pred);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x != 0) return false;
  uint32_t t = 0;
  for (int k = 0; k < TB / 64; k++) t += wc[k];
  total = t;
  return true;
}
// two predicates behind the one barrier; wc: 2 * TB / 64 words
template <int TB>
__device__ __forceinline__ bool block_count(bool pa, bool pb, uint32_t* wc, uint32_t& ta, uint32_t& tb) {
  const uint32_t ca = wave_count(pa), cb = wave_count(pb);
  if ((threadIdx.x & 63) == 0) {
    wc[threadIdx.x >> 6] = ca;
    wc[TB / 64 + (threadIdx.x >> 6)] = cb;
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  uint32_t a = 0, b = 0;
  for (int k = 0; k < TB / 64; k++) {
    a += wc[k];
    b += wc[TB / 64 + k];
  }
  ta = a;
  tb = b;
  return true;
}

// The rank of a pred thread among the pred threads of the workgroup, in thread order; 0 to the other threads.
__device__ __forceinline__ uint32_t block_rank(bool pred, uint32_t* wc) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(pred);
  if (lane == 0) wc[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0;
  if (pred) {
    for (int k = 0; k < w; k++) before += wc[k];
    before += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  }
  return before;
}
// The number of pred threads before this one, to every thread, and the number of pred threads (TB threads)
template <int TB>
__device__ __forceinline__ uint32_t block_rank(bool pred, uint32_t* wc, uint32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(pred);
  if (lane == 0) wc[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), tot = 0;
  for (int k = 0; k < TB / 64; k++) {
    if (k < w) before += wc[k];
    tot += wc[k];
  }
  total = tot;
  return before;
}
// ---- append -------------------------------------------------------------------------------------------------------
// Wave-aggregated append: one atomicAdd on *counter per wave with a pred lane (none when no lane has pred); a pred lane
// gets its slot, in lane order behind the wave's base.  Every lane of the wave calls it.
__device__ __forceinline__ uint32_t wave_append(bool pred, uint32_t* counter) {
  const int lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(pred);
  if (!m) return 0;  // wave-uniform
  const int leader = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, leader, 64);
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}
