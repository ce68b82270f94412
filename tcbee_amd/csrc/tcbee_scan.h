// tcbee_scan.h — what the segmented-scan kernels over flow-major columns share
// (tcbee_series.hip, tcbee_peer.hip): the workgroup's exclusive scan of any monoid, and
// the search that places a grouped position in its segment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tcbee {

// The combination of everything before this lane in the workgroup (lanes of the wave
// by shuffles, earlier waves through s_w), and the whole workgroup's in `total`. S needs
// combine(S, S) and shfl_up_v(S, offset) beside it.
template <uint32_t WAVES, class S>
__device__ __forceinline__ S block_excl(const S& v, const S& id, S* s_w, S& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  S x = v;
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const S y = shfl_up_v(x, o);
    if (lane >= o) x = combine(y, x);
  }
  if (lane == 63) s_w[wave] = x;
  S ex = shfl_up_v(x, 1);
  if (lane == 0) ex = id;
  __syncthreads();
  S pre = id;
  total = id;
  for (uint32_t w = 0; w < WAVES; ++w) {
    const S t = s_w[w];
    if (w < wave) pre = combine(pre, t);
    total = combine(total, t);
  }
  __syncthreads();
  return combine(pre, ex);
}

// segment of position j: the k with flow_start[k] <= j < flow_start[k + 1] (an upper
// bound, so among equal bounds of empty segments the non-empty one is found)
__device__ __forceinline__ uint32_t series_segment(const uint32_t* fs, uint32_t n_ids, uint32_t j) {
  uint32_t lo = 0, len = n_ids + 2u;
  while (len > 0) {
    const uint32_t half = len >> 1, mid = lo + half;
    if (fs[mid] <= j) {
      lo = mid + 1u;
      len -= half + 1u;
    } else {
      len = half;
    }
  }
  const uint32_t k = lo ? lo - 1u : 0u;
  return k < n_ids ? k : n_ids;
}

}  // namespace tcbee
