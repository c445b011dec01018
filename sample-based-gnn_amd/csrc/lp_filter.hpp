// The is-edge test of link prediction's filters: the graph's
// row_indices sorted ascending within each destination's segment (srows) and
// its column_offset (goff).  nts_hip_lp_batch_filtered rejects a negative with
// it; nts_hip_lp_rank drops a candidate with it.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace nts_hip {

// x in rows[beg, end), a segment sorted ascending
__device__ __forceinline__ bool lp_row_has(const uint32_t* __restrict__ rows, uint64_t beg,
                                           uint64_t end, uint32_t x) {
  while (beg < end) {
    const uint64_t mid = beg + ((end - beg) >> 1);
    const uint32_t r = rows[mid];
    if (r == x) return true;
    if (r < x) beg = mid + 1;
    else end = mid;
  }
  return false;
}

// the pair (u, w) is free: w != u and the graph holds neither u -> w (u in
// w's segment) nor w -> u (w in u's segment)
__device__ __forceinline__ bool lp_pair_free(const uint64_t* __restrict__ goff,
                                             const uint32_t* __restrict__ srows, uint32_t u,
                                             uint32_t w) {
  return w != u && !lp_row_has(srows, goff[w], goff[(uint64_t)w + 1], u) &&
         !lp_row_has(srows, goff[u], goff[(uint64_t)u + 1], w);
}

}  // namespace nts_hip
