// Launch shapes shared by the row-gather kernels of aggregate.hip and
// aggmax.hip: the vector width the operands allow, the lane group per output
// row, the neighbour rows in flight and the CSR backward's long-row rule.
// Host side only; the kernels take the results as template arguments.
#pragma once
#include <initializer_list>

#include "common.hpp"

namespace nts_hip {

constexpr int kAggThreads = 256;

// The CSR backward's long rows (k_spmm_gather's COOP, aggregate.hip): a row of
// more than kLongRow(U) edges is summed as the block's lane groups' in-order
// pieces; a lane group takes at most kCoopRows rows
constexpr uint32_t kLongRow(int u) { return 4 * u; }
constexpr uint32_t kCoopRows = 16;

// The widest vector (4, 2 or 1 floats) the rows of these operands allow: F a
// multiple of it and every row start aligned to it (a NULL operand is absent).
// pad: rows padded to a 16-byte multiple (the 128-byte feature / output pitch)
// take float4 whatever F is, the partial last vector reading pitch padding
// and storing only its valid floats.
struct Rows {
  const void* p;
  uint64_t ld;  // pitch in floats
};
static inline int row_vec(uint32_t F, std::initializer_list<Rows> ops, bool pad = false) {
  auto fits = [&](uint32_t cols, int vec) {
    bool ok = cols % vec == 0;
    for (const Rows& r : ops)
      ok = ok && (!r.p || (cols <= r.ld && r.ld % vec == 0 && (uintptr_t)r.p % (4 * vec) == 0));
    return ok;
  };
  if (pad && fits((F + 3) / 4 * 4, 4)) return 4;
  return fits(F, 4) ? 4 : fits(F, 2) ? 2 : 1;
}

struct Shape {
  int lpd, nch;
};
// (128-float rows on 16-lane groups of two float4 per lane — four rows per
// wave instead of two — measured: hop-0 backward 42.5 vs 44.8 us, the bottom
// CSR backward 125-127 vs 122, C2 0.824 vs 0.807 ms/step; not kept)
static inline Shape pick_shape(uint32_t nv) {
  if (nv <= 8) return {8, 1};
  if (nv <= 16) return {16, 1};
  if (nv <= 32) return {32, 1};
  if (nv <= 64) return {64, 1};
  uint32_t nch = (nv + 63) / 64;
  return {64, (int)std::min<uint32_t>(nch, 8)};
}

// rows in flight per lane group, by the floats a lane holds of one row
constexpr int gather_u(int floats_per_lane) {
  return floats_per_lane <= 4 ? 8 : floats_per_lane <= 12 ? 5 : 4;
}
constexpr uint32_t kGatherGridCap = 1u << 24;

}  // namespace nts_hip
