// Link prediction, all-candidate ranking: for M (head, tail)
// queries the counts of candidates that score above / equal to the true tail,
// from an [n_cand, D] x [D, M] product on the f32 matrix cores that is never
// written: the epilogue compares each accumulator with its query's positive
// score and counts.  No counterpart in the reference; the metric is OGB's
// MRR / Hits@K over all candidate tails.
#include "common.hpp"
#include "lp_filter.hpp"

namespace nts_hip {

constexpr int kRkThreads = 256;  // 4 waves, 2 (candidates) x 2 (queries)
constexpr int kRkTile = 128;     // candidates and queries per block tile
constexpr int kRkK = 32;         // k columns per LDS slab
// k-major slabs [kRkK][kRkLd]: fragment reads run along a row of the slab; 130:
// the two lanes of a row write k and k + 16, 16 * 130 = 32 (mod 64) banks apart
constexpr int kRkLd = kRkTile + 2;
constexpr uint32_t kRkNone = 0xFFFFFFFFu;  // no row (ids are < n_rows <= 2^32 - 1)
constexpr int kRkValidPerWave = 2048;      // candidates per wave of k_lp_rank_valid

using f32x16 = __attribute__((ext_vector_type(16))) float;

// The positive's score, the same chain the tile code computes (fmaf over k
// ascending from 0), and the zeroed outputs.
__global__ __launch_bounds__(kRkThreads) void k_lp_rank_init(
    const float* __restrict__ H, uint64_t ldh, uint32_t D, const uint32_t* __restrict__ q_head,
    const uint32_t* __restrict__ q_tail, uint32_t M, float* __restrict__ s_pos,
    uint32_t* __restrict__ greater, uint32_t* __restrict__ equal, uint32_t* __restrict__ n_valid) {
  const uint32_t i = blockIdx.x * kRkThreads + threadIdx.x;
  if (i >= M) return;
  const float* hu = H + (uint64_t)q_head[i] * ldh;
  const float* hv = H + (uint64_t)q_tail[i] * ldh;
  float acc = 0.f;
  for (uint32_t k = 0; k < D; ++k) acc = fmaf(hv[k], hu[k], acc);
  s_pos[i] = acc;
  greater[i] = 0u;
  equal[i] = 0u;
  n_valid[i] = 0u;
}

// columns [k0 + 16 half, + 16) of row `rid` into column r of a k-major slab;
// columns >= D and a missing row are zeros (the row's pad is never read)
template <bool VEC>
__device__ __forceinline__ void lp_rank_stage(const float* __restrict__ H, uint64_t ldh, uint32_t D,
                                              uint32_t k0, uint32_t rid, int half, float* slab_col) {
  const float* row = H + (uint64_t)(rid == kRkNone ? 0u : rid) * ldh;
  const uint32_t kb = k0 + 16u * half;
  float v[16];
  if constexpr (VEC) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rid != kRkNone && kb + 4u * j < D) x = *reinterpret_cast<const float4*>(row + kb + 4u * j);
      v[4 * j] = x.x;
      v[4 * j + 1] = x.y;
      v[4 * j + 2] = x.z;
      v[4 * j + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = (rid != kRkNone && kb + j < D) ? row[kb + j] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) slab_col[(16 * half + j) * kRkLd] = v[j];
}

// Block (x: query tile, y: a stride class of candidate tiles).  The MFMA's A
// operand is the candidate tile, B the query tile, so a lane's 16 accumulators
// of a 32x32 tile are 16 candidates of ONE query (column lane & 31): the
// counts stay in the lane over every candidate tile of the block, the two lane
// halves are added once, and one integer atomicAdd per (query, wave) leaves.
// FILTER: the two binary searches run only for a candidate that would be
// counted (s >= s_pos); n_valid is then k_lp_rank_valid's.
template <bool VEC, bool FILTER>
__global__ __launch_bounds__(kRkThreads, 2) void k_lp_rank(
    const float* __restrict__ H, uint64_t ldh, uint32_t D, const uint32_t* __restrict__ q_head,
    const uint32_t* __restrict__ q_tail, uint32_t M, const uint32_t* __restrict__ cand,
    uint64_t n_cand, const uint64_t* __restrict__ goff, const uint32_t* __restrict__ srows,
    const float* __restrict__ s_pos, uint32_t* __restrict__ greater, uint32_t* __restrict__ equal,
    uint32_t* __restrict__ n_valid) {
  __shared__ float s_a[kRkK * kRkLd];  // candidates, k-major
  __shared__ float s_b[kRkK * kRkLd];  // queries, k-major
  __shared__ uint32_t s_cid[kRkTile], s_qid[kRkTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;  // the wave's 64 candidates x 64 queries
  const int lr = lane & 31, lh = lane >> 5;
  const int srow = tid >> 1, shalf = tid & 1;  // staging: two lanes per row
  const uint32_t q0 = blockIdx.x * kRkTile;
  if (tid < kRkTile) s_qid[tid] = q0 + tid < M ? q_head[q0 + tid] : kRkNone;
  // the lane's two queries
  uint32_t qu[2], qv[2], cg[2] = {0u, 0u}, ce[2] = {0u, 0u}, cv[2] = {0u, 0u};
  float sp[2];
  bool qlive[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const uint32_t q = q0 + wn * 64 + ni * 32 + lr;
    qlive[ni] = q < M;
    qu[ni] = qlive[ni] ? q_head[q] : 0u;
    qv[ni] = qlive[ni] ? q_tail[q] : 0u;
    sp[ni] = qlive[ni] ? s_pos[q] : 0.f;
  }
  __syncthreads();
  const uint32_t my_qid = s_qid[srow];
  const uint32_t n_ct = (uint32_t)((n_cand + kRkTile - 1) / kRkTile);
  for (uint32_t ct = blockIdx.y; ct < n_ct; ct += gridDim.y) {
    const uint64_t gi = (uint64_t)ct * kRkTile + srow;
    const uint32_t my_cid = gi < n_cand ? (cand ? cand[gi] : (uint32_t)gi) : kRkNone;
    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    for (uint32_t k0 = 0; k0 < D; k0 += kRkK) {
      __syncthreads();  // the slabs' and s_cid's readers are done
      if (k0 == 0 && shalf == 0) s_cid[srow] = my_cid;
      lp_rank_stage<VEC>(H, ldh, D, k0, my_cid, shalf, s_a + srow);
      lp_rank_stage<VEC>(H, ldh, D, k0, my_qid, shalf, s_b + srow);
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < kRkK; kk += 2) {
        const float* pa = s_a + (kk + lh) * kRkLd + wm * 64 + lr;
        const float* pb = s_b + (kk + lh) * kRkLd + wn * 64 + lr;
        const float a0 = pa[0], a1 = pa[32], b0 = pb[0], b1 = pb[32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    // accumulator r of the lane: candidate row (r & 3) + 8 (r >> 2) + 4 lh
    // one bit per accumulator: valid, above, equal
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const uint32_t* cid = s_cid + wm * 64 + mi * 32 + 4 * lh;
      uint32_t mv[2] = {0u, 0u}, mg[2] = {0u, 0u}, me[2] = {0u, 0u};
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t w = cid[(r & 3) + 8 * (r >> 2)];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const float s = acc[mi][ni][r];
          const bool ok = qlive[ni] && w != kRkNone && w != qv[ni];
          mv[ni] |= (ok ? 1u : 0u) << r;
          mg[ni] |= ((ok && s > sp[ni]) ? 1u : 0u) << r;
          me[ni] |= ((ok && s == sp[ni]) ? 1u : 0u) << r;
        }
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        if constexpr (FILTER) {  // lazily: only what would be counted is looked up
          for (uint32_t m = mg[ni] | me[ni]; m; m &= m - 1u) {
            const uint32_t r = (uint32_t)__ffs((int)m) - 1u;
            if (!lp_pair_free(goff, srows, qu[ni], cid[(r & 3u) + 8u * (r >> 2)])) {
              mg[ni] &= ~(1u << r);
              me[ni] &= ~(1u << r);
            }
          }
        } else {
          cv[ni] += (uint32_t)__popc(mv[ni]);
        }
        cg[ni] += (uint32_t)__popc(mg[ni]);
        ce[ni] += (uint32_t)__popc(me[ni]);
      }
    }
  }
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const uint32_t g = cg[ni] + __shfl_xor(cg[ni], 32, 64);
    const uint32_t e = ce[ni] + __shfl_xor(ce[ni], 32, 64);
    const uint32_t v = cv[ni] + __shfl_xor(cv[ni], 32, 64);
    const uint32_t q = q0 + wn * 64 + ni * 32 + lr;
    if (lh == 0 && q < M) {
      if (g) atomicAdd(greater + q, g);
      if (e) atomicAdd(equal + q, e);
      if (!FILTER && v) atomicAdd(n_valid + q, v);
    }
  }
}

// The filtered n_valid: a wave per (query, kRkValidPerWave candidates), every
// candidate through the filter, one atomicAdd per wave.
__global__ __launch_bounds__(kRkThreads) void k_lp_rank_valid(
    const uint32_t* __restrict__ q_head, const uint32_t* __restrict__ q_tail, uint32_t M,
    const uint32_t* __restrict__ cand, uint64_t n_cand, const uint64_t* __restrict__ goff,
    const uint32_t* __restrict__ srows, uint32_t* __restrict__ n_valid) {
  const int lane = threadIdx.x & 63;
  const uint32_t q = blockIdx.y * (kRkThreads / 64) + (threadIdx.x >> 6);
  if (q >= M) return;  // (wave-uniform)
  const uint32_t u = q_head[q], v = q_tail[q];
  const uint64_t beg = (uint64_t)blockIdx.x * kRkValidPerWave;
  const uint64_t end = beg + kRkValidPerWave < n_cand ? beg + kRkValidPerWave : n_cand;
  uint32_t n = 0;
  for (uint64_t j = beg + lane; j < end; j += 64) {
    const uint32_t w = cand ? cand[j] : (uint32_t)j;
    if (w != v && lp_pair_free(goff, srows, u, w)) ++n;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if (lane == 0 && n) atomicAdd(n_valid + q, n);
}

}  // namespace nts_hip

using namespace nts_hip;

extern "C" {

int nts_hip_lp_rank(nts_hip_ctx* ctx, const float* H, uint64_t ldh, uint32_t D, uint32_t n_rows,
                    const uint32_t* q_head, const uint32_t* q_tail, uint32_t M,
                    const uint32_t* cand, uint64_t n_cand, const uint64_t* adj_offset,
                    const uint32_t* adj_sorted, uint32_t* greater, uint32_t* equal,
                    uint32_t* n_valid) {
  NTS_CHECK_ARG(ctx, "ctx is NULL");
  NTS_CHECK_ARG(H && q_head && q_tail && greater && equal && n_valid, "NULL pointer");
  NTS_CHECK_ARG(D >= 1 && D <= 1024, "D must be in 1..1024");
  NTS_CHECK_ARG(ldh >= D, "ldh < D");
  NTS_CHECK_ARG(M >= 1, "M == 0");
  NTS_CHECK_ARG(n_rows >= 1, "n_rows == 0");
  NTS_CHECK_ARG((adj_offset != nullptr) == (adj_sorted != nullptr),
                "adj_offset and adj_sorted go together (both NULL: unfiltered)");
  if (!cand) n_cand = n_rows;
  NTS_CHECK_ARG(n_cand >= 1 && n_cand <= 0xFFFFFFFFull, "n_cand must be in 1..2^32 - 1");
  NTS_RET(ensure_scratch(ctx, (size_t)M * sizeof(float)));
  float* s_pos = (float*)ctx->scratch;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_lp_rank_init, dim3(ceil_div(M, kRkThreads)), dim3(kRkThreads), 0, st, H, ldh,
                     D, q_head, q_tail, M, s_pos, greater, equal, n_valid);
  NTS_LAUNCH_CHECK();
  const bool filter = adj_offset != nullptr;
  const bool vec = D % 4 == 0 && ldh % 4 == 0 && (reinterpret_cast<uintptr_t>(H) & 15u) == 0;
  const uint32_t q_tiles = ceil_div(M, kRkTile), c_tiles = ceil_div(n_cand, kRkTile);
  // about eight blocks per CU of a 256-CU part, each over >= 1 candidate tile
  const uint32_t split = std::min<uint32_t>({c_tiles, std::max<uint32_t>(1u, 2048u / q_tiles), 65535u});
  const dim3 grid(q_tiles, split), block(kRkThreads);
#define NTS_LP_RANK(VEC, FILTER)                                                              \
  hipLaunchKernelGGL((k_lp_rank<VEC, FILTER>), grid, block, 0, st, H, ldh, D, q_head, q_tail, M, \
                     cand, n_cand, adj_offset, adj_sorted, (const float*)s_pos, greater, equal,  \
                     n_valid)
  if (vec && filter) NTS_LP_RANK(true, true);
  else if (vec) NTS_LP_RANK(true, false);
  else if (filter) NTS_LP_RANK(false, true);
  else NTS_LP_RANK(false, false);
#undef NTS_LP_RANK
  NTS_LAUNCH_CHECK();
  if (filter) {
    // grid.y is limited to 65535: queries in passes of that many waves' worth
    const uint32_t per_pass = 65535u * (kRkThreads / 64);
    for (uint32_t m0 = 0; m0 < M; m0 += per_pass) {
      const uint32_t m = std::min<uint32_t>(per_pass, M - m0);
      hipLaunchKernelGGL(k_lp_rank_valid,
                         dim3(ceil_div(n_cand, kRkValidPerWave), ceil_div(m, kRkThreads / 64)), block,
                         0, st, q_head + m0, q_tail + m0, m, cand, n_cand, adj_offset, adj_sorted,
                         n_valid + m0);
      NTS_LAUNCH_CHECK();
    }
  }
  return NTS_OK;
}

}  // extern "C"
