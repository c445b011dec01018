// Link prediction: the batch builder (positive pairs, uniform
// negatives, the distinct endpoints as the seed set, the incidence CSR of the
// pairs over those seeds) and the fused dot-product scorer + sigmoid BCE loss
// with its gathered, atomic-free backward; §8u: the key table of a batch's
// target edges, the mask that gives them the coefficient 0 in the sampled
// blocks, and negatives filtered against the graph.  No counterpart in the reference
// (its toolkits are node classifiers); the semantics follow DGL's
// as_edge_prediction_sampler + negative_sampler.Uniform and PyG's
// LinkNeighborLoader.
#include "common.hpp"
#include "lp_filter.hpp"

namespace nts_hip {

constexpr uint32_t kLpLayerTag = 0x20000000u;  // next to 0x80000000 (shared), 0x40000000 (weighted)
constexpr uint32_t kLpTries = 16;  // draws per filtered negative (tags kLpLayerTag | 0..15)
constexpr int kLpThreads = 256;
constexpr int kLpPosPerBlock = 16;  // positives (with their negatives) per block of the loss kernels

// ---------------------------------------------------------------------------
// batch construction
// ---------------------------------------------------------------------------
// keys[2p] / keys[2p + 1] = the global ids of pair p's two ends.  FILTER
// (DESIGN §8u): up to kLpTries draws, try t under the tag kLpLayerTag | t (t = 0
// is the unfiltered draw); a tail w is rejected when w == u or the graph holds
// u -> w or w -> u (srows: row_indices sorted within each destination's
// segment); the first accepted one is taken, else the last is kept and counted.
template <bool FILTER>
__global__ __launch_bounds__(kLpThreads) void k_lp_pairs(const uint32_t* __restrict__ pos_src,
                                                         const uint32_t* __restrict__ pos_dst,
                                                         uint32_t B, uint32_t K, uint64_t V,
                                                         uint64_t seed, uint64_t batch_seq,
                                                         uint32_t* __restrict__ keys,
                                                         const uint64_t* __restrict__ goff,
                                                         const uint32_t* __restrict__ srows,
                                                         uint32_t* __restrict__ unresolved) {
  const uint32_t P = B * (1u + K);
  const uint32_t p = blockIdx.x * kLpThreads + threadIdx.x;
  if (p >= P) return;
  uint32_t u, v;
  if (p < B) {
    u = pos_src[p];
    v = pos_dst[p];
  } else {
    const uint32_t q = p - B, i = q / K, k = q - i * K;
    u = pos_src[i];
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32) ^ (uint32_t)(batch_seq >> 32));
    const uint32_t j = k & 3u;
    const uint32_t tries = FILTER ? kLpTries : 1u;
    bool ok = false;
    for (uint32_t t = 0; t < tries && !ok; ++t) {
      // the sampler's counter layout (philox_word, sampler.hip) under the tag
      const uint4 c = make_uint4(k >> 2, i, kLpLayerTag | t, (uint32_t)batch_seq);
      const uint4 r = philox4x32_10(c, key);
      const uint32_t x = j == 0 ? r.x : (j == 1 ? r.y : (j == 2 ? r.z : r.w));
      v = (uint32_t)(((uint64_t)x * V) >> 32);
      if constexpr (FILTER) ok = lp_pair_free(goff, srows, u, v);
    }
    if constexpr (FILTER)
      if (!ok) atomicAdd(unresolved, 1u);
  }
  keys[2 * (uint64_t)p] = u;
  keys[2 * (uint64_t)p + 1] = v;
}

// flag[i] = 1 where sorted slot i opens a new endpoint id
__global__ __launch_bounds__(kLpThreads) void k_lp_heads(const uint32_t* __restrict__ skeys,
                                                         uint32_t n, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * kLpThreads + threadIdx.x;
  if (i < n) flag[i] = (i == 0 || skeys[i] != skeys[i - 1]) ? 1u : 0u;
}

// rank = exclusive scan of the flags; the local row of sorted slot i is
// rank[i] + flag - 1.  Rows past the live count get the end offset, so
// inc_offset is a whole CSR over v_cap rows.
__global__ __launch_bounds__(kLpThreads) void k_lp_finish(
    const uint32_t* __restrict__ skeys, const uint32_t* __restrict__ rank,
    const uint32_t* __restrict__ inc_slot, uint32_t n, uint32_t v_cap,
    uint32_t* __restrict__ destination, uint32_t* __restrict__ v_size,
    uint32_t* __restrict__ pair_u, uint32_t* __restrict__ pair_v,
    uint32_t* __restrict__ inc_offset) {
  const uint32_t i = blockIdx.x * kLpThreads + threadIdx.x;
  const uint32_t rows = rank[n];
  if (i == 0) *v_size = rows;
  if (i >= rows && i <= v_cap) inc_offset[i] = n;
  if (i >= n) return;
  const uint32_t key = skeys[i];
  const bool head = i == 0 || key != skeys[i - 1];
  const uint32_t local = rank[i] + (head ? 1u : 0u) - 1u;
  if (head) {
    destination[local] = key;
    inc_offset[local] = i;
  }
  const uint32_t slot = inc_slot[i];
  ((slot & 1u) ? pair_v : pair_u)[slot >> 1] = local;
}

// ---------------------------------------------------------------------------
// target-edge exclusion
// ---------------------------------------------------------------------------
// item i < B: the positive (src, dst) as (lo, hi) = (pos_src, pos_dst); item
// B + i (reverse): the same edge turned round
__global__ __launch_bounds__(kLpThreads) void k_lp_excl_ends(const uint32_t* __restrict__ pos_src,
                                                             const uint32_t* __restrict__ pos_dst,
                                                             uint32_t B, uint32_t n,
                                                             uint32_t* __restrict__ lo,
                                                             uint32_t* __restrict__ hi) {
  const uint32_t i = blockIdx.x * kLpThreads + threadIdx.x;
  if (i >= n) return;
  const bool rev = i >= B;
  const uint32_t j = rev ? i - B : i;
  const uint32_t s = pos_src[j], d = pos_dst[j];
  lo[i] = rev ? d : s;
  hi[i] = rev ? s : d;
}

__global__ __launch_bounds__(kLpThreads) void k_lp_excl_gather(const uint32_t* __restrict__ in,
                                                               const uint32_t* __restrict__ idx,
                                                               uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * kLpThreads + threadIdx.x;
  if (i < n) out[i] = in[idx[i]];
}

// flag[i] = 1 where sorted item i opens a new (hi, lo) key
__global__ __launch_bounds__(kLpThreads) void k_lp_excl_heads(const uint32_t* __restrict__ hi,
                                                              const uint32_t* __restrict__ lo,
                                                              uint32_t n, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * kLpThreads + threadIdx.x;
  if (i < n) flag[i] = (i == 0 || hi[i] != hi[i - 1] || lo[i] != lo[i - 1]) ? 1u : 0u;
}

// the distinct keys in ascending order and their count (rank: the exclusive
// scan of the flags); nothing past the count is written
__global__ __launch_bounds__(kLpThreads) void k_lp_excl_finish(
    const uint32_t* __restrict__ hi, const uint32_t* __restrict__ lo,
    const uint32_t* __restrict__ rank, uint32_t n, uint64_t* __restrict__ keys_out,
    uint32_t* __restrict__ n_keys) {
  const uint32_t i = blockIdx.x * kLpThreads + threadIdx.x;
  if (i == 0) *n_keys = rank[n];
  if (i >= n) return;
  if (i == 0 || hi[i] != hi[i - 1] || lo[i] != lo[i - 1])
    keys_out[rank[i]] = ((uint64_t)hi[i] << 32) | (uint64_t)lo[i];
}

// key in keys[0, n), ascending and distinct
__device__ __forceinline__ bool lp_key_hit(const uint64_t* __restrict__ keys, uint32_t n,
                                           uint64_t key) {
  uint32_t beg = 0, end = n;
  while (beg < end) {
    const uint32_t mid = beg + ((end - beg) >> 1);
    const uint64_t k = keys[mid];
    if (k == key) return true;
    if (k < key) beg = mid + 1;
    else end = mid;
  }
  return false;
}

// One thread per live CSC edge (blockIdx.y == 0) or CSR slot (blockIdx.y ==
// 1): its (global dst, global src) looked up in the key table (at most 2 B
// 8-byte keys, cache resident); a hit's coefficient becomes 0, a miss keeps
// its value (had_weights) or becomes 1.  A CSR slot finds its row by a binary
// search of row_offset over the live rows.  A block with its overflow flag
// set, and everything past the live sizes, is neither read nor written.
__global__ __launch_bounds__(kLpThreads) void k_lp_mask(
    const uint32_t* __restrict__ sizes, uint32_t v_cap, uint32_t e_cap, uint32_t s_cap,
    const uint32_t* __restrict__ destination, const uint32_t* __restrict__ edge_dst,
    const uint32_t* __restrict__ sample_ans, const uint32_t* __restrict__ source,
    const uint32_t* __restrict__ row_offset, const uint32_t* __restrict__ column_indices,
    float* __restrict__ w_fwd, float* __restrict__ w_bwd, const uint64_t* __restrict__ keys,
    const uint32_t* __restrict__ n_keys_dev, int had_weights, uint32_t* __restrict__ excluded) {
  if (sizes[3] != 0) return;  // (uniform: every thread of the grid leaves)
  const uint32_t e_live = min(sizes[1], e_cap), n_keys = *n_keys_dev;
  const uint32_t i = blockIdx.x * kLpThreads + threadIdx.x;
  const bool csr = blockIdx.y == 1;
  bool live = i < e_live, hit = false;
  uint32_t d = 0, s = 0;
  if (live && !csr) {
    const uint32_t dl = edge_dst[i];
    live = dl < v_cap;
    if (live) {
      d = destination[dl];
      s = sample_ans[i];
    }
  } else if (live) {
    // the row r with row_offset[r] <= i < row_offset[r + 1], r < the live rows
    const uint32_t rows = min(sizes[2], s_cap);
    uint32_t beg = 0, end = rows;
    while (beg < end) {
      const uint32_t mid = beg + ((end - beg) >> 1);
      if (row_offset[mid + 1] <= i) beg = mid + 1;
      else end = mid;
    }
    const uint32_t dl = column_indices[i];
    live = beg < rows && row_offset[beg] <= i && dl < v_cap;
    if (live) {
      d = destination[dl];
      s = source[beg];
    }
  }
  if (live) {
    hit = lp_key_hit(keys, n_keys, ((uint64_t)d << 32) | (uint64_t)s);
    float* w = csr ? w_bwd : w_fwd;
    if (hit) w[i] = 0.0f;
    else if (!had_weights) w[i] = 1.0f;
  }
  const int cnt = __syncthreads_count(hit && !csr);
  if (threadIdx.x == 0 && cnt) atomicAdd(excluded, (uint32_t)cnt);
}

// ---------------------------------------------------------------------------
// scorer + loss
// ---------------------------------------------------------------------------
__device__ __forceinline__ float lp_sigmoid(float s) {
  if (s >= 0.f) return 1.f / (1.f + expf(-s));
  const float e = expf(s);
  return e / (1.f + e);
}

// <H[u, :], H[v, :]> over D columns by the G lanes of a group; every lane of
// the group returns the sum
template <int G, bool VEC>
__device__ __forceinline__ float lp_dot(const float* __restrict__ hu, const float* __restrict__ hv,
                                        uint32_t D, int gl) {
  float acc = 0.f;
  if constexpr (VEC) {
    for (uint32_t c = 4u * gl; c < D; c += 4u * G) {
      const float4 a = *reinterpret_cast<const float4*>(hu + c);
      const float4 b = *reinterpret_cast<const float4*>(hv + c);
      acc = fmaf(a.x, b.x, acc);
      acc = fmaf(a.y, b.y, acc);
      acc = fmaf(a.z, b.z, acc);
      acc = fmaf(a.w, b.w, acc);
    }
  } else {
    for (uint32_t c = gl; c < D; c += G) acc = fmaf(hu[c], hv[c], acc);
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  return acc;
}

// One group of G lanes per positive i and its K negatives (so the rank of the
// positive is known to the group); a block covers kLpPosPerBlock consecutive
// positives whatever G is, and leaves one loss partial and one 1/rank partial,
// each summed over its positives in ascending order.
template <int G, bool VEC>
__global__ __launch_bounds__(kLpThreads) void k_lp_score(
    const float* __restrict__ H, uint64_t ldh, uint32_t D, const uint32_t* __restrict__ pair_u,
    const uint32_t* __restrict__ pair_v, uint32_t B, uint32_t K, float inv_p,
    float* __restrict__ score, float* __restrict__ g_out, float* __restrict__ part_loss,
    float* __restrict__ part_rr) {
  constexpr int kGroups = kLpThreads / G;
  constexpr int kPer = kLpPosPerBlock / kGroups;
  static_assert(kGroups * kPer == kLpPosPerBlock, "a block covers kLpPosPerBlock positives");
  __shared__ float s_loss[kLpPosPerBlock], s_rr[kLpPosPerBlock];
  const int gl = threadIdx.x % G, grp = threadIdx.x / G;
  for (int j = 0; j < kPer; ++j) {
    const int slot = grp * kPer + j;
    const uint64_t i = (uint64_t)blockIdx.x * kLpPosPerBlock + slot;
    float loss = 0.f, rr = 0.f;
    if (i < B) {
      float s_pos = 0.f;
      uint32_t above = 0;
      for (uint32_t t = 0; t <= K; ++t) {
        const uint64_t p = t == 0 ? i : (uint64_t)B + i * K + (t - 1);
        const float* hu = H + (uint64_t)pair_u[p] * ldh;
        const float* hv = H + (uint64_t)pair_v[p] * ldh;
        const float s = lp_dot<G, VEC>(hu, hv, D, gl);
        const float y = t == 0 ? 1.f : 0.f;
        loss += fmaxf(s, 0.f) - s * y + log1pf(expf(-fabsf(s)));
        if (t == 0) s_pos = s;
        else if (s >= s_pos) ++above;
        if (gl == 0) {
          score[p] = s;
          if (g_out) g_out[p] = (lp_sigmoid(s) - y) * inv_p;
        }
      }
      rr = 1.f / (float)(1u + above);
    }
    if (gl == 0) {
      s_loss[slot] = loss;
      s_rr[slot] = rr;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float l = 0.f, r = 0.f;
    for (int k = 0; k < kLpPosPerBlock; ++k) {
      l += s_loss[k];
      r += s_rr[k];
    }
    part_loss[blockIdx.x] = l;
    part_rr[blockIdx.x] = r;
  }
}

// The block partials in block order (one block; chunks of kLpThreads partials
// staged in LDS, summed by thread 0): loss = sum / P, mrr[0] += sum of 1/rank,
// mrr[1] += B.
__global__ __launch_bounds__(kLpThreads) void k_lp_final(const float* __restrict__ part_loss,
                                                         const float* __restrict__ part_rr,
                                                         uint32_t nblk, float inv_p, float n_pos,
                                                         float* __restrict__ loss,
                                                         float* __restrict__ mrr) {
  __shared__ float s_l[kLpThreads], s_r[kLpThreads];
  float l = 0.f, r = 0.f;
  for (uint32_t c0 = 0; c0 < nblk; c0 += kLpThreads) {
    const uint32_t b = c0 + threadIdx.x;
    s_l[threadIdx.x] = b < nblk ? part_loss[b] : 0.f;
    s_r[threadIdx.x] = b < nblk ? part_rr[b] : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t m = min((uint32_t)kLpThreads, nblk - c0);
      for (uint32_t k = 0; k < m; ++k) {
        l += s_l[k];
        r += s_r[k];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *loss = l * inv_p;
    if (mrr) {
      mrr[0] += r;
      mrr[1] += n_pos;
    }
  }
}

// dH[r, :] = sum over row r's incidence slots, ascending, of g[pair] * H[other
// end, :].  One group of G lanes per row r < *v_size; a gather, no atomics.
template <int G, bool VEC>
__global__ __launch_bounds__(kLpThreads) void k_lp_bwd(
    const float* __restrict__ H, uint64_t ldh, uint32_t D, const uint32_t* __restrict__ pair_u,
    const uint32_t* __restrict__ pair_v, const uint32_t* __restrict__ inc_offset,
    const uint32_t* __restrict__ inc_slot, const uint32_t* __restrict__ v_size, uint32_t v_cap,
    const float* __restrict__ g, float* __restrict__ dH, uint64_t lddh) {
  constexpr int kGroups = kLpThreads / G;
  const int gl = threadIdx.x % G;
  const uint32_t r = blockIdx.x * kGroups + threadIdx.x / G;
  const uint32_t rows = min(*v_size, v_cap);
  if (r >= rows) return;
  const uint32_t beg = inc_offset[r], end = inc_offset[r + 1];
  float* out = dH + (uint64_t)r * lddh;
  if constexpr (VEC) {
    for (uint32_t c = 4u * gl; c < D; c += 4u * G) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (uint32_t t = beg; t < end; ++t) {
        const uint32_t slot = inc_slot[t], p = slot >> 1;
        const uint32_t other = (slot & 1u) ? pair_u[p] : pair_v[p];
        const float gp = g[p];
        const float4 h = *reinterpret_cast<const float4*>(H + (uint64_t)other * ldh + c);
        acc.x += gp * h.x;
        acc.y += gp * h.y;
        acc.z += gp * h.z;
        acc.w += gp * h.w;
      }
      *reinterpret_cast<float4*>(out + c) = acc;
    }
  } else {
    for (uint32_t c = gl; c < D; c += G) {
      float acc = 0.f;
      for (uint32_t t = beg; t < end; ++t) {
        const uint32_t slot = inc_slot[t], p = slot >> 1;
        const uint32_t other = (slot & 1u) ? pair_u[p] : pair_v[p];
        acc += g[p] * H[(uint64_t)other * ldh + c];
      }
      out[c] = acc;
    }
  }
}

static bool lp_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static int lp_check_score_args(nts_hip_ctx* ctx, const float* H, uint64_t ldh, uint32_t D,
                               const uint32_t* pair_u, const uint32_t* pair_v, uint32_t B,
                               uint32_t K, const float* score, const float* loss) {
  NTS_CHECK_ARG(ctx, "ctx is NULL");
  NTS_CHECK_ARG(H && pair_u && pair_v && score && loss, "NULL pointer");
  NTS_CHECK_ARG(D >= 1 && D <= 1024, "D must be in 1..1024");
  NTS_CHECK_ARG(ldh >= D, "ldh < D");
  NTS_CHECK_ARG(B >= 1 && K >= 1, "B and K must be >= 1");
  NTS_CHECK_ARG((uint64_t)B * (1ull + K) <= (1ull << 30), "more than 2^30 pairs");
  return NTS_OK;
}

// scratch of the loss entries: g[P] | part_loss[nblk] | part_rr[nblk]
static int lp_score(nts_hip_ctx* ctx, const float* H, uint64_t ldh, uint32_t D,
                    const uint32_t* pair_u, const uint32_t* pair_v, uint32_t B, uint32_t K,
                    float* score, float* loss, float* mrr, bool want_g, float** g_out) {
  const uint32_t P = B * (1u + K);
  const uint32_t nblk = ceil_div(B, kLpPosPerBlock);
  const size_t g_al = ((size_t)P + 63) / 64 * 64;
  NTS_RET(ensure_scratch(ctx, (g_al + 2 * (size_t)nblk) * sizeof(float)));
  float* g = (float*)ctx->scratch;
  float* part_loss = g + g_al;
  float* part_rr = part_loss + nblk;
  const float inv_p = 1.f / (float)P;
  const bool vec = D % 4 == 0 && ldh % 4 == 0 && lp_aligned16(H);
  float* gp = want_g ? g : nullptr;
#define NTS_LP_SCORE(G, VEC)                                                                   \
  hipLaunchKernelGGL((k_lp_score<G, VEC>), dim3(nblk), dim3(kLpThreads), 0, ctx->stream, H, ldh, \
                     D, pair_u, pair_v, B, K, inv_p, score, gp, part_loss, part_rr)
  if (vec) {
    if (D <= 64) NTS_LP_SCORE(16, true);
    else NTS_LP_SCORE(64, true);
  } else {
    if (D <= 16) NTS_LP_SCORE(16, false);
    else NTS_LP_SCORE(64, false);
  }
#undef NTS_LP_SCORE
  NTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_lp_final, dim3(1), dim3(kLpThreads), 0, ctx->stream, part_loss, part_rr, nblk,
                     inv_p, (float)B, loss, mrr);
  NTS_LAUNCH_CHECK();
  if (g_out) *g_out = g;
  return NTS_OK;
}

}  // namespace nts_hip

using namespace nts_hip;

extern "C" {

// the body of nts_hip_lp_batch and nts_hip_lp_batch_filtered (goff != NULL:
// the redraw rule of k_lp_pairs<true>)
static int lp_batch(nts_hip_ctx* ctx, const uint32_t* pos_src, const uint32_t* pos_dst, uint32_t B,
                    uint32_t K, uint64_t n_vertices, uint64_t batch_seq, uint32_t v_cap,
                    uint32_t* destination, uint32_t* v_size, uint32_t* pair_u, uint32_t* pair_v,
                    uint32_t* inc_offset, uint32_t* inc_slot, const uint64_t* goff,
                    const uint32_t* srows, uint32_t* unresolved) {
  NTS_CHECK_ARG(ctx, "ctx is NULL");
  NTS_CHECK_ARG(pos_src && pos_dst && destination && v_size && pair_u && pair_v && inc_offset &&
                    inc_slot,
                "NULL pointer");
  NTS_CHECK_ARG(K >= 1, "K (negatives per positive) must be >= 1");
  NTS_CHECK_ARG(B >= 1, "B == 0");
  NTS_CHECK_ARG(n_vertices >= 1 && n_vertices <= (1ull << 32), "n_vertices must be in 1..2^32");
  const uint64_t P64 = (uint64_t)B * (1ull + K);
  NTS_CHECK_ARG(P64 <= (1ull << 30), "more than 2^30 pairs");
  NTS_CHECK_ARG((uint64_t)v_cap >= 2 * P64, "v_cap < 2 P (one row per pair end)");
  const uint32_t n = (uint32_t)(2 * P64);
  // scratch: keys[n] | sorted keys[n] | head flags[n] | rank[n + 1] | radix temporaries
  const size_t n_al = ((size_t)n + 64) / 64 * 64;
  NTS_RET(ensure_scratch(ctx, 4 * n_al * sizeof(uint32_t) + radix_tmp_bytes(n)));
  uint32_t* keys = (uint32_t*)ctx->scratch;
  uint32_t* skeys = keys + n_al;
  uint32_t* flag = skeys + n_al;
  uint32_t* rank = flag + n_al;
  void* rtmp = rank + n_al;
  hipStream_t st = ctx->stream;
  if (goff)
    hipLaunchKernelGGL(k_lp_pairs<true>, dim3(ceil_div(P64, kLpThreads)), dim3(kLpThreads), 0, st,
                       pos_src, pos_dst, B, K, n_vertices, ctx->seed, batch_seq, keys, goff, srows,
                       unresolved);
  else
    hipLaunchKernelGGL(k_lp_pairs<false>, dim3(ceil_div(P64, kLpThreads)), dim3(kLpThreads), 0, st,
                       pos_src, pos_dst, B, K, n_vertices, ctx->seed, batch_seq, keys, nullptr,
                       nullptr, nullptr);
  NTS_LAUNCH_CHECK();
  // stable: the slots of one endpoint stay in ascending order
  NTS_RET(radix_sort_pairs(keys, nullptr, skeys, inc_slot, nullptr, n, ceil_log2(n_vertices), rtmp,
                           st, ctx));
  hipLaunchKernelGGL(k_lp_heads, dim3(ceil_div(n, kLpThreads)), dim3(kLpThreads), 0, st,
                     (const uint32_t*)skeys, n, flag);
  NTS_LAUNCH_CHECK();
  NTS_RET(scan1_exclusive(ctx, flag, rank, nullptr, n, st));
  const uint64_t span = std::max<uint64_t>(n, (uint64_t)v_cap + 1);
  hipLaunchKernelGGL(k_lp_finish, dim3(ceil_div(span, kLpThreads)), dim3(kLpThreads), 0, st,
                     (const uint32_t*)skeys, (const uint32_t*)rank, (const uint32_t*)inc_slot, n,
                     v_cap, destination, v_size, pair_u, pair_v, inc_offset);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

int nts_hip_lp_batch(nts_hip_ctx* ctx, const uint32_t* pos_src, const uint32_t* pos_dst, uint32_t B,
                     uint32_t K, uint64_t n_vertices, uint64_t batch_seq, uint32_t v_cap,
                     uint32_t* destination, uint32_t* v_size, uint32_t* pair_u, uint32_t* pair_v,
                     uint32_t* inc_offset, uint32_t* inc_slot) {
  return lp_batch(ctx, pos_src, pos_dst, B, K, n_vertices, batch_seq, v_cap, destination, v_size,
                  pair_u, pair_v, inc_offset, inc_slot, nullptr, nullptr, nullptr);
}

int nts_hip_lp_batch_filtered(nts_hip_ctx* ctx, const uint32_t* pos_src, const uint32_t* pos_dst,
                              uint32_t B, uint32_t K, uint64_t n_vertices, uint64_t batch_seq,
                              uint32_t v_cap, uint32_t* destination, uint32_t* v_size,
                              uint32_t* pair_u, uint32_t* pair_v, uint32_t* inc_offset,
                              uint32_t* inc_slot, const nts_graph_dev* graph,
                              const uint32_t* sorted_rows, uint32_t* unresolved_dev) {
  NTS_CHECK_ARG(graph && graph->column_offset && sorted_rows && unresolved_dev, "NULL pointer");
  NTS_CHECK_ARG(graph->n_vertices == n_vertices, "graph->n_vertices != n_vertices");
  return lp_batch(ctx, pos_src, pos_dst, B, K, n_vertices, batch_seq, v_cap, destination, v_size,
                  pair_u, pair_v, inc_offset, inc_slot, graph->column_offset, sorted_rows,
                  unresolved_dev);
}

int nts_hip_lp_exclude_keys(nts_hip_ctx* ctx, const uint32_t* pos_src, const uint32_t* pos_dst,
                            uint32_t B, int reverse, uint64_t n_vertices, uint32_t key_cap,
                            uint64_t* keys_out, uint32_t* n_keys_dev) {
  NTS_CHECK_ARG(ctx, "ctx is NULL");
  NTS_CHECK_ARG(pos_src && pos_dst && keys_out && n_keys_dev, "NULL pointer");
  NTS_CHECK_ARG(B >= 1, "B == 0");
  NTS_CHECK_ARG(B <= (1u << 30), "more than 2^30 positives");
  NTS_CHECK_ARG(n_vertices >= 1 && n_vertices <= (1ull << 32), "n_vertices must be in 1..2^32");
  const uint32_t n = reverse ? 2 * B : B;
  NTS_CHECK_ARG(key_cap >= n, "key_cap < B (2 B with reverse)");
  // scratch: four [n] arrays, each reused once its first content is dead | radix temporaries
  const size_t n_al = ((size_t)n + 64) / 64 * 64;
  NTS_RET(ensure_scratch(ctx, 4 * n_al * sizeof(uint32_t) + radix_tmp_bytes(n)));
  uint32_t* a0 = (uint32_t*)ctx->scratch;  // lo, then hi in lo order, then the head flags
  uint32_t* a1 = a0 + n_al;                // hi, then hi sorted
  uint32_t* a2 = a1 + n_al;                // lo sorted, then rank[n + 1]
  uint32_t* a3 = a2 + n_al;                // the first sort's order, then lo in (hi, lo) order
  void* rtmp = a3 + n_al;
  hipStream_t st = ctx->stream;
  const dim3 grid(ceil_div(n, kLpThreads)), block(kLpThreads);
  const uint32_t bits = ceil_log2(n_vertices);
  hipLaunchKernelGGL(k_lp_excl_ends, grid, block, 0, st, pos_src, pos_dst, B, n, a0, a1);
  NTS_LAUNCH_CHECK();
  // two stable sorts, the low word first, give the 64-bit order
  NTS_RET(radix_sort_pairs(a0, nullptr, a2, a3, nullptr, n, bits, rtmp, st, ctx));
  hipLaunchKernelGGL(k_lp_excl_gather, grid, block, 0, st, (const uint32_t*)a1, (const uint32_t*)a3,
                     n, a0);
  NTS_LAUNCH_CHECK();
  NTS_RET(radix_sort_pairs(a0, a2, a1, a3, nullptr, n, bits, rtmp, st, ctx));
  hipLaunchKernelGGL(k_lp_excl_heads, grid, block, 0, st, (const uint32_t*)a1, (const uint32_t*)a3,
                     n, a0);
  NTS_LAUNCH_CHECK();
  NTS_RET(scan1_exclusive(ctx, a0, a2, nullptr, n, st));
  hipLaunchKernelGGL(k_lp_excl_finish, grid, block, 0, st, (const uint32_t*)a1, (const uint32_t*)a3,
                     (const uint32_t*)a2, n, keys_out, n_keys_dev);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

int nts_hip_lp_mask_block(nts_hip_ctx* ctx, const nts_sampcsc_dev* block, const uint64_t* keys,
                          const uint32_t* n_keys_dev, int had_weights,
                          uint32_t* excluded_count_dev) {
  NTS_CHECK_ARG(ctx, "ctx is NULL");
  NTS_CHECK_ARG(block && keys && n_keys_dev && excluded_count_dev, "NULL pointer");
  NTS_CHECK_ARG(block->edge_weight_forward, "the block has no edge_weight_forward");
  NTS_CHECK_ARG(block->destination && block->sizes && block->edge_dst && block->sample_ans,
                "NULL pointer in the block");
  const bool csr = block->row_offset != nullptr;
  NTS_CHECK_ARG(!csr || (block->column_indices && block->source && block->edge_weight_backward),
                "a block with row_offset needs column_indices, source and edge_weight_backward");
  if (block->e_cap == 0) return NTS_OK;
  hipLaunchKernelGGL(k_lp_mask, dim3(ceil_div(block->e_cap, kLpThreads), csr ? 2 : 1),
                     dim3(kLpThreads), 0, ctx->stream, (const uint32_t*)block->sizes, block->v_cap,
                     block->e_cap, block->s_cap, block->destination,
                     (const uint32_t*)block->edge_dst, (const uint32_t*)block->sample_ans,
                     (const uint32_t*)block->source, (const uint32_t*)block->row_offset,
                     (const uint32_t*)block->column_indices, block->edge_weight_forward,
                     block->edge_weight_backward, keys, n_keys_dev, had_weights,
                     excluded_count_dev);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

int nts_hip_lp_bce_fwd(nts_hip_ctx* ctx, const float* H, uint64_t ldh, uint32_t D,
                       const uint32_t* pair_u, const uint32_t* pair_v, uint32_t B, uint32_t K,
                       float* score, float* loss, float* mrr) {
  NTS_RET(lp_check_score_args(ctx, H, ldh, D, pair_u, pair_v, B, K, score, loss));
  return lp_score(ctx, H, ldh, D, pair_u, pair_v, B, K, score, loss, mrr, false, nullptr);
}

int nts_hip_lp_bce_train(nts_hip_ctx* ctx, const float* H, uint64_t ldh, uint32_t D,
                         const uint32_t* pair_u, const uint32_t* pair_v, uint32_t B, uint32_t K,
                         const uint32_t* inc_offset, const uint32_t* inc_slot,
                         const uint32_t* v_size, uint32_t v_cap, float* score, float* loss,
                         float* dH, uint64_t lddh, float* mrr) {
  NTS_RET(lp_check_score_args(ctx, H, ldh, D, pair_u, pair_v, B, K, score, loss));
  NTS_CHECK_ARG(inc_offset && inc_slot && v_size && dH, "NULL pointer");
  NTS_CHECK_ARG(lddh >= D, "lddh < D");
  NTS_CHECK_ARG(v_cap >= 1, "v_cap == 0");
  float* g = nullptr;
  NTS_RET(lp_score(ctx, H, ldh, D, pair_u, pair_v, B, K, score, loss, mrr, true, &g));
  const bool vec = D % 4 == 0 && ldh % 4 == 0 && lddh % 4 == 0 && lp_aligned16(H) && lp_aligned16(dH);
#define NTS_LP_BWD(G, VEC)                                                                        \
  hipLaunchKernelGGL((k_lp_bwd<G, VEC>), dim3(ceil_div(v_cap, kLpThreads / G)), dim3(kLpThreads), 0, \
                     ctx->stream, H, ldh, D, pair_u, pair_v, inc_offset, inc_slot, v_size, v_cap,   \
                     (const float*)g, dH, lddh)
  if (vec) {
    if (D <= 64) NTS_LP_BWD(16, true);
    else NTS_LP_BWD(64, true);
  } else {
    if (D <= 16) NTS_LP_BWD(16, false);
    else NTS_LP_BWD(64, false);
  }
#undef NTS_LP_BWD
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

}  // extern "C"
