// Full-neighbour aggregation over the replicated global CSC (layer-wise
// inference over the whole graph): Y[d,:] = sum over ALL in-edges of d of
// w(e) X[src(e),:], 64-bit offsets, global ids on both sides, weights
// recomputed from the degrees (no E-sized weight array).
//
// The arithmetic is nts_hip_spmm_csc_fwd's (aggregate.hip): per output element
// a serial sum in CSC edge order, acc + x*w with contraction off, from 0 — so
// the result is bit-identical to the reference's serial loop (nts_comp,
// core/ntsBaseOp.hpp:546-562) run over the whole graph, at any degree.  The
// reference itself has no full-graph inference pass for its sampled trainers.
//
// Scheduling.  A work item is (row, column slice): one lane group of LPD
// lanes, one VEC-float vector per lane, walks the row's edges in order for its
// LPD*VEC columns.  Per LPD edges the group loads the ids one per lane (and
// each lane its edge's weight from the two per-vertex sqrt tables), then
// fetches the neighbour rows U at a time, ids broadcast by __shfl.
//   * rows of up to kHubEdges edges: LPD as wide as the row (8..64 lanes, so
//     short narrow rows are packed several per wave), one item per 64-vector
//     slice;
//   * hub rows (more than kHubEdges edges; a power-law graph's reach tens of
//     thousands): never split by edge range — split by column slice into
//     kHubLpd-lane items, each walking every edge of the hub in order for its
//     columns.  A cheap per-call pass lists them (flag, scan, scatter: V
//     ints) and their kernel is issued first.
// No atomics, no grid barrier, no spin waits: it may run beside another stream.
//
// The GAT layer over the whole graph (nts_hip_gat_scores, nts_hip_gat_graph_fwd,
// below) runs on the same items with an online softmax per lane.
#include "graph_hubs.hpp"

#pragma clang fp contract(off)

namespace nts_hip {

// (kInfThreads, kInfU, kHubEdges, kHubLpd, kHubGrid: graph_hubs.hpp)

template <int VEC>
struct IV;
template <>
struct IV<1> {
  using T = float;
};
template <>
struct IV<2> {
  using T = float2;
};
template <>
struct IV<4> {
  using T = float4;
};

struct GraphAgg {
  static constexpr bool kCoef = false;
  const uint64_t* co;      // [V+1] global CSC offsets
  const uint32_t* ri;      // [E] global src ids
  const float* so;         // [V] degree_sqrt(out_degree)   (weight_type != NONE)
  const float* si;         // [V] degree_sqrt(in_degree)
  const uint32_t* in_deg;  // [V] (MEAN)
  int weight_type;
  int relu;
  const float* x;
  uint64_t ldx;
  float* y;
  uint64_t ldy;
  uint32_t nv;             // VEC-float vectors per row (the last may be partial)
  uint32_t last_valid;     // floats of the last vector
  uint64_t v_begin, n;     // rows [v_begin, v_begin + n)
  const uint32_t* hubs;    // HUB: the hub rows, ascending; hubs_n[0] of them
  const uint32_t* hubs_n;
};

// nts_hip_spmm_graph_fwd_coef: edge e uses fl32(w(e) * ec[e]), ec
// one fp32 per edge in CSC order, streamed beside the edge's source id.  A
// struct of its own, so the kernels above keep their kernarg layout and code.
struct GraphAggCoef : GraphAgg {
  static constexpr bool kCoef = true;
  const float* ec;         // [E] per-edge coefficient
};

__global__ void k_degree_sqrt(uint64_t n, const uint32_t* __restrict__ out_deg,
                              const uint32_t* __restrict__ in_deg, float* __restrict__ so,
                              float* __restrict__ si) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    so[i] = degree_sqrt(out_deg[i]);
    si[i] = degree_sqrt(in_deg[i]);
  }
}

// flag[i] = 1 where row v_begin + i is a hub
__global__ void k_hub_flag(const uint64_t* __restrict__ co, uint64_t v_begin, uint64_t n,
                           uint32_t* __restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x)
    flag[i] = (co[v_begin + i + 1] - co[v_begin + i] > (uint64_t)kHubEdges) ? 1u : 0u;
}
// pos = exclusive scan of the flags ([n+1], pos[n] = the hub count)
__global__ void k_hub_scatter(const uint32_t* __restrict__ pos, uint64_t v_begin, uint64_t n,
                              uint32_t* __restrict__ hubs) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x)
    if (pos[i + 1] != pos[i]) hubs[pos[i]] = (uint32_t)(v_begin + i);
}

// one (row d, column slice) item on the calling LPD-lane group: vector column
// `col` of the row (col >= nv: an idle lane, it still takes part in the shuffles)
template <int VEC, int LPD, typename A>
__device__ __forceinline__ void graph_row_slice(const A& a, uint64_t d, uint32_t col, int sl) {
  using T = typename IV<VEC>::T;
  const uint64_t beg = a.co[d], end = a.co[d + 1];
  const bool weighted = a.weight_type != NTS_WEIGHT_NONE;
  const float sid = weighted ? a.si[d] : 1.0f;
  const uint32_t ind = a.weight_type == NTS_WEIGHT_MEAN ? a.in_deg[d] : 1u;
  const bool live = col < a.nv;
  float acc[VEC];
#pragma unroll
  for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
  for (uint64_t cb = beg; cb < end; cb += LPD) {
    const uint32_t ne = (uint32_t)min(end - cb, (uint64_t)LPD);
    uint32_t my_r = 0;
    float my_w = 0.f;
    if ((uint32_t)sl < ne) {  // the edge list is streamed once
      my_r = __builtin_nontemporal_load(a.ri + cb + sl);
      my_w = 1.0f;
      if (weighted) {
        my_w = norm_from_sqrt(a.so[my_r], sid);
        if (a.weight_type == NTS_WEIGHT_MEAN) my_w = mean_weight(my_w, ind);
      }
      if constexpr (A::kCoef) my_w = my_w * __builtin_nontemporal_load(a.ec + cb + sl);
    }
    for (uint32_t j0 = 0; j0 < ne; j0 += kInfU) {
      T xv[kInfU];
      float ww[kInfU];
#pragma unroll
      for (int j = 0; j < kInfU; ++j) {
        const int src = (int)(j0 + j) & (LPD - 1);
        const uint32_t r = (uint32_t)__shfl((int)my_r, src, LPD);
        ww[j] = __shfl(my_w, src, LPD);
        T v;
#pragma unroll
        for (int q = 0; q < VEC; ++q) reinterpret_cast<float*>(&v)[q] = 0.f;
        if (live && j0 + j < ne) v = reinterpret_cast<const T*>(a.x + (uint64_t)r * a.ldx)[col];
        xv[j] = v;
      }
#pragma unroll
      for (int j = 0; j < kInfU; ++j)
        if (j0 + j < ne) {
#pragma unroll
          for (int q = 0; q < VEC; ++q)
            acc[q] = acc[q] + reinterpret_cast<const float*>(&xv[j])[q] * ww[j];
        }
    }
  }
  if (!live) return;
  if (a.relu) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = acc[q] > 0.f ? acc[q] : 0.f;
  }
  float* yp = a.y + d * a.ldy + (uint64_t)col * VEC;
  if (col + 1 < a.nv || a.last_valid == (uint32_t)VEC) {
    T v;
#pragma unroll
    for (int q = 0; q < VEC; ++q) reinterpret_cast<float*>(&v)[q] = acc[q];
    *reinterpret_cast<T*>(yp) = v;
  } else {  // partial last vector: only the valid floats
#pragma unroll
    for (int q = 0; q < VEC; ++q)
      if ((uint32_t)q < a.last_valid) yp[q] = acc[q];
  }
}

// HUB = false: items (i, s) = row v_begin + i, slice s of LPD vectors, item id
// i * nsl + s; hub rows are skipped.  HUB = true: items (h, s) over the hub list.
// Neighbouring groups take neighbouring slices of one row: its edge ids are
// fetched from memory once and hit in cache for the other slices.
template <int VEC, int LPD, bool HUB, typename A>
__global__ __launch_bounds__(kInfThreads) void k_spmm_graph(A a) {
  constexpr int GPB = kInfThreads / LPD;
  const int grp = threadIdx.x / LPD, sl = threadIdx.x % LPD;
  const uint64_t nsl = (a.nv + LPD - 1) / LPD;
  const uint64_t rows = HUB ? (uint64_t)a.hubs_n[0] : a.n;
  const uint64_t items = rows * nsl;
  for (uint64_t it = (uint64_t)blockIdx.x * GPB + grp; it < items; it += (uint64_t)gridDim.x * GPB) {
    const uint64_t i = it / nsl;
    const uint32_t s = (uint32_t)(it - i * nsl);
    uint64_t d;
    if (HUB) {
      d = a.hubs[i];
    } else {
      d = a.v_begin + i;
      if (a.co[d + 1] - a.co[d] > (uint64_t)kHubEdges) continue;  // (uniform in the group)
    }
    graph_row_slice<VEC, LPD>(a, d, s * LPD + sl, sl);
  }
}

template <int VEC, int LPD, bool HUB, typename A>
static int launch_graph(hipStream_t st, uint32_t grid, const A& a) {
  hipLaunchKernelGGL((k_spmm_graph<VEC, LPD, HUB, A>), dim3(grid), dim3(kInfThreads), 0, st, a);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

template <int VEC, typename A>
static int launch_graph_vec(hipStream_t st, const A& a) {
  // hubs first: they are the longest items of the call
  NTS_RET((launch_graph<VEC, kHubLpd, true>(st, kHubGrid, a)));
  const int lpd = a.nv <= 8 ? 8 : a.nv <= 16 ? 16 : a.nv <= 32 ? 32 : 64;
  const uint64_t items = a.n * ((a.nv + lpd - 1) / lpd);
  const uint32_t gpb = kInfThreads / lpd;
  // one item per lane group up to 2^20 blocks, grid-stride beyond
  const uint32_t grid = (uint32_t)std::min<uint64_t>((items + gpb - 1) / gpb, 1u << 20);
  switch (lpd) {
    case 8: return launch_graph<VEC, 8, false>(st, grid, a);
    case 16: return launch_graph<VEC, 16, false>(st, grid, a);
    case 32: return launch_graph<VEC, 32, false>(st, grid, a);
    default: return launch_graph<VEC, 64, false>(st, grid, a);
  }
}

// (HubScratch: graph_hubs.hpp)
int list_hubs(nts_hip_ctx* ctx, const nts_graph_dev* graph, uint64_t v_begin, uint64_t n,
              HubScratch& h, size_t extra_words) {
  const uint64_t V = graph->n_vertices;
  hipStream_t st = ctx->stream;
  auto pad = [](uint64_t e) { return (e + 63) / 64 * 64; };
  const size_t words = 2 * pad(V) + pad(n + 1) + pad(n) + pad(scan_tmp_elems<uint32_t>(n)) + 64;
  NTS_RET(ensure_scratch(ctx, (words + extra_words) * 4));
  h.so = (float*)ctx->scratch;
  h.extra = h.so + words;
  h.si = h.so + pad(V);
  h.pos = (uint32_t*)(h.si + pad(V));
  h.hubs = h.pos + pad(n + 1);
  uint32_t* tmp = h.hubs + pad(n);
  const uint32_t g = std::min(ceil_div(n, 256), kMaxGrid);
  hipLaunchKernelGGL(k_hub_flag, dim3(g), dim3(256), 0, st, graph->column_offset, v_begin, n,
                     h.pos);
  NTS_LAUNCH_CHECK();
  NTS_RET(scan_exclusive<uint32_t>(h.pos, h.pos, nullptr, n, tmp, st));
  hipLaunchKernelGGL(k_hub_scatter, dim3(g), dim3(256), 0, st, (const uint32_t*)h.pos, v_begin, n,
                     h.hubs);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

int degree_sqrt_tables(nts_hip_ctx* ctx, const nts_graph_dev* graph, float* so, float* si) {
  const uint64_t V = graph->n_vertices;
  hipLaunchKernelGGL(k_degree_sqrt, dim3(std::min(ceil_div(V, 256), kMaxGrid)), dim3(256), 0,
                     ctx->stream, V, graph->out_degree, graph->in_degree, so, si);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

// ---- the max aggregator over the whole graph (nts_hip_spmm_graph_fwd_max) ----
// The items, the lane groups and the hub split are the sum's above; per column
// the running maximum starts from the first edge's value and is replaced on a
// strict > (nts_hip_spmm_csc_fwd_max's rule; a hub's column slices walk every
// edge in order too, so the scan is the serial one).
template <int VEC, int LPD>
__device__ __forceinline__ void graph_row_slice_max(const GraphAgg& a, uint64_t d, uint32_t col,
                                                    int sl) {
  using T = typename IV<VEC>::T;
  const uint64_t beg = a.co[d], end = a.co[d + 1];
  const bool live = col < a.nv;
  float m[VEC];
#pragma unroll
  for (int q = 0; q < VEC; ++q) m[q] = 0.f;
  for (uint64_t cb = beg; cb < end; cb += LPD) {
    const uint32_t ne = (uint32_t)min(end - cb, (uint64_t)LPD);
    uint32_t my_r = 0;
    if ((uint32_t)sl < ne) my_r = __builtin_nontemporal_load(a.ri + cb + sl);
    for (uint32_t j0 = 0; j0 < ne; j0 += kInfU) {
      T xv[kInfU];
#pragma unroll
      for (int j = 0; j < kInfU; ++j) {
        const uint32_t r = (uint32_t)__shfl((int)my_r, (int)(j0 + j) & (LPD - 1), LPD);
        T v;
#pragma unroll
        for (int q = 0; q < VEC; ++q) reinterpret_cast<float*>(&v)[q] = 0.f;
        if (live && j0 + j < ne) v = reinterpret_cast<const T*>(a.x + (uint64_t)r * a.ldx)[col];
        xv[j] = v;
      }
#pragma unroll
      for (int j = 0; j < kInfU; ++j)
        if (j0 + j < ne) {
          const bool first = cb + j0 + j == beg;
#pragma unroll
          for (int q = 0; q < VEC; ++q) {
            const float v = reinterpret_cast<const float*>(&xv[j])[q];
            if (first || v > m[q]) m[q] = v;
          }
        }
    }
  }
  if (!live) return;
  if (a.relu) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) m[q] = m[q] > 0.f ? m[q] : 0.f;
  }
  float* yp = a.y + d * a.ldy + (uint64_t)col * VEC;
  if (col + 1 < a.nv || a.last_valid == (uint32_t)VEC) {
    T v;
#pragma unroll
    for (int q = 0; q < VEC; ++q) reinterpret_cast<float*>(&v)[q] = m[q];
    *reinterpret_cast<T*>(yp) = v;
  } else {  // partial last vector: only the valid floats
#pragma unroll
    for (int q = 0; q < VEC; ++q)
      if ((uint32_t)q < a.last_valid) yp[q] = m[q];
  }
}

template <int VEC, int LPD, bool HUB>
__global__ __launch_bounds__(kInfThreads) void k_spmm_graph_max(GraphAgg a) {
  constexpr int GPB = kInfThreads / LPD;
  const int grp = threadIdx.x / LPD, sl = threadIdx.x % LPD;
  const uint64_t nsl = (a.nv + LPD - 1) / LPD;
  const uint64_t rows = HUB ? (uint64_t)a.hubs_n[0] : a.n;
  const uint64_t items = rows * nsl;
  for (uint64_t it = (uint64_t)blockIdx.x * GPB + grp; it < items; it += (uint64_t)gridDim.x * GPB) {
    const uint64_t i = it / nsl;
    const uint32_t s = (uint32_t)(it - i * nsl);
    uint64_t d;
    if (HUB) {
      d = a.hubs[i];
    } else {
      d = a.v_begin + i;
      if (a.co[d + 1] - a.co[d] > (uint64_t)kHubEdges) continue;  // (uniform in the group)
    }
    graph_row_slice_max<VEC, LPD>(a, d, s * LPD + sl, sl);
  }
}

template <int VEC>
static int launch_graph_max_vec(hipStream_t st, const GraphAgg& a) {
  hipLaunchKernelGGL((k_spmm_graph_max<VEC, kHubLpd, true>), dim3(kHubGrid), dim3(kInfThreads), 0,
                     st, a);
  NTS_LAUNCH_CHECK();
  const int lpd = a.nv <= 8 ? 8 : a.nv <= 16 ? 16 : a.nv <= 32 ? 32 : 64;
  const uint64_t items = a.n * ((a.nv + lpd - 1) / lpd);
  const uint32_t gpb = kInfThreads / lpd;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((items + gpb - 1) / gpb, 1u << 20);
  switch (lpd) {
    case 8: hipLaunchKernelGGL((k_spmm_graph_max<VEC, 8, false>), dim3(grid), dim3(kInfThreads), 0, st, a); break;
    case 16: hipLaunchKernelGGL((k_spmm_graph_max<VEC, 16, false>), dim3(grid), dim3(kInfThreads), 0, st, a); break;
    case 32: hipLaunchKernelGGL((k_spmm_graph_max<VEC, 32, false>), dim3(grid), dim3(kInfThreads), 0, st, a); break;
    default: hipLaunchKernelGGL((k_spmm_graph_max<VEC, 64, false>), dim3(grid), dim3(kInfThreads), 0, st, a); break;
  }
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

// vector width of a full-graph call: float4 where the rows are 16-byte aligned
// — F a multiple of 4, or pitches that pad the row to one (the partial last
// vector then reads pitch padding and stores only its valid floats); else
// float2 or scalar columns
static int graph_vec(uint32_t F, const float* x, uint64_t ldx, const float* y, uint64_t ldy) {
  const uint32_t F4 = (F + 3) / 4 * 4;
  auto al = [](const void* p, uintptr_t b) { return ((uintptr_t)p % b) == 0; };
  if (F4 <= ldx && F4 <= ldy && ldx % 4 == 0 && ldy % 4 == 0 && al(x, 16) && al(y, 16)) return 4;
  if (F % 2 == 0 && ldx % 2 == 0 && ldy % 2 == 0 && al(x, 8) && al(y, 8)) return 2;
  return 1;
}

// ---- GAT over the whole graph (nts_hip_gat_scores, nts_hip_gat_graph_fwd) ----
// K heads of D columns, F = K D, gat.hip's layout: head h owns columns
// [hD, (h+1)D) of H, a1 = att[0:F] and a2 = att[F:2F].  Over the whole graph
// every vertex is a source many times, so the two dot products of a row are
// taken once per vertex (S [rows, 2K]: H[v]_h . a1_h, then H[v]_h . a2_h) and an
// edge's score is leaky_relu(S[src, h] + S[d, K + h]): two scalar reads, no
// per-edge reduction, and no E-sized array (the sampled kernels' m and a are
// for their backward).
//
// Scores: one G-lane group per (row, head), G the power of two that covers
// the head's D / VEC vectors (at most 64).  Lane s adds the products of vectors
// s, s + G, ... in that order, then an xor butterfly over the group: one fixed
// summation order.
struct GatScores {
  const float* h;
  uint64_t ldh;
  uint64_t rows;
  uint32_t heads, g;  // g = D / VEC vectors per head
  const float* att;
  float* s;
};

template <int VEC>
__global__ __launch_bounds__(kInfThreads) void k_gat_scores(GatScores a, uint32_t G) {
  using T = typename IV<VEC>::T;
  const uint32_t gpb = kInfThreads / G;
  const uint32_t grp = threadIdx.x / G, sl = threadIdx.x % G;
  const uint64_t items = a.rows * a.heads;
  const uint64_t F = (uint64_t)a.heads * a.g * VEC;
  // every group of a block takes the same number of trips: the shuffles below
  // always have their whole group
  for (uint64_t base = (uint64_t)blockIdx.x * gpb; base < items; base += (uint64_t)gridDim.x * gpb) {
    const uint64_t it = base + grp;
    const bool live = it < items;
    const uint64_t v = live ? it / a.heads : 0;
    const uint32_t h = live ? (uint32_t)(it - v * a.heads) : 0;
    float p1 = 0.f, p2 = 0.f;
    if (live) {
      const T* hr = reinterpret_cast<const T*>(a.h + v * a.ldh) + (uint64_t)h * a.g;
      const T* a1 = reinterpret_cast<const T*>(a.att) + (uint64_t)h * a.g;
      const T* a2 = reinterpret_cast<const T*>(a.att + F) + (uint64_t)h * a.g;
      for (uint32_t c = sl; c < a.g; c += G) {
        const T x = hr[c], w1 = a1[c], w2 = a2[c];
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const float xq = reinterpret_cast<const float*>(&x)[q];
          p1 = p1 + xq * reinterpret_cast<const float*>(&w1)[q];
          p2 = p2 + xq * reinterpret_cast<const float*>(&w2)[q];
        }
      }
    }
    for (uint32_t o = G >> 1; o >= 1; o >>= 1) {
      p1 = p1 + __shfl_xor(p1, (int)o, 64);
      p2 = p2 + __shfl_xor(p2, (int)o, 64);
    }
    if (live && sl == 0) {
      float* sp = a.s + v * 2 * a.heads;
      sp[h] = p1;
      sp[a.heads + h] = p2;
    }
  }
}

struct GatAgg {
  const uint64_t* co;   // [V+1] global CSC offsets
  const uint32_t* ri;   // [E] global src ids
  const float* s;       // [V, 2K] the scores
  const float* h;       // [V, F]
  uint64_t ldh;
  float* y;             // concat: Y; mean: the [n, F] scratch Z, row 0 = v_begin
  uint64_t ldy;
  int relu;             // concat: relu in the store; mean: left to the epilogue
  uint32_t heads, g;    // g = D / VEC vectors per head
  uint32_t nv;          // VEC-float vectors per row (D % VEC == 0: all whole)
  uint64_t v_begin, n;  // rows [v_begin, v_begin + n)
  uint64_t y_row0;      // the row of y that holds vertex v_begin
  const uint32_t* hubs;
  const uint32_t* hubs_n;
};

__device__ __forceinline__ float gat_leaky(float u) { return u > 0.f ? u : 0.2f * u; }

// one (row d, column slice) item on the calling LPD-lane group.  The lane owns
// vector column `col` of head hc = col / g and keeps that head's online
// softmax (running max M, running sum S, accumulator rescaled when the max
// grows): gat.hip's recurrence, edge by edge in CSC order.  Of its two
// exponentials exp(M - max(M, m)) and exp(m - max(M, m)) one is exp(0) = 1, so
// one expf of -|m - M| gives both.  Every lane of a head sees the same scalars,
// so an output element's arithmetic does not depend on LPD or the slice.
template <int VEC, int LPD>
__device__ __forceinline__ void gat_row_slice(const GatAgg& a, uint64_t d, uint32_t col, int sl) {
  using T = typename IV<VEC>::T;
  const uint64_t beg = a.co[d], end = a.co[d + 1];
  const bool live = col < a.nv;
  const uint32_t hc = live ? col / a.g : 0u;
  const uint32_t K2 = 2 * a.heads;
  const float s2 = a.s[d * K2 + a.heads + hc];
  float acc[VEC];
#pragma unroll
  for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
  float M = -INFINITY, S = 0.f;
  for (uint64_t cb = beg; cb < end; cb += LPD) {
    const uint32_t ne = (uint32_t)min(end - cb, (uint64_t)LPD);
    uint32_t my_r = 0;
    if ((uint32_t)sl < ne) my_r = __builtin_nontemporal_load(a.ri + cb + sl);
    for (uint32_t j0 = 0; j0 < ne; j0 += kInfU) {
      T xv[kInfU];
      float s1[kInfU];
#pragma unroll
      for (int j = 0; j < kInfU; ++j) {
        const uint32_t r = (uint32_t)__shfl((int)my_r, (int)(j0 + j) & (LPD - 1), LPD);
        T v;
#pragma unroll
        for (int q = 0; q < VEC; ++q) reinterpret_cast<float*>(&v)[q] = 0.f;
        float sc = 0.f;
        if (live && j0 + j < ne) {
          v = reinterpret_cast<const T*>(a.h + (uint64_t)r * a.ldh)[col];
          sc = a.s[(uint64_t)r * K2 + hc];
        }
        xv[j] = v;
        s1[j] = sc;
      }
#pragma unroll
      for (int j = 0; j < kInfU; ++j)
        if (j0 + j < ne) {
          const float m = gat_leaky(s1[j] + s2);
          const bool up = m > M;  // (the first edge: M = -inf)
          const float e = expf(-fabsf(m - M));
          const float sc = up ? e : 1.0f, p = up ? 1.0f : e;
          S = S * sc + p;
#pragma unroll
          for (int q = 0; q < VEC; ++q)
            acc[q] = acc[q] * sc + p * reinterpret_cast<const float*>(&xv[j])[q];
          M = up ? m : M;
        }
    }
  }
  if (!live) return;
  const float inv = S > 0.f ? 1.f / S : 0.f;  // an empty column: a zero row
  T v;
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    const float z = acc[q] * inv;
    reinterpret_cast<float*>(&v)[q] = (a.relu && !(z > 0.f)) ? 0.f : z;
  }
  reinterpret_cast<T*>(a.y + (d - a.v_begin + a.y_row0) * a.ldy)[col] = v;
}

template <int VEC, int LPD, bool HUB>
__global__ __launch_bounds__(kInfThreads) void k_gat_graph(GatAgg a) {
  constexpr int GPB = kInfThreads / LPD;
  const int grp = threadIdx.x / LPD, sl = threadIdx.x % LPD;
  const uint64_t nsl = (a.nv + LPD - 1) / LPD;
  const uint64_t rows = HUB ? (uint64_t)a.hubs_n[0] : a.n;
  const uint64_t items = rows * nsl;
  for (uint64_t it = (uint64_t)blockIdx.x * GPB + grp; it < items; it += (uint64_t)gridDim.x * GPB) {
    const uint64_t i = it / nsl;
    const uint32_t s = (uint32_t)(it - i * nsl);
    uint64_t d;
    if (HUB) {
      d = a.hubs[i];
    } else {
      d = a.v_begin + i;
      if (a.co[d + 1] - a.co[d] > (uint64_t)kHubEdges) continue;  // (uniform in the group)
    }
    gat_row_slice<VEC, LPD>(a, d, s * LPD + sl, sl);
  }
}

template <int VEC>
static int launch_gat_graph_vec(hipStream_t st, const GatAgg& a) {
  // hubs first: they are the longest items of the call
  hipLaunchKernelGGL((k_gat_graph<VEC, kHubLpd, true>), dim3(kHubGrid), dim3(kInfThreads), 0, st, a);
  NTS_LAUNCH_CHECK();
  const int lpd = a.nv <= 8 ? 8 : a.nv <= 16 ? 16 : a.nv <= 32 ? 32 : 64;
  const uint64_t items = a.n * ((a.nv + lpd - 1) / lpd);
  const uint32_t gpb = kInfThreads / lpd;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((items + gpb - 1) / gpb, 1u << 20);
  switch (lpd) {
    case 8: hipLaunchKernelGGL((k_gat_graph<VEC, 8, false>), dim3(grid), dim3(kInfThreads), 0, st, a); break;
    case 16: hipLaunchKernelGGL((k_gat_graph<VEC, 16, false>), dim3(grid), dim3(kInfThreads), 0, st, a); break;
    case 32: hipLaunchKernelGGL((k_gat_graph<VEC, 32, false>), dim3(grid), dim3(kInfThreads), 0, st, a); break;
    default: hipLaunchKernelGGL((k_gat_graph<VEC, 64, false>), dim3(grid), dim3(kInfThreads), 0, st, a); break;
  }
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

// mean mode's epilogue: Y[v_begin + i, j] = relu((Z[i, j] + Z[i, D + j] + ...) / K),
// heads added in order, then scaled (k_gat_fwd_heads' arithmetic)
__global__ void k_gat_mean_heads(const float* __restrict__ z, uint64_t n, uint32_t heads, uint32_t D,
                                 float* __restrict__ y, uint64_t ldy) {
  const uint64_t F = (uint64_t)heads * D, total = n * D;
  const float rk = 1.f / (float)heads;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = i / D;
    const uint32_t j = (uint32_t)(i - r * D);
    const float* zr = z + r * F + j;
    float t = zr[0];
    for (uint32_t h = 1; h < heads; ++h) t = t + zr[(uint64_t)h * D];
    t = t * rk;
    y[r * ldy + j] = t > 0.f ? t : 0.f;
  }
}

// vector width of a GAT call over the whole graph: graph_vec's rule, and D a
// multiple of the width, so that a vector never straddles two heads
static int gat_graph_vec(uint32_t D, uint32_t F, const float* x, uint64_t ldx, const float* y,
                         uint64_t ldy) {
  int vec = graph_vec(F, x, ldx, y, ldy);
  while (vec > 1 && D % (uint32_t)vec != 0) vec >>= 1;
  return vec;
}

}  // namespace nts_hip

using namespace nts_hip;

// nts_hip_spmm_graph_fwd and its _coef sibling: A = GraphAgg or GraphAggCoef
template <typename A>
static int spmm_graph_fwd(nts_hip_ctx* ctx, const nts_graph_dev* graph, const float* edge_coef,
                          uint64_t v_begin, uint64_t v_end, int weight_type, int relu,
                          const float* x, uint64_t ldx, uint32_t feature_size, float* y,
                          uint64_t ldy) {
  NTS_CHECK_ARG(graph != nullptr, "graph is NULL");
  NTS_CHECK_ARG(v_begin <= v_end, "v_begin > v_end");
  NTS_CHECK_ARG(ctx && x && y, "NULL argument");
  NTS_CHECK_ARG(v_end <= graph->n_vertices && graph->n_vertices <= 0xFFFFFFFFull,
                "vertex range outside the graph");
  NTS_CHECK_ARG(graph->column_offset && (graph->n_edges == 0 || graph->row_indices),
                "graph without its CSC");
  NTS_CHECK_ARG(weight_type == NTS_WEIGHT_SUM || weight_type == NTS_WEIGHT_MEAN ||
                    weight_type == NTS_WEIGHT_NONE,
                "weight type: SUM, MEAN or NONE (no MEAN_SAMPLED, no UP_DEGREE over the full graph)");
  NTS_CHECK_ARG(weight_type == NTS_WEIGHT_NONE || (graph->in_degree && graph->out_degree),
                "graph without its degrees");
  NTS_CHECK_ARG(ldx >= feature_size && ldy >= feature_size, "leading dimension < feature_size");
  const uint64_t n = v_end - v_begin;
  if (n == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  HubScratch h;
  NTS_RET(list_hubs(ctx, graph, v_begin, n, h));
  float *so = h.so, *si = h.si;
  uint32_t *pos = h.pos, *hubs = h.hubs;
  if (weight_type != NTS_WEIGHT_NONE) NTS_RET(degree_sqrt_tables(ctx, graph, so, si));

  A a;
  if constexpr (A::kCoef) a.ec = edge_coef;
  a.co = graph->column_offset;
  a.ri = graph->row_indices;
  a.so = so;
  a.si = si;
  a.in_deg = graph->in_degree;
  a.weight_type = weight_type;
  a.relu = relu ? 1 : 0;
  a.x = x;
  a.ldx = ldx;
  a.y = y;
  a.ldy = ldy;
  a.v_begin = v_begin;
  a.n = n;
  a.hubs = hubs;
  a.hubs_n = pos + n;
  const uint32_t F = feature_size;
  const int vec = graph_vec(F, x, ldx, y, ldy);
  a.nv = (F + vec - 1) / vec;
  a.last_valid = F - (a.nv - 1) * vec;
  if (vec == 4) return launch_graph_vec<4>(st, a);
  if (vec == 2) return launch_graph_vec<2>(st, a);
  return launch_graph_vec<1>(st, a);
}

extern "C" {

int nts_hip_spmm_graph_fwd(nts_hip_ctx* ctx, const nts_graph_dev* graph, uint64_t v_begin,
                           uint64_t v_end, int weight_type, int relu, const float* x, uint64_t ldx,
                           uint32_t feature_size, float* y, uint64_t ldy) {
  return spmm_graph_fwd<GraphAgg>(ctx, graph, nullptr, v_begin, v_end, weight_type, relu, x, ldx,
                                  feature_size, y, ldy);
}

int nts_hip_spmm_graph_fwd_coef(nts_hip_ctx* ctx, const nts_graph_dev* graph,
                                const float* edge_coef, uint64_t v_begin, uint64_t v_end,
                                int weight_type, int relu, const float* x, uint64_t ldx,
                                uint32_t feature_size, float* y, uint64_t ldy) {
  NTS_CHECK_ARG(graph != nullptr, "graph is NULL");
  NTS_CHECK_ARG(edge_coef || graph->n_edges == 0, "edge_coef is NULL");
  return spmm_graph_fwd<GraphAggCoef>(ctx, graph, edge_coef, v_begin, v_end, weight_type, relu, x,
                                      ldx, feature_size, y, ldy);
}

int nts_hip_spmm_graph_fwd_max(nts_hip_ctx* ctx, const nts_graph_dev* graph, uint64_t v_begin,
                               uint64_t v_end, int relu, const float* x, uint64_t ldx,
                               uint32_t feature_size, float* y, uint64_t ldy) {
  NTS_CHECK_ARG(graph != nullptr, "graph is NULL");
  NTS_CHECK_ARG(v_begin <= v_end, "v_begin > v_end");
  NTS_CHECK_ARG(ctx && x && y, "NULL argument");
  NTS_CHECK_ARG(v_end <= graph->n_vertices && graph->n_vertices <= 0xFFFFFFFFull,
                "vertex range outside the graph");
  NTS_CHECK_ARG(graph->column_offset && (graph->n_edges == 0 || graph->row_indices),
                "graph without its CSC");
  NTS_CHECK_ARG(ldx >= feature_size && ldy >= feature_size, "leading dimension < feature_size");
  const uint64_t n = v_end - v_begin;
  if (n == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  HubScratch h;
  NTS_RET(list_hubs(ctx, graph, v_begin, n, h));
  GraphAgg a{};
  a.co = graph->column_offset;
  a.ri = graph->row_indices;
  a.weight_type = NTS_WEIGHT_NONE;
  a.relu = relu ? 1 : 0;
  a.x = x;
  a.ldx = ldx;
  a.y = y;
  a.ldy = ldy;
  a.v_begin = v_begin;
  a.n = n;
  a.hubs = h.hubs;
  a.hubs_n = h.pos + n;
  const int vec = graph_vec(feature_size, x, ldx, y, ldy);
  a.nv = (feature_size + vec - 1) / vec;
  a.last_valid = feature_size - (a.nv - 1) * vec;
  if (vec == 4) return launch_graph_max_vec<4>(ctx->stream, a);
  if (vec == 2) return launch_graph_max_vec<2>(ctx->stream, a);
  return launch_graph_max_vec<1>(ctx->stream, a);
}

int nts_hip_gat_scores(nts_hip_ctx* ctx, const float* H, uint64_t ldh, uint64_t rows,
                       uint32_t heads, uint32_t D, const float* att, float* S) {
  NTS_CHECK_ARG(heads >= 1 && D >= 1, "heads must be >= 1 and D >= 1");
  NTS_CHECK_ARG((uint64_t)heads * D <= 0x7FFFFFFFull, "heads * D too large");
  NTS_CHECK_ARG(ctx && H && att && S, "NULL argument");
  const uint32_t F = heads * D;
  NTS_CHECK_ARG(ldh >= F, "leading dimension < heads * D");
  if (rows == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  auto al = [](const void* p) { return ((uintptr_t)p % 16) == 0; };
  const bool v4 = D % 4 == 0 && ldh % 4 == 0 && al(H) && al(att);
  GatScores a;
  a.h = H;
  a.ldh = ldh;
  a.rows = rows;
  a.heads = heads;
  a.g = v4 ? D / 4 : D;
  a.att = att;
  a.s = S;
  uint32_t G = 1;
  while (G < 64 && G < a.g) G <<= 1;
  const uint64_t gpb = kInfThreads / G;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((rows * heads + gpb - 1) / gpb, 1u << 20);
  if (v4)
    hipLaunchKernelGGL(k_gat_scores<4>, dim3(grid), dim3(kInfThreads), 0, ctx->stream, a, G);
  else
    hipLaunchKernelGGL(k_gat_scores<1>, dim3(grid), dim3(kInfThreads), 0, ctx->stream, a, G);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

int nts_hip_gat_graph_fwd(nts_hip_ctx* ctx, const nts_graph_dev* graph, uint64_t v_begin,
                          uint64_t v_end, const float* H, uint64_t ldh, uint32_t heads, uint32_t D,
                          const float* S, float* Y, uint64_t ldy, int mean) {
  NTS_CHECK_ARG(graph != nullptr, "graph is NULL");
  NTS_CHECK_ARG(v_begin <= v_end, "v_begin > v_end");
  NTS_CHECK_ARG(heads >= 1 && D >= 1, "heads must be >= 1 and D >= 1");
  NTS_CHECK_ARG((uint64_t)heads * D <= 0x7FFFFFFFull, "heads * D too large");
  NTS_CHECK_ARG(v_end <= graph->n_vertices && graph->n_vertices <= 0xFFFFFFFFull,
                "vertex range outside the graph");
  NTS_CHECK_ARG(ctx && H && S && Y, "NULL argument");
  NTS_CHECK_ARG(graph->column_offset && (graph->n_edges == 0 || graph->row_indices),
                "graph without its CSC");
  if (heads == 1) mean = 0;  // one head: both modes are the single-head layer
  const uint32_t F = heads * D, FY = mean ? D : F;
  NTS_CHECK_ARG(ldh >= F && ldy >= FY, "leading dimension");
  const uint64_t n = v_end - v_begin;
  if (n == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  HubScratch h;
  // mean mode: the heads' normalised rows Z [n, F], summed by the epilogue
  NTS_RET(list_hubs(ctx, graph, v_begin, n, h, mean ? (size_t)n * F : 0));
  GatAgg a;
  a.co = graph->column_offset;
  a.ri = graph->row_indices;
  a.s = S;
  a.h = H;
  a.ldh = ldh;
  a.y = mean ? h.extra : Y;
  a.ldy = mean ? (uint64_t)F : ldy;
  a.relu = mean ? 0 : 1;
  a.heads = heads;
  a.v_begin = v_begin;
  a.n = n;
  a.y_row0 = mean ? 0 : v_begin;
  a.hubs = h.hubs;
  a.hubs_n = h.pos + n;
  const int vec = gat_graph_vec(D, F, H, ldh, a.y, a.ldy);
  a.g = D / vec;
  a.nv = F / vec;
  if (vec == 4)
    NTS_RET(launch_gat_graph_vec<4>(st, a));
  else if (vec == 2)
    NTS_RET(launch_gat_graph_vec<2>(st, a));
  else
    NTS_RET(launch_gat_graph_vec<1>(st, a));
  if (mean) {
    const uint32_t grid = std::min(ceil_div(n * D, 256), kMaxGrid);
    hipLaunchKernelGGL(k_gat_mean_heads, dim3(grid), dim3(256), 0, st, (const float*)h.extra, n,
                       heads, D, Y + v_begin * ldy, ldy);
    NTS_LAUNCH_CHECK();
  }
  return NTS_OK;
}

}  // extern "C"
