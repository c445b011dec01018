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
#include "common.hpp"

#pragma clang fp contract(off)

namespace nts_hip {

constexpr int kInfThreads = 256;
constexpr int kInfU = 8;             // neighbour rows in flight per lane group
constexpr uint32_t kHubEdges = 2048; // rows longer than this are column-sliced
constexpr int kHubLpd = 16;          // lanes per hub item
constexpr uint32_t kHubGrid = 1024;  // hub kernel: grid-stride over the hub items

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
template <int VEC, int LPD>
__device__ __forceinline__ void graph_row_slice(const GraphAgg& a, uint64_t d, uint32_t col, int sl) {
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
template <int VEC, int LPD, bool HUB>
__global__ __launch_bounds__(kInfThreads) void k_spmm_graph(GraphAgg a) {
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

template <int VEC, int LPD, bool HUB>
static int launch_graph(hipStream_t st, uint32_t grid, const GraphAgg& a) {
  hipLaunchKernelGGL((k_spmm_graph<VEC, LPD, HUB>), dim3(grid), dim3(kInfThreads), 0, st, a);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

template <int VEC>
static int launch_graph_vec(hipStream_t st, const GraphAgg& a) {
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

// The call's scratch (the two sqrt tables [V], the hub flags / their scan
// [n + 1], the hub list [n], the scan's temporaries) and the hub list of rows
// [v_begin, v_begin + n): flag, scan, scatter on the context's stream.
struct HubScratch {
  float *so, *si;
  uint32_t *pos, *hubs;  // pos[n] = the hub count
};
static int list_hubs(nts_hip_ctx* ctx, const nts_graph_dev* graph, uint64_t v_begin, uint64_t n,
                     HubScratch& h) {
  const uint64_t V = graph->n_vertices;
  hipStream_t st = ctx->stream;
  auto pad = [](uint64_t e) { return (e + 63) / 64 * 64; };
  const size_t words = 2 * pad(V) + pad(n + 1) + pad(n) + scan_tmp_elems<uint32_t>(n) + 64;
  NTS_RET(ensure_scratch(ctx, words * 4));
  h.so = (float*)ctx->scratch;
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

}  // namespace nts_hip

using namespace nts_hip;

extern "C" {

int nts_hip_spmm_graph_fwd(nts_hip_ctx* ctx, const nts_graph_dev* graph, uint64_t v_begin,
                           uint64_t v_end, int weight_type, int relu, const float* x, uint64_t ldx,
                           uint32_t feature_size, float* y, uint64_t ldy) {
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
  const uint64_t n = v_end - v_begin, V = graph->n_vertices;
  if (n == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  HubScratch h;
  NTS_RET(list_hubs(ctx, graph, v_begin, n, h));
  float *so = h.so, *si = h.si;
  uint32_t *pos = h.pos, *hubs = h.hubs;
  if (weight_type != NTS_WEIGHT_NONE) {
    hipLaunchKernelGGL(k_degree_sqrt, dim3(std::min(ceil_div(V, 256), kMaxGrid)), dim3(256), 0, st,
                       V, graph->out_degree, graph->in_degree, so, si);
    NTS_LAUNCH_CHECK();
  }

  GraphAgg a;
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

}  // extern "C"
