// The gathers over an IEEE-half feature table (GCNConfig::feature_f16): the
// sampled CSC aggregation, the full-neighbour aggregation over the global CSC
// and the row gather, each reading f16 rows and writing fp32 rows.
//
// Storage is f16, arithmetic is fp32.  A half widens to fp32 exactly (the
// hardware convert, subnormals included), and the sum is the fp32 kernels':
// per output element serial in CSC edge order, acc + x*w from 0, contraction
// off.  Neither the lane-group shape nor the vector width enters an element's
// arithmetic, so every call here gives the bytes its fp32 sibling
// (nts_hip_spmm_csc_fwd, nts_hip_spmm_graph_fwd, nts_hip_gather_rows) gives on
// the widened table.
//
// Layout and schedule are k_spmm_gather's (aggregate.hip) and k_spmm_graph's
// (infer.hip): one LPD-lane group per destination row (per row and column
// slice over the whole graph), a lane NCH vectors of HV halves of it — 16
// bytes where the table's base and pitch allow, else 8, 4 or 2 —, the group's
// edge ids loaded one per lane and the neighbour rows fetched U at a time.
// The partial last vector of a row reads pitch padding (the fp32 `pad` rule)
// and stores only its valid floats.  No LDS, no atomics, no grid barrier.
#include "agg_shape.hpp"
#include "graph_hubs.hpp"

#pragma clang fp contract(off)

namespace nts_hip {

template <int HV>
struct HT {
  typedef _Float16 T __attribute__((ext_vector_type(HV)));
};
template <>
struct HT<1> {
  using T = _Float16;
};
template <int HV>
__device__ __forceinline__ float hwiden(const typename HT<HV>::T& v, int q) {
  if constexpr (HV == 1) return (float)v;
  else return (float)v[q];
}
template <int HV>
__device__ __forceinline__ typename HT<HV>::T hzero() {
  typename HT<HV>::T v;
  if constexpr (HV == 1) {
    v = (_Float16)0.f;
  } else {
#pragma unroll
    for (int q = 0; q < HV; ++q) v[q] = (_Float16)0.f;
  }
  return v;
}

// Rows kept in flight per lane group, by the dwords a lane loads of one row
// (HV NCH / 2).  A half row is half the bytes of the fp32 row of its width, but
// pick_shape halves the lane group with it (128 columns: 16 lanes against 32),
// so a wave covers twice the rows and keeps the fp32 kernel's bytes in flight
// at the fp32 count; only where the group is already 64 lanes wide (more than
// 512 columns) does the row's share per lane shrink, and the count goes up
// until the loads in flight reach the fp32 kernel's dwords per lane (5 x 12 at
// 602 columns -> 7 x 8 here).  gather_u's steps, taken in dwords:
constexpr int gather_u_h(int dwords_per_lane) {
  return dwords_per_lane <= 4 ? 8 : dwords_per_lane <= 8 ? 7 : dwords_per_lane <= 12 ? 5 : 4;
}
constexpr int kMaxNchH = 4;  // vectors a lane holds of a row; wider rows take more rounds

// nvalid floats of a[0..HV) to the fp32 row at p (column a multiple of HV), in
// pieces of yal floats (the row's alignment: 4, 2 or 1) where a piece is whole
template <int HV, bool NT>
__device__ __forceinline__ void store_widened(float* p, const float (&a)[HV], uint32_t nvalid,
                                              int yal) {
  auto st = [&](auto* q, auto v) {
    if constexpr (NT) __builtin_nontemporal_store(v, q);
    else *q = v;
  };
  if constexpr (HV >= 4) {
    if (yal == 4) {
      typedef float f4 __attribute__((ext_vector_type(4)));
#pragma unroll
      for (int q = 0; q < HV; q += 4) {
        if ((uint32_t)q + 4 <= nvalid) {
          f4 u = {a[q], a[q + 1], a[q + 2], a[q + 3]};
          st(reinterpret_cast<f4*>(p + q), u);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if ((uint32_t)(q + k) < nvalid) st(p + q + k, a[q + k]);
        }
      }
      return;
    }
  }
  if constexpr (HV >= 2) {
    if (yal >= 2) {
      typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int q = 0; q < HV; q += 2) {
        if ((uint32_t)q + 2 <= nvalid) {
          f2 u = {a[q], a[q + 1]};
          st(reinterpret_cast<f2*>(p + q), u);
        } else if ((uint32_t)q < nvalid) {
          st(p + q, a[q]);
        }
      }
      return;
    }
  }
#pragma unroll
  for (int q = 0; q < HV; ++q)
    if ((uint32_t)q < nvalid) st(p + q, a[q]);
}

// y[d, :] = sum_{e in [off[d], off[d+1])} w[e] * float(x[row(e), :])
// row(e) = MAP ? map[idx[e]] : idx[e];  w == nullptr -> weight 1.
// nv vectors of HV halves per row, F columns (the last vector may be partial)
template <int HV, int LPD, int NCH, bool MAP, int U>
__global__ __launch_bounds__(kAggThreads) void k_spmm_gather_h(
    const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx,
    const float* __restrict__ w, const uint32_t* n_dev, uint32_t n_cap,
    const uint16_t* __restrict__ x, uint64_t ldx, const uint32_t* __restrict__ map, uint32_t nv,
    uint32_t F, float* __restrict__ y, uint64_t ldy, int yal) {
  using T = typename HT<HV>::T;
  const uint32_t n = n_dev ? min(*n_dev, n_cap) : n_cap;
  constexpr int GPB = kAggThreads / LPD;
  const int grp = threadIdx.x / LPD, sl = threadIdx.x % LPD;
  for (uint32_t d = blockIdx.x * GPB + grp; d < n; d += gridDim.x * GPB) {
    const uint32_t beg = off[d], end = off[d + 1];
    for (uint32_t c0 = 0; c0 < nv; c0 += LPD * NCH) {
      float acc[NCH][HV];
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int q = 0; q < HV; ++q) acc[c][q] = 0.f;
      for (uint32_t cb = beg; cb < end; cb += LPD) {
        const uint32_t ne = min(end - cb, (uint32_t)LPD);
        uint32_t my_r = 0;
        float my_w = 0.f;
        if ((uint32_t)sl < ne) {  // streamed once: do not keep in cache
          my_r = __builtin_nontemporal_load(idx + cb + sl);
          my_w = w ? __builtin_nontemporal_load(w + cb + sl) : 1.0f;
          if (MAP) my_r = map[my_r];
        }
        for (uint32_t j0 = 0; j0 < ne; j0 += U) {
          T xv[U][NCH];
          float ww[U];
#pragma unroll
          for (int j = 0; j < U; ++j) {
            const int src = (int)(j0 + j) & (LPD - 1);
            const uint32_t r = (uint32_t)__shfl((int)my_r, src, LPD);
            ww[j] = __shfl(my_w, src, LPD);
            const bool ok = j0 + j < ne;
            const T* xrow = reinterpret_cast<const T*>(x + (uint64_t)r * ldx);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
              const uint32_t col = c0 + sl + c * LPD;
              xv[j][c] = (ok && col < nv) ? xrow[col] : hzero<HV>();
            }
          }
#pragma unroll
          for (int j = 0; j < U; ++j)
            if (j0 + j < ne) {
#pragma unroll
              for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int q = 0; q < HV; ++q)
                  acc[c][q] = acc[c][q] + hwiden<HV>(xv[j][c], q) * ww[j];
            }
        }
      }
      float* yrow = y + (uint64_t)d * ldy;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {  // output rows are not re-read here: non-temporal
        const uint32_t col = c0 + sl + c * LPD;
        if (col >= nv) continue;
        const uint32_t f0 = col * HV;
        store_widened<HV, true>(yrow + f0, acc[c], min(F - f0, (uint32_t)HV), yal);
      }
    }
  }
}

// out[i, :] = float(table[index[i], :])
template <int HV, int LPD>
__global__ __launch_bounds__(kAggThreads) void k_gather_rows_h(
    const uint16_t* __restrict__ table, uint64_t ldt, const uint32_t* __restrict__ index,
    const uint32_t* n_dev, uint32_t n_cap, uint32_t nv, uint32_t F, float* __restrict__ out,
    uint64_t ldo, int yal) {
  using T = typename HT<HV>::T;
  const uint32_t n = n_dev ? min(*n_dev, n_cap) : n_cap;
  constexpr int GPB = kAggThreads / LPD;
  const int grp = threadIdx.x / LPD, sl = threadIdx.x % LPD;
  for (uint32_t i = blockIdx.x * GPB + grp; i < n; i += gridDim.x * GPB) {
    const T* src = reinterpret_cast<const T*>(table + (uint64_t)index[i] * ldt);
    float* dst = out + (uint64_t)i * ldo;
    for (uint32_t c = sl; c < nv; c += LPD) {
      const T v = src[c];
      float a[HV];
#pragma unroll
      for (int q = 0; q < HV; ++q) a[q] = hwiden<HV>(v, q);
      const uint32_t f0 = c * HV;
      store_widened<HV, false>(dst + f0, a, min(F - f0, (uint32_t)HV), yal);
    }
  }
}

struct GraphAggH {
  static constexpr bool kCoef = false;
  const uint64_t* co;      // [V+1] global CSC offsets
  const uint32_t* ri;      // [E] global src ids
  const float* so;         // [V] degree_sqrt(out_degree)   (weight_type != NONE)
  const float* si;         // [V] degree_sqrt(in_degree)
  const uint32_t* in_deg;  // [V] (MEAN)
  int weight_type;
  int relu;
  const uint16_t* x;
  uint64_t ldx;            // halves
  float* y;
  uint64_t ldy;
  int yal;                 // floats the rows of y are aligned to (4, 2, 1)
  uint32_t nv;             // HV-half vectors per row (the last may be partial)
  uint32_t F;
  uint64_t v_begin, n;     // rows [v_begin, v_begin + n)
  const uint32_t* hubs;    // HUB: the hub rows, ascending; hubs_n[0] of them
  const uint32_t* hubs_n;
};

// nts_hip_spmm_graph_fwd_coef_h: GraphAggCoef (infer.hip) over the half table
struct GraphAggCoefH : GraphAggH {
  static constexpr bool kCoef = true;
  const float* ec;         // [E] per-edge coefficient, CSC order
};

// graph_row_slice (infer.hip) over half rows: one (row d, column slice) item on
// the calling LPD-lane group, vector column `col` of the row (col >= nv: an
// idle lane, it still takes part in the shuffles).  The weights and the edge
// walk are that function's, on both sides of the hub switch.
template <int HV, int LPD, typename A>
__device__ __forceinline__ void graph_row_slice_h(const A& a, uint64_t d, uint32_t col, int sl) {
  using T = typename HT<HV>::T;
  const uint64_t beg = a.co[d], end = a.co[d + 1];
  const bool weighted = a.weight_type != NTS_WEIGHT_NONE;
  const float sid = weighted ? a.si[d] : 1.0f;
  const uint32_t ind = a.weight_type == NTS_WEIGHT_MEAN ? a.in_deg[d] : 1u;
  const bool live = col < a.nv;
  float acc[HV];
#pragma unroll
  for (int q = 0; q < HV; ++q) acc[q] = 0.f;
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
        T v = hzero<HV>();
        if (live && j0 + j < ne) v = reinterpret_cast<const T*>(a.x + (uint64_t)r * a.ldx)[col];
        xv[j] = v;
      }
#pragma unroll
      for (int j = 0; j < kInfU; ++j)
        if (j0 + j < ne) {
#pragma unroll
          for (int q = 0; q < HV; ++q) acc[q] = acc[q] + hwiden<HV>(xv[j], q) * ww[j];
        }
    }
  }
  if (!live) return;
  if (a.relu) {
#pragma unroll
    for (int q = 0; q < HV; ++q) acc[q] = acc[q] > 0.f ? acc[q] : 0.f;
  }
  const uint32_t f0 = col * HV;
  store_widened<HV, false>(a.y + d * a.ldy + f0, acc, min(a.F - f0, (uint32_t)HV), a.yal);
}

// k_spmm_graph's items (infer.hip): HUB = false: (row v_begin + i, slice s of
// LPD vectors), hub rows skipped; HUB = true: (h, s) over the hub list
template <int HV, int LPD, bool HUB, typename A>
__global__ __launch_bounds__(kInfThreads) void k_spmm_graph_h(A a) {
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
    graph_row_slice_h<HV, LPD>(a, d, s * LPD + sl, sl);
  }
}

// ---------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------
// Halves per lane vector the table's rows allow: the widest of 8, 4, 2, 1 with
// the base aligned to it, the pitch a multiple of it and the row, rounded up to
// it, inside the pitch (the partial last vector reads pitch padding).
static int half_vec(uint32_t F, const uint16_t* xh, uint64_t ldxh) {
  for (int hv = 8; hv > 1; hv >>= 1)
    if ((uintptr_t)xh % (2 * hv) == 0 && ldxh % hv == 0 && ((uint64_t)F + hv - 1) / hv * hv <= ldxh)
      return hv;
  return 1;
}
// floats the fp32 output rows are aligned to
static int out_align(const float* y, uint64_t ldy) {
  if ((uintptr_t)y % 16 == 0 && ldy % 4 == 0) return 4;
  if ((uintptr_t)y % 8 == 0 && ldy % 2 == 0) return 2;
  return 1;
}

template <int HV, bool MAP>
static int launch_gather_h(hipStream_t st, const uint32_t* off, const uint32_t* idx, const float* w,
                           const uint32_t* n_dev, uint32_t n_cap, const uint16_t* x, uint64_t ldx,
                           const uint32_t* map, uint32_t F, float* y, uint64_t ldy) {
  const uint32_t nv = (F + HV - 1) / HV;
  const Shape s = pick_shape(nv);
  const int yal = out_align(y, ldy);
  const uint32_t grid =
      std::max(1u, std::min(ceil_div(n_cap, kAggThreads / s.lpd), kGatherGridCap));
#define NTS_G(LPD, NCH)                                                                         \
  hipLaunchKernelGGL((k_spmm_gather_h<HV, LPD, NCH, MAP, gather_u_h((HV * NCH + 1) / 2)>),       \
                     dim3(grid), dim3(kAggThreads), 0, st, off, idx, w, n_dev, n_cap, x, ldx,   \
                     map, nv, F, y, ldy, yal)
  if (s.lpd == 8) NTS_G(8, 1);
  else if (s.lpd == 16) NTS_G(16, 1);
  else if (s.lpd == 32) NTS_G(32, 1);
  else if (s.nch == 1) NTS_G(64, 1);
  else if (s.nch == 2) NTS_G(64, 2);
  else if (s.nch == 3) NTS_G(64, 3);
  else NTS_G(64, kMaxNchH);
#undef NTS_G
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

template <int HV>
static int launch_rows_h(hipStream_t st, const uint16_t* table, uint64_t ldt, const uint32_t* index,
                         const uint32_t* n, uint32_t n_cap, uint32_t F, float* out, uint64_t ldo) {
  const uint32_t nv = (F + HV - 1) / HV;
  const int lpd = nv <= 16 ? 16 : (nv <= 32 ? 32 : 64);
  const int yal = out_align(out, ldo);
  const uint32_t grid = std::max(1u, std::min(ceil_div(n_cap, kAggThreads / lpd), 4096u));
#define NTS_R(LPD)                                                                              \
  hipLaunchKernelGGL((k_gather_rows_h<HV, LPD>), dim3(grid), dim3(kAggThreads), 0, st, table, ldt, \
                     index, n, n_cap, nv, F, out, ldo, yal)
  if (lpd == 16) NTS_R(16); else if (lpd == 32) NTS_R(32); else NTS_R(64);
#undef NTS_R
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

template <int HV, typename A>
static int launch_graph_h(hipStream_t st, const A& a) {
  // hubs first: they are the longest items of the call
  hipLaunchKernelGGL((k_spmm_graph_h<HV, kHubLpd, true, A>), dim3(kHubGrid), dim3(kInfThreads), 0, st,
                     a);
  NTS_LAUNCH_CHECK();
  const int lpd = a.nv <= 8 ? 8 : a.nv <= 16 ? 16 : a.nv <= 32 ? 32 : 64;
  const uint64_t items = a.n * ((a.nv + lpd - 1) / lpd);
  const uint32_t gpb = kInfThreads / lpd;
  // one item per lane group up to 2^20 blocks, grid-stride beyond
  const uint32_t grid = (uint32_t)std::min<uint64_t>((items + gpb - 1) / gpb, 1u << 20);
#define NTS_I(LPD) \
  hipLaunchKernelGGL((k_spmm_graph_h<HV, LPD, false, A>), dim3(grid), dim3(kInfThreads), 0, st, a)
  if (lpd == 8) NTS_I(8); else if (lpd == 16) NTS_I(16); else if (lpd == 32) NTS_I(32); else NTS_I(64);
#undef NTS_I
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

// the dispatch over the table's vector width
#define NTS_BY_HALF_VEC(hv, CALL) \
  do {                            \
    if ((hv) == 8) return CALL(8); \
    if ((hv) == 4) return CALL(4); \
    if ((hv) == 2) return CALL(2); \
    return CALL(1);               \
  } while (0)

}  // namespace nts_hip

using namespace nts_hip;

// nts_hip_spmm_graph_fwd_h and its _coef sibling: A = GraphAggH or GraphAggCoefH
template <typename A>
static int spmm_graph_fwd_h(nts_hip_ctx* ctx, const nts_graph_dev* graph, const float* edge_coef,
                            uint64_t v_begin, uint64_t v_end, int weight_type, int relu,
                            const uint16_t* xh, uint64_t ldxh, uint32_t feature_size, float* y,
                            uint64_t ldy) {
  NTS_CHECK_ARG(graph != nullptr, "graph is NULL");
  NTS_CHECK_ARG(v_begin <= v_end, "v_begin > v_end");
  NTS_CHECK_ARG(xh != nullptr, "the half table is NULL");
  NTS_CHECK_ARG(ctx && y, "NULL argument");
  NTS_CHECK_ARG(v_end <= graph->n_vertices && graph->n_vertices <= 0xFFFFFFFFull,
                "vertex range outside the graph");
  NTS_CHECK_ARG(graph->column_offset && (graph->n_edges == 0 || graph->row_indices),
                "graph without its CSC");
  NTS_CHECK_ARG(weight_type == NTS_WEIGHT_SUM || weight_type == NTS_WEIGHT_MEAN ||
                    weight_type == NTS_WEIGHT_NONE,
                "weight type: SUM, MEAN or NONE (no MEAN_SAMPLED, no UP_DEGREE over the full graph)");
  NTS_CHECK_ARG(weight_type == NTS_WEIGHT_NONE || (graph->in_degree && graph->out_degree),
                "graph without its degrees");
  NTS_CHECK_ARG(feature_size > 0, "feature_size is 0");
  NTS_CHECK_ARG(ldxh >= feature_size && ldy >= feature_size, "leading dimension < feature_size");
  NTS_CHECK_ARG((uintptr_t)xh % 2 == 0, "the half table's address is odd");
  const uint64_t n = v_end - v_begin;
  if (n == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  HubScratch h;
  NTS_RET(list_hubs(ctx, graph, v_begin, n, h));
  if (weight_type != NTS_WEIGHT_NONE) NTS_RET(degree_sqrt_tables(ctx, graph, h.so, h.si));
  A a;
  if constexpr (A::kCoef) a.ec = edge_coef;
  a.co = graph->column_offset;
  a.ri = graph->row_indices;
  a.so = h.so;
  a.si = h.si;
  a.in_deg = graph->in_degree;
  a.weight_type = weight_type;
  a.relu = relu ? 1 : 0;
  a.x = xh;
  a.ldx = ldxh;
  a.y = y;
  a.ldy = ldy;
  a.yal = out_align(y, ldy);
  a.F = feature_size;
  a.v_begin = v_begin;
  a.n = n;
  a.hubs = h.hubs;
  a.hubs_n = h.pos + n;
  const int hv = half_vec(feature_size, xh, ldxh);
  a.nv = (feature_size + hv - 1) / hv;
#define NTS_C(HV) launch_graph_h<HV>(ctx->stream, a)
  NTS_BY_HALF_VEC(hv, NTS_C);
#undef NTS_C
}

extern "C" {

int nts_hip_spmm_csc_fwd_h(nts_hip_ctx* ctx, const uint32_t* column_offset,
                           const uint32_t* row_indices, const float* weight, const uint32_t* v,
                           uint32_t v_cap, const uint16_t* xh, uint64_t ldxh,
                           const uint32_t* x_row_map, uint32_t feature_size, float* y,
                           uint64_t ldy) {
  NTS_CHECK_ARG(xh != nullptr, "the half table is NULL");
  NTS_CHECK_ARG(ctx && column_offset && row_indices && y, "NULL argument");
  NTS_CHECK_ARG(feature_size > 0, "feature_size is 0");
  NTS_CHECK_ARG(ldxh >= feature_size && ldy >= feature_size, "leading dimension < feature_size");
  NTS_CHECK_ARG((uintptr_t)xh % 2 == 0, "the half table's address is odd");
  if (v_cap == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const int hv = half_vec(feature_size, xh, ldxh);
#define NTS_C(HV)                                                                               \
  (x_row_map ? launch_gather_h<HV, true>(ctx->stream, column_offset, row_indices, weight, v,    \
                                         v_cap, xh, ldxh, x_row_map, feature_size, y, ldy)      \
             : launch_gather_h<HV, false>(ctx->stream, column_offset, row_indices, weight, v,   \
                                          v_cap, xh, ldxh, nullptr, feature_size, y, ldy))
  NTS_BY_HALF_VEC(hv, NTS_C);
#undef NTS_C
}

int nts_hip_gather_rows_h(nts_hip_ctx* ctx, const uint16_t* tableh, uint64_t ld_table,
                          const uint32_t* index, const uint32_t* n, uint32_t n_cap,
                          uint32_t feature_size, float* out, uint64_t ld_out) {
  NTS_CHECK_ARG(tableh != nullptr, "the half table is NULL");
  NTS_CHECK_ARG(ctx && index && out, "NULL argument");
  NTS_CHECK_ARG(feature_size > 0, "feature_size is 0");
  NTS_CHECK_ARG(ld_table >= feature_size && ld_out >= feature_size,
                "leading dimension < feature_size");
  NTS_CHECK_ARG((uintptr_t)tableh % 2 == 0, "the half table's address is odd");
  if (n_cap == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const int hv = half_vec(feature_size, tableh, ld_table);
#define NTS_C(HV) \
  launch_rows_h<HV>(ctx->stream, tableh, ld_table, index, n, n_cap, feature_size, out, ld_out)
  NTS_BY_HALF_VEC(hv, NTS_C);
#undef NTS_C
}

int nts_hip_spmm_graph_fwd_h(nts_hip_ctx* ctx, const nts_graph_dev* graph, uint64_t v_begin,
                             uint64_t v_end, int weight_type, int relu, const uint16_t* xh,
                             uint64_t ldxh, uint32_t feature_size, float* y, uint64_t ldy) {
  return spmm_graph_fwd_h<GraphAggH>(ctx, graph, nullptr, v_begin, v_end, weight_type, relu, xh,
                                     ldxh, feature_size, y, ldy);
}

int nts_hip_spmm_graph_fwd_coef_h(nts_hip_ctx* ctx, const nts_graph_dev* graph,
                                  const float* edge_coef, uint64_t v_begin, uint64_t v_end,
                                  int weight_type, int relu, const uint16_t* xh, uint64_t ldxh,
                                  uint32_t feature_size, float* y, uint64_t ldy) {
  NTS_CHECK_ARG(graph != nullptr, "graph is NULL");
  NTS_CHECK_ARG(edge_coef || graph->n_edges == 0, "edge_coef is NULL");
  return spmm_graph_fwd_h<GraphAggCoefH>(ctx, graph, edge_coef, v_begin, v_end, weight_type, relu,
                                         xh, ldxh, feature_size, y, ldy);
}

}  // extern "C"
