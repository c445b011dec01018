// GraphSAGE max aggregator over a sampled layer (no counterpart in the
// reference, whose graph ops are weighted sums): the CSC gather that keeps a
// running (max, arg) per column, and the CSR backward that routes each
// gradient to the one edge that won.
//
// Forward.  Layout and schedule are k_spmm_gather's (aggregate.hip): one
// LPD-lane group per destination row, each lane NCH vectors of VEC floats of
// it, the group's edge ids loaded one per lane and the neighbour rows fetched
// U at a time.  Per column the edges are scanned serially in CSC edge order:
// the first edge's value starts the maximum and a later one replaces it on a
// strict >, so ties (+0 / -0 included) stay with the earliest edge; an empty
// column gives 0 and the arg kNoEdge.
//
// Backward.  g_in[s] = sum over the CSR slots j of row s whose CSC edge
// csr_edge_id[j] is the arg of its destination, of g_y[ci[j]] — a slot that
// did not win adds an exact +0.  The rows are split as nts_hip_spmm_csr_bwd
// splits them for the same operands (lane-group width, long-row threshold,
// in-order pieces added in group order through LDS), so where every slot won
// the two agree to the bit.  No float atomics, no grid barrier.
#include "agg_shape.hpp"

#pragma clang fp contract(off)

namespace nts_hip {

template <int VEC>
struct MV;
template <>
struct MV<1> {
  using T = float;
  using I = uint32_t;
};
template <>
struct MV<2> {
  using T = float2;
  using I = uint2;
};
template <>
struct MV<4> {
  using T = float4;
  using I = uint4;
};

constexpr uint32_t kNoEdge = 0xFFFFFFFFu;
constexpr int kMaxNch = 4;  // vectors a lane holds of a row; wider rows take more rounds

template <int VEC>
__device__ __forceinline__ float& fcomp(typename MV<VEC>::T& v, int q) {
  return reinterpret_cast<float*>(&v)[q];
}
template <int VEC>
__device__ __forceinline__ uint32_t& icomp(typename MV<VEC>::I& v, int q) {
  return reinterpret_cast<uint32_t*>(&v)[q];
}
template <int VEC>
__device__ __forceinline__ typename MV<VEC>::T fzero() {
  typename MV<VEC>::T v;
#pragma unroll
  for (int q = 0; q < VEC; ++q) fcomp<VEC>(v, q) = 0.f;
  return v;
}

// nvalid floats of vector v to p (nvalid == VEC: one vector store)
template <int VEC, bool NT>
__device__ __forceinline__ void store_f(float* p, typename MV<VEC>::T v, uint32_t nvalid) {
  if (nvalid == (uint32_t)VEC) {
    typedef float fv __attribute__((ext_vector_type(VEC)));
    fv u;
#pragma unroll
    for (int q = 0; q < VEC; ++q) u[q] = fcomp<VEC>(v, q);
    if constexpr (NT) __builtin_nontemporal_store(u, reinterpret_cast<fv*>(p));
    else *reinterpret_cast<fv*>(p) = u;
  } else {
#pragma unroll
    for (int q = 0; q < VEC; ++q)
      if ((uint32_t)q < nvalid) p[q] = fcomp<VEC>(v, q);
  }
}

// y[d, c] = max over the column's edges of x[row(e), c], arg[d, c] = the first
// edge that holds it (ARG); with self, y[d, F:2F] = x[self[d], :].
// nv vectors per row, the last one of last_valid floats (pitch padding read,
// not stored); arg rows have pitch F = (nv - 1) VEC + last_valid, written as
// vectors where arg_vec (F a multiple of VEC and the base aligned to it).
template <int VEC, int LPD, int NCH, bool MAP, int U, bool ARG>
__global__ __launch_bounds__(kAggThreads) void k_max_gather(
    const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx, const uint32_t* n_dev,
    uint32_t n_cap, const float* __restrict__ x, uint64_t ldx, const uint32_t* __restrict__ map,
    const uint32_t* __restrict__ self, uint32_t nv, uint32_t last_valid, float* __restrict__ y,
    uint64_t ldy, uint32_t* __restrict__ arg, int arg_vec) {
  using T = typename MV<VEC>::T;
  using I = typename MV<VEC>::I;
  const uint32_t n = n_dev ? min(*n_dev, n_cap) : n_cap;
  const uint32_t F = (nv - 1) * VEC + last_valid;
  constexpr int GPB = kAggThreads / LPD;
  const int grp = threadIdx.x / LPD, sl = threadIdx.x % LPD;
  for (uint32_t d = blockIdx.x * GPB + grp; d < n; d += gridDim.x * GPB) {
    const uint32_t beg = off[d], end = off[d + 1];
    for (uint32_t c0 = 0; c0 < nv; c0 += LPD * NCH) {
      T m[NCH], sv[NCH];
      I a[ARG ? NCH : 1];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        m[c] = fzero<VEC>();
        sv[c] = fzero<VEC>();
        if constexpr (ARG) {
#pragma unroll
          for (int q = 0; q < VEC; ++q) icomp<VEC>(a[c], q) = kNoEdge;
        }
      }
      if (self) {  // (uniform) known before the edges are: its latency overlaps the gather
        const T* srow = reinterpret_cast<const T*>(x + (uint64_t)self[d] * ldx);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const uint32_t col = c0 + sl + c * LPD;
          if (col < nv) sv[c] = srow[col];
        }
      }
      for (uint32_t cb = beg; cb < end; cb += LPD) {
        const uint32_t ne = min(end - cb, (uint32_t)LPD);
        uint32_t my_r = 0;
        if ((uint32_t)sl < ne) {  // streamed once: do not keep in cache
          my_r = __builtin_nontemporal_load(idx + cb + sl);
          if (MAP) my_r = map[my_r];
        }
        for (uint32_t j0 = 0; j0 < ne; j0 += U) {
          T xv[U][NCH];
#pragma unroll
          for (int j = 0; j < U; ++j) {
            const uint32_t r = (uint32_t)__shfl((int)my_r, (int)(j0 + j) & (LPD - 1), LPD);
            const bool ok = j0 + j < ne;
            const T* xrow = reinterpret_cast<const T*>(x + (uint64_t)r * ldx);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
              const uint32_t col = c0 + sl + c * LPD;
              xv[j][c] = (ok && col < nv) ? xrow[col] : fzero<VEC>();
            }
          }
#pragma unroll
          for (int j = 0; j < U; ++j)
            if (j0 + j < ne) {
              const uint32_t e = cb + j0 + j;
              const bool first = e == beg;  // starts the maximum whatever its value
#pragma unroll
              for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                  const float v = fcomp<VEC>(xv[j][c], q);
                  const bool take = first || v > fcomp<VEC>(m[c], q);
                  if (take) fcomp<VEC>(m[c], q) = v;
                  if constexpr (ARG) {
                    if (take) icomp<VEC>(a[c], q) = e;
                  }
                }
            }
        }
      }
      float* yrow = y + (uint64_t)d * ldy;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const uint32_t col = c0 + sl + c * LPD;
        if (col >= nv) continue;
        const uint32_t nvalid = col + 1 == nv ? last_valid : (uint32_t)VEC;
        store_f<VEC, true>(yrow + (uint64_t)col * VEC, m[c], nvalid);
        // (self: F is a multiple of VEC, every vector is whole)
        if (self) store_f<VEC, false>(yrow + F + (uint64_t)col * VEC, sv[c], nvalid);
        if constexpr (ARG) {
          uint32_t* ap = arg + (uint64_t)d * F + (uint64_t)col * VEC;
          if (arg_vec) {
            typedef uint32_t uv __attribute__((ext_vector_type(VEC)));
            uv u;
#pragma unroll
            for (int q = 0; q < VEC; ++q) u[q] = icomp<VEC>(a[c], q);
            __builtin_nontemporal_store(u, reinterpret_cast<uv*>(ap));  // read again in the backward only
          } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q)
              if ((uint32_t)q < nvalid) ap[q] = icomp<VEC>(a[c], q);
          }
        }
      }
    }
  }
}

struct MaxBwd {
  const uint32_t* off;   // CSR row offsets, column indices (dst of each slot),
  const uint32_t* idx;   // and each slot's CSC edge
  const uint32_t* eid;
  const uint32_t* n_dev;
  uint32_t n_cap;
  const float* g;        // [v, ldg]: g_y, the self half at column F
  uint64_t ldg;
  const uint32_t* arg;   // [v, F]
  const uint32_t* self;  // src_dst or NULL
  const float* mx;       // x_act or NULL
  uint64_t ldm;
  float scale;
  uint32_t nv;           // vectors per row (F = nv VEC)
  uint32_t long_row;     // rows above it are summed by the whole block
  float* y;              // g_in
  uint64_t ldy;
};

// acc[c] += over the slots [beg, end) in order: arg[dst, col] == eid ? g[dst, col] : +0
template <int VEC, int LPD, int NCH, int U>
__device__ __forceinline__ void route_slots(typename MV<VEC>::T (&acc)[NCH], uint32_t beg,
                                            uint32_t end, uint32_t c0, int sl, const MaxBwd& a) {
  using T = typename MV<VEC>::T;
  using I = typename MV<VEC>::I;
  const uint32_t F = a.nv * VEC;
  for (uint32_t cb = beg; cb < end; cb += LPD) {
    const uint32_t ne = min(end - cb, (uint32_t)LPD);
    uint32_t my_r = 0, my_e = 0;
    if ((uint32_t)sl < ne) {
      my_r = __builtin_nontemporal_load(a.idx + cb + sl);
      my_e = __builtin_nontemporal_load(a.eid + cb + sl);
    }
    for (uint32_t j0 = 0; j0 < ne; j0 += U) {
      T gv[U][NCH];
      I av[U][NCH];
      uint32_t ee[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const int src = (int)(j0 + j) & (LPD - 1);
        const uint32_t r = (uint32_t)__shfl((int)my_r, src, LPD);
        ee[j] = (uint32_t)__shfl((int)my_e, src, LPD);
        const bool ok = j0 + j < ne;
        const T* grow = reinterpret_cast<const T*>(a.g + (uint64_t)r * a.ldg);
        const I* arow = reinterpret_cast<const I*>(a.arg + (uint64_t)r * F);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const uint32_t col = c0 + sl + c * LPD;
          const bool in = ok && col < a.nv;
          gv[j][c] = in ? grow[col] : fzero<VEC>();
          if (in) {
            av[j][c] = arow[col];
          } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q) icomp<VEC>(av[j][c], q) = kNoEdge;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < U; ++j)
        if (j0 + j < ne) {
#pragma unroll
          for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int q = 0; q < VEC; ++q)
              fcomp<VEC>(acc[c], q) =
                  fcomp<VEC>(acc[c], q) +
                  (icomp<VEC>(av[j][c], q) == ee[j] ? fcomp<VEC>(gv[j][c], q) : 0.f);
        }
    }
  }
}

// one output row after its sum: the self term (one more add), the mask, the store
template <int VEC, int LPD, int NCH>
__device__ __forceinline__ void finish_row(typename MV<VEC>::T (&acc)[NCH], uint32_t s, uint32_t c0,
                                           int sl, const MaxBwd& a) {
  using T = typename MV<VEC>::T;
  const uint32_t sd = a.self ? a.self[s] : kNoEdge;  // (NTS_NOT_CACHED: no self term)
  const T* srow =
      sd != kNoEdge ? reinterpret_cast<const T*>(a.g + (uint64_t)sd * a.ldg) + a.nv : nullptr;
  const T* mrow = a.mx ? reinterpret_cast<const T*>(a.mx + (uint64_t)s * a.ldm) : nullptr;
  T* yrow = reinterpret_cast<T*>(a.y + (uint64_t)s * a.ldy);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = c0 + sl + c * LPD;
    if (col >= a.nv) continue;
    T v = acc[c];
    if (srow) {
      T t = srow[col];
#pragma unroll
      for (int q = 0; q < VEC; ++q) fcomp<VEC>(v, q) = fcomp<VEC>(v, q) + fcomp<VEC>(t, q);
    }
    if (mrow) {
      T t = mrow[col];
#pragma unroll
      for (int q = 0; q < VEC; ++q)
        fcomp<VEC>(v, q) = fcomp<VEC>(t, q) > 0.f ? fcomp<VEC>(v, q) * a.scale : 0.f;
    }
    yrow[col] = v;
  }
}

template <int VEC, int LPD, int NCH, int U>
__global__ __launch_bounds__(kAggThreads) void k_max_route(MaxBwd a) {
  using T = typename MV<VEC>::T;
  const uint32_t n = a.n_dev ? min(*a.n_dev, a.n_cap) : a.n_cap;
  constexpr int GPB = kAggThreads / LPD;
  const int grp = threadIdx.x / LPD, sl = threadIdx.x % LPD;
  __shared__ uint32_t long_rows[GPB * kCoopRows];
  __shared__ uint32_t n_long;
  __shared__ T part[GPB * LPD * NCH];
  if (threadIdx.x == 0) n_long = 0;
  __syncthreads();
  // (the grid gives a lane group at most kCoopRows rows: the list holds them)
  for (uint32_t s = blockIdx.x * GPB + grp; s < n; s += gridDim.x * GPB) {
    const uint32_t beg = a.off[s], end = a.off[s + 1];
    if (end - beg > a.long_row) {
      if (sl == 0) long_rows[atomicAdd(&n_long, 1u)] = s;
      continue;
    }
    for (uint32_t c0 = 0; c0 < a.nv; c0 += LPD * NCH) {
      T acc[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) acc[c] = fzero<VEC>();
      route_slots<VEC, LPD, NCH, U>(acc, beg, end, c0, sl, a);
      finish_row<VEC, LPD, NCH>(acc, s, c0, sl, a);
    }
  }
  __syncthreads();
  const uint32_t nl = n_long;
  for (uint32_t i = 0; i < nl; ++i) {
    const uint32_t s = long_rows[i];
    const uint32_t beg = a.off[s], len = a.off[s + 1] - beg;
    const uint32_t pb = beg + (uint32_t)(((uint64_t)len * grp) / GPB);
    const uint32_t pe = beg + (uint32_t)(((uint64_t)len * (grp + 1)) / GPB);
    for (uint32_t c0 = 0; c0 < a.nv; c0 += LPD * NCH) {
      T acc[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) acc[c] = fzero<VEC>();
      route_slots<VEC, LPD, NCH, U>(acc, pb, pe, c0, sl, a);
#pragma unroll
      for (int c = 0; c < NCH; ++c) part[(grp * NCH + c) * LPD + sl] = acc[c];
      __syncthreads();
      if (grp == 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          T t = part[c * LPD + sl];
          for (int g = 1; g < GPB; ++g) {
            T q = part[(g * NCH + c) * LPD + sl];
#pragma unroll
            for (int k = 0; k < VEC; ++k) fcomp<VEC>(t, k) = fcomp<VEC>(t, k) + fcomp<VEC>(q, k);
          }
          acc[c] = t;
        }
        finish_row<VEC, LPD, NCH>(acc, s, c0, sl, a);
      }
      __syncthreads();
    }
  }
}

// the lane-group shapes both kernels are built for: pick_shape's, at most
// kMaxNch vectors a lane
#define NTS_MAX_SHAPES(X)                 \
  if (s.lpd == 8) X(8, 1);                \
  else if (s.lpd == 16) X(16, 1);         \
  else if (s.lpd == 32) X(32, 1);         \
  else switch (std::min(s.nch, kMaxNch)) { \
      case 1: X(64, 1); break;            \
      case 2: X(64, 2); break;            \
      case 3: X(64, 3); break;            \
      default: X(64, 4); break;           \
    }

template <int VEC, bool MAP, bool ARG>
static int launch_max_fwd(hipStream_t st, Shape s, uint32_t grid, const uint32_t* off,
                          const uint32_t* idx, const uint32_t* n_dev, uint32_t n_cap,
                          const float* x, uint64_t ldx, const uint32_t* map, const uint32_t* self,
                          uint32_t nv, uint32_t last_valid, float* y, uint64_t ldy, uint32_t* arg,
                          int arg_vec) {
#define NTS_X(LPD, NCH)                                                                          \
  hipLaunchKernelGGL((k_max_gather<VEC, LPD, NCH, MAP, gather_u(VEC * NCH), ARG>), dim3(grid),    \
                     dim3(kAggThreads), 0, st, off, idx, n_dev, n_cap, x, ldx, map, self, nv,    \
                     last_valid, y, ldy, arg, arg_vec)
  NTS_MAX_SHAPES(NTS_X)
#undef NTS_X
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

template <int VEC>
static int launch_max_bwd(hipStream_t st, Shape s, uint32_t grid, const MaxBwd& a) {
  // a slot loads a gradient and an arg vector: half the sum gather's rows in flight
#define NTS_X(LPD, NCH)                                                                      \
  hipLaunchKernelGGL((k_max_route<VEC, LPD, NCH, gather_u(2 * VEC * NCH)>), dim3(grid),       \
                     dim3(kAggThreads), 0, st, a)
  NTS_MAX_SHAPES(NTS_X)
#undef NTS_X
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

}  // namespace nts_hip

using namespace nts_hip;

extern "C" {

int nts_hip_spmm_csc_fwd_max(nts_hip_ctx* ctx, const uint32_t* column_offset,
                             const uint32_t* row_indices, const uint32_t* v, uint32_t v_cap,
                             const float* x, uint64_t ldx, const uint32_t* x_row_map,
                             const uint32_t* self_index, uint32_t feature_size, float* y,
                             uint64_t ldy, uint32_t* arg) {
  NTS_CHECK_ARG(ctx && column_offset && row_indices && v && x && y, "NULL argument");
  NTS_CHECK_ARG(feature_size > 0, "feature_size is 0");
  NTS_CHECK_ARG(ldx >= feature_size, "leading dimension < feature_size");
  NTS_CHECK_ARG(ldy >= (self_index ? 2 : 1) * (uint64_t)feature_size,
                self_index ? "ldy < 2 feature_size" : "leading dimension < feature_size");
  if (v_cap == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const uint32_t F = feature_size;
  // the right half starts at column F: whole vectors only with self_index
  const int vec = row_vec(F, {{x, ldx}, {y, ldy}}, !self_index);
  const uint32_t nv = (F + vec - 1) / vec, last_valid = F - (nv - 1) * vec;
  const int arg_vec = F % vec == 0 && (uintptr_t)arg % (4 * vec) == 0;
  const Shape s = pick_shape(nv);
  const uint32_t grid =
      std::max(1u, std::min(ceil_div(v_cap, kAggThreads / s.lpd), kGatherGridCap));
  hipStream_t st = ctx->stream;
#define NTS_F(VEC)                                                                               \
  do {                                                                                           \
    if (x_row_map && arg)                                                                        \
      return launch_max_fwd<VEC, true, true>(st, s, grid, column_offset, row_indices, v, v_cap,  \
                                             x, ldx, x_row_map, self_index, nv, last_valid, y,   \
                                             ldy, arg, arg_vec);                                 \
    if (x_row_map)                                                                               \
      return launch_max_fwd<VEC, true, false>(st, s, grid, column_offset, row_indices, v, v_cap, \
                                              x, ldx, x_row_map, self_index, nv, last_valid, y,  \
                                              ldy, arg, arg_vec);                                \
    if (arg)                                                                                     \
      return launch_max_fwd<VEC, false, true>(st, s, grid, column_offset, row_indices, v, v_cap, \
                                              x, ldx, nullptr, self_index, nv, last_valid, y,    \
                                              ldy, arg, arg_vec);                                \
    return launch_max_fwd<VEC, false, false>(st, s, grid, column_offset, row_indices, v, v_cap,  \
                                             x, ldx, nullptr, self_index, nv, last_valid, y,     \
                                             ldy, arg, arg_vec);                                 \
  } while (0)
  if (vec == 4) NTS_F(4);
  if (vec == 2) NTS_F(2);
  NTS_F(1);
#undef NTS_F
}

int nts_hip_spmm_csr_bwd_max(nts_hip_ctx* ctx, const uint32_t* row_offset,
                             const uint32_t* column_indices, const uint32_t* csr_edge_id,
                             const uint32_t* s, uint32_t s_cap, const float* g_y, uint64_t ld_g,
                             const uint32_t* arg, const uint32_t* src_dst, const float* x_act,
                             uint64_t ld_act, float scale, uint32_t feature_size, float* g_in,
                             uint64_t ld_gin) {
  NTS_CHECK_ARG(ctx && row_offset && column_indices && csr_edge_id && s && g_y && arg && g_in,
                "NULL argument");
  NTS_CHECK_ARG(feature_size > 0, "feature_size is 0");
  NTS_CHECK_ARG(ld_g >= (src_dst ? 2 : 1) * (uint64_t)feature_size,
                src_dst ? "ld_g < 2 feature_size" : "leading dimension < feature_size");
  NTS_CHECK_ARG(ld_gin >= feature_size && (!x_act || ld_act >= feature_size),
                "leading dimension < feature_size");
  if (s_cap == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const uint32_t F = feature_size;
  // the lane-group width and the long-row threshold nts_hip_spmm_csr_bwd takes
  // for the same operands, so that every row is summed in its pieces; this
  // call's own vector width only sets how many rounds a row takes
  const int plain = row_vec(F, {{g_y, ld_g}, {g_in, ld_gin}}, true);
  const Shape sh = pick_shape((F + plain - 1) / plain);
  const int vec = row_vec(F, {{g_y, ld_g}, {g_in, ld_gin}, {x_act, ld_act}, {arg, F}});
  MaxBwd a;
  a.off = row_offset;
  a.idx = column_indices;
  a.eid = csr_edge_id;
  a.n_dev = s;
  a.n_cap = s_cap;
  a.g = g_y;
  a.ldg = ld_g;
  a.arg = arg;
  a.self = src_dst;
  a.mx = x_act;
  a.ldm = ld_act;
  a.scale = x_act ? scale : 1.f;
  a.nv = F / vec;
  a.long_row = kLongRow(gather_u(plain * sh.nch));
  a.y = g_in;
  a.ldy = ld_gin;
  const uint32_t gpb = kAggThreads / sh.lpd;
  const uint32_t grid = std::max({1u, std::min(ceil_div(s_cap, gpb), kGatherGridCap),
                                  ceil_div(s_cap, gpb * kCoopRows)});
  if (vec == 4) return launch_max_bwd<4>(ctx->stream, sh, grid, a);
  if (vec == 2) return launch_max_bwd<2>(ctx->stream, sh, grid, a);
  return launch_max_bwd<1>(ctx->stream, sh, grid, a);
}

}  // extern "C"
