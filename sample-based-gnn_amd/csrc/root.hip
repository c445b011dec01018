// GraphSAGE root weight (SAGEConv): the graph op of X' = act([A X | X_dst] W).
//
//   forward   ycat[d, 0:F]  = sum_e w[e] x[row(e), :]   (CSC edge order, acc + x*w,
//             ycat[d, F:2F] = x[self(d), :]              contraction off, from 0)
//   backward  g_in[s, :] = mask_s ⊙ scale (sum_j w_b[j] dycat[ci[j], 0:F]
//                                          + dycat[src_dst[s], F:2F])
//   inverse   src_dst[s] = the d with dst_local_id[d] == s, or NTS_NOT_CACHED
//
// Lane-group layout as k_spmm_gather (aggregate.hip): LPD lanes per row, each
// lane NCH vectors of VEC floats a chunk, the row's edge ids / weights loaded
// one per lane and broadcast by __shfl, U neighbour rows in flight.  The sums
// are those of nts_hip_spmm_csc_fwd / nts_hip_spmm_csr_bwd to the bit: the
// backward takes the lane-group shape and the long-row rule that call takes
// for the same operands (rows longer than long_row edges are summed as GPB
// in-order pieces added in group order through LDS), so only the vector width
// may differ, which changes no float.  No atomics on floats, no grid barrier.
#include "common.hpp"

#pragma clang fp contract(off)

namespace nts_hip {
namespace root {

constexpr int kRootThreads = 256;
constexpr uint32_t kRootCoopRows = 16;  // long rows a lane group may list (grid sized for it)
constexpr uint32_t kNone = 0xFFFFFFFFu;

template <int VEC>
struct RV;
template <>
struct RV<1> {
  using T = float;
};
template <>
struct RV<2> {
  using T = float2;
};
template <>
struct RV<4> {
  using T = float4;
};
template <int VEC>
__device__ __forceinline__ float& rcomp(typename RV<VEC>::T& v, int q) {
  return reinterpret_cast<float*>(&v)[q];
}
template <int VEC>
__device__ __forceinline__ float rcomp(const typename RV<VEC>::T& v, int q) {
  return reinterpret_cast<const float*>(&v)[q];
}
template <int VEC>
__device__ __forceinline__ typename RV<VEC>::T rzero() {
  typename RV<VEC>::T z;
#pragma unroll
  for (int q = 0; q < VEC; ++q) rcomp<VEC>(z, q) = 0.f;
  return z;
}

// acc[c] += sum over the edges [beg, end) in edge order of w[e] * x[row(e)][col],
// col = c0 + sl + c * LPD in vectors; nv vectors a row
template <int VEC, int LPD, int NCH, int U, bool MAP>
__device__ __forceinline__ void root_edges(typename RV<VEC>::T (&acc)[NCH], uint32_t beg,
                                           uint32_t end, uint32_t c0, int sl,
                                           const uint32_t* __restrict__ idx,
                                           const float* __restrict__ w,
                                           const float* __restrict__ x, uint64_t ldx,
                                           const uint32_t* __restrict__ map, uint32_t nv) {
  using T = typename RV<VEC>::T;
  for (uint32_t cb = beg; cb < end; cb += LPD) {
    const uint32_t ne = min(end - cb, (uint32_t)LPD);
    uint32_t my_r = 0;
    float my_w = 0.f;
    if ((uint32_t)sl < ne) {
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
          xv[j][c] = (ok && col < nv) ? xrow[col] : rzero<VEC>();
        }
      }
#pragma unroll
      for (int j = 0; j < U; ++j)
        if (j0 + j < ne) {
#pragma unroll
          for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int q = 0; q < VEC; ++q)
              rcomp<VEC>(acc[c], q) = rcomp<VEC>(acc[c], q) + rcomp<VEC>(xv[j][c], q) * ww[j];
        }
    }
  }
}

// BWD = false: off/idx/w the sampled CSC, x the source rows (MAP: the global
//   table through map), self = self_index; y = ycat, the self row copied to
//   columns [F, 2F)
// BWD = true: off/idx/w the CSR transpose, x = dycat (its left half gathered),
//   self = src_dst, the self row dycat[self, F:2F] added last, then the mask
//   of row d (mx != NULL); y = g_in
template <int VEC, int LPD, int NCH, int U, bool MAP, bool BWD>
__global__ __launch_bounds__(kRootThreads) void k_root(
    const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx,
    const float* __restrict__ w, const uint32_t* __restrict__ n_dev, uint32_t n_cap,
    const float* __restrict__ x, uint64_t ldx, const uint32_t* __restrict__ map,
    const uint32_t* __restrict__ self, uint32_t nv, float* __restrict__ y, uint64_t ldy,
    const float* __restrict__ mx, uint64_t ldm, float scale, uint32_t long_row) {
  using T = typename RV<VEC>::T;
  static_assert(!(MAP && BWD), "the backward gathers local rows");
  const uint32_t n = min(*n_dev, n_cap);
  constexpr int GPB = kRootThreads / LPD;
  const int grp = threadIdx.x / LPD, sl = threadIdx.x % LPD;
  __shared__ uint32_t long_rows[BWD ? GPB * kRootCoopRows : 1];
  __shared__ uint32_t n_long;
  if (BWD) {
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
  }
  // one output row's epilogue: forward the self copy, backward self add + mask
  auto finish = [&](T (&acc)[NCH], uint32_t d, uint32_t c0, const T (&sv)[NCH],
                    const T (&mv)[NCH]) {
    T* yrow = reinterpret_cast<T*>(y + (uint64_t)d * ldy);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint32_t col = c0 + sl + c * LPD;
      if (col >= nv) continue;
      if constexpr (BWD) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          float v = rcomp<VEC>(acc[c], q) + rcomp<VEC>(sv[c], q);
          if (mx) v = rcomp<VEC>(mv[c], q) > 0.f ? v * scale : 0.f;
          rcomp<VEC>(acc[c], q) = v;
        }
        yrow[col] = acc[c];
      } else {
        yrow[col] = acc[c];
        yrow[nv + col] = sv[c];  // F = nv VEC: the right half starts nv vectors in
      }
    }
  };
  // the self row and the mask row of output row d (loaded ahead of the gather)
  auto side_rows = [&](uint32_t d, uint32_t c0, T (&sv)[NCH], T (&mv)[NCH]) {
    uint32_t sr = self[d];
    const bool has = !BWD || sr != kNone;
    if (!has) sr = 0;
    // forward: x[self] (a global row under MAP); backward: dycat[self, F:2F]
    const T* srow = reinterpret_cast<const T*>(x + (uint64_t)sr * ldx) + (BWD ? nv : 0);
    const T* mrow = reinterpret_cast<const T*>(mx + (BWD && mx ? (uint64_t)d * ldm : 0));
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint32_t col = c0 + sl + c * LPD;
      sv[c] = (has && col < nv) ? srow[col] : rzero<VEC>();
      mv[c] = (BWD && mx && col < nv) ? mrow[col] : rzero<VEC>();
    }
  };
  for (uint32_t d = blockIdx.x * GPB + grp; d < n; d += gridDim.x * GPB) {
    const uint32_t beg = off[d], end = off[d + 1];
    if (BWD && end - beg > long_row) {  // summed by the whole block below
      if (sl == 0) long_rows[atomicAdd(&n_long, 1u)] = d;
      continue;
    }
    for (uint32_t c0 = 0; c0 < nv; c0 += LPD * NCH) {
      T acc[NCH], sv[NCH], mv[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) acc[c] = rzero<VEC>();
      side_rows(d, c0, sv, mv);
      root_edges<VEC, LPD, NCH, U, MAP>(acc, beg, end, c0, sl, idx, w, x, ldx, map, nv);
      finish(acc, d, c0, sv, mv);
    }
  }
  if constexpr (BWD) {
    __shared__ T part[GPB * LPD * NCH];
    __syncthreads();
    const uint32_t nl = n_long;
    for (uint32_t i = 0; i < nl; ++i) {
      const uint32_t d = long_rows[i];
      const uint32_t beg = off[d], end = off[d + 1], len = end - beg;
      const uint32_t pb = beg + (uint32_t)(((uint64_t)len * grp) / GPB);
      const uint32_t pe = beg + (uint32_t)(((uint64_t)len * (grp + 1)) / GPB);
      for (uint32_t c0 = 0; c0 < nv; c0 += LPD * NCH) {
        T acc[NCH], sv[NCH], mv[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] = rzero<VEC>();
        if (grp == 0) side_rows(d, c0, sv, mv);
        root_edges<VEC, LPD, NCH, U, false>(acc, pb, pe, c0, sl, idx, w, x, ldx, nullptr, nv);
#pragma unroll
        for (int c = 0; c < NCH; ++c) part[(grp * NCH + c) * LPD + sl] = acc[c];
        __syncthreads();
        if (grp == 0) {
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            T s = part[c * LPD + sl];
            for (int g = 1; g < GPB; ++g) {
              const T q = part[(g * NCH + c) * LPD + sl];
#pragma unroll
              for (int k = 0; k < VEC; ++k) rcomp<VEC>(s, k) = rcomp<VEC>(s, k) + rcomp<VEC>(q, k);
            }
            acc[c] = s;
          }
          finish(acc, d, c0, sv, mv);
        }
        __syncthreads();
      }
    }
  }
}

__global__ void k_root_fill(uint32_t* __restrict__ out, const uint32_t* __restrict__ n_dev,
                            uint32_t n_cap) {
  const uint32_t n = min(*n_dev, n_cap);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = kNone;
}
// dst_local_id is one-to-one: every slot has at most one writer
__global__ void k_root_scatter(uint32_t* __restrict__ out, const uint32_t* __restrict__ dst_local,
                               const uint32_t* __restrict__ v_dev, uint32_t v_cap,
                               const uint32_t* __restrict__ s_dev, uint32_t s_cap) {
  const uint32_t v = min(*v_dev, v_cap), s = min(*s_dev, s_cap);
  for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < v; d += gridDim.x * blockDim.x) {
    const uint32_t loc = dst_local[d];
    if (loc < s) out[loc] = d;
  }
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

// the widest vector every row start of both halves allows
int strict_vec(uint32_t F, std::initializer_list<uint64_t> lds, std::initializer_list<const void*> ps) {
  for (int vec = 4; vec > 1; vec /= 2) {
    bool ok = F % vec == 0;
    for (uint64_t ld : lds) ok = ok && ld % vec == 0;
    for (const void* p : ps) ok = ok && (p == nullptr || aligned(p, 4 * vec));
    if (ok) return vec;
  }
  return 1;
}

struct RShape {
  int lpd, nch;
};
// nts_hip_spmm_csr_bwd's choices (aggregate.hip: pick_shape, gather_u, plain_vec)
RShape root_shape(uint32_t nv) {
  if (nv <= 8) return {8, 1};
  if (nv <= 16) return {16, 1};
  if (nv <= 32) return {32, 1};
  return {64, (int)std::min<uint32_t>((nv + 63) / 64, 8)};
}
constexpr int root_u(int floats_per_lane) {
  return floats_per_lane <= 4 ? 8 : floats_per_lane <= 12 ? 5 : 4;
}
int gather_vec(uint32_t F, uint64_t ldx, uint64_t ldy, const void* x, const void* y) {
  int vec = strict_vec(F, {ldx, ldy}, {x, y});
  const uint32_t F4 = (F + 3) / 4 * 4;
  if (vec < 4 && F4 <= ldx && F4 <= ldy && ldx % 4 == 0 && ldy % 4 == 0 && aligned(x, 16) &&
      aligned(y, 16))
    vec = 4;
  return vec;
}

template <int VEC, bool MAP, bool BWD>
int launch_root(hipStream_t st, RShape s, uint32_t grid, const uint32_t* off, const uint32_t* idx,
                const float* w, const uint32_t* n_dev, uint32_t n_cap, const float* x,
                uint64_t ldx, const uint32_t* map, const uint32_t* self, uint32_t nv, float* y,
                uint64_t ldy, const float* mx, uint64_t ldm, float scale, uint32_t long_row) {
#define NTS_R(LPD, NCH)                                                                        \
  hipLaunchKernelGGL((k_root<VEC, LPD, NCH, root_u(VEC * NCH), MAP, BWD>), dim3(grid),         \
                     dim3(kRootThreads), 0, st, off, idx, w, n_dev, n_cap, x, ldx, map, self,  \
                     nv, y, ldy, mx, ldm, scale, long_row)
  if (s.lpd == 8) NTS_R(8, 1);
  else if (s.lpd == 16) NTS_R(16, 1);
  else if (s.lpd == 32) NTS_R(32, 1);
  else switch (s.nch) {
      case 1: NTS_R(64, 1); break;
      case 2: NTS_R(64, 2); break;
      case 3: NTS_R(64, 3); break;
      case 4: NTS_R(64, 4); break;
      case 5: NTS_R(64, 5); break;
      case 6: NTS_R(64, 6); break;
      case 7: NTS_R(64, 7); break;
      default: NTS_R(64, 8); break;
    }
#undef NTS_R
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

template <bool MAP, bool BWD>
int launch_root_any(int vec, hipStream_t st, RShape s, uint32_t grid, const uint32_t* off,
                    const uint32_t* idx, const float* w, const uint32_t* n_dev, uint32_t n_cap,
                    const float* x, uint64_t ldx, const uint32_t* map, const uint32_t* self,
                    uint32_t F, float* y, uint64_t ldy, const float* mx, uint64_t ldm,
                    float scale, uint32_t long_row) {
  const uint32_t nv = F / vec;
  if (vec == 4)
    return launch_root<4, MAP, BWD>(st, s, grid, off, idx, w, n_dev, n_cap, x, ldx, map, self, nv,
                                    y, ldy, mx, ldm, scale, long_row);
  if (vec == 2)
    return launch_root<2, MAP, BWD>(st, s, grid, off, idx, w, n_dev, n_cap, x, ldx, map, self, nv,
                                    y, ldy, mx, ldm, scale, long_row);
  return launch_root<1, MAP, BWD>(st, s, grid, off, idx, w, n_dev, n_cap, x, ldx, map, self, nv, y,
                                  ldy, mx, ldm, scale, long_row);
}

}  // namespace root
}  // namespace nts_hip

using namespace nts_hip;
using namespace nts_hip::root;

extern "C" {

int nts_hip_spmm_csc_fwd_root(nts_hip_ctx* ctx, const uint32_t* column_offset,
                              const uint32_t* row_indices, const float* weight, const uint32_t* v,
                              uint32_t v_cap, const float* x, uint64_t ldx,
                              const uint32_t* x_row_map, const uint32_t* self_index,
                              uint32_t feature_size, float* ycat, uint64_t ld_ycat) {
  NTS_CHECK_ARG(ctx && column_offset && row_indices && v && x && self_index && ycat,
                "NULL argument");
  NTS_CHECK_ARG(feature_size > 0, "feature_size is 0");
  NTS_CHECK_ARG(ldx >= feature_size, "leading dimension < feature_size");
  NTS_CHECK_ARG(ld_ycat >= 2 * (uint64_t)feature_size, "ld_ycat < 2 feature_size");
  if (v_cap == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const int vec = strict_vec(feature_size, {ldx, ld_ycat}, {x, ycat});
  const RShape s = root_shape(feature_size / vec);
  const uint32_t grid = std::max(1u, ceil_div(v_cap, kRootThreads / s.lpd));
  if (x_row_map)
    return launch_root_any<true, false>(vec, ctx->stream, s, grid, column_offset, row_indices,
                                        weight, v, v_cap, x, ldx, x_row_map, self_index,
                                        feature_size, ycat, ld_ycat, nullptr, 0, 1.f, 0);
  return launch_root_any<false, false>(vec, ctx->stream, s, grid, column_offset, row_indices,
                                       weight, v, v_cap, x, ldx, nullptr, self_index, feature_size,
                                       ycat, ld_ycat, nullptr, 0, 1.f, 0);
}

int nts_hip_root_inverse_map(nts_hip_ctx* ctx, const uint32_t* dst_local_id, const uint32_t* v,
                             uint32_t v_cap, const uint32_t* s, uint32_t s_cap,
                             uint32_t* src_dst) {
  NTS_CHECK_ARG(ctx && dst_local_id && v && s && src_dst, "NULL argument");
  if (s_cap == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_root_fill, dim3(std::min(ceil_div(s_cap, 256), kMaxGrid)), dim3(256), 0,
                     ctx->stream, src_dst, s, s_cap);
  NTS_LAUNCH_CHECK();
  if (v_cap == 0) return NTS_OK;
  hipLaunchKernelGGL(k_root_scatter, dim3(std::min(ceil_div(v_cap, 256), kMaxGrid)), dim3(256), 0,
                     ctx->stream, src_dst, dst_local_id, v, v_cap, s, s_cap);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

int nts_hip_spmm_csr_bwd_root(nts_hip_ctx* ctx, const uint32_t* row_offset,
                              const uint32_t* column_indices, const float* weight_backward,
                              const uint32_t* s, uint32_t s_cap, const float* g_ycat,
                              uint64_t ld_g, const uint32_t* src_dst, const float* x_act,
                              uint64_t ld_act, float scale, uint32_t feature_size, float* g_in,
                              uint64_t ld_gin) {
  NTS_CHECK_ARG(ctx && row_offset && column_indices && s && g_ycat && src_dst && g_in,
                "NULL argument");
  NTS_CHECK_ARG(feature_size > 0, "feature_size is 0");
  NTS_CHECK_ARG(ld_g >= 2 * (uint64_t)feature_size, "ld_ycat < 2 feature_size");
  NTS_CHECK_ARG(ld_gin >= feature_size && (!x_act || ld_act >= feature_size),
                "leading dimension < feature_size");
  if (s_cap == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  // the lane-group shape and long-row rule of nts_hip_spmm_csr_bwd on the same
  // operands; this kernel's own vectors also need the right half aligned
  const int ref_vec = gather_vec(feature_size, ld_g, ld_gin, g_ycat, g_in);
  const RShape sh = root_shape((feature_size + ref_vec - 1) / ref_vec);
  const uint32_t long_row = 4u * (uint32_t)root_u(ref_vec * sh.nch);
  const int vec = x_act ? strict_vec(feature_size, {ld_g, ld_gin, ld_act}, {g_ycat, g_in, x_act})
                        : strict_vec(feature_size, {ld_g, ld_gin}, {g_ycat, g_in});
  const uint32_t grid = std::max(1u, ceil_div(s_cap, kRootThreads / sh.lpd));
  return launch_root_any<false, true>(vec, ctx->stream, sh, grid, row_offset, column_indices,
                                      weight_backward, s, s_cap, g_ycat, ld_g, nullptr, src_dst,
                                      feature_size, g_in, ld_gin, x_act, ld_act,
                                      x_act ? scale : 1.f, long_row);
}

}  // extern "C"
