// Helpers shared by the attention kernels (gat.hip, gatv2.hip): the vector
// types, the dropout keep bits, the segmented per-head wave
// reductions (§8i) and the host-side shape / rate checks and dispatch macros.
#pragma once
#include "common.hpp"

namespace nts_hip {

constexpr int kGatThreads = 256;  // 4 waves, one destination / source each
constexpr int kGatU = 4;          // neighbour rows in flight per wave

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

template <int VEC>
struct GV;
template <>
struct GV<1> {
  using T = float;
  __device__ static T zero() { return 0.f; }
  __device__ static float dot(T a, T b) { return a * b; }
  __device__ static T axpy(T acc, float w, T x) { return acc + w * x; }
  __device__ static T scale(T x, float s) { return x * s; }
  __device__ static T relu(T x) { return x > 0.f ? x : 0.f; }
  __device__ static T mask(T g, T y) { return y > 0.f ? g : 0.f; }
};
template <>
struct GV<4> {
  using T = float4;
  __device__ static T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ static float dot(T a, T b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
  __device__ static T axpy(T acc, float w, T x) {
    return make_float4(acc.x + w * x.x, acc.y + w * x.y, acc.z + w * x.z, acc.w + w * x.w);
  }
  __device__ static T scale(T x, float s) { return make_float4(x.x * s, x.y * s, x.z * s, x.w * s); }
  __device__ static T relu(T x) {
    return make_float4(x.x > 0.f ? x.x : 0.f, x.y > 0.f ? x.y : 0.f, x.z > 0.f ? x.z : 0.f,
                       x.w > 0.f ? x.w : 0.f);
  }
  __device__ static T mask(T g, T y) {
    return make_float4(y.x > 0.f ? g.x : 0.f, y.y > 0.f ? g.y : 0.f, y.z > 0.f ? g.z : 0.f,
                       y.w > 0.f ? g.w : 0.f);
  }
};

__device__ __forceinline__ float leaky(float u) { return u > 0.f ? u : 0.2f * u; }

// ---- dropout forms ------------------------------------------------
// Every kernel below has a `DROP` flag and an optional trailing GatDrop
// argument (the pack DR: empty or GatDrop).  KERNEL<VEC, NCH[, MODE]> is the
// plain kernel, signature and code as without the flag (the dropout code is
// compiled out); KERNEL<..., true, GatDrop> adds the two dropouts of a GAT
// recipe, both from the shared keep bits of common.hpp:
//   attention  edge e of head h is kept iff the bit of element (row = CSC edge
//              position e, col = h) at off_attn is set; the softmax still sums
//              over all edges (a stays the undropped softmax), the aggregate
//              takes the kept ones, scaled by 1 / (1 - p_attn);
//   output     element (d, col) of the written Y at off_out, after the relu.
// The backward regenerates the attention bits (no mask is stored); the output
// mask is Y > 0 itself.  A threshold of 0 draws nothing.
struct GatDrop {
  uint32_t thr_attn = 0, thr_out = 0;  // dropout_threshold of the two rates
  float scale_attn = 1.f, scale_out = 1.f;
  uint64_t seed = 0, off_attn = 0, off_out = 0;
};

__device__ __forceinline__ GatDrop drop_of() { return GatDrop(); }
__device__ __forceinline__ const GatDrop& drop_of(const GatDrop& dr) { return dr; }

__device__ __forceinline__ uint32_t row_word(const uint4& r, uint32_t row) {
  return (row & 2u) ? ((row & 1u) ? r.w : r.z) : ((row & 1u) ? r.y : r.x);
}

// single head: is CSC edge e kept
__device__ __forceinline__ bool edge_kept(uint32_t e, const GatDrop& dr) {
  if (!dr.thr_attn) return true;
  return dropout_bits(row_word(dropout_words(e, 0u, dr.seed, dr.off_attn), e), 0u) >= dr.thr_attn;
}

// K heads: the keep bits of CSC edge e, bit h % 64 of kb[h / 64].  One generator
// call gives heads 2 hp and 2 hp + 1 (word e % 4 of its 4-edge x 2-head block:
// e is the global edge position).  The head of vector column col is at most
// col, so NW = NCH words hold every head of the row.
template <int NW>
__device__ __forceinline__ void edge_keep_bits(uint64_t (&kb)[NW], uint32_t e, uint32_t heads,
                                               const GatDrop& dr) {
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    kb[w] = ~0ull;
    if (!dr.thr_attn) continue;
    kb[w] = 0ull;
    const uint32_t hp_end = min((heads + 1u) >> 1, 32u * (w + 1));
    for (uint32_t hp = 32u * w; hp < hp_end; ++hp) {
      const uint32_t wd = row_word(dropout_words(e, 2u * hp, dr.seed, dr.off_attn), e);
      const uint64_t two = (uint64_t)((wd & 0xFFFFu) >= dr.thr_attn) |
                           ((uint64_t)((wd >> 16) >= dr.thr_attn) << 1);
      kb[w] |= two << (2u * (hp & 31u));
    }
  }
}
// the owner lane's bits in every lane (the words past the last head are not moved)
template <int NW>
__device__ __forceinline__ void keep_bits_from(uint64_t (&kj)[NW], const uint64_t (&kb)[NW],
                                               int src_lane, uint32_t heads) {
#pragma unroll
  for (int w = 0; w < NW; ++w)
    kj[w] = (uint32_t)(64 * w) < heads ? __shfl(kb[w], src_lane, 64) : 0ull;
}
// head h's bit; c: the chunk of the asking vector column (h / 64 <= c)
template <int NW>
__device__ __forceinline__ bool head_kept(const uint64_t (&kj)[NW], uint32_t h, int c) {
  uint64_t w = kj[0];
#pragma unroll
  for (int i = 1; i < NW; ++i)
    if (i <= c && (h >> 6) == (uint32_t)i) w = kj[i];
  return (w >> (h & 63u)) & 1ull;
}

// output dropout of the vector at (row d, vector column col) of the written Y
template <int VEC>
__device__ __forceinline__ typename GV<VEC>::T out_drop(typename GV<VEC>::T v, uint32_t d,
                                                        uint32_t col, const GatDrop& dr) {
  if constexpr (VEC == 1) {
    const uint32_t wd = row_word(dropout_words(d, col, dr.seed, dr.off_out), d);
    return dropout_bits(wd, col) >= dr.thr_out ? v * dr.scale_out : 0.f;
  } else {  // scalar columns 4 col ... 4 col + 3: two column pairs
    const uint32_t w0 = row_word(dropout_words(d, 4u * col, dr.seed, dr.off_out), d);
    const uint32_t w1 = row_word(dropout_words(d, 4u * col + 2u, dr.seed, dr.off_out), d);
    return make_float4((w0 & 0xFFFFu) >= dr.thr_out ? v.x * dr.scale_out : 0.f,
                       (w0 >> 16) >= dr.thr_out ? v.y * dr.scale_out : 0.f,
                       (w1 & 0xFFFFu) >= dr.thr_out ? v.z * dr.scale_out : 0.f,
                       (w1 >> 16) >= dr.thr_out ? v.w * dr.scale_out : 0.f);
  }
}

// ---- multi-head reductions (the layout is described in gat.hip) -------------------
enum { kHeadsPow2 = 0, kHeadsChunk = 1, kHeadsAny = 2 };

// p[u][c]: this lane's partial dot product of row u in chunk c.  On return
// p[u][c] is the sum over the whole head of (lane, c), in every lane of it.
template <int MODE, int NCH, int U>
__device__ __forceinline__ void head_sums(float (&p)[U][NCH], const uint32_t (&hc)[NCH],
                                          uint32_t g, uint32_t heads) {
  if (MODE == kHeadsPow2) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
      if ((uint32_t)o < g) {  // wave-uniform
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int c = 0; c < NCH; ++c) p[u][c] += __shfl_xor(p[u][c], o, 64);
      }
  } else if (MODE == kHeadsChunk) {
    float q[U][NCH];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        q[u][c] = 0.f;
#pragma unroll
        for (int c2 = 0; c2 < NCH; ++c2)
          if (hc[c2] == hc[c]) q[u][c] += p[u][c2];  // wave-uniform: 64 | g
      }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < NCH; ++c) q[u][c] += __shfl_xor(q[u][c], o, 64);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < NCH; ++c) p[u][c] = q[u][c];
  } else {
    float q[U][NCH];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < NCH; ++c) q[u][c] = 0.f;
    for (uint32_t h = 0; h < heads; ++h) {
      float t[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        t[u] = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) t[u] += hc[c] == h ? p[u][c] : 0.f;
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] += __shfl_xor(t[u], o, 64);
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < NCH; ++c)
          if (hc[c] == h) q[u][c] = t[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < NCH; ++c) p[u][c] = q[u][c];
  }
}

[[maybe_unused]] static bool gat_vec4(uint32_t F, uint64_t l1, uint64_t l2, const void* p1, const void* p2,
                     const void* att) {
  return F % 4 == 0 && l1 % 4 == 0 && l2 % 4 == 0 && ((uintptr_t)p1 % 16) == 0 &&
         ((uintptr_t)p2 % 16) == 0 && ((uintptr_t)att % 16) == 0;
}

// argument check of an entry point: `fn` (in scope) is its name for the error text
#define GAT_CHECK(cond, msg)                                                \
  do {                                                                      \
    if (!(cond)) {                                                          \
      ::nts_hip::set_error("%s: invalid argument: %s", fn, msg);            \
      return NTS_ERR_INVALID;                                               \
    }                                                                       \
  } while (0)

static const char kGatRateMsg[] = "dropout probability must be in [0, 1]";

namespace {
bool gat_rate_ok(float p) { return p >= 0.f && p <= 1.f; }  // (a NaN fails both)
GatDrop gat_drop(float p_attn, float p_out, uint64_t seed, uint64_t off_attn, uint64_t off_out) {
  GatDrop dr;
  dr.thr_attn = dropout_threshold(p_attn);
  dr.thr_out = dropout_threshold(p_out);
  dr.scale_attn = p_attn >= 1.f ? 0.f : 1.0f / (1.0f - p_attn);
  dr.scale_out = p_out >= 1.f ? 0.f : 1.0f / (1.0f - p_out);
  dr.seed = seed;
  dr.off_attn = off_attn;
  dr.off_out = off_out;
  return dr;
}
}  // namespace

// The tail of a kernel's template arguments: none for the plain kernel,
// GAT_T_DROP with `*dr` as the last argument.  The single-head dispatch takes
// it as TAIL, the multi-head macros read GAT_T where they are used.
#define GAT_T_NONE
#define GAT_T_DROP , true, GatDrop

static const char kGatHeadsWidthMsg[] =
    "feature width too large (F = heads * D <= 1024 on 16-byte aligned rows with pitches that "
    "are multiples of 4 and D a multiple of 4, F <= 256 otherwise)";

namespace {
struct HeadsShape {
  uint32_t nvec, g;
  int nch, mode;
};
// the shape of a (heads, D) layer on the float4 (v4) or the scalar path
HeadsShape heads_shape(uint32_t heads, uint32_t D, bool v4) {
  HeadsShape s;
  s.g = v4 ? D / 4 : D;
  s.nvec = heads * s.g;
  s.nch = (int)((s.nvec + 63) / 64);
  s.mode = (s.g < 64 && (s.g & (s.g - 1)) == 0) ? kHeadsPow2
           : s.g % 64 == 0                      ? kHeadsChunk
                                                : kHeadsAny;
  return s;
}
}  // namespace

#define NTS_GAT_HEADS_NCH(KERNEL, V, ...)                                                       \
  switch (hs.nch) {                                                                             \
    case 1: hipLaunchKernelGGL((KERNEL<V, 1, __VA_ARGS__ GAT_T>), grid, dim3(kGatThreads), lds, st, ARGS); break; \
    case 2: hipLaunchKernelGGL((KERNEL<V, 2, __VA_ARGS__ GAT_T>), grid, dim3(kGatThreads), lds, st, ARGS); break; \
    case 3: hipLaunchKernelGGL((KERNEL<V, 3, __VA_ARGS__ GAT_T>), grid, dim3(kGatThreads), lds, st, ARGS); break; \
    default: hipLaunchKernelGGL((KERNEL<V, 4, __VA_ARGS__ GAT_T>), grid, dim3(kGatThreads), lds, st, ARGS); break; \
  }
#define NTS_GAT_HEADS_MODE(KERNEL, V)                                     \
  switch (hs.mode) {                                                      \
    case kHeadsPow2: NTS_GAT_HEADS_NCH(KERNEL, V, kHeadsPow2) break;      \
    case kHeadsChunk: NTS_GAT_HEADS_NCH(KERNEL, V, kHeadsChunk) break;    \
    default: NTS_GAT_HEADS_NCH(KERNEL, V, kHeadsAny) break;               \
  }
// KERNEL<VEC, NCH, MODE> over n waves (hs, v4, st, lds and ARGS in scope)
#define NTS_GAT_HEADS_DISPATCH(KERNEL)                                    \
  do {                                                                    \
    const dim3 grid(std::max(1u, ceil_div(n, kGatThreads / 64)));         \
    if (v4) {                                                             \
      NTS_GAT_HEADS_MODE(KERNEL, 4)                                       \
    } else {                                                              \
      NTS_GAT_HEADS_MODE(KERNEL, 1)                                       \
    }                                                                     \
    NTS_LAUNCH_CHECK();                                                   \
  } while (0)

}  // namespace nts_hip
