// Helpers shared by the attention kernels (gat.hip, gatv2.hip): the vector
// types, the dropout keep bits, the segmented per-head wave
// reductions (§8i) and the host side of the entry points: the shape / rate
// checks, the float4 rule, the typed kernel dispatch and the launch.
#pragma once
#include <initializer_list>
#include <optional>
#include <type_traits>

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

// What lane j of a chunk of ne edges holds (a row index, an edge id), in every
// lane; past the chunk's end the last lane's, a valid index the caller masks.
__device__ __forceinline__ uint32_t chunk_get(uint32_t mine, uint32_t j, uint32_t ne) {
  return (uint32_t)__shfl((int)mine, (int)min(j, ne - 1), 64);
}

// ---- host side: checks, shapes and dispatch of the entry points -------------------
// argument check of an entry point: `fn` (in scope) is its name for the error text
#define GAT_CHECK(cond, msg)                                                \
  do {                                                                      \
    if (!(cond)) {                                                          \
      ::nts_hip::set_error("%s: invalid argument: %s", fn, msg);            \
      return NTS_ERR_INVALID;                                               \
    }                                                                       \
  } while (0)

static const char kGatRateMsg[] = "dropout probability must be in [0, 1]";

inline bool gat_rate_ok(float p) { return p >= 0.f && p <= 1.f; }  // (a NaN fails both)

// The dropout of an entry point `fn`: refused unless both rates are in [0, 1],
// empty when both are 0 (the plain kernels, the same launches as without the
// options).
inline int gat_drop(const char* fn, float p_attn, float p_out, uint64_t seed, uint64_t off_attn,
                    uint64_t off_out, std::optional<GatDrop>* out) {
  GAT_CHECK(gat_rate_ok(p_attn) && gat_rate_ok(p_out), kGatRateMsg);
  if (p_attn > 0.f || p_out > 0.f) {
    GatDrop dr;
    dr.thr_attn = dropout_threshold(p_attn);
    dr.thr_out = dropout_threshold(p_out);
    dr.scale_attn = p_attn >= 1.f ? 0.f : 1.0f / (1.0f - p_attn);
    dr.scale_out = p_out >= 1.f ? 0.f : 1.0f / (1.0f - p_out);
    dr.seed = seed;
    dr.off_attn = off_attn;
    dr.off_out = off_out;
    *out = dr;
  }
  return NTS_OK;
}
inline const GatDrop* gat_drop_ptr(const std::optional<GatDrop>& dr) { return dr ? &*dr : nullptr; }

// The float4 path: the per-head (or single-head) width a multiple of 4 and
// every operand on a 16-byte base with a pitch (in floats; 0: one row) that is a
// multiple of 4.
struct GatOperand {
  const void* p;
  uint64_t ld;
};
inline bool gat_vec4(uint32_t D, std::initializer_list<GatOperand> ops) {
  bool ok = D % 4 == 0;
  for (const GatOperand& o : ops) ok = ok && o.ld % 4 == 0 && ((uintptr_t)o.p % 16) == 0;
  return ok;
}

static const char kGatHeadsWidthMsg[] =
    "feature width too large (F = heads * D <= 1024 on 16-byte aligned rows with pitches that "
    "are multiples of 4 and D a multiple of 4, F <= 256 otherwise)";

struct HeadsShape {
  uint32_t nvec, g;
  int nch, mode;
};
// the shape of a (heads, D) layer on the float4 (v4) or the scalar path
inline HeadsShape heads_shape(uint32_t heads, uint32_t D, bool v4) {
  HeadsShape s;
  s.g = v4 ? D / 4 : D;
  s.nvec = heads * s.g;
  s.nch = (int)((s.nvec + 63) / 64);
  s.mode = (s.g < 64 && (s.g & (s.g - 1)) == 0) ? kHeadsPow2
           : s.g % 64 == 0                      ? kHeadsChunk
                                                : kHeadsAny;
  return s;
}

// the checks every multi-head entry point `fn` starts with, and its shape once
// the path is known (at most 4 vectors per lane)
inline int gat_heads_check(const char* fn, uint32_t heads, uint32_t D) {
  GAT_CHECK(heads >= 1 && D >= 1, "heads must be >= 1 and D >= 1");
  GAT_CHECK((uint64_t)heads * D <= 1024, kGatHeadsWidthMsg);
  return NTS_OK;
}
inline int gat_heads_shape(const char* fn, uint32_t heads, uint32_t D, bool v4, HeadsShape* hs) {
  *hs = heads_shape(heads, D, v4);
  GAT_CHECK(hs->nch <= 4, kGatHeadsWidthMsg);
  return NTS_OK;
}

// one wave per row, kGatThreads / 64 rows a block
inline dim3 gat_grid(uint32_t rows) { return dim3(std::max(1u, ceil_div(rows, kGatThreads / 64))); }
// mean mode of the multi-head forward: one row of nch * 64 vectors per wave
// (16 KiB a block at VEC 4, NCH 4); none in concat mode
inline size_t gat_mean_lds(int mean, int nch, bool v4) {
  return mean ? (size_t)(kGatThreads / 64) * nch * 64 * (v4 ? 16 : 4) : 0;
}

// The run-time (v4, nch[, mode]) as compile-time constants: f(V, N[, M]) is
// called with std::integral_constants, so a generic lambda can name
// KERNEL<V(), N(), M()>; its status is returned.  nch is 1 ... 4 (checked by
// the caller), mode one of kHeads*.
template <int I>
using GatInt = std::integral_constant<int, I>;

template <class F>
int gat_dispatch(bool v4, int nch, F&& f) {
  auto chunks = [&](auto V) {
    switch (nch) {
      case 1: return f(V, GatInt<1>());
      case 2: return f(V, GatInt<2>());
      case 3: return f(V, GatInt<3>());
      default: return f(V, GatInt<4>());
    }
  };
  return v4 ? chunks(GatInt<4>()) : chunks(GatInt<1>());
}
template <class F>
int gat_dispatch(bool v4, int nch, int mode, F&& f) {
  return gat_dispatch(v4, nch, [&](auto V, auto N) {
    switch (mode) {
      case kHeadsPow2: return f(V, N, GatInt<kHeadsPow2>());
      case kHeadsChunk: return f(V, N, GatInt<kHeadsChunk>());
      default: return f(V, N, GatInt<kHeadsAny>());
    }
  });
}

// One launch of kGatThreads-wide blocks and its check: the plain kernel, or
// with a dropout its <..., true, GatDrop> form, which takes *dr last.  The
// kernels' trailing pack DR is what lets k<V, N> (DR empty) and
// k<V, N, true, GatDrop> deduce P... here.
template <class... P, class... A>
int gat_launch(void (*plain)(P...), void (*drop)(P..., GatDrop), dim3 grid, size_t lds,
               hipStream_t st, const GatDrop* dr, A... args) {
  if (!dr)
    hipLaunchKernelGGL(plain, grid, dim3(kGatThreads), lds, st, args...);
  else
    hipLaunchKernelGGL(drop, grid, dim3(kGatThreads), lds, st, args..., *dr);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

}  // namespace nts_hip
