// Sampled aggregation (CSC gather SpMM, CSR transpose gather, atomic scatter,
// the GraphSAGE root weight's graph op), row/label gathers and the fused Adam step.
//
// The aggregation is HBM-bound (~2 flop/B).  Layout: X/Y row-major
// fp32 [rows, ld]; one wave-group (LPD lanes) per destination row, each lane
// owning NCH vectors of VEC floats of the row; neighbour rows are fetched 4
// edges ahead so every lane keeps 4*NCH independent loads in flight.  The sum
// runs in CSC edge order as acc + x*w with contraction disabled: bit-identical
// to the reference's MiniBatchFuseOp/nts_comp (core/ntsBaseOp.hpp:546-562,
// `_mm256_add_ps(_mm256_mul_ps(source,w),destination)`) for the same sampCSC.
#include "agg_shape.hpp"

#pragma clang fp contract(off)

namespace nts_hip {

template <int VEC>
struct VT;
template <>
struct VT<1> {
  using T = float;
  __device__ static __forceinline__ T zero() { return 0.f; }
  __device__ static __forceinline__ T madd(T a, T x, float w) { return a + x * w; }
  __device__ static __forceinline__ T scale(T x, float w) { return x * w; }
  __device__ static __forceinline__ void st_nt(T* p, T v) { __builtin_nontemporal_store(v, p); }
  __device__ static __forceinline__ void st_part(T* p, T v, uint32_t) { st_nt(p, v); }
};
template <>
struct VT<2> {
  using T = float2;
  __device__ static __forceinline__ T zero() { return make_float2(0.f, 0.f); }
  __device__ static __forceinline__ T madd(T a, T x, float w) {
    return make_float2(a.x + x.x * w, a.y + x.y * w);
  }
  __device__ static __forceinline__ T scale(T x, float w) { return make_float2(x.x * w, x.y * w); }
  __device__ static __forceinline__ void st_nt(T* p, T v) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 u = {v.x, v.y};
    __builtin_nontemporal_store(u, reinterpret_cast<f2*>(p));
  }
  __device__ static __forceinline__ void st_part(T* p, T v, uint32_t) {  // 1 of 2 valid
    __builtin_nontemporal_store(v.x, reinterpret_cast<float*>(p));
  }
};
template <>
struct VT<4> {
  using T = float4;
  __device__ static __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ static __forceinline__ T madd(T a, T x, float w) {
    return make_float4(a.x + x.x * w, a.y + x.y * w, a.z + x.z * w, a.w + x.w * w);
  }
  __device__ static __forceinline__ T scale(T x, float w) {
    return make_float4(x.x * w, x.y * w, x.z * w, x.w * w);
  }
  __device__ static __forceinline__ void st_nt(T* p, T v) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 u = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(u, reinterpret_cast<f4*>(p));
  }
  __device__ static __forceinline__ void st_part(T* p, T v, uint32_t nvalid) {  // 1..3 valid
    float* q = reinterpret_cast<float*>(p);
    __builtin_nontemporal_store(v.x, q);
    if (nvalid > 1) __builtin_nontemporal_store(v.y, q + 1);
    if (nvalid > 2) __builtin_nontemporal_store(v.z, q + 2);
  }
};

// y[d, :] = sum_{e in [off[d], off[d+1])} w[e] * x[row(e), :]
// row(e) = MAP ? map[idx[e]] : idx[e];  w == nullptr -> weight 1.
// Per destination the LPD-lane group loads up to LPD edges' (row, weight) at
// once — one lane per edge, the map lookup included — and then fetches the
// neighbour rows U at a time (row ids broadcast by __shfl, the tail batch
// predicated), so a row costs off -> idx/map -> ceil(deg/U) row rounds of
// memory latency instead of two dependent loads per U edges plus a serial
// remainder.  The sum order is still the CSC edge order.
//
// TIER (two-tier feature table, load_feature_gpu_cache semantics,
// core/ntsFastSampler.hpp:263-317): x is the HBM cache of the hottest rows
// and tier.cmap[g] its slot for global row g, or kNotCached, in which case the
// row is read from the host-pinned table tier.host (zero-copy over the host
// link).  The per-edge id carries the tier in bit 31 (vertex ids < 2^31).
// host_local: the non-cached rows were staged by local src id (tier.host is
// then an HBM buffer [src_size, ldh], see nts_hip_stage_uncached_rows)
struct Tier {
  const uint32_t* cmap;
  const float* host;
  uint64_t ldh;
  int host_local;
};
constexpr uint32_t kNotCached = 0xFFFFFFFFu;
constexpr uint32_t kHostBit = 0x80000000u;

// MODE: what the gather computes around the weighted sum (MAP/TIER only with
// kAggPlain, MAP also with kAggRootFwd)
//   kAggPlain: y = A x
//   kAggAct:   y = dropout(relu(A x), p) — vertexForward's activation in the
//              epilogue, keep bits keyed exactly like the GEMM epilogue of
//              nts_hip_gemm_relu_dropout_f32 (dropout_words(row, col, seed, offset))
//   kAggMask:  y = A (x ⊙ [mx > 0] · scale) — that activation's backward fused
//              into the row loads (mx = the forward activation, same shape as x)
//   kAggPostMask: y = (A x) ⊙ [mx > 0] · scale with mx indexed by the OUTPUT
//              row (the activation backward applied to the gathered sum: the
//              graph-op backward feeding a transform-first bottom layer)
//   kAggColmax: kAggPlain, and per block the column maxima of |y| over the
//     block's output rows into row blockIdx.x of ax.cm_out (the f16
//     pair-table TN GEMM's per-chunk column scales, nts_hip_spmm_csr_bwd_colmax)
//   kAggRootFwd: the GraphSAGE root weight's forward (X' = act([A X | X_dst] W)):
//     y[d, 0:F] = (A x)[d] as kAggPlain, y[d, F:2F] = x[ax.self[d]] (MAP: a
//     global row, not looked up in map); F a multiple of VEC
//   kAggRootBwd (COOP): y[s] = mask_s ⊙ scale ((A x[:, 0:F])[s] + x[ax.self[s], F:2F])
//     with x = dYcat; the self row is added last and skipped where ax.self[s]
//     is kNotCached, the mask is ax.mx's row s as kAggPostMask's (ax.mx NULL:
//     none).  Rows above ax.long_row edges are the long ones: the threshold
//     nts_hip_spmm_csr_bwd takes for the same operands, whose float4 over pitch
//     padding this mode cannot follow (the right half starts at column F)
enum {
  kAggPlain = 0, kAggAct = 1, kAggMask = 2, kAggPostMask = 3, kAggColmax = 4, kAggRootFwd = 5,
  kAggRootBwd = 6
};
struct AggExtra {
  const float* mx = nullptr;
  uint64_t ldm = 0;
  float scale = 1.f;
  uint32_t keep_threshold = 0;
  uint64_t seed = 0, offset = 0;
  // per-block column maxima of the output (nts_hip_spmm_csr_bwd_colmax):
  // cm_out[b * F + col] = max over block b's rows d of |rs(d) y[d, col]|, float
  // bits, rs(d) = cm_rs[cm_map[d]] (cm_map NULL: cm_rs[d]; cm_rs NULL: 1)
  uint32_t* cm_out = nullptr;
  const float* cm_rs = nullptr;
  const uint32_t* cm_map = nullptr;
  // the activation's keep mask as bits (nts_hip_act_bits_words): kAggAct
  // writes them beside its output (bits_out), kAggPostMask reads them instead
  // of the output's rows (bits_in); ldb words per row
  uint32_t* bits_out = nullptr;
  const uint32_t* bits_in = nullptr;
  uint64_t ldb = 0;
  // the root modes (appended: the fields above keep their kernel-argument
  // offsets): the self row of every output row, and kAggRootBwd's long-row threshold
  const uint32_t* self = nullptr;
  uint32_t long_row = 0;
};

// Mask bits of a float4 row on LPD >= 32 lanes (one chunk of NCH float4 a
// lane): word (h NCH + c) 4 + q of a row holds, at bit b, whether component q
// of chunk c of lane 32 h + b is > 0 (h = 0 for 32-lane groups)
// (nts_hip_act_bits_words: (LPD / 32) NCH 4 words a row)

template <int VEC>
__device__ __forceinline__ float& vcomp(typename VT<VEC>::T& v, int q) {
  return reinterpret_cast<float*>(&v)[q];
}
template <int VEC>
__device__ __forceinline__ float vcomp(const typename VT<VEC>::T& v, int q) {
  return reinterpret_cast<const float*>(&v)[q];
}

// acc[c] += sum over the edges [beg, end) in edge order of w[e] * row(e)[col],
// col = c0 + sl + c * LPD (one LPD-lane group, see k_spmm_gather)
template <int VEC, int LPD, int NCH, bool MAP, int U, bool TIER, int MODE>
__device__ __forceinline__ void gather_edges(typename VT<VEC>::T (&acc)[NCH], uint32_t beg,
                                             uint32_t end, uint32_t c0, int sl,
                                             const uint32_t* __restrict__ idx,
                                             const float* __restrict__ w,
                                             const float* __restrict__ x, uint64_t ldx,
                                             const uint32_t* __restrict__ map, uint32_t nv,
                                             const Tier& tier, const AggExtra& ax) {
  using V = VT<VEC>;
  using T = typename V::T;
  for (uint32_t cb = beg; cb < end; cb += LPD) {
    const uint32_t ne = min(end - cb, (uint32_t)LPD);
    uint32_t my_r = 0;
    float my_w = 0.f;
    if ((uint32_t)sl < ne) {  // streamed once: do not keep in cache
      my_r = __builtin_nontemporal_load(idx + cb + sl);
      my_w = w ? __builtin_nontemporal_load(w + cb + sl) : 1.0f;
      const uint32_t loc = my_r;
      if (MAP) my_r = map[my_r];
      if (TIER) {
        const uint32_t slot = tier.cmap[my_r];
        my_r = slot != kNotCached ? slot : ((tier.host_local ? loc : my_r) | kHostBit);
      }
    }
    for (uint32_t j0 = 0; j0 < ne; j0 += U) {
      T xv[U][NCH];
      T mv[MODE == kAggMask ? U : 1][MODE == kAggMask ? NCH : 1];
      float ww[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const int src = (int)(j0 + j) & (LPD - 1);
        const uint32_t r = (uint32_t)__shfl((int)my_r, src, LPD);
        ww[j] = __shfl(my_w, src, LPD);
        const bool ok = j0 + j < ne;
        const T* xrow = reinterpret_cast<const T*>(
            TIER && (r & kHostBit) ? tier.host + (uint64_t)(r & ~kHostBit) * tier.ldh
                                   : x + (uint64_t)r * ldx);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const uint32_t col = c0 + sl + c * LPD;
          xv[j][c] = (ok && col < nv) ? xrow[col] : V::zero();
        }
        if constexpr (MODE == kAggMask) {
          const T* mrow = reinterpret_cast<const T*>(ax.mx + (uint64_t)r * ax.ldm);
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            const uint32_t col = c0 + sl + c * LPD;
            mv[j][c] = (ok && col < nv) ? mrow[col] : V::zero();
          }
        }
      }
      if constexpr (MODE == kAggMask) {  // dZ = dX ⊙ [X > 0] · scale
#pragma unroll
        for (int j = 0; j < U; ++j)
#pragma unroll
          for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
              float& g = vcomp<VEC>(xv[j][c], q);
              g = vcomp<VEC>(mv[j][c], q) > 0.f ? g * ax.scale : 0.f;
            }
      }
#pragma unroll
      for (int j = 0; j < U; ++j)
        if (j0 + j < ne) {
#pragma unroll
          for (int c = 0; c < NCH; ++c) acc[c] = V::madd(acc[c], xv[j][c], ww[j]);
        }
    }
  }
}

// The activation mask of output row d over a lane's NCH vectors (kAggPostMask,
// kAggRootBwd), dZ = dX ⊙ [X > 0] · scale: the floats of ax.mx's row d, or
// (BITS: float4 rows on LPD >= 32 lanes, where ax.bits_in is set) its keep bits
template <int VEC, int LPD, int NCH, bool BITS>
struct RowMask {
  static constexpr bool kBits = BITS && VEC == 4 && LPD >= 32;
  typename VT<VEC>::T m[NCH];
  uint4 b[kBits ? NCH : 1];
  bool bits;  // (uniform)
};
template <int VEC, int LPD, int NCH, bool BITS>
__device__ __forceinline__ void load_mask(RowMask<VEC, LPD, NCH, BITS>& rm, uint32_t d,
                                          uint32_t c0, int sl, uint32_t nv, const AggExtra& ax) {
  using T = typename VT<VEC>::T;
  rm.bits = false;
  if constexpr (RowMask<VEC, LPD, NCH, BITS>::kBits) {
    if (ax.bits_in) {
      rm.bits = true;
      const uint4* brow = reinterpret_cast<const uint4*>(ax.bits_in + (uint64_t)d * ax.ldb) +
                          (LPD == 64 ? (sl >> 5) : 0) * NCH;
#pragma unroll
      for (int c = 0; c < NCH; ++c) rm.b[c] = brow[c];
    }
  }
  if (!rm.bits) {
    const T* mrow = reinterpret_cast<const T*>(ax.mx + (uint64_t)d * ax.ldm);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint32_t col = c0 + sl + c * LPD;
      rm.m[c] = col < nv ? mrow[col] : VT<VEC>::zero();
    }
  }
}
template <int VEC>
__device__ __forceinline__ void mask_vec(typename VT<VEC>::T& a, const typename VT<VEC>::T& m,
                                         float scale) {
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    float& v = vcomp<VEC>(a, q);
    v = vcomp<VEC>(m, q) > 0.f ? v * scale : 0.f;
  }
}
template <int VEC, int LPD, int NCH, bool BITS>
__device__ __forceinline__ void apply_mask(typename VT<VEC>::T (&acc)[NCH],
                                           const RowMask<VEC, LPD, NCH, BITS>& rm, int sl,
                                           float scale) {
  if constexpr (RowMask<VEC, LPD, NCH, BITS>::kBits) {
    if (rm.bits) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const uint32_t wq[4] = {rm.b[c].x, rm.b[c].y, rm.b[c].z, rm.b[c].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float& v = vcomp<VEC>(acc[c], q);
          v = ((wq[q] >> (sl & 31)) & 1u) ? v * scale : 0.f;
        }
      }
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) mask_vec<VEC>(acc[c], rm.m[c], scale);
}

// epilogue of one output row: activation (kAggAct), the mask of a long row
// (kAggPostMask) and the store, non-temporal or (NT = false) plain
template <int VEC, int LPD, int NCH, int MODE, bool NT = true>
__device__ __forceinline__ void store_row(typename VT<VEC>::T (&acc)[NCH], uint32_t d, uint32_t c0,
                                          int sl, uint32_t nv, uint32_t last_valid,
                                          float* __restrict__ y, uint64_t ldy, const AggExtra& ax) {
  using V = VT<VEC>;
  using T = typename V::T;
  if constexpr (MODE == kAggAct) {  // relu + inverted dropout, mask never stored
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint32_t f0 = (c0 + sl + c * LPD) * VEC;  // first float column
#pragma unroll
      for (int q2 = 0; q2 < (VEC + 1) / 2; ++q2) {
        uint4 rnd = make_uint4(0u, 0u, 0u, 0u);
        if (ax.keep_threshold) rnd = dropout_words((uint64_t)d, f0 + 2 * q2, ax.seed, ax.offset);
        const uint32_t wd = (d & 3) == 0 ? rnd.x : (d & 3) == 1 ? rnd.y : (d & 3) == 2 ? rnd.z : rnd.w;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (2 * q2 + h >= VEC) break;
          const uint32_t col = f0 + 2 * q2 + h;
          float& v = vcomp<VEC>(acc[c], 2 * q2 + h);
          v = (dropout_bits(wd, col) >= ax.keep_threshold && v > 0.f) ? v * ax.scale : 0.f;
        }
      }
    }
    if constexpr (VEC == 4 && LPD >= 32) {
      if (ax.bits_out) {  // (uniform) the row's keep mask, one ballot per component
        const int hw = (threadIdx.x & 63) >> 5;
        uint32_t* brow = ax.bits_out + (uint64_t)d * ax.ldb + (LPD == 64 ? hw : 0) * NCH * 4;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          uint32_t wq[4];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            wq[q] = (uint32_t)(__ballot(vcomp<VEC>(acc[c], q) > 0.f) >> (32 * hw));
          if ((threadIdx.x & 31) == 0)
            *reinterpret_cast<uint4*>(brow + 4 * c) = make_uint4(wq[0], wq[1], wq[2], wq[3]);
        }
      }
    }
  }
  if constexpr (MODE == kAggPostMask) {
    // a long row, masked after its LDS sum.  The float mask is loaded vector
    // by vector as it is applied: nothing overlaps the load here, and the
    // whole row preloaded (load_mask) costs registers (occupancy 3 -> 2 at
    // four float4 chunks a lane)
    RowMask<VEC, LPD, NCH, true> rm;
    rm.bits = false;
    if constexpr (RowMask<VEC, LPD, NCH, true>::kBits) {
      if (ax.bits_in) {
        load_mask(rm, d, c0, sl, nv, ax);
        apply_mask(acc, rm, sl, ax.scale);
      }
    }
    if (!rm.bits) {
      const T* mrow = reinterpret_cast<const T*>(ax.mx + (uint64_t)d * ax.ldm);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const uint32_t col = c0 + sl + c * LPD;
        if (col < nv) mask_vec<VEC>(acc[c], mrow[col], ax.scale);
      }
    }
  }
  T* yrow = reinterpret_cast<T*>(y + (uint64_t)d * ldy);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {  // output rows are not re-read here: keep them
    const uint32_t col = c0 + sl + c * LPD;  // out of the cache that serves x rows
    if (col + 1 < nv || (col + 1 == nv && last_valid == (uint32_t)VEC)) {
      if constexpr (NT) V::st_nt(yrow + col, acc[c]);
      else yrow[col] = acc[c];
    } else if (col + 1 == nv) {  // partial last vector: only the valid floats
      V::st_part(yrow + col, acc[c], last_valid);
    }
  }
}

// COOP (the CSR transposes, whose rows are as long as a source is popular —
// hundreds of edges for the hubs of a power-law graph against ~6 on average):
// a row longer than kLongRow(U) edges is not summed by its own lane group,
// which would serialise ~len/U rounds of memory latency and set the whole
// launch's time; the block's GPB groups each sum a contiguous GPB-th of its
// edges (in edge order) and the partial sums are added in group order through
// LDS.  Deterministic; rows up to kLongRow edges keep the serial edge order
// (bit-identical to MiniBatchFuseOp::backward's), longer rows are summed as
// GPB in-order pieces.  A group takes at most kCoopRows rows (grid >=
// ceil(n_cap / (GPB kCoopRows))): the block's long rows fit its list.
// (kLongRow, kCoopRows: agg_shape.hpp)

// Each row's loads run off -> ids -> rows with nothing loaded ahead.  A row
// software pipeline (1: the next row's offsets; 2: the offsets two rows ahead
// and the first id / weight chunk one row ahead) measured, at C2 size with
// scripts/micro_agg.py, bottom fwd / CSR bwd 105.9 / 130.5 us (1) and
// 102.3 / 130.6 (2) against 103.7 / 121.7 without, and 114.4 / 152.1 with 2
// under a floor of 6 waves per SIMD (spills): the prefetch registers cost a
// wave per SIMD (occupancy 6 -> 5) and the gather needs the waves more than
// the shorter chain.
template <int VEC, int LPD, int NCH, bool MAP, int U, bool TIER, int MODE = kAggPlain,
          bool COOP = false>
__global__ __launch_bounds__(kAggThreads) void k_spmm_gather(
    const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx,
    const float* __restrict__ w, const uint32_t* n_dev, uint32_t n_cap,
    const float* __restrict__ x, uint64_t ldx, const uint32_t* __restrict__ map, uint32_t nv,
    float* __restrict__ y, uint64_t ldy, uint32_t last_valid, Tier tier, AggExtra ax) {
  using V = VT<VEC>;
  using T = typename V::T;
  constexpr bool CM = MODE == kAggColmax;
  constexpr bool ROOT = MODE == kAggRootFwd || MODE == kAggRootBwd;
  constexpr bool MASK = MODE == kAggPostMask || MODE == kAggRootBwd;  // of the output row
  static_assert(MODE == kAggPlain || (!TIER && (!MAP || MODE == kAggRootFwd)),
                "activation and backward modes gather local rows only");
  static_assert(MODE != kAggRootBwd || COOP, "the root backward follows the CSR backward's split");
  constexpr int EM = CM || ROOT ? kAggPlain : MODE;  // the gather and store proper
  // (the root modes keep the plain stores their timings in DESIGN §8g were
  // taken with; non-temporal ones have not been measured for them)
  constexpr bool NT = !ROOT;
  const uint32_t long_row = MODE == kAggRootBwd ? ax.long_row : kLongRow(U);
  const uint32_t n = n_dev ? min(*n_dev, n_cap) : n_cap;
  constexpr int GPB = kAggThreads / LPD;
  const int grp = threadIdx.x / LPD, sl = threadIdx.x % LPD;
  __shared__ uint32_t long_rows[COOP ? GPB * kCoopRows : 1];
  __shared__ uint32_t n_long;
  if (COOP) {
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
  }
  // kAggColmax: the block's column maxima in LDS (float bits; non-negative
  // floats order as their bits), one LDS atomic per lane and column per row
  const uint32_t ncol = (nv - 1) * VEC + last_valid;
  __shared__ uint32_t smax[CM ? 512 : 1];
  if constexpr (CM) {
    for (uint32_t c = threadIdx.x; c < ncol; c += kAggThreads) smax[c] = 0u;
    __syncthreads();
  }
  auto colmax_row = [&](const T (&acc)[NCH], uint32_t c0, uint32_t d) {
    // the row's scale (a power of two: the product is exact unless it leaves
    // the float range)
    const float rsd = ax.cm_rs ? ax.cm_rs[ax.cm_map ? ax.cm_map[d] : d] : 1.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        const uint32_t col = (c0 + sl + c * LPD) * VEC + q;
        if (col < ncol)
          atomicMax(&smax[col], __float_as_uint(fabsf(vcomp<VEC>(acc[c], q) * rsd)));
      }
  };
  // The rows known before the edges are — the output row's mask (MASK) and
  // the root modes' self row — are loaded ahead of the gather, so that their
  // latency overlaps it instead of following it
  struct Side {
    T self[ROOT ? NCH : 1];
    RowMask<VEC, LPD, NCH, MODE == kAggPostMask> rm;
  };
  auto load_side = [&](Side& sd, uint32_t d, uint32_t c0) {
    if constexpr (ROOT) {
      // forward: x[self] (a global row under MAP); backward: x[self, F:2F],
      // F = nv VEC, zeros where the row has no self term
      uint32_t sr = ax.self[d];
      const bool has = MODE == kAggRootFwd || sr != kNotCached;
      if (!has) sr = 0;
      const T* srow =
          reinterpret_cast<const T*>(x + (uint64_t)sr * ldx) + (MODE == kAggRootBwd ? nv : 0);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const uint32_t col = c0 + sl + c * LPD;
        sd.self[c] = (has && col < nv) ? srow[col] : V::zero();
      }
    }
    if constexpr (MASK) {
      if (MODE == kAggPostMask || ax.mx) load_mask(sd.rm, d, c0, sl, nv, ax);
    }
  };
  // one output row after its sum: the self term (one more add, last), the
  // mask, the store, the forward's self copy into columns [F, 2F), the maxima
  // (long: a long row's kAggPostMask is store_row's, loaded after the sum)
  auto finish = [&](T (&acc)[NCH], Side& sd, uint32_t d, uint32_t c0, auto long_row_tag) {
    constexpr bool LATE = MODE == kAggPostMask && decltype(long_row_tag)::value;
    if constexpr (MODE == kAggRootBwd) {
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int q = 0; q < VEC; ++q)
          vcomp<VEC>(acc[c], q) = vcomp<VEC>(acc[c], q) + vcomp<VEC>(sd.self[c], q);
    }
    if constexpr (MASK && !LATE) {
      if (MODE == kAggPostMask || ax.mx) apply_mask(acc, sd.rm, sl, ax.scale);
    }
    store_row<VEC, LPD, NCH, LATE ? kAggPostMask : EM == kAggPostMask ? kAggPlain : EM, NT>(
        acc, d, c0, sl, nv, last_valid, y, ldy, ax);
    if constexpr (MODE == kAggRootFwd)
      store_row<VEC, LPD, NCH, kAggPlain, NT>(sd.self, d, c0, sl, nv, last_valid,
                                              y + (uint64_t)nv * VEC, ldy, ax);
    if constexpr (CM) colmax_row(acc, c0, d);
  };
  const uint32_t stride = gridDim.x * GPB;
  for (uint32_t d = blockIdx.x * GPB + grp; d < n; d += stride) {
    const uint32_t beg = off[d], end = off[d + 1];
    if (COOP && end - beg > long_row) {  // summed by the whole block below
      if (sl == 0) long_rows[atomicAdd(&n_long, 1u)] = d;
      continue;
    }
    for (uint32_t c0 = 0; c0 < nv; c0 += LPD * NCH) {
      T acc[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) acc[c] = V::zero();
      Side sd;
      load_side(sd, d, c0);
      gather_edges<VEC, LPD, NCH, MAP, U, TIER, EM>(acc, beg, end, c0, sl, idx, w, x, ldx, map, nv,
                                                    tier, ax);
      finish(acc, sd, d, c0, std::false_type{});
    }
  }
  if constexpr (COOP) {
    __shared__ T part[GPB * LPD * NCH];
    __syncthreads();
    const uint32_t nl = n_long;  // the order rows are handled in does not matter
    for (uint32_t i = 0; i < nl; ++i) {
      const uint32_t d = long_rows[i];
      const uint32_t beg = off[d], end = off[d + 1], len = end - beg;
      const uint32_t pb = beg + (uint32_t)(((uint64_t)len * grp) / GPB);
      const uint32_t pe = beg + (uint32_t)(((uint64_t)len * (grp + 1)) / GPB);
      for (uint32_t c0 = 0; c0 < nv; c0 += LPD * NCH) {
        T acc[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] = V::zero();
        Side sd;
        if constexpr (ROOT) {
          if (grp == 0) load_side(sd, d, c0);
        }
        gather_edges<VEC, LPD, NCH, MAP, U, TIER, EM>(acc, pb, pe, c0, sl, idx, w, x, ldx, map,
                                                        nv, tier, ax);
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
              for (int k = 0; k < VEC; ++k) vcomp<VEC>(s, k) = vcomp<VEC>(s, k) + vcomp<VEC>(q, k);
            }
            acc[c] = s;
          }
          // (kAggPostMask: a long row's mask is loaded after its sum)
          finish(acc, sd, d, c0, std::true_type{});
        }
        __syncthreads();
      }
    }
  }
  if constexpr (CM) {  // the block's maxima -> its row of the per-block buffer
    __syncthreads();
    uint32_t* row = ax.cm_out + (uint64_t)blockIdx.x * ncol;
    for (uint32_t c = threadIdx.x; c < ncol; c += kAggThreads) row[c] = smax[c];
  }
}

// g_in[idx[e], :] += w[e] * g_out[d, :]   (float atomics, order not deterministic)
template <int VEC, int LPD>
__global__ __launch_bounds__(kAggThreads) void k_spmm_scatter_atomic(
    const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx,
    const float* __restrict__ w, const uint32_t* n_dev, uint32_t n_cap,
    const float* __restrict__ g, uint64_t ldg, uint32_t nv, float* __restrict__ gin,
    uint64_t ldgi) {
  using V = VT<VEC>;
  using T = typename V::T;
  const uint32_t n = n_dev ? min(*n_dev, n_cap) : n_cap;
  constexpr int GPB = kAggThreads / LPD;
  const int grp = threadIdx.x / LPD, sl = threadIdx.x % LPD;
  for (uint32_t d = blockIdx.x * GPB + grp; d < n; d += gridDim.x * GPB) {
    const uint32_t beg = off[d], end = off[d + 1];
    const T* grow = reinterpret_cast<const T*>(g + (uint64_t)d * ldg);
    for (uint32_t col = sl; col < nv; col += LPD) {
      const T gv = grow[col];
      for (uint32_t e = beg; e < end; ++e) {
        const float we = w ? w[e] : 1.0f;
        const T v = V::scale(gv, we);
        float* dst = gin + (uint64_t)idx[e] * ldgi + (uint64_t)col * VEC;
        const float* vs = reinterpret_cast<const float*>(&v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) unsafeAtomicAdd(dst + k, vs[k]);
      }
    }
  }
}

// out[i,:] = table[index[i],:]; TIER: table is the HBM cache, rows whose
// tier.cmap entry is kNotCached come from the host-pinned tier.host
// (zero_copy_feature_move_gpu_cache + gather_feature_from_gpu_cache,
// cuda/ntsCUDATransferKernel.cuh:154-183, in one pass).
// STAGE (with TIER): only the rows that are not cached are copied, out row i
// = host row index[i]; cached rows of `out` are left untouched.
template <int VEC, int LPD, bool TIER, bool STAGE = false>
__global__ __launch_bounds__(kAggThreads) void k_gather_rows(const float* __restrict__ table,
                                                            uint64_t ldt,
                                                            const uint32_t* __restrict__ index,
                                                            const uint32_t* n_dev, uint32_t n_cap,
                                                            uint32_t nv, float* __restrict__ out,
                                                            uint64_t ldo, Tier tier) {
  using T = typename VT<VEC>::T;
  const uint32_t n = n_dev ? min(*n_dev, n_cap) : n_cap;
  constexpr int GPB = kAggThreads / LPD;
  const int grp = threadIdx.x / LPD, sl = threadIdx.x % LPD;
  for (uint32_t i = blockIdx.x * GPB + grp; i < n; i += gridDim.x * GPB) {
    const uint32_t g = index[i];
    const uint32_t slot = TIER ? tier.cmap[g] : g;
    if (STAGE && slot != kNotCached) continue;  // group-uniform
    const T* src = reinterpret_cast<const T*>(
        TIER && slot == kNotCached ? tier.host + (uint64_t)g * tier.ldh
                                   : table + (uint64_t)slot * ldt);
    T* dst = reinterpret_cast<T*>(out + (uint64_t)i * ldo);
    for (uint32_t c = sl; c < nv; c += LPD) dst[c] = src[c];
  }
}

// out = g ⊙ [x > 0] · scale — the backward of dropout(relu(.)) given its
// output x (relu zeroes and dropped elements are exactly the zeros of x)
__global__ void k_act_backward(const float4* __restrict__ g, const float4* __restrict__ x,
                               float4* __restrict__ out, uint64_t n4, float scale) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const float4 a = g[i], b = x[i];
    out[i] = make_float4(b.x > 0.f ? a.x * scale : 0.f, b.y > 0.f ? a.y * scale : 0.f,
                         b.z > 0.f ? a.z * scale : 0.f, b.w > 0.f ? a.w * scale : 0.f);
  }
}
__global__ void k_act_backward_2d(const float* __restrict__ g, uint64_t ldg,
                                  const float* __restrict__ x, uint64_t ldx, float* __restrict__ out,
                                  uint64_t ldo, uint32_t rows, uint32_t F, float scale) {
  const uint64_t n = (uint64_t)rows * F;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = i / F, c = i % F;
    out[r * ldo + c] = x[r * ldx + c] > 0.f ? g[r * ldg + c] * scale : 0.f;
  }
}

__global__ void k_gather_labels(const int64_t* __restrict__ labels,
                                const uint32_t* __restrict__ index, const uint32_t* n_dev,
                                uint32_t n_cap, int64_t* __restrict__ out) {
  const uint32_t n = n_dev ? min(*n_dev, n_cap) : n_cap;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = labels[index[i]];
}

// src_dst[s] = the d with dst_local_id[d] == s, or kNotCached (the root
// backward's self index): fill, then scatter
__global__ void k_root_fill(uint32_t* __restrict__ out, const uint32_t* __restrict__ n_dev,
                            uint32_t n_cap) {
  const uint32_t n = min(*n_dev, n_cap);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = kNotCached;
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

// Adam, element-wise in the exact operation order of the reference's torch
// expressions (core/NtsScheduler.hpp:863-880 and :937-945).
__global__ void k_adam(float* __restrict__ W, const float* __restrict__ G, float* __restrict__ M,
                       float* __restrict__ Vv, uint64_t n, float alpha, float beta1, float beta2,
                       float eps, float wd, float beta1_t, float beta2_t, int bias_correction) {
  const float omb1 = 1.0f - beta1, omb2 = 1.0f - beta2;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const float w = W[i];
    if (bias_correction) {
      // W_g = W_gradient + weight_decay * S
      const float wg = G[i] + wd * w;
      const float m = beta1 * M[i] + omb1 * wg;
      const float v = beta2 * Vv[i] + omb2 * (wg * wg);
      M[i] = m;
      Vv[i] = v;
      const float mt = m / (1.0f - beta1_t);
      const float vt = v / (1.0f - beta2_t);
      W[i] = w - (alpha * mt) / (sqrtf(vt) + eps);
    } else {
      // W_g = W * weight_decay + W.grad();  V = b2*V + (1-b2)*W_g*W_g
      const float wg = w * wd + G[i];
      const float m = beta1 * M[i] + omb1 * wg;
      const float v = beta2 * Vv[i] + (omb2 * wg) * wg;
      M[i] = m;
      Vv[i] = v;
      W[i] = w - (alpha * m) / (sqrtf(v) + eps);
    }
  }
}


// ---------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------
// (row_vec, pick_shape, gather_u, kGatherGridCap: agg_shape.hpp)

template <int VEC, bool MAP, bool TIER, int MODE, bool COOP>
static int launch_gather_vec(hipStream_t st, uint32_t grid, uint32_t last_valid, Shape s,
                             const uint32_t* off,
                             const uint32_t* idx, const float* w, const uint32_t* n_dev,
                             uint32_t n_cap, const float* x, uint64_t ldx, const uint32_t* map,
                             uint32_t nv, float* y, uint64_t ldy, Tier tier, const AggExtra& ax) {
// rows in flight per lane group: 8 for narrow rows, 5 for mid-width rows
// (F ~ 600: 3 float4 per lane; fanout 10/25 -> full batches), 4 for the
// widest (register budget); the post-mask CSR gather takes the same counts
#define NTS_G(LPD, NCH)                                                                     \
  do {                                                                                      \
    constexpr int u = gather_u(VEC * NCH);                                                  \
    hipLaunchKernelGGL((k_spmm_gather<VEC, LPD, NCH, MAP, u, TIER, MODE, COOP>), dim3(grid), \
                       dim3(kAggThreads), 0, st, off, idx, w, n_dev, n_cap, x, ldx, map,   \
                       nv, y, ldy, last_valid, tier, ax);                                   \
  } while (0)
  if (s.lpd == 8) NTS_G(8, 1);
  else if (s.lpd == 16) NTS_G(16, 1);
  else if (s.lpd == 32) NTS_G(32, 1);
  else switch (s.nch) {
      case 1: NTS_G(64, 1); break;
      case 2: NTS_G(64, 2); break;
      case 3: NTS_G(64, 3); break;
      case 4: NTS_G(64, 4); break;
      case 5: NTS_G(64, 5); break;
      case 6: NTS_G(64, 6); break;
      case 7: NTS_G(64, 7); break;
      default: NTS_G(64, 8); break;
    }
#undef NTS_G
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

template <bool MAP, bool TIER = false, int MODE = kAggPlain, bool COOP = false>
static int launch_gather(hipStream_t st, const uint32_t* off, const uint32_t* idx,
                         const float* w, const uint32_t* n_dev, uint32_t n_cap, const float* x,
                         uint64_t ldx, const uint32_t* map, uint32_t F, float* y, uint64_t ldy,
                         Tier tier = Tier{nullptr, nullptr, 0, 0}, AggExtra ax = AggExtra(),
                         uint32_t expect_grid = 0) {
  // (the modes that mask, activate or place a second half at column F keep
  // to whole vectors)
  const bool pad = MODE == kAggPlain || MODE == kAggColmax;
  const int vec = row_vec(F, {{x, ldx}, {y, ldy}, {TIER ? tier.host : nullptr, tier.ldh},
                              {ax.bits_in ? nullptr : ax.mx, ax.ldm}}, pad);
  const uint32_t nv = (F + vec - 1) / vec;
  const uint32_t last_valid = F - (nv - 1) * vec;
  Shape s = pick_shape(nv);
  if (MODE == kAggRootBwd) {
    // the lane-group shape and the long-row threshold nts_hip_spmm_csr_bwd
    // takes for the same operands, so that every row is summed in its pieces;
    // where that call's vector is wider than this one the row takes more c0 rounds
    const int plain = row_vec(F, {{x, ldx}, {y, ldy}}, true);
    s = pick_shape((F + plain - 1) / plain);
    ax.long_row = kLongRow(gather_u(plain * s.nch));
  }
  const uint32_t gpb = kAggThreads / s.lpd;
  // One destination per lane group, every row's dependent loads (offsets ->
  // ids -> rows) in flight at once.  Fewer blocks with several rows per group
  // measured slower or no faster (C2: 1.069 vs 1.097 ms per step at 4096
  // blocks, the narrow CSR backward 50 -> ~25 us; the post-mask CSR gather
  // 44.7 / 44.6 / 51.7 us at 4096 / 8192 / 2048 blocks against 44.9), so the
  // cap only bounds the grid.  COOP: at most kCoopRows rows per lane group.
  const uint32_t grid = std::max({1u, std::min(ceil_div(n_cap, gpb), kGatherGridCap),
                                  COOP ? ceil_div(n_cap, gpb * kCoopRows) : 0u});
  // kAggColmax: the per-block buffer was sized for this grid
  NTS_CHECK_ARG(expect_grid == 0 || expect_grid == grid, "aggregation grid != the sized one");
  if (vec == 4)
    return launch_gather_vec<4, MAP, TIER, MODE, COOP>(st, grid, last_valid, s, off, idx, w, n_dev,
                                                 n_cap, x, ldx, map, nv, y, ldy, tier, ax);
  if (vec == 2)
    return launch_gather_vec<2, MAP, TIER, MODE, COOP>(st, grid, last_valid, s, off, idx, w, n_dev,
                                                 n_cap, x, ldx, map, nv, y, ldy, tier, ax);
  return launch_gather_vec<1, MAP, TIER, MODE, COOP>(st, grid, last_valid, s, off, idx, w, n_dev, n_cap,
                                               x, ldx, map, nv, y, ldy, tier, ax);
}


}  // namespace nts_hip

using namespace nts_hip;

extern "C" {

int nts_hip_spmm_csc_fwd(nts_hip_ctx* ctx, const uint32_t* column_offset,
                         const uint32_t* row_indices, const float* weight, const uint32_t* v,
                         uint32_t v_cap, const float* x, uint64_t ldx,
                         const uint32_t* x_row_map, uint32_t feature_size, float* y,
                         uint64_t ldy) {
  NTS_CHECK_ARG(ctx && column_offset && row_indices && x && y, "NULL argument");
  NTS_CHECK_ARG(ldx >= feature_size && ldy >= feature_size, "leading dimension < feature_size");
  if (v_cap == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  if (x_row_map)
    return launch_gather<true>(ctx->stream, column_offset, row_indices, weight, v, v_cap, x, ldx,
                               x_row_map, feature_size, y, ldy);
  return launch_gather<false>(ctx->stream, column_offset, row_indices, weight, v, v_cap, x, ldx,
                              nullptr, feature_size, y, ldy);
}

int nts_hip_spmm_csr_bwd(nts_hip_ctx* ctx, const uint32_t* row_offset,
                         const uint32_t* column_indices, const float* weight_backward,
                         const uint32_t* s, uint32_t s_cap, const float* g_out, uint64_t ld_gout,
                         uint32_t feature_size, float* g_in, uint64_t ld_gin) {
  NTS_CHECK_ARG(ctx && row_offset && column_indices && g_out && g_in, "NULL argument");
  NTS_CHECK_ARG(ld_gout >= feature_size && ld_gin >= feature_size,
                "leading dimension < feature_size");
  if (s_cap == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  return launch_gather<false, false, kAggPlain, true>(ctx->stream, row_offset, column_indices,
                                                      weight_backward, s, s_cap,
                              g_out, ld_gout, nullptr, feature_size, g_in, ld_gin);
}

uint32_t nts_hip_csr_bwd_colmax_rows_per_part(uint32_t feature_size) {
  if (feature_size == 0) return 0;
  // (the colmax gather always runs on float4 rows: vec 4)
  return (uint32_t)(kAggThreads / pick_shape((feature_size + 3) / 4).lpd);
}

int nts_hip_spmm_csr_bwd_colmax(nts_hip_ctx* ctx, const uint32_t* row_offset,
                                const uint32_t* column_indices, const float* weight_backward,
                                const uint32_t* s, uint32_t s_cap, const float* g_out,
                                uint64_t ld_gout, uint32_t feature_size, float* g_in,
                                uint64_t ld_gin, uint32_t* part_max, const float* row_scale,
                                const uint32_t* row_map) {
  NTS_CHECK_ARG(ctx && row_offset && column_indices && g_out && g_in && part_max, "NULL argument");
  NTS_CHECK_ARG(row_scale || !row_map, "row_map without row_scale");
  NTS_CHECK_ARG(ld_gout >= feature_size && ld_gin >= feature_size,
                "leading dimension < feature_size");
  NTS_CHECK_ARG(feature_size <= 512, "column maxima: at most 512 columns");
  if (s_cap == 0 || feature_size == 0) return NTS_OK;
  // the parts follow the COOP grid (one output row per lane group): the
  // float4 row shape nts_hip_csr_bwd_colmax_rows_per_part assumes
  NTS_CHECK_ARG(row_vec(feature_size, {{g_out, ld_gout}, {g_in, ld_gin}}, true) == 4,
                "column maxima: 16-byte aligned rows with ld % 4 == 0");
  const uint32_t rpp = nts_hip_csr_bwd_colmax_rows_per_part(feature_size);
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  AggExtra ax;
  ax.cm_out = part_max;
  ax.cm_rs = row_scale;
  ax.cm_map = row_map;
  return launch_gather<false, false, kAggColmax, true>(ctx->stream, row_offset, column_indices,
                                                       weight_backward, s, s_cap, g_out, ld_gout,
                                                       nullptr, feature_size, g_in, ld_gin,
                                                       Tier{nullptr, nullptr, 0, 0}, ax,
                                                       ceil_div(s_cap, rpp));
}

int nts_hip_spmm_csc_fwd_act(nts_hip_ctx* ctx, const uint32_t* column_offset,
                             const uint32_t* row_indices, const float* weight, const uint32_t* v,
                             uint32_t v_cap, const float* x, uint64_t ldx, uint32_t feature_size,
                             float* y, uint64_t ldy, float p, uint64_t seed, uint64_t offset) {
  NTS_CHECK_ARG(ctx && column_offset && row_indices && x && y, "NULL argument");
  NTS_CHECK_ARG(ldx >= feature_size && ldy >= feature_size, "leading dimension < feature_size");
  NTS_CHECK_ARG(p >= 0.f && p <= 1.f, "dropout probability must be in [0, 1]");
  if (v_cap == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  AggExtra ax;
  ax.keep_threshold = dropout_threshold(p);
  ax.scale = p >= 1.f ? 0.f : 1.0f / (1.0f - p);  // as the GEMM epilogue
  ax.seed = seed;
  ax.offset = offset;
  return launch_gather<false, false, kAggAct>(ctx->stream, column_offset, row_indices, weight, v,
                                              v_cap, x, ldx, nullptr, feature_size, y, ldy,
                                              Tier{nullptr, nullptr, 0, 0}, ax);
}

int nts_hip_spmm_csr_bwd_masked(nts_hip_ctx* ctx, const uint32_t* row_offset,
                                const uint32_t* column_indices, const float* weight_backward,
                                const uint32_t* s, uint32_t s_cap, const float* g_out,
                                uint64_t ld_gout, const float* x_act, uint64_t ld_act, float scale,
                                uint32_t feature_size, float* g_in, uint64_t ld_gin) {
  NTS_CHECK_ARG(ctx && row_offset && column_indices && g_out && x_act && g_in, "NULL argument");
  NTS_CHECK_ARG(ld_gout >= feature_size && ld_act >= feature_size && ld_gin >= feature_size,
                "leading dimension < feature_size");
  if (s_cap == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  AggExtra ax;
  ax.mx = x_act;
  ax.ldm = ld_act;
  ax.scale = scale;
  return launch_gather<false, false, kAggMask, true>(ctx->stream, row_offset, column_indices,
                                               weight_backward, s, s_cap, g_out, ld_gout, nullptr,
                                               feature_size, g_in, ld_gin,
                                               Tier{nullptr, nullptr, 0, 0}, ax);
}

int nts_hip_spmm_csr_bwd_postmask(nts_hip_ctx* ctx, const uint32_t* row_offset,
                                  const uint32_t* column_indices, const float* weight_backward,
                                  const uint32_t* s, uint32_t s_cap, const float* g_out,
                                  uint64_t ld_gout, const float* x_act, uint64_t ld_act, float scale,
                                  uint32_t feature_size, float* g_in, uint64_t ld_gin) {
  NTS_CHECK_ARG(ctx && row_offset && column_indices && g_out && x_act && g_in, "NULL argument");
  NTS_CHECK_ARG(ld_gout >= feature_size && ld_act >= feature_size && ld_gin >= feature_size,
                "leading dimension < feature_size");
  if (s_cap == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  AggExtra ax;
  ax.mx = x_act;
  ax.ldm = ld_act;
  ax.scale = scale;
  return launch_gather<false, false, kAggPostMask, true>(ctx->stream, row_offset, column_indices,
                                                         weight_backward, s, s_cap, g_out, ld_gout,
                                                         nullptr, feature_size, g_in, ld_gin,
                                                         Tier{nullptr, nullptr, 0, 0}, ax);
}

uint32_t nts_hip_act_bits_words(uint32_t feature_size) {
  if (feature_size == 0 || feature_size % 4) return 0;
  const uint32_t nv = feature_size / 4;
  const Shape s = pick_shape(nv);
  if (s.lpd < 32 || nv > (uint32_t)(s.lpd * s.nch)) return 0;  // float4 rows of one chunk
  return (uint32_t)(s.lpd / 32) * (uint32_t)s.nch * 4u;  // act_bits_words<LPD, NCH>()
}

int nts_hip_spmm_csc_fwd_act_bits(nts_hip_ctx* ctx, const uint32_t* column_offset,
                                  const uint32_t* row_indices, const float* weight,
                                  const uint32_t* v, uint32_t v_cap, const float* x, uint64_t ldx,
                                  uint32_t feature_size, float* y, uint64_t ldy, float p,
                                  uint64_t seed, uint64_t offset, uint32_t* mask_bits) {
  NTS_CHECK_ARG(ctx && column_offset && row_indices && x && y && mask_bits, "NULL argument");
  NTS_CHECK_ARG(ldx >= feature_size && ldy >= feature_size, "leading dimension < feature_size");
  NTS_CHECK_ARG(p >= 0.f && p <= 1.f, "dropout probability must be in [0, 1]");
  const uint32_t words = nts_hip_act_bits_words(feature_size);
  if (words == 0) return NTS_ERR_UNSUPPORTED;
  NTS_CHECK_ARG(row_vec(feature_size, {{x, ldx}, {y, ldy}}) == 4 && (uintptr_t)mask_bits % 16 == 0,
                "mask bits: 16-byte aligned rows with ld % 4 == 0");
  if (v_cap == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  AggExtra ax;
  ax.keep_threshold = dropout_threshold(p);
  ax.scale = p >= 1.f ? 0.f : 1.0f / (1.0f - p);
  ax.seed = seed;
  ax.offset = offset;
  ax.bits_out = mask_bits;
  ax.ldb = words;
  return launch_gather<false, false, kAggAct>(ctx->stream, column_offset, row_indices, weight, v,
                                              v_cap, x, ldx, nullptr, feature_size, y, ldy,
                                              Tier{nullptr, nullptr, 0, 0}, ax);
}

int nts_hip_spmm_csr_bwd_postmask_bits(nts_hip_ctx* ctx, const uint32_t* row_offset,
                                       const uint32_t* column_indices,
                                       const float* weight_backward, const uint32_t* s,
                                       uint32_t s_cap, const float* g_out, uint64_t ld_gout,
                                       const uint32_t* mask_bits, float scale,
                                       uint32_t feature_size, float* g_in, uint64_t ld_gin) {
  NTS_CHECK_ARG(ctx && row_offset && column_indices && g_out && mask_bits && g_in, "NULL argument");
  NTS_CHECK_ARG(ld_gout >= feature_size && ld_gin >= feature_size,
                "leading dimension < feature_size");
  const uint32_t words = nts_hip_act_bits_words(feature_size);
  if (words == 0) return NTS_ERR_UNSUPPORTED;
  NTS_CHECK_ARG(row_vec(feature_size, {{g_out, ld_gout}, {g_in, ld_gin}}) == 4 &&
                    (uintptr_t)mask_bits % 16 == 0,
                "mask bits: 16-byte aligned rows with ld % 4 == 0");
  if (s_cap == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  AggExtra ax;
  ax.bits_in = mask_bits;
  ax.ldb = words;
  ax.scale = scale;
  return launch_gather<false, false, kAggPostMask, true>(ctx->stream, row_offset, column_indices,
                                                         weight_backward, s, s_cap, g_out, ld_gout,
                                                         nullptr, feature_size, g_in, ld_gin,
                                                         Tier{nullptr, nullptr, 0, 0}, ax);
}

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
  AggExtra ax;
  ax.self = self_index;
  if (x_row_map)
    return launch_gather<true, false, kAggRootFwd>(ctx->stream, column_offset, row_indices, weight,
                                                   v, v_cap, x, ldx, x_row_map, feature_size, ycat,
                                                   ld_ycat, Tier{nullptr, nullptr, 0, 0}, ax);
  return launch_gather<false, false, kAggRootFwd>(ctx->stream, column_offset, row_indices, weight,
                                                  v, v_cap, x, ldx, nullptr, feature_size, ycat,
                                                  ld_ycat, Tier{nullptr, nullptr, 0, 0}, ax);
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
  AggExtra ax;
  ax.self = src_dst;
  ax.mx = x_act;
  ax.ldm = ld_act;
  ax.scale = x_act ? scale : 1.f;
  return launch_gather<false, false, kAggRootBwd, true>(ctx->stream, row_offset, column_indices,
                                                        weight_backward, s, s_cap, g_ycat, ld_g,
                                                        nullptr, feature_size, g_in, ld_gin,
                                                        Tier{nullptr, nullptr, 0, 0}, ax);
}

int nts_hip_spmm_csc_bwd_atomic(nts_hip_ctx* ctx, const uint32_t* column_offset,
                                const uint32_t* row_indices, const float* weight,
                                const uint32_t* v, uint32_t v_cap, const float* g_out,
                                uint64_t ld_gout, uint32_t feature_size, float* g_in,
                                uint64_t ld_gin) {
  NTS_CHECK_ARG(ctx && column_offset && row_indices && g_out && g_in, "NULL argument");
  NTS_CHECK_ARG(ld_gout >= feature_size && ld_gin >= feature_size,
                "leading dimension < feature_size");
  if (v_cap == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const int vec = row_vec(feature_size, {{g_out, ld_gout}, {g_in, ld_gin}});
  const uint32_t nv = feature_size / vec;
  const int lpd = nv <= 16 ? 16 : (nv <= 32 ? 32 : 64);
  const uint32_t grid = std::max(1u, std::min(ceil_div(v_cap, kAggThreads / lpd), 4096u));
#define NTS_S(VEC, LPD)                                                                    \
  hipLaunchKernelGGL((k_spmm_scatter_atomic<VEC, LPD>), dim3(grid), dim3(kAggThreads), 0,   \
                     ctx->stream, column_offset, row_indices, weight, v, v_cap, g_out, ld_gout, \
                     nv, g_in, ld_gin)
  if (vec == 4) {
    if (lpd == 16) NTS_S(4, 16); else if (lpd == 32) NTS_S(4, 32); else NTS_S(4, 64);
  } else if (vec == 2) {
    if (lpd == 16) NTS_S(2, 16); else if (lpd == 32) NTS_S(2, 32); else NTS_S(2, 64);
  } else {
    if (lpd == 16) NTS_S(1, 16); else if (lpd == 32) NTS_S(1, 32); else NTS_S(1, 64);
  }
#undef NTS_S
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

}  // extern "C"

template <bool TIER, bool STAGE = false>
static int gather_rows(nts_hip_ctx* ctx, const float* table, uint64_t ld_table,
                       const uint32_t* index, const uint32_t* n, uint32_t n_cap,
                       uint32_t feature_size, float* out, uint64_t ld_out, Tier tier) {
  const int vec = row_vec(feature_size, {{table, ld_table}, {out, ld_out},
                                         {TIER ? tier.host : nullptr, tier.ldh}});
  const uint32_t nv = feature_size / vec;
  const int lpd = nv <= 16 ? 16 : (nv <= 32 ? 32 : 64);
  const uint32_t grid = std::max(1u, std::min(ceil_div(n_cap, kAggThreads / lpd), 4096u));
#define NTS_R(VEC, LPD)                                                                      \
  hipLaunchKernelGGL((k_gather_rows<VEC, LPD, TIER, STAGE>), dim3(grid), dim3(kAggThreads), 0, \
                     ctx->stream, table, ld_table, index, n, n_cap, nv, out, ld_out, tier)
  if (vec == 4) {
    if (lpd == 16) NTS_R(4, 16); else if (lpd == 32) NTS_R(4, 32); else NTS_R(4, 64);
  } else if (vec == 2) {
    if (lpd == 16) NTS_R(2, 16); else if (lpd == 32) NTS_R(2, 32); else NTS_R(2, 64);
  } else {
    if (lpd == 16) NTS_R(1, 16); else if (lpd == 32) NTS_R(1, 32); else NTS_R(1, 64);
  }
#undef NTS_R
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

extern "C" {

int nts_hip_gather_rows(nts_hip_ctx* ctx, const float* table, uint64_t ld_table,
                        const uint32_t* index, const uint32_t* n, uint32_t n_cap,
                        uint32_t feature_size, float* out, uint64_t ld_out) {
  NTS_CHECK_ARG(ctx && table && index && out, "NULL argument");
  NTS_CHECK_ARG(ld_table >= feature_size && ld_out >= feature_size,
                "leading dimension < feature_size");
  if (n_cap == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  return gather_rows<false>(ctx, table, ld_table, index, n, n_cap, feature_size, out, ld_out,
                            Tier{nullptr, nullptr, 0, 0});
}

int nts_hip_gather_rows_cached(nts_hip_ctx* ctx, const float* cache, uint64_t ld_cache,
                               const uint32_t* cache_map, const float* host_table,
                               uint64_t ld_host, const uint32_t* index, const uint32_t* n,
                               uint32_t n_cap, uint32_t feature_size, float* out,
                               uint64_t ld_out) {
  NTS_CHECK_ARG(ctx && cache_map && host_table && index && out, "NULL argument");
  NTS_CHECK_ARG(ld_cache >= feature_size && ld_host >= feature_size && ld_out >= feature_size,
                "leading dimension < feature_size");
  if (n_cap == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  // an empty cache (no HBM rows) still needs a non-NULL, aligned base
  if (!cache) cache = host_table, ld_cache = ld_host;
  return gather_rows<true>(ctx, cache, ld_cache, index, n, n_cap, feature_size, out, ld_out,
                           Tier{cache_map, host_table, ld_host, 0});
}

int nts_hip_stage_uncached_rows(nts_hip_ctx* ctx, const uint32_t* cache_map,
                                const float* host_table, uint64_t ld_host, const uint32_t* index,
                                const uint32_t* n, uint32_t n_cap, uint32_t feature_size,
                                float* stage, uint64_t ld_stage) {
  NTS_CHECK_ARG(ctx && cache_map && host_table && index && stage, "NULL argument");
  NTS_CHECK_ARG(ld_host >= feature_size && ld_stage >= feature_size,
                "leading dimension < feature_size");
  if (n_cap == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  return gather_rows<true, true>(ctx, host_table, ld_host, index, n, n_cap, feature_size, stage,
                                 ld_stage, Tier{cache_map, host_table, ld_host, 0});
}

int nts_hip_spmm_csc_fwd_cached(nts_hip_ctx* ctx, const uint32_t* column_offset,
                                const uint32_t* row_indices, const float* weight,
                                const uint32_t* v, uint32_t v_cap, const float* cache,
                                uint64_t ld_cache, const uint32_t* cache_map,
                                const float* host_table, uint64_t ld_host, int host_local,
                                const uint32_t* x_row_map, uint32_t feature_size, float* y,
                                uint64_t ldy) {
  NTS_CHECK_ARG(ctx && column_offset && row_indices && cache_map && host_table && x_row_map && y,
                "NULL argument");
  NTS_CHECK_ARG(ld_cache >= feature_size && ld_host >= feature_size && ldy >= feature_size,
                "leading dimension < feature_size");
  if (v_cap == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  if (!cache) cache = host_table, ld_cache = ld_host;
  return launch_gather<true, true>(ctx->stream, column_offset, row_indices, weight, v, v_cap,
                                   cache, ld_cache, x_row_map, feature_size, y, ldy,
                                   Tier{cache_map, host_table, ld_host, host_local});
}

int nts_hip_act_backward(nts_hip_ctx* ctx, uint32_t rows, uint32_t feature_size, const float* g,
                         uint64_t ldg, const float* x_act, uint64_t ldx, float scale, float* out,
                         uint64_t ldo) {
  NTS_CHECK_ARG(ctx && g && x_act && out, "NULL argument");
  NTS_CHECK_ARG(ldg >= feature_size && ldx >= feature_size && ldo >= feature_size,
                "leading dimension < feature_size");
  if (rows == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const uint64_t n = (uint64_t)rows * feature_size;
  const bool flat = ldg == feature_size && ldx == feature_size && ldo == feature_size &&
                    n % 4 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)x_act % 16 == 0 &&
                    (uintptr_t)out % 16 == 0;
  if (flat) {
    const uint32_t grid = std::max(1u, std::min(ceil_div(n / 4, 256), kMaxGrid));
    hipLaunchKernelGGL(k_act_backward, dim3(grid), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const float4*>(g), reinterpret_cast<const float4*>(x_act),
                       reinterpret_cast<float4*>(out), n / 4, scale);
  } else {
    const uint32_t grid = std::max(1u, std::min(ceil_div(n, 256), kMaxGrid));
    hipLaunchKernelGGL(k_act_backward_2d, dim3(grid), dim3(256), 0, ctx->stream, g, ldg, x_act,
                       ldx, out, ldo, rows, feature_size, scale);
  }
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

int nts_hip_gather_labels(nts_hip_ctx* ctx, const int64_t* labels, const uint32_t* index,
                          const uint32_t* n, uint32_t n_cap, int64_t* out) {
  NTS_CHECK_ARG(ctx && labels && index && out, "NULL argument");
  if (n_cap == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const uint32_t grid = std::max(1u, std::min(ceil_div(n_cap, 256), kMaxGrid));
  hipLaunchKernelGGL(k_gather_labels, dim3(grid), dim3(256), 0, ctx->stream, labels, index, n,
                     n_cap, out);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

int nts_hip_adam(nts_hip_ctx* ctx, float* w, const float* grad, float* m, float* v, uint64_t n,
                 float alpha, float beta1, float beta2, float epsilon, float weight_decay,
                 float beta1_t, float beta2_t, int bias_correction) {
  NTS_CHECK_ARG(ctx && w && grad && m && v, "NULL argument");
  if (n == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const uint32_t grid = std::max(1u, std::min(ceil_div(n, 256), kMaxGrid));
  hipLaunchKernelGGL(k_adam, dim3(grid), dim3(256), 0, ctx->stream, w, grad, m, v, n, alpha,
                     beta1, beta2, epsilon, weight_decay, beta1_t, beta2_t, bias_correction);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

}  // extern "C"
