// Output layer + loss of the GCN/GraphSAGE drivers, fused.
//
// Reference (toolkits/GCN_SAMPLE_ALLGPU.hpp:214-222, 247-252):
//   vertexForward, last layer:  y = (a.matmul(W)).log_softmax(1)
//   Loss:                       loss = nll_loss(y.log_softmax(1), target)   (mean)
// i.e. logits Z = Y W, log_softmax applied twice (the second is numerically
// ~idempotent but kept: same arithmetic as the reference), the mean negative
// log-likelihood of the target class, and libtorch's backward of all of it.
// On the GPU drivers that is ~12 tiny kernels per step (GEMM, 2 softmax, NLL,
// fills, their backwards, dW and dY GEMMs).  Here one kernel template:
//   LOSS: the loss (block partials);
//   GRAD: dY and per-wave dW partials for the upstream gradient (*grad, or
//         exactly 1 for the training call);
// then k_top_finish sums the partials in a fixed order (deterministic, no
// atomics).  dW partials are stored as chunks [k][ct][wave][16]: a wave
// writes 64-byte runs and the finish kernel reads 256-byte runs.
// forward = <LOSS>, backward = <GRAD>, train = <LOSS, GRAD> (bit-identical
// to forward + backward with grad 1: same code, same orders).
//
// (What follows describes the form for C <= 64, W resident in LDS; above 64
// classes, to 512, k_top_xent_wide below streams W from global memory.)
//
// (The multi-label form of the layer, sigmoid BCE over bit-packed targets with
// the micro-F1 counters, is k_top_bce_ks below: the same block shape, shared
// staging and products, an element-wise middle.)
//
// One wave owns 16 rows.  Its Y tile is staged into LDS with coalesced
// 16-byte loads (all issued up front), then the three products run on
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation):
//   Z  [16 x Cp] = Y [16 x K] W [K x Cp]      (Cp = C rounded up to 16, <= 64)
//   dY [16 x K]  = dZ [16 x Cp] W^T            (dZ staged through LDS)
//   dW_part [K x Cp] = Y^T [K x 16] dZ [16 x Cp]  (one slab per wave)
// W lives in LDS (zero-padded to Cp columns).  In the accumulator layout a lane
// (i, g) holds Z[4g + v][16 ct + i]; row-wise softmax reductions run over the
// 16 lanes of a group g (xor shuffles 1..8).  Y tile pitch K + 4: the logits'
// A reads (row i, k0 + g) hit 64 distinct banks.
// Layout: Y [n x K] (ld ldy), W [K x C] row-major, labels int64 [n].
#include "common.hpp"

namespace nts_hip {

typedef float f32x4 __attribute__((ext_vector_type(4)));
// waves per block
constexpr int kTopWaves = 4;
constexpr int kTopThreads = kTopWaves * 64;
constexpr int kTopRowsPerWave = 16;
constexpr int kTopRows = kTopWaves * kTopRowsPerWave;  // rows per block

struct TopArgs {
  const float* Y;
  uint64_t ldy;
  const float* W;
  const int64_t* labels;
  const float* grad;  // GRAD: d loss (device scalar); nullptr = exactly 1
  int n, K, C;
  float* lpart;       // LOSS: [blocks] loss partials
  float* part;        // GRAD: dW partials [K][Cp/16][waves][16]
  float* dY;          // GRAD: [n x K]
  uint32_t* cpart;    // LOSS with accuracy: [blocks] rows whose argmax is the label
};

// Reductions over the 16 lanes of a group (a DPP row) by DPP moves: the
// partner of each step is lane ^ 1, lane ^ 2 (quad permutes), then the other
// quad of the 8-lane half (half mirror) and the other half (row mirror) — the
// pairing tree of an xor butterfly 1, 2, 4, 8, so every lane ends with the
// same sum as that butterfly's.  (The butterfly by __shfl_xor is a chain of
// ds_bpermute round trips: 4-8 us of each block's softmax phase, by phase
// timers.)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
constexpr int kDppX1 = 0xB1, kDppX2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;
__device__ __forceinline__ float grp_max(float v) {
  v = fmaxf(v, dpp_f<kDppX1>(v));
  v = fmaxf(v, dpp_f<kDppX2>(v));
  v = fmaxf(v, dpp_f<kDppHalfMirror>(v));
  return fmaxf(v, dpp_f<kDppMirror>(v));
}
__device__ __forceinline__ float grp_sum(float v) {
  v += dpp_f<kDppX1>(v);
  v += dpp_f<kDppX2>(v);
  v += dpp_f<kDppHalfMirror>(v);
  return v + dpp_f<kDppMirror>(v);
}
// argmax over the group (first index among equal values)
__device__ __forceinline__ void grp_argmax_step(float& best, int& bi, float ob, int oi) {
  if (ob > best || (ob == best && oi < bi)) {
    best = ob;
    bi = oi;
  }
}
__device__ __forceinline__ int grp_argmax(float best, int bi) {
  grp_argmax_step(best, bi, dpp_f<kDppX1>(best), dpp_i<kDppX1>(bi));
  grp_argmax_step(best, bi, dpp_f<kDppX2>(best), dpp_i<kDppX2>(bi));
  grp_argmax_step(best, bi, dpp_f<kDppHalfMirror>(best), dpp_i<kDppHalfMirror>(bi));
  grp_argmax_step(best, bi, dpp_f<kDppMirror>(best), dpp_i<kDppMirror>(bi));
  return bi;
}

// Stage W into LDS as sW[k][Cp] (zero columns >= C): coalesced loads of the
// contiguous [K x C] matrix.  K % 16 == 0 makes K x C a multiple of 4: with a
// 16-byte aligned W the whole matrix goes as float4s, up to 16 per thread in
// flight (one memory round trip for C3's 256 x 47; the scalar form took six
// dependent rounds of 8 loads, most of the kernel at 16 blocks).
template <int CP, class Args>
__device__ __forceinline__ void stage_w(const Args& a, float* sW) {
  const int C = a.C, KC = a.K * C;
  if (((uintptr_t)a.W & 15) == 0) {
    const float4* W4 = reinterpret_cast<const float4*>(a.W);
    const int nq = KC / 4;
    constexpr int B = 16;
    for (int q0 = threadIdx.x; q0 < nq; q0 += B * kTopThreads) {
      float4 v[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int q = q0 + u * kTopThreads;
        v[u] = q < nq ? W4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int q = q0 + u * kTopThreads;
        if (q < nq) {
          const float x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
          int r = 4 * q / C, cc = 4 * q - r * C;  // one division per float4
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            sW[r * CP + cc] = x[c];
            if (++cc == C) {
              cc = 0;
              ++r;
            }
          }
        }
      }
    }
  } else {
    constexpr int B = 8;
    for (int e0 = threadIdx.x; e0 < KC; e0 += B * kTopThreads) {
      float v[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int e = e0 + u * kTopThreads;
        v[u] = e < KC ? a.W[e] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int e = e0 + u * kTopThreads;
        if (e < KC) sW[(e / C) * CP + e % C] = v[u];
      }
    }
  }
  const int pad = CP - C;
  for (int e = threadIdx.x; e < a.K * pad; e += kTopThreads)
    sW[(e / pad) * CP + C + e % pad] = 0.f;
}

// Stage this wave's 16 Y rows into sY[16][K + 4] (rows >= n are zero).
// VEC4: 16-byte loads (ldy % 4 == 0, Y 16-byte aligned).
template <bool VEC4>
__device__ __forceinline__ void stage_y(const TopArgs& a, float* sY, int r0, int lane) {
  const int K = a.K, P = K + 4;
  constexpr int B = VEC4 ? 16 : 8;  // loads in flight per lane (K = 256: one round)
  if (VEC4) {
    const int kq = K / 4, it = K / 16;  // float4 per row; per lane (16 rows x kq / 64)
    for (int j0 = 0; j0 < it; j0 += B) {
      float4 v[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int q = lane + kWave * (j0 + u), rr = q / kq, r = r0 + rr;
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j0 + u < it && r < a.n)
          v[u] = *reinterpret_cast<const float4*>(a.Y + (uint64_t)r * a.ldy + 4 * (q % kq));
      }
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int q = lane + kWave * (j0 + u);
        if (j0 + u < it) *reinterpret_cast<float4*>(sY + (q / kq) * P + 4 * (q % kq)) = v[u];
      }
    }
  } else {
    const int it = K / 4;  // 16 rows x K / 64 per lane
    for (int j0 = 0; j0 < it; j0 += B) {
      float v[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int q = lane + kWave * (j0 + u), r = r0 + q / K;
        v[u] = (j0 + u < it && r < a.n) ? a.Y[(uint64_t)r * a.ldy + q % K] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int q = lane + kWave * (j0 + u);
        if (j0 + u < it) sY[(q / K) * P + q % K] = v[u];
      }
    }
  }
}

// Z tile of this wave's 16 rows: z[ct][v] = Z[r0 + 4g + v][16 ct + i].
template <int NCT>
__device__ __forceinline__ void wave_logits(int K, const float* sW, const float* sY, int i, int g,
                                            f32x4 (&z)[NCT]) {
  constexpr int CP = 16 * NCT;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) z[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* yr = sY + i * (K + 4);
  for (int k1 = 0; k1 < K; k1 += 16) {  // K % 16 == 0
#pragma unroll
    for (int k0 = k1; k0 < k1 + 16; k0 += 4) {
      const float av = yr[k0 + g];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
        z[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sW[(k0 + g) * CP + 16 * ct + i], z[ct],
                                                     0, 0, 0);
    }
  }
}

// log_softmax of rows 4g+v (one value per column tile per lane), twice.
// lp/lp2 in the same layout; columns >= C excluded.
template <int NCT>
__device__ __forceinline__ void log_softmax2(const f32x4 (&z)[NCT], int C, int i,
                                             float (&lp)[NCT][4], float (&lp2)[NCT][4]) {
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    float m = -INFINITY;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
      if (16 * ct + i < C) m = fmaxf(m, z[ct][v]);
    m = grp_max(m);
    float s = 0.f;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
      if (16 * ct + i < C) s += expf(z[ct][v] - m);
    s = grp_sum(s);
    const float lse = m + logf(s);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) lp[ct][v] = z[ct][v] - lse;
    float m2 = -INFINITY;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
      if (16 * ct + i < C) m2 = fmaxf(m2, lp[ct][v]);
    m2 = grp_max(m2);
    float s2 = 0.f;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
      if (16 * ct + i < C) s2 += expf(lp[ct][v] - m2);
    s2 = grp_sum(s2);
    const float lse2 = m2 + logf(s2);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) lp2[ct][v] = lp[ct][v] - lse2;
  }
}

// LDS of the retired one-wave-per-tile form: still the K x C bound that the
// argument check (top_check) applies
static inline size_t top_lds(int K, int Cp) {
  return ((size_t)K * Cp + (size_t)kTopWaves * 16 * (K + 4) + (size_t)kTopRows * Cp) *
         sizeof(float);
}

// K-split form: one block of kTopWaves waves per 16-row tile, wave w taking
// the k tiles kt = w, w + kTopWaves, ... of every product.
// The retired per-wave form ran a whole tile's three products on one wave —
// ~600 dependent v_mfma_f32_16x16x4_f32 at K = 256 with one wave per SIMD,
// 35 us however few rows (C3: 1,024 rows, 64 waves on 256 CUs).  Here the
// logits are four partial chains summed in a fixed order (w = 0..3) through
// LDS; every wave then holds the same Z and log-softmax, wave 0 writes dZ
// and the loss; dY and dW run on each wave's k tiles (two at a time).  One dW
// slab per block.  Deterministic; the logits' summation order differs from
// the per-wave form by rounding only.
static inline size_t top_ks_lds(int K, int Cp) {
  return ((size_t)K * Cp + (size_t)16 * (K + 4) + (size_t)(kTopWaves + 1) * 16 * Cp) * sizeof(float);
}

// Stage the 16 Y rows r0 .. r0 + 15 of a K-split block into sY[16][K + 4], all
// threads of the block (rows >= n are zero).  VEC4: 16-byte loads
// (ldy % 4 == 0, Y 16-byte aligned).
template <bool VEC4, class Args>
__device__ __forceinline__ void stage_y_tile(const Args& a, float* sY, int r0) {
  const int K = a.K, P = K + 4;
  constexpr int B = 8;
  if (VEC4) {
    const int kq = K / 4, tot = 16 * kq;
    for (int q0 = threadIdx.x; q0 < tot; q0 += B * kTopThreads) {
      float4 v[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int q = q0 + u * kTopThreads, rr = q / kq, r = r0 + rr;
        v[u] = (q < tot && r < a.n) ? *reinterpret_cast<const float4*>(a.Y + (uint64_t)r * a.ldy + 4 * (q % kq))
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int q = q0 + u * kTopThreads;
        if (q < tot) *reinterpret_cast<float4*>(sY + (q / kq) * P + 4 * (q % kq)) = v[u];
      }
    }
  } else {
    const int tot = 16 * K;
    for (int q0 = threadIdx.x; q0 < tot; q0 += B * kTopThreads) {
      float v[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int q = q0 + u * kTopThreads, r = r0 + q / K;
        v[u] = (q < tot && r < a.n) ? a.Y[(uint64_t)r * a.ldy + q % K] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int q = q0 + u * kTopThreads;
        if (q < tot) sY[(q / K) * P + q % K] = v[u];
      }
    }
  }
}

// This wave's share of the logits: the partial chains of its k tiles
// (kt = w, w + kTopWaves, ...) of Z = Y W, stored to zp[w][16][CP]; the caller
// sums the waves' slabs in wave order after a barrier.
template <int NCT>
__device__ __forceinline__ void split_logits(int K, const float* sW, const float* sY, float* zp,
                                             int w, int i, int g) {
  constexpr int CP = 16 * NCT, NW = kTopWaves;
  const int P = K + 4, nkt = K / 16;
  f32x4 z[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) z[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    const float* yr = sY + i * P;
    for (int kt = w; kt < nkt; kt += NW) {
#pragma unroll
      for (int k0 = 16 * kt; k0 < 16 * kt + 16; k0 += 4) {
        const float av = yr[k0 + g];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
          z[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sW[(k0 + g) * CP + 16 * ct + i], z[ct], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int v = 0; v < 4; ++v) zp[(w * 16 + 4 * g + v) * CP + 16 * ct + i] = z[ct][v];
}

// dY [16 x K] = dZ W^T and this block's dW slab [K x CP] = Y^T dZ from the dZ
// tile in LDS, each wave on its k tiles.
template <int NCT, class Args>
__device__ __forceinline__ void grad_products(const Args& a, const float* sW, const float* sY,
                                              const float* dz, int r0, int w, int i, int g) {
  constexpr int CP = 16 * NCT, NW = kTopWaves;
  const int K = a.K, P = K + 4, nkt = K / 16;
  // dY [16 x K] = dZ W^T on this wave's k tiles, two at a time
  constexpr int KT = 2;
  for (int j0 = w; j0 < nkt; j0 += KT * NW) {
    f32x4 acc[KT];
    int ktu[KT];
#pragma unroll
    for (int u = 0; u < KT; ++u) {
      acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      ktu[u] = min(j0 + u * NW, nkt - 1);
    }
#pragma unroll
    for (int c0 = 0; c0 < CP; c0 += 4) {
      const float av = dz[i * CP + c0 + g];
#pragma unroll
      for (int u = 0; u < KT; ++u)
        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sW[(16 * ktu[u] + i) * CP + c0 + g], acc[u],
                                                      0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < KT; ++u) {
      const int kt = j0 + u * NW;
      if (kt >= nkt) break;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int r = r0 + 4 * g + v;
        if (r < a.n) a.dY[(uint64_t)r * K + 16 * kt + i] = acc[u][v];
      }
    }
  }
  // dW slab of this block [K x CP] = Y^T dZ, rows of this wave's k tiles
  const uint64_t nslab = gridDim.x, slab = blockIdx.x;
  for (int j0 = w; j0 < nkt; j0 += KT * NW) {
    f32x4 acc[KT][NCT];
    int ktu[KT];
#pragma unroll
    for (int u = 0; u < KT; ++u) {
      ktu[u] = min(j0 + u * NW, nkt - 1);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[u][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      float bv[NCT];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) bv[ct] = dz[(4 * s4 + g) * CP + 16 * ct + i];
#pragma unroll
      for (int u = 0; u < KT; ++u) {
        const float av = sY[(4 * s4 + g) * P + 16 * ktu[u] + i];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
          acc[u][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[ct], acc[u][ct], 0, 0, 0);
      }
    }
#pragma unroll
    for (int u = 0; u < KT; ++u) {
      const int kt = j0 + u * NW;
      if (kt >= nkt) break;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const uint64_t q = (uint64_t)(16 * kt + 4 * g + v) * NCT + ct;
          a.part[(q * nslab + slab) * 16 + i] = acc[u][ct][v];
        }
    }
  }
}

template <int NCT, bool LOSS, bool GRAD, bool VEC4>
__global__ __launch_bounds__(kTopThreads) void k_top_xent_ks(TopArgs a) {
  constexpr int CP = 16 * NCT, NW = kTopWaves;
  extern __shared__ float smem[];
  __shared__ float wl[NW];
  __shared__ uint32_t wc[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int K = a.K, P = K + 4;
  float* sW = smem;                // [K][CP]
  float* sY = sW + K * CP;         // [16][K + 4]
  float* zp = sY + 16 * P;         // [NW][16][CP] partial logits
  float* dz = zp + NW * 16 * CP;   // [16][CP]
  const int r0 = blockIdx.x * 16;
  // the rows' labels and the upstream gradient first: their global loads
  // then overlap the staging instead of following the logits (a dependent
  // memory latency of 4-6 us per block there, measured with phase timers)
  constexpr int VPW = 4 / NW;  // rows 4 g + v per lane group finished by this wave
  static_assert(4 % NW == 0, "kTopWaves must divide 4");
  int tgt[VPW];
#pragma unroll
  for (int vv = 0; vv < VPW; ++vv) {
    const int r = r0 + 4 * g + w + vv * NW;
    tgt[vv] = r < a.n ? (int)a.labels[r] : -1;
  }
  const float gl = GRAD ? (a.grad ? *a.grad : 1.0f) / (float)a.n : 0.f;
  stage_y_tile<VEC4>(a, sY, r0);
  stage_w<CP>(a, sW);
  __syncthreads();
  split_logits<NCT>(K, sW, sY, zp, w, i, g);
  __syncthreads();
  // each wave finishes the rows 4 g + v of its own v (v = w, w + NW, ...): the
  // logits' sum over the waves' k-splits, log_softmax twice (log_softmax2's
  // arithmetic per row), the loss and accuracy terms and dZ — a quarter of the
  // tile each (the whole tile on wave 0 was 4-6 us of every block, phase timers)
  float lw = 0.f;
  uint32_t okw = 0;
#pragma unroll
  for (int vv = 0; vv < VPW; ++vv) {
    const int v = w + vv * NW;
    float zv[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      float t = zp[(4 * g + v) * CP + 16 * ct + i];
#pragma unroll
      for (int q = 1; q < NW; ++q) t += zp[(q * 16 + 4 * g + v) * CP + 16 * ct + i];
      zv[ct] = t;
    }
    float lp[NCT], lp2[NCT];
    {
      float m = -INFINITY;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
        if (16 * ct + i < a.C) m = fmaxf(m, zv[ct]);
      m = grp_max(m);
      float sm = 0.f;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
        if (16 * ct + i < a.C) sm += expf(zv[ct] - m);
      sm = grp_sum(sm);
      const float lse = m + logf(sm);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) lp[ct] = zv[ct] - lse;
      float m2 = -INFINITY;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
        if (16 * ct + i < a.C) m2 = fmaxf(m2, lp[ct]);
      m2 = grp_max(m2);
      float s2 = 0.f;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
        if (16 * ct + i < a.C) s2 += expf(lp[ct] - m2);
      s2 = grp_sum(s2);
      const float lse2 = m2 + logf(s2);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) lp2[ct] = lp[ct] - lse2;
    }
    if (LOSS) {
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
        if (16 * ct + i == tgt[vv]) lw -= lp2[ct];
      if (a.cpart) {  // getCorrect (toolkits/GCN_SAMPLE_ALLGPU.hpp:166-172), as k_top_xent
        float best = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
          if (16 * ct + i < a.C && lp[ct] > best) {
            best = lp[ct];
            bi = 16 * ct + i;
          }
        bi = grp_argmax(best, bi);
        okw += (i == 0 && tgt[vv] >= 0 && bi == tgt[vv]) ? 1u : 0u;
      }
    }
    if (GRAD) {
      const int r = r0 + 4 * g + v;
      float d2[NCT], s2 = 0.f;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        d2[ct] = (16 * ct + i == tgt[vv]) ? -gl : 0.f;
        s2 += d2[ct];
      }
      s2 = grp_sum(s2);
      float d1[NCT], s1 = 0.f;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const bool on = 16 * ct + i < a.C;
        d1[ct] = on ? d2[ct] - expf(lp2[ct]) * s2 : 0.f;
        s1 += d1[ct];
      }
      s1 = grp_sum(s1);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const bool on = 16 * ct + i < a.C && r < a.n;
        dz[(4 * g + v) * CP + 16 * ct + i] = on ? d1[ct] - expf(lp[ct]) * s1 : 0.f;
      }
    }
  }
  if (LOSS) {  // the wave's terms, then the block's in wave order (below)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lw += __shfl_down(lw, o, kWave);
    if (lane == 0) wl[w] = lw;
    if (a.cpart) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) okw += __shfl_down(okw, o, kWave);
      if (lane == 0) wc[w] = okw;
    }
  }
  if (GRAD) {
    __syncthreads();
    grad_products<NCT>(a, sW, sY, dz, r0, w, i, g);
  }
  if (LOSS) {
    __syncthreads();
    if (threadIdx.x == 0) {
      float l = 0.f;
      uint32_t c = 0;
      for (int q = 0; q < NW; ++q) {
        l += wl[q];
        c += wc[q];
      }
      a.lpart[blockIdx.x] = l;
      if (a.cpart) a.cpart[blockIdx.x] = c;
    }
  }
}

// ---- wide-class form: 64 < C <= 512 ------------------------------------------
// The same contract as k_top_xent_ks at class counts whose W [K x Cp] does not
// fit LDS (K = 256, Cp = 176 is 180 KB).  W stays in global memory (it is
// L2-resident) and goes to the MFMAs through registers: with the waves split
// over column tiles every element of W is the B operand of exactly one MFMA of
// a 16-row tile, so an LDS copy would be written once and read once.
//   logits  wave w takes the column tiles ct = w, w + 4, ..., two at a time
//           (independent chains over the whole K), 32 k per round with the
//           next round's 16 loads in flight behind the MFMAs; the tile goes to
//           sZ [16][Cp + 4];
//   finish  wave w takes the rows 4 g + w; a lane holds Cp / 16 entries of its
//           row, re-read from sZ in each pass (max; sum; sum + argmax of lp;
//           sum of d1; dZ) — the arithmetic per entry and the order of every sum
//           (ct ascending in the lane, then the DPP tree) are k_top_xent_ks's;
//           dZ overwrites the logits in place, each lane the entries it read;
//   dY      wave w takes the k tiles kt = w, w + 4, ..., two at a time, W^T
//           read from global (lane (i, g): W[16 kt + i][c0 + g]);
//   dW      wave w takes the rows of its k tiles, the column tiles two at a
//           time, into this block's slab (k_top_xent_ks's chunk layout).
// A block walks the row tiles blockIdx.x, + gridDim.x, ...; the grid is capped
// so that the slabs stay within kWideSlabBytes (wide_blocks), and a block's
// later tiles are added onto its slab in walk order: the summation order is a
// function of (n, K, C) alone.  Loss and accuracy partials are per row tile.
// LDS: (16 (K + 4) + 16 (Cp + 4) + 16) floats — 66,112 bytes at K = Cp = 512,
// the largest shape taken, so no LDS bound is checked beyond K, C <= 512.
constexpr int kWideMaxC = 512, kWideMaxK = 512;
constexpr size_t kWideSlabBytes = (size_t)128 << 20;

static inline size_t top_wide_lds(int K, int Cp) {
  return ((size_t)16 * (K + 4) + (size_t)16 * (Cp + 4) + 16) * sizeof(float);
}
// blocks (= dW slabs) of the wide form for ntiles 16-row tiles
static inline int wide_blocks(int ntiles, int K, int Cp) {
  const size_t cap = kWideSlabBytes / ((size_t)K * Cp * sizeof(float));  // >= 128
  return (int)std::min<size_t>((size_t)ntiles, cap);
}

template <bool LOSS, bool GRAD, bool VEC4>
__global__ __launch_bounds__(kTopThreads) void k_top_xent_wide(TopArgs a) {
  constexpr int NW = kTopWaves;
  static_assert(NW == 4, "one row 4 g + w per lane group and wave");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int K = a.K, C = a.C, P = K + 4, nkt = K / 16;
  const int NCT = (C + 15) / 16, CP = 16 * NCT, PZ = CP + 4;
  float* sY = smem;              // [16][K + 4]
  float* sZ = sY + 16 * P;       // [16][CP + 4] logits, then dZ
  float* wl = sZ + 16 * PZ;      // [NW] loss terms of the waves
  uint32_t* wc = reinterpret_cast<uint32_t*>(wl + NW);  // [NW]
  const int ntiles = (a.n + 15) / 16;
  const float gl = GRAD ? (a.grad ? *a.grad : 1.0f) / (float)a.n : 0.f;
  const uint64_t nslab = gridDim.x, slab = blockIdx.x;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int r0 = tile * 16;
    const int rl = 4 * g + w, r = r0 + rl;  // the row this lane group finishes
    const int tgt = r < a.n ? (int)a.labels[r] : -1;
    stage_y_tile<VEC4>(a, sY, r0);
    __syncthreads();
    // ---- logits: this wave's column tiles, two at a time
    for (int ct0 = w; ct0 < NCT; ct0 += 2 * NW) {
      const int c0 = 16 * ct0 + i, c1 = c0 + 16 * NW;
      const bool on0 = c0 < C, on1 = ct0 + NW < NCT && c1 < C;
      const float* w0 = a.W + (on0 ? c0 : 0);
      const float* w1 = a.W + (on1 ? c1 : 0);
      constexpr int B = 8;  // k steps of 4 per round
      float b0[B], b1[B], n0[B], n1[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int k = 4 * u + g;
        b0[u] = (on0 && k < K) ? w0[(size_t)k * C] : 0.f;
        b1[u] = (on1 && k < K) ? w1[(size_t)k * C] : 0.f;
      }
      f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
      for (int k1 = 0; k1 < K; k1 += 4 * B) {
#pragma unroll
        for (int u = 0; u < B; ++u) {  // the next round's loads (zeros past K)
          const int k = k1 + 4 * B + 4 * u + g;
          n0[u] = (on0 && k < K) ? w0[(size_t)k * C] : 0.f;
          n1[u] = (on1 && k < K) ? w1[(size_t)k * C] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < B; ++u) {
          const int k = k1 + 4 * u + g;
          const float av = k < K ? sY[i * P + k] : 0.f;
          z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0[u], z0, 0, 0, 0);
          z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1[u], z1, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < B; ++u) {
          b0[u] = n0[u];
          b1[u] = n1[u];
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        sZ[(4 * g + v) * PZ + 16 * ct0 + i] = z0[v];
        if (ct0 + NW < NCT) sZ[(4 * g + v) * PZ + 16 * (ct0 + NW) + i] = z1[v];
      }
    }
    __syncthreads();
    // ---- finish row rl: log_softmax twice, loss and accuracy terms, dZ in place
    float lw = 0.f;
    uint32_t okw = 0;
    {
      float* zr = sZ + rl * PZ + i;  // entry ct of this lane: zr[16 ct]
      float m = -INFINITY;
      for (int ct = 0; ct < NCT; ++ct)
        if (16 * ct + i < C) m = fmaxf(m, zr[16 * ct]);
      m = grp_max(m);
      float sm = 0.f;
      for (int ct = 0; ct < NCT; ++ct)
        if (16 * ct + i < C) sm += expf(zr[16 * ct] - m);
      sm = grp_sum(sm);
      const float lse = m + logf(sm);
      // max over c of lp[c] = z[c] - lse: rounding is monotone, so it is m - lse
      const float m2 = m - lse;
      float s2 = 0.f, best = -INFINITY;
      int bi = 0x7fffffff;
      for (int ct = 0; ct < NCT; ++ct) {
        const float lp = zr[16 * ct] - lse;
        if (16 * ct + i < C) {
          s2 += expf(lp - m2);
          if (lp > best) {  // first index among equal values: ct ascends
            best = lp;
            bi = 16 * ct + i;
          }
        }
      }
      s2 = grp_sum(s2);
      const float lse2 = m2 + logf(s2);
      const bool mine = tgt >= 0 && tgt < C && (tgt & 15) == i;  // this lane holds the label's entry
      if (LOSS) {
        if (mine) lw -= (zr[tgt - i] - lse) - lse2;
        if (a.cpart) {  // getCorrect: argmax of lp, first index among equal values
          bi = grp_argmax(best, bi);
          okw = (i == 0 && tgt >= 0 && bi == tgt) ? 1u : 0u;
        }
      }
      if (GRAD) {
        // d2 is -gl at the label and 0 elsewhere: its row sum is exact
        const float s2g = grp_sum(mine ? -gl : 0.f);
        float s1 = 0.f;
        for (int ct = 0; ct < NCT; ++ct) {
          const int c = 16 * ct + i;
          const float lp2 = (zr[16 * ct] - lse) - lse2;
          const float d2 = c == tgt ? -gl : 0.f;
          if (c < C) s1 += d2 - expf(lp2) * s2g;
        }
        s1 = grp_sum(s1);
        for (int ct = 0; ct < NCT; ++ct) {
          const int c = 16 * ct + i;
          const float lp = zr[16 * ct] - lse, lp2 = lp - lse2;
          const float d2 = c == tgt ? -gl : 0.f;
          const float d1 = d2 - expf(lp2) * s2g;
          zr[16 * ct] = (c < C && r < a.n) ? d1 - expf(lp) * s1 : 0.f;
        }
      }
    }
    if (LOSS) {  // the wave's terms, then the tile's in wave order (below)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) lw += __shfl_down(lw, o, kWave);
      if (lane == 0) wl[w] = lw;
      if (a.cpart) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) okw += __shfl_down(okw, o, kWave);
        if (lane == 0) wc[w] = okw;
      }
    }
    __syncthreads();
    if (LOSS && threadIdx.x == 0) {
      float l = 0.f;
      uint32_t c = 0;
      for (int q = 0; q < NW; ++q) {
        l += wl[q];
        if (a.cpart) c += wc[q];
      }
      a.lpart[tile] = l;
      if (a.cpart) a.cpart[tile] = c;
    }
    if (GRAD) {
      const bool first = tile == (int)blockIdx.x;
      // ---- dY [16 x K] = dZ W^T: this wave's k tiles, two at a time
      for (int kt0 = w; kt0 < nkt; kt0 += 2 * NW) {
        const bool has1 = kt0 + NW < nkt;
        const float* w0 = a.W + (size_t)(16 * kt0 + i) * C;
        const float* w1 = a.W + (size_t)(16 * (has1 ? kt0 + NW : kt0) + i) * C;
        constexpr int B = 8;  // class steps of 4 per round
        float b0[B], b1[B], n0[B], n1[B];
#pragma unroll
        for (int u = 0; u < B; ++u) {
          const int c = 4 * u + g;
          b0[u] = c < C ? w0[c] : 0.f;
          b1[u] = c < C ? w1[c] : 0.f;
        }
        f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
        for (int c1 = 0; c1 < CP; c1 += 4 * B) {
#pragma unroll
          for (int u = 0; u < B; ++u) {
            const int c = c1 + 4 * B + 4 * u + g;
            n0[u] = c < C ? w0[c] : 0.f;
            n1[u] = c < C ? w1[c] : 0.f;
          }
#pragma unroll
          for (int u = 0; u < B; ++u) {
            const int c = c1 + 4 * u + g;
            const float av = c < C ? sZ[i * PZ + c] : 0.f;
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0[u], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1[u], d1, 0, 0, 0);
          }
#pragma unroll
          for (int u = 0; u < B; ++u) {
            b0[u] = n0[u];
            b1[u] = n1[u];
          }
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int rr = r0 + 4 * g + v;
          if (rr < a.n) {
            a.dY[(uint64_t)rr * K + 16 * kt0 + i] = d0[v];
            if (has1) a.dY[(uint64_t)rr * K + 16 * (kt0 + NW) + i] = d1[v];
          }
        }
      }
      // ---- dW slab [K x CP] += Y^T dZ: the rows of this wave's k tiles
      for (int kt = w; kt < nkt; kt += NW) {
        float av[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) av[s4] = sY[(4 * s4 + g) * P + 16 * kt + i];
        for (int ct0 = 0; ct0 < NCT; ct0 += 2) {
          const bool has1 = ct0 + 1 < NCT;
          const int ct1 = has1 ? ct0 + 1 : ct0;
          f32x4 e0 = {0.f, 0.f, 0.f, 0.f}, e1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) {
            const float* dzr = sZ + (4 * s4 + g) * PZ + i;
            e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4], dzr[16 * ct0], e0, 0, 0, 0);
            e1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4], dzr[16 * ct1], e1, 0, 0, 0);
          }
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const uint64_t q = (uint64_t)(16 * kt + 4 * g + v) * NCT + ct0;
            float* p0 = a.part + (q * nslab + slab) * 16 + i;
            float* p1 = a.part + ((q + 1) * nslab + slab) * 16 + i;
            if (first) {
              *p0 = e0[v];
              if (has1) *p1 = e1[v];
            } else {  // a later tile of the walk: onto the slab, in walk order
              *p0 += e0[v];
              if (has1) *p1 += e1[v];
            }
          }
        }
      }
    }
    __syncthreads();  // sY, sZ and the waves' terms are rewritten by the next tile
  }
}

// ---- multi-label output layer: Z = Y W + mean sigmoid-BCE --------------------
// The same block shape as k_top_xent_ks (16 rows, the waves split K, W in LDS,
// the three products on v_mfma_f32_16x16x4_f32) with an element-wise middle:
//   loss = mean over the n C entries of max(z, 0) - z t + log1p(exp(-|z|))
//   dZ   = (sigmoid(z) - t) / (n C)
// and the micro-F1 counters of the prediction z > 0: true positives, false
// positives, false negatives.  Targets are bits: label c of vertex u is bit
// c & 31 of bits[u * wpr + (c >> 5)]; bits at positions >= C are ignored.  Row
// r reads vertex index[r] (the batch's seeds), or r itself without an index.
struct BceArgs {
  const float* Y;
  uint64_t ldy;
  const float* W;
  const uint32_t* bits;   // [V x wpr] packed targets
  const uint32_t* index;  // [n] vertex of each row, or nullptr
  uint32_t wpr;
  int n, K, C;
  float* lpart;     // [blocks] loss partials
  float* part;      // GRAD: dW partials [K][Cp/16][blocks][16]
  float* dY;        // GRAD: [n x K]
  uint32_t* cpart;  // [blocks][3] tp, fp, fn partials, or nullptr
};

// the K-split tiles plus the waves' loss and counter terms (no static LDS:
// the whole 160 KB is the dynamic segment's to use)
static inline size_t top_bce_lds(int K, int Cp) {
  return top_ks_lds(K, Cp) + (size_t)4 * kTopWaves * sizeof(float);
}

template <int NCT, bool GRAD, bool VEC4>
__global__ __launch_bounds__(kTopThreads) void k_top_bce_ks(BceArgs a) {
  constexpr int CP = 16 * NCT, NW = kTopWaves, NWD = (NCT + 1) / 2;  // label words per row
  extern __shared__ float smem[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int K = a.K, P = K + 4;
  float* sW = smem;                // [K][CP]
  float* sY = sW + K * CP;         // [16][K + 4]
  float* zp = sY + 16 * P;         // [NW][16][CP] partial logits
  float* dz = zp + NW * 16 * CP;   // [16][CP]
  float* wl = dz + 16 * CP;        // [NW] loss terms of the waves
  uint32_t* wc = reinterpret_cast<uint32_t*>(wl + NW);  // [NW][3]
  const int r0 = blockIdx.x * 16;
  constexpr int VPW = 4 / NW;  // rows 4 g + v per lane group finished by this wave
  static_assert(4 % NW == 0, "kTopWaves must divide 4");
  // the rows' label words first (index, then the words: two dependent loads
  // that overlap the staging)
  uint32_t tw[VPW][NWD];
#pragma unroll
  for (int vv = 0; vv < VPW; ++vv) {
    const int r = r0 + 4 * g + w + vv * NW;
    const uint64_t u = r < a.n ? (a.index ? (uint64_t)a.index[r] : (uint64_t)r) : 0;
#pragma unroll
    for (int j = 0; j < NWD; ++j)
      tw[vv][j] = (r < a.n && 32 * j < a.C) ? a.bits[u * a.wpr + j] : 0u;
  }
  const float gl = 1.0f / ((float)a.n * (float)a.C);
  stage_y_tile<VEC4>(a, sY, r0);
  stage_w<CP>(a, sW);
  __syncthreads();
  split_logits<NCT>(K, sW, sY, zp, w, i, g);
  __syncthreads();
  // each wave finishes the rows 4 g + v of its own v: the logits' sum over the
  // waves' k-splits in wave order, then the element-wise terms
  float lw = 0.f;
  uint32_t tp = 0, fp = 0, fn = 0;
#pragma unroll
  for (int vv = 0; vv < VPW; ++vv) {
    const int v = w + vv * NW, r = r0 + 4 * g + v;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const int c = 16 * ct + i;
      float z = zp[(4 * g + v) * CP + c];
#pragma unroll
      for (int q = 1; q < NW; ++q) z += zp[(q * 16 + 4 * g + v) * CP + c];
      const bool on = c < a.C && r < a.n;
      const bool t = (tw[vv][ct >> 1] >> (c & 31)) & 1u;
      const float e = expf(-fabsf(z));  // in (0, 1]: nothing overflows
      if (on) {
        lw += (fmaxf(z, 0.f) - (t ? z : 0.f)) + log1pf(e);
        const bool pos = z > 0.f;
        tp += (pos && t) ? 1u : 0u;
        fp += (pos && !t) ? 1u : 0u;
        fn += (!pos && t) ? 1u : 0u;
      }
      if (GRAD) {
        const float sg = (z >= 0.f ? 1.0f : e) / (1.0f + e);  // sigmoid(z)
        dz[(4 * g + v) * CP + c] = on ? (sg - (t ? 1.0f : 0.f)) * gl : 0.f;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lw += __shfl_down(lw, o, kWave);
    tp += __shfl_down(tp, o, kWave);
    fp += __shfl_down(fp, o, kWave);
    fn += __shfl_down(fn, o, kWave);
  }
  if (lane == 0) {
    wl[w] = lw;
    wc[3 * w] = tp;
    wc[3 * w + 1] = fp;
    wc[3 * w + 2] = fn;
  }
  __syncthreads();
  if (GRAD) grad_products<NCT>(a, sW, sY, dz, r0, w, i, g);
  if (threadIdx.x == 0) {  // the block's terms in wave order
    float l = 0.f;
    uint32_t c[3] = {0, 0, 0};
    for (int q = 0; q < NW; ++q) {
      l += wl[q];
      for (int k = 0; k < 3; ++k) c[k] += wc[3 * q + k];
    }
    a.lpart[blockIdx.x] = l;
    if (a.cpart)
      for (int k = 0; k < 3; ++k) a.cpart[3 * (uint64_t)blockIdx.x + k] = c[k];
  }
}

// Blocks [0, K*NCT): dW chunk (k, ct) = sum over the wave slabs — thread
// (sg, i) sums slabs sg, sg+16, ... in order (40 loads in flight), then a fixed
// pairwise tree over the 16 slab groups.  Block K*NCT (or 0 without GRAD):
// loss = (sum of block partials, fixed tree) / denom, and the NCNT counters
// of every block (cpart [blocks][NCNT]) added to correct[0 .. NCNT).
template <int NCT, int NCNT>
__global__ __launch_bounds__(256) void k_top_finish(const float* __restrict__ part, int nslab,
                                                    const float* __restrict__ lpart, int nblk,
                                                    float denom, int C, int nchunks,
                                                    float* __restrict__ dW, float* loss,
                                                    const uint32_t* __restrict__ cpart,
                                                    uint32_t* correct) {
  __shared__ float red[256];
  const int t = threadIdx.x;
  float acc = 0.f;
  if ((int)blockIdx.x < nchunks) {
    const int q = blockIdx.x, sg = t >> 4, i = t & 15;
    const float* p = part + (uint64_t)q * nslab * 16 + i;
    // every load of a thread in flight at once up to 640 slabs (C2: 625; the
    // sum order is unchanged: z ascending)
    constexpr int B = 40;
    for (int z = sg; z < nslab; z += 16 * B) {
      float v[B];
#pragma unroll
      for (int u = 0; u < B; ++u) v[u] = z + 16 * u < nslab ? p[(uint64_t)(z + 16 * u) * 16] : 0.f;
#pragma unroll
      for (int u = 0; u < B; ++u)
        if (z + 16 * u < nslab) acc += v[u];
    }
    red[t] = acc;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 16; h >>= 1) {
      if (t < h) red[t] += red[t + h];
      __syncthreads();
    }
    // NCT == 0: the wide form's column-tile count (5 .. 32), from C at run time
    const int nct = NCT ? NCT : (C + 15) / 16;
    const int k = q / nct, c = 16 * (q % nct) + t;
    if (t < 16 && c < C) dW[(uint64_t)k * C + c] = red[t];
  } else {
    uint32_t c[NCNT] = {};
    for (int b = t; b < nblk; b += 256) {
      acc += lpart[b];
      if (cpart)
#pragma unroll
        for (int k = 0; k < NCNT; ++k) c[k] += cpart[(uint64_t)b * NCNT + k];
    }
    red[t] = acc;
    __shared__ uint32_t cred[NCNT][256];
#pragma unroll
    for (int k = 0; k < NCNT; ++k) cred[k][t] = c[k];
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
      if (t < h) {
        red[t] += red[t + h];
#pragma unroll
        for (int k = 0; k < NCNT; ++k) cred[k][t] += cred[k][t + h];
      }
      __syncthreads();
    }
    if (t == 0) {
      *loss = red[0] / denom;
      if (correct)  // accumulates over batches
#pragma unroll
        for (int k = 0; k < NCNT; ++k) correct[k] += cred[k][0];
    }
  }
}

template <int NCT, bool LOSS, bool GRAD>
static int launch_top(hipStream_t st, int nblk, const TopArgs& a) {
  const size_t lds = top_ks_lds(a.K, 16 * NCT);
  const bool v4 = a.ldy % 4 == 0 && (uintptr_t)a.Y % 16 == 0;
  const void* f = v4 ? reinterpret_cast<const void*>(&k_top_xent_ks<NCT, LOSS, GRAD, true>)
                     : reinterpret_cast<const void*>(&k_top_xent_ks<NCT, LOSS, GRAD, false>);
  NTS_HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (v4)
    hipLaunchKernelGGL((k_top_xent_ks<NCT, LOSS, GRAD, true>), dim3(nblk), dim3(kTopThreads), lds,
                       st, a);
  else
    hipLaunchKernelGGL((k_top_xent_ks<NCT, LOSS, GRAD, false>), dim3(nblk), dim3(kTopThreads), lds,
                       st, a);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

template <bool LOSS, bool GRAD>
static int launch_top_any(hipStream_t st, int nblk, int Cp, const TopArgs& a) {
  switch (Cp / 16) {
    case 1: return launch_top<1, LOSS, GRAD>(st, nblk, a);
    case 2: return launch_top<2, LOSS, GRAD>(st, nblk, a);
    case 3: return launch_top<3, LOSS, GRAD>(st, nblk, a);
    default: return launch_top<4, LOSS, GRAD>(st, nblk, a);
  }
}

template <bool LOSS, bool GRAD>
static int launch_top_wide(hipStream_t st, int nblk, int Cp, const TopArgs& a) {
  const size_t lds = top_wide_lds(a.K, Cp);
  const bool v4 = a.ldy % 4 == 0 && (uintptr_t)a.Y % 16 == 0;
  const void* f = v4 ? reinterpret_cast<const void*>(&k_top_xent_wide<LOSS, GRAD, true>)
                     : reinterpret_cast<const void*>(&k_top_xent_wide<LOSS, GRAD, false>);
  NTS_HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (v4)
    hipLaunchKernelGGL((k_top_xent_wide<LOSS, GRAD, true>), dim3(nblk), dim3(kTopThreads), lds, st,
                       a);
  else
    hipLaunchKernelGGL((k_top_xent_wide<LOSS, GRAD, false>), dim3(nblk), dim3(kTopThreads), lds, st,
                       a);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

template <int NCT, bool GRAD>
static int launch_bce(hipStream_t st, int nblk, const BceArgs& a) {
  const size_t lds = top_bce_lds(a.K, 16 * NCT);
  const bool v4 = a.ldy % 4 == 0 && (uintptr_t)a.Y % 16 == 0;
  const void* f = v4 ? reinterpret_cast<const void*>(&k_top_bce_ks<NCT, GRAD, true>)
                     : reinterpret_cast<const void*>(&k_top_bce_ks<NCT, GRAD, false>);
  NTS_HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (v4)
    hipLaunchKernelGGL((k_top_bce_ks<NCT, GRAD, true>), dim3(nblk), dim3(kTopThreads), lds, st, a);
  else
    hipLaunchKernelGGL((k_top_bce_ks<NCT, GRAD, false>), dim3(nblk), dim3(kTopThreads), lds, st, a);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

template <bool GRAD>
static int launch_bce_any(hipStream_t st, int nblk, int Cp, const BceArgs& a) {
  switch (Cp / 16) {
    case 1: return launch_bce<1, GRAD>(st, nblk, a);
    case 2: return launch_bce<2, GRAD>(st, nblk, a);
    case 3: return launch_bce<3, GRAD>(st, nblk, a);
    case 4: return launch_bce<4, GRAD>(st, nblk, a);
    case 5: return launch_bce<5, GRAD>(st, nblk, a);
    case 6: return launch_bce<6, GRAD>(st, nblk, a);
    case 7: return launch_bce<7, GRAD>(st, nblk, a);
    default: return launch_bce<8, GRAD>(st, nblk, a);
  }
}

// NCNT: counters per block (1: the xent rows whose argmax is the label; 3: the
// BCE tp / fp / fn); denom: what the summed loss partials are divided by
template <int NCNT>
static int launch_finish(hipStream_t st, int Cp, const float* part, int nslab, const float* lpart,
                         int nblk, float denom, int K, int C, bool grad, bool loss_on, float* dW,
                         float* loss, const uint32_t* cpart, uint32_t* correct,
                         bool wide = false) {
  const int nchunks = grad ? K * (Cp / 16) : 0;
  const dim3 grid(nchunks + (loss_on ? 1 : 0));
#define NTS_F(NCT)                                                                            \
  hipLaunchKernelGGL((k_top_finish<NCT, NCNT>), grid, dim3(256), 0, st, part, nslab, lpart, nblk, \
                     denom, C, nchunks, dW, loss, cpart, correct)
  if constexpr (NCNT == 1) {
    if (wide) {  // the wide xent form (Cp = 80 .. 512): never the switch's default
      NTS_F(0);
      NTS_LAUNCH_CHECK();
      return NTS_OK;
    }
  }
  switch (Cp / 16) {
    case 1: NTS_F(1); break;
    case 2: NTS_F(2); break;
    case 3: NTS_F(3); break;
    case 4: NTS_F(4); break;
    case 5: NTS_F(5); break;
    case 6: NTS_F(6); break;
    case 7: NTS_F(7); break;
    default: NTS_F(8); break;
  }
#undef NTS_F
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

}  // namespace nts_hip

using namespace nts_hip;

extern "C" {

static int top_check(nts_hip_ctx* ctx, int n, int K, int C, uint64_t ldy) {
  NTS_CHECK_ARG(n > 0 && K > 0 && C > 0 && ldy >= (uint64_t)K, "shape");
  NTS_CHECK_ARG(C <= kWideMaxC, "class count above 512 is not supported by the fused loss");
  NTS_CHECK_ARG(K % 16 == 0, "the fused loss needs K % 16 == 0");
  if (C > kWave)  // the wide form: W is not held in LDS, (K, Cp) = (512, 512) takes 66,112 bytes
    NTS_CHECK_ARG(K <= kWideMaxK, "K above 512 is not supported by the fused loss above 64 classes");
  else
    NTS_CHECK_ARG(top_lds(K, (C + 15) / 16 * 16) <= 160 * 1024, "K x C too large for the fused loss");
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  return NTS_OK;
}

// 64 < C <= 512: k_top_xent_wide + the finish at its run-time tile count.
// scratch: [loss partials per row tile, 64-float aligned][correct partials]
//          [dW slabs: min(ceil(n / 16), 128 MiB / (4 K Cp)) x K x Cp floats]
static int top_run_wide(nts_hip_ctx* ctx, bool loss_on, bool grad_on, const float* Y, uint64_t ldy,
                        int n, int K, const float* W, int C, const int64_t* labels,
                        const float* grad_loss, float* loss, float* dY, float* dW,
                        uint32_t* correct) {
  const int Cp = (C + 15) / 16 * 16;
  const int ntiles = (n + 15) / 16, nblk = wide_blocks(ntiles, K, Cp);
  const size_t lp = ((size_t)ntiles + 63) / 64 * 64;
  NTS_RET(ensure_scratch(
      ctx, (2 * lp + (grad_on ? (size_t)nblk * K * Cp : 0)) * sizeof(float)));
  float* base = (float*)ctx->scratch;
  uint32_t* cpart = (loss_on && correct) ? reinterpret_cast<uint32_t*>(base + lp) : nullptr;
  TopArgs a{Y, ldy, W, labels, grad_loss, n, K, C, base, base + 2 * lp, dY, cpart};
  hipStream_t st = ctx->stream;
  if (loss_on && grad_on) NTS_RET((launch_top_wide<true, true>(st, nblk, Cp, a)));
  else if (loss_on) NTS_RET((launch_top_wide<true, false>(st, nblk, Cp, a)));
  else NTS_RET((launch_top_wide<false, true>(st, nblk, Cp, a)));
  return launch_finish<1>(st, Cp, a.part, nblk, a.lpart, ntiles, (float)n, K, C, grad_on, loss_on,
                          dW, loss, cpart, cpart ? correct : nullptr, true);
}

// scratch: [loss partials, 64-float aligned][correct partials][dW partial chunks]
static int top_run(nts_hip_ctx* ctx, bool loss_on, bool grad_on, const float* Y, uint64_t ldy,
                   int n, int K, const float* W, int C, const int64_t* labels,
                   const float* grad_loss, float* loss, float* dY, float* dW, uint32_t* correct) {
  NTS_RET(top_check(ctx, n, K, C, ldy));
  if (C > kWave)  // never launch_top_any's default
    return top_run_wide(ctx, loss_on, grad_on, Y, ldy, n, K, W, C, labels, grad_loss, loss, dY, dW,
                        correct);
  const int Cp = (C + 15) / 16 * 16;
  const int nblk = (n + 15) / 16, nslab = nblk;  // one dW slab per 16-row block
  const size_t lp = ((size_t)nblk + 63) / 64 * 64;
  NTS_RET(ensure_scratch(
      ctx, (2 * lp + (grad_on ? (size_t)nslab * K * Cp : 0)) * sizeof(float)));
  float* base = (float*)ctx->scratch;
  uint32_t* cpart = (loss_on && correct) ? reinterpret_cast<uint32_t*>(base + lp) : nullptr;
  TopArgs a{Y, ldy, W, labels, grad_loss, n, K, C, base, base + 2 * lp, dY, cpart};
  hipStream_t st = ctx->stream;
  if (loss_on && grad_on) NTS_RET((launch_top_any<true, true>(st, nblk, Cp, a)));
  else if (loss_on) NTS_RET((launch_top_any<true, false>(st, nblk, Cp, a)));
  else NTS_RET((launch_top_any<false, true>(st, nblk, Cp, a)));
  return launch_finish<1>(st, Cp, a.part, nslab, a.lpart, nblk, (float)n, K, C, grad_on, loss_on,
                          dW, loss, cpart, cpart ? correct : nullptr);
}

int nts_hip_linear_xent_fwd(nts_hip_ctx* ctx, const float* Y, uint64_t ldy, int n, int K,
                            const float* W, int C, const int64_t* labels, float* loss,
                            uint32_t* correct) {
  NTS_CHECK_ARG(ctx && Y && W && labels && loss, "NULL argument");
  return top_run(ctx, true, false, Y, ldy, n, K, W, C, labels, nullptr, loss, nullptr, nullptr,
                 correct);
}

int nts_hip_linear_xent_bwd(nts_hip_ctx* ctx, const float* Y, uint64_t ldy, int n, int K,
                            const float* W, int C, const int64_t* labels, const float* grad_loss,
                            float* dY, float* dW) {
  NTS_CHECK_ARG(ctx && Y && W && labels && grad_loss && dY && dW, "NULL argument");
  return top_run(ctx, false, true, Y, ldy, n, K, W, C, labels, grad_loss, nullptr, dY, dW,
                 nullptr);
}

int nts_hip_linear_xent_train(nts_hip_ctx* ctx, const float* Y, uint64_t ldy, int n, int K,
                              const float* W, int C, const int64_t* labels, float* loss,
                              float* dY, float* dW, uint32_t* correct) {
  NTS_CHECK_ARG(ctx && Y && W && labels && loss && dY && dW, "NULL argument");
  return top_run(ctx, true, true, Y, ldy, n, K, W, C, labels, nullptr, loss, dY, dW, correct);
}

// ---- multi-label output layer -------------------------------------------------
static int bce_check(nts_hip_ctx* ctx, int n, int K, int C, uint64_t ldy, uint32_t wpr) {
  NTS_CHECK_ARG(n > 0 && K > 0 && C > 0 && ldy >= (uint64_t)K, "shape");
  NTS_CHECK_ARG(C <= 128, "label count above 128 is not supported by the fused BCE loss");
  NTS_CHECK_ARG(wpr >= (uint32_t)(C + 31) / 32, "label_bits rows need ceil(C / 32) words");
  NTS_CHECK_ARG(K % 16 == 0, "the fused BCE loss needs K % 16 == 0");
  NTS_CHECK_ARG(top_bce_lds(K, (C + 15) / 16 * 16) <= 160 * 1024,
                "K x C too large for the fused BCE loss");
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  return NTS_OK;
}

// scratch: [loss partials, 64-float aligned][3 counter partials per block][dW partial chunks]
static int bce_run(nts_hip_ctx* ctx, bool grad_on, const float* Y, uint64_t ldy, int n, int K,
                   const float* W, int C, const uint32_t* label_bits, uint32_t wpr,
                   const uint32_t* index, float* loss, float* dY, float* dW, uint32_t* counts) {
  NTS_RET(bce_check(ctx, n, K, C, ldy, wpr));
  const int Cp = (C + 15) / 16 * 16;
  const int nblk = (n + 15) / 16, nslab = nblk;  // one dW slab per 16-row block
  const size_t lp = ((size_t)nblk + 63) / 64 * 64;
  NTS_RET(ensure_scratch(
      ctx, (4 * lp + (grad_on ? (size_t)nslab * K * Cp : 0)) * sizeof(float)));
  float* base = (float*)ctx->scratch;
  uint32_t* cpart = counts ? reinterpret_cast<uint32_t*>(base + lp) : nullptr;
  BceArgs a{Y, ldy, W, label_bits, index, wpr, n, K, C, base, base + 4 * lp, dY, cpart};
  hipStream_t st = ctx->stream;
  if (grad_on) NTS_RET((launch_bce_any<true>(st, nblk, Cp, a)));
  else NTS_RET((launch_bce_any<false>(st, nblk, Cp, a)));
  return launch_finish<3>(st, Cp, a.part, nslab, a.lpart, nblk, (float)n * (float)C, K, C, grad_on,
                          true, dW, loss, cpart, counts);
}

int nts_hip_linear_bce_fwd(nts_hip_ctx* ctx, const float* Y, uint64_t ldy, int n, int K,
                           const float* W, int C, const uint32_t* label_bits, uint32_t wpr,
                           const uint32_t* index, float* loss, uint32_t* counts) {
  NTS_CHECK_ARG(ctx && Y && W && label_bits && loss, "NULL argument");
  return bce_run(ctx, false, Y, ldy, n, K, W, C, label_bits, wpr, index, loss, nullptr, nullptr,
                 counts);
}

int nts_hip_linear_bce_train(nts_hip_ctx* ctx, const float* Y, uint64_t ldy, int n, int K,
                             const float* W, int C, const uint32_t* label_bits, uint32_t wpr,
                             const uint32_t* index, float* loss, float* dY, float* dW,
                             uint32_t* counts) {
  NTS_CHECK_ARG(ctx && Y && W && label_bits && loss && dY && dW, "NULL argument");
  return bce_run(ctx, true, Y, ldy, n, K, W, C, label_bits, wpr, index, loss, dY, dW, counts);
}

}  // extern "C"
