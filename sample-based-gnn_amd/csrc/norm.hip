// LayerNorm + relu + dropout of a hidden layer in one pass (GCNConfig::layer_norm,
// DESIGN §8l): the forward, and the backward with its parameter gradients.
//   k_ln_act_fwd  one wave per row, the row held in registers: read once,
//                 mean -> centred row -> variance -> gamma/beta -> relu ->
//                 dropout (the GEMM epilogue's keep bits) -> written once
//   k_ln_act_bwd  one wave per row for dz; each block owns a contiguous run of
//                 rows and writes its [2F] dgamma | dbeta partial
//   k_ln_param_reduce  sums the partials in a fixed order
// Every wave reduction is a __shfl_xor butterfly (a fixed lane order, the same
// bits in every lane); no atomics anywhere, so two calls give the same bytes.
#include "common.hpp"

namespace nts_hip {
namespace {

constexpr uint32_t kLnMaxF = 1024;      // 64 lanes x 16 floats of a row
constexpr int kLnWaves = 4;             // rows of a 256-thread block in flight
constexpr uint32_t kLnBwdBlocks = 1024; // the backward's block count stays at or under this
constexpr int kLnSegs = 4;              // k_ln_param_reduce: block segments per column

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// A lane's share of a row: N pieces of W columns (W = 4: one float4), piece i
// at columns (lane + 64 i) W ...  Pieces past F hold zeros.
template <int N, bool VEC>
struct Piece {
  static constexpr int W = VEC ? 4 : 1;
  static constexpr int E = N * W;
  static __device__ __forceinline__ uint32_t col(int lane, int i) {
    return (uint32_t)(lane + 64 * i) * W;
  }
  static __device__ __forceinline__ void load(const float* __restrict__ p, uint32_t F, int lane,
                                              float (&v)[E]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const uint32_t c = col(lane, i);
      if constexpr (VEC) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < F) t = *reinterpret_cast<const float4*>(p + c);
        v[4 * i] = t.x, v[4 * i + 1] = t.y, v[4 * i + 2] = t.z, v[4 * i + 3] = t.w;
      } else {
        v[i] = c < F ? p[c] : 0.f;
      }
    }
  }
  static __device__ __forceinline__ void store(float* __restrict__ p, uint32_t F, int lane,
                                               const float (&v)[E]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const uint32_t c = col(lane, i);
      if (c >= F) continue;
      if constexpr (VEC)
        *reinterpret_cast<float4*>(p + c) =
            make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
      else
        p[c] = v[i];
    }
  }
  static __device__ __forceinline__ float sum(const float (&v)[E]) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s += v[e];
    return s;
  }
};

// The centred row of z around `mu`, re-centred once: d = z - mu, d -= mean(d).
// mu is a float, so for a row far from zero it carries up to half an ulp of
// the row's size; the second step takes that out of the centred values.  The
// backward repeats these operations on the saved mu and gets the forward's
// bits.
template <int N, bool VEC>
__device__ __forceinline__ void centre(float (&d)[N * (VEC ? 4 : 1)], float mu, uint32_t F,
                                       int lane) {
  using P = Piece<N, VEC>;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const bool in = P::col(lane, i) < F;
#pragma unroll
    for (int j = 0; j < P::W; ++j) d[i * P::W + j] = in ? d[i * P::W + j] - mu : 0.f;
  }
  const float c = wave_sum(P::sum(d)) / (float)F;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const bool in = P::col(lane, i) < F;
#pragma unroll
    for (int j = 0; j < P::W; ++j) d[i * P::W + j] = in ? d[i * P::W + j] - c : 0.f;
  }
}

template <int N, bool VEC>
__global__ __launch_bounds__(64 * kLnWaves) void k_ln_act_fwd(
    uint64_t rows, uint32_t F, const float* __restrict__ z, uint64_t ldz,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    uint32_t keep_threshold, float scale, uint64_t seed, uint64_t offset, float* __restrict__ y,
    uint64_t ldy, float* __restrict__ mean, float* __restrict__ rstd) {
  using P = Piece<N, VEC>;
  const int lane = threadIdx.x & 63;
  const uint64_t r = (uint64_t)blockIdx.x * kLnWaves + threadIdx.x / kWave;
  if (r >= rows) return;
  float d[P::E];
  P::load(z + r * ldz, F, lane, d);
  const float mu = wave_sum(P::sum(d)) / (float)F;
  centre<N, VEC>(d, mu, F, lane);
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < P::E; ++e) q += d[e] * d[e];
  const float rs = 1.0f / sqrtf(wave_sum(q) / (float)F + eps);
  if (mean && lane == 0) mean[r] = mu;
  if (rstd && lane == 0) rstd[r] = rs;
  float ga[P::E], be[P::E];
  P::load(gamma, F, lane, ga);
  P::load(beta, F, lane, be);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint32_t c0 = P::col(lane, i);
    if (c0 >= F) continue;
#pragma unroll
    for (int j = 0; j < P::W; j += 2) {  // one generator call per column pair
      // (the scalar path's columns are 64 apart: a call each)
      uint32_t wd = 0;
      if (keep_threshold) {
        const uint4 rnd = dropout_words(r, c0 + j, seed, offset);
        const uint32_t k = (uint32_t)r & 3u;  // the row's word of the 4 x 2 block
        wd = k == 0 ? rnd.x : k == 1 ? rnd.y : k == 2 ? rnd.z : rnd.w;
      }
#pragma unroll
      for (int h = 0; h < (VEC ? 2 : 1); ++h) {
        const int e = i * P::W + j + h;
        const float a = ga[e] * (d[e] * rs) + be[e];
        d[e] = (dropout_bits(wd, c0 + j + h) >= keep_threshold && a > 0.f) ? a * scale : 0.f;
      }
    }
  }
  P::store(y + r * ldy, F, lane, d);
}

// Block b owns rows [b rpb, (b + 1) rpb), wave w of it the quarter
// [w rpb / 4, (w + 1) rpb / 4) of those, which it walks in row order with
// dgamma / dbeta in registers; the four waves' sums are then added in wave
// order through LDS and the block writes part[b] = [dgamma | dbeta].
template <int N, bool VEC>
__global__ __launch_bounds__(64 * kLnWaves) void k_ln_act_bwd(
    uint64_t rows, uint32_t F, uint32_t rpb, const float* __restrict__ dy, uint64_t lddy,
    const float* __restrict__ y, uint64_t ldy, const float* __restrict__ z, uint64_t ldz,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, float scale, float* __restrict__ dz, uint64_t lddz,
    float* __restrict__ part) {
  using P = Piece<N, VEC>;
  __shared__ float s_acc[2 * kLnMaxF];
  const int lane = threadIdx.x & 63, wave = threadIdx.x / kWave;
  const uint32_t rpw = rpb / kLnWaves;
  const uint64_t r0 = (uint64_t)blockIdx.x * rpb + (uint64_t)wave * rpw;
  const uint64_t r1 = min(r0 + rpw, rows);
  float ga[P::E], dg[P::E], db[P::E];
  P::load(gamma, F, lane, ga);
#pragma unroll
  for (int e = 0; e < P::E; ++e) dg[e] = db[e] = 0.f;
  for (uint64_t r = r0; r < r1; ++r) {
    float xh[P::E], g[P::E], yv[P::E];
    P::load(z + r * ldz, F, lane, xh);
    P::load(dy + r * lddy, F, lane, g);
    P::load(y + r * ldy, F, lane, yv);
    const float rs = rstd[r];
    centre<N, VEC>(xh, mean[r], F, lane);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < P::E; ++e) {
      xh[e] *= rs;
      g[e] = yv[e] > 0.f ? g[e] * scale : 0.f;
      db[e] += g[e];
      dg[e] += g[e] * xh[e];
      g[e] *= ga[e];  // t
      s1 += g[e];
      s2 += g[e] * xh[e];
    }
    s1 = wave_sum(s1) / (float)F;
    s2 = wave_sum(s2) / (float)F;
#pragma unroll
    for (int e = 0; e < P::E; ++e) g[e] = rs * ((g[e] - s1) - xh[e] * s2);
    P::store(dz + r * lddz, F, lane, g);
  }
  for (int w = 0; w < kLnWaves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const uint32_t c0 = P::col(lane, i);
        if (c0 >= F) continue;
#pragma unroll
        for (int j = 0; j < P::W; ++j) {
          const int e = i * P::W + j;
          s_acc[c0 + j] = w ? s_acc[c0 + j] + dg[e] : dg[e];
          s_acc[F + c0 + j] = w ? s_acc[F + c0 + j] + db[e] : db[e];
        }
      }
    }
    __syncthreads();
  }
  float* out = part + (uint64_t)blockIdx.x * 2 * F;
  for (uint32_t c = threadIdx.x; c < 2 * F; c += blockDim.x) out[c] = s_acc[c];
}

// out[c] = sum over blocks of part[b][c], c < 2F (dgamma | dbeta): the blocks
// in kLnSegs contiguous segments, each summed in block order by one thread,
// the segments then added in order.
__global__ __launch_bounds__(64 * kLnSegs) void k_ln_param_reduce(
    const float* __restrict__ part, uint32_t nblk, uint32_t F, float* __restrict__ dgamma,
    float* __restrict__ dbeta) {
  __shared__ float s_seg[kLnSegs][64];
  const uint32_t lane = threadIdx.x & 63, seg = threadIdx.x / 64;
  const uint32_t c = blockIdx.x * 64 + lane;
  const uint32_t per = (nblk + kLnSegs - 1) / kLnSegs;
  const uint32_t b0 = min(seg * per, nblk), b1 = min(b0 + per, nblk);
  float s = 0.f;
  if (c < 2 * F) {
#pragma unroll 8
    for (uint32_t b = b0; b < b1; ++b) s += part[(uint64_t)b * 2 * F + c];
  }
  s_seg[seg][lane] = s;
  __syncthreads();
  if (seg == 0 && c < 2 * F) {
    float t = s_seg[0][lane];
#pragma unroll
    for (int k = 1; k < kLnSegs; ++k) t += s_seg[k][lane];
    if (c < F) dgamma[c] = t;
    else dbeta[c - F] = t;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

// rows of one backward block: a function of `rows` alone (a multiple of the
// block's waves, at least 4 rows a wave), so the summation order of dgamma /
// dbeta never depends on the device
uint32_t ln_rows_per_block(uint64_t rows) {
  const uint64_t per = (rows + kLnBwdBlocks - 1) / kLnBwdBlocks;
  return (uint32_t)std::max<uint64_t>(16, (per + kLnWaves - 1) / kLnWaves * kLnWaves);
}

}  // namespace nts_hip

using namespace nts_hip;

#define NTS_LN_DISPATCH(KERNEL, vec, F, ...)                                              \
  do {                                                                                    \
    if (vec) {                                                                            \
      if ((F) <= 256) KERNEL(1, true, __VA_ARGS__);                                       \
      else if ((F) <= 512) KERNEL(2, true, __VA_ARGS__);                                  \
      else KERNEL(4, true, __VA_ARGS__);                                                  \
    } else {                                                                              \
      if ((F) <= 64) KERNEL(1, false, __VA_ARGS__);                                       \
      else if ((F) <= 256) KERNEL(4, false, __VA_ARGS__);                                 \
      else KERNEL(16, false, __VA_ARGS__);                                                \
    }                                                                                     \
  } while (0)

extern "C" {

int nts_hip_ln_act_fwd(nts_hip_ctx* ctx, uint64_t rows, uint32_t feature_size, const float* z,
                       uint64_t ldz, const float* gamma, const float* beta, float eps, float p,
                       uint64_t seed, uint64_t offset, float* y, uint64_t ldy, float* mean,
                       float* rstd) {
  NTS_CHECK_ARG(ctx && gamma && beta, "NULL argument");
  NTS_CHECK_ARG(feature_size >= 1 && feature_size <= kLnMaxF, "feature_size must be in [1, 1024]");
  NTS_CHECK_ARG((z && y) || rows == 0, "NULL rows");
  NTS_CHECK_ARG(ldz >= feature_size && ldy >= feature_size, "leading dimension");
  NTS_CHECK_ARG(p >= 0.f && p <= 1.f, "dropout probability must be in [0, 1]");
  NTS_CHECK_ARG(eps > 0.f, "eps must be positive");
  NTS_CHECK_ARG((uint64_t)(rows + kLnWaves - 1) / kLnWaves <= 0x7FFFFFFFull, "too many rows");
  if (rows == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const uint32_t F = feature_size;
  const bool vec = F % 4 == 0 && ldz % 4 == 0 && ldy % 4 == 0 && aligned16(z) && aligned16(y) &&
                   aligned16(gamma) && aligned16(beta);
  const uint32_t thr = dropout_threshold(p);
  const float scale = p >= 1.f ? 0.f : 1.0f / (1.0f - p);
  const dim3 grid((uint32_t)((rows + kLnWaves - 1) / kLnWaves));
#define NTS_LN_FWD(N, V, ...)                                                                  \
  hipLaunchKernelGGL((k_ln_act_fwd<N, V>), grid, dim3(64 * kLnWaves), 0, ctx->stream, rows, F, \
                     z, ldz, gamma, beta, eps, thr, scale, seed, offset, y, ldy, mean, rstd)
  NTS_LN_DISPATCH(NTS_LN_FWD, vec, F, 0);
#undef NTS_LN_FWD
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

int nts_hip_ln_act_bwd(nts_hip_ctx* ctx, uint64_t rows, uint32_t feature_size, const float* dy,
                       uint64_t lddy, const float* y, uint64_t ldy, const float* z, uint64_t ldz,
                       const float* mean, const float* rstd, const float* gamma, float scale,
                       float* dz, uint64_t lddz, float* dgamma, float* dbeta) {
  NTS_CHECK_ARG(ctx && gamma && dgamma && dbeta, "NULL argument");
  NTS_CHECK_ARG(feature_size >= 1 && feature_size <= kLnMaxF, "feature_size must be in [1, 1024]");
  NTS_CHECK_ARG((dy && y && z && mean && rstd && dz) || rows == 0, "NULL rows");
  NTS_CHECK_ARG(lddy >= feature_size && ldy >= feature_size && ldz >= feature_size &&
                    lddz >= feature_size,
                "leading dimension");
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const uint32_t F = feature_size;
  if (rows == 0) {
    NTS_HIP_TRY(hipMemsetAsync(dgamma, 0, F * sizeof(float), ctx->stream));
    NTS_HIP_TRY(hipMemsetAsync(dbeta, 0, F * sizeof(float), ctx->stream));
    return NTS_OK;
  }
  const uint32_t rpb = ln_rows_per_block(rows);
  const uint64_t nblk64 = (rows + rpb - 1) / rpb;
  NTS_CHECK_ARG(nblk64 <= kLnBwdBlocks, "too many rows");
  const uint32_t nblk = (uint32_t)nblk64;
  NTS_RET(ensure_scratch(ctx, (size_t)nblk * 2 * F * sizeof(float)));
  float* part = reinterpret_cast<float*>(ctx->scratch);
  const bool vec = F % 4 == 0 && lddy % 4 == 0 && ldy % 4 == 0 && ldz % 4 == 0 && lddz % 4 == 0 &&
                   aligned16(dy) && aligned16(y) && aligned16(z) && aligned16(dz) &&
                   aligned16(gamma);
#define NTS_LN_BWD(N, V, ...)                                                                   \
  hipLaunchKernelGGL((k_ln_act_bwd<N, V>), dim3(nblk), dim3(64 * kLnWaves), 0, ctx->stream,     \
                     rows, F, rpb, dy, lddy, y, ldy, z, ldz, mean, rstd, gamma, scale, dz, lddz, \
                     part)
  NTS_LN_DISPATCH(NTS_LN_BWD, vec, F, 0);
#undef NTS_LN_BWD
  NTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ln_param_reduce, dim3(ceil_div(2 * F, 64)), dim3(64 * kLnSegs), 0,
                     ctx->stream, part, nblk, F, dgamma, dbeta);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

}  // extern "C"
