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
//
// BatchNorm + relu + dropout (GCNConfig::batch_norm): the statistics
// run down the columns of a tall [rows, F] matrix, so a block is a tile of
// TX column threads x TY row threads (TX TY = 256, TX the power of two that
// covers the row's float4 or scalar pieces, wider rows in grid.y chunks) and
// owns a contiguous run of rows whose length depends on `rows` alone.
//   k_bn_stats       z read once: a Welford (count, mean, M2) of z - z[0, c]
//                    per thread over its rows in row order, the TY threads of
//                    a column merged in order by Chan's formula, one
//                    [mean | M2 | mean of z] partial a block
//   k_bn_finish      the partials merged in block order; mean, rstd and the
//                    running statistics written by the column's one thread
//   k_bn_apply       z -> y, elementwise (the GEMM epilogue's keep bits)
//   k_bn_eval        the same from the running statistics, no dropout
//   k_bn_bwd_reduce  dy, y, z read once: per-block partials of sum g,
//                    sum g (z - mean) rstd and sum (z - mean)
//   k_bn_param_reduce  the partials summed in block order -> dgamma, dbeta
//   k_bn_bwd_apply   dy, y, z -> dz, elementwise
// The saved mean is a float: for a column far from zero it carries up to half
// an ulp of the column's size.  The forward keeps what the rounding dropped
// (the statistics are those of z - z[0, c], small numbers) and the backward
// recovers it as mean_r (z - mean); both centre with it, xh = ((z - mean) - d) rstd.
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

// ---- BatchNorm ---------------------------------------------------------------
constexpr int kBnThreads = 256;
constexpr int kBnSegs = 16;  // k_bn_finish: block segments per column

// A thread's piece of a row: W columns from c0 (W = 4: one float4).
template <bool VEC>
struct BnPiece {
  static constexpr int W = VEC ? 4 : 1;
  static __device__ __forceinline__ void load(const float* __restrict__ p, float (&v)[W]) {
    if constexpr (VEC) {
      const float4 t = *reinterpret_cast<const float4*>(p);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
      v[0] = *p;
    }
  }
  static __device__ __forceinline__ void store(float* __restrict__ p, const float (&v)[W]) {
    if constexpr (VEC) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
  }
};

// (na, ma, Ma) <- (na, ma, Ma) merged with (nb, mb, Mb): Chan, Golub & LeVeque.
// Equal means give delta = 0: a constant column keeps M2 = 0 and its mean exactly.
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& Ma, float nb, float mb,
                                           float Mb) {
  if (nb == 0.f) return;
  if (na == 0.f) {
    na = nb, ma = mb, Ma = Mb;
    return;
  }
  const float n = na + nb, d = mb - ma, f = nb / n;
  ma += d * f;
  Ma = (Ma + Mb) + (d * d) * (na * f);
  na = n;
}

// ua <- the mean of na values of mean ua and nb of mean ub (na is chan_merge's to update)
__device__ __forceinline__ void mean_merge(float na, float& ua, float nb, float ub) {
  if (nb == 0.f) return;
  ua = na == 0.f ? ub : ua + (ub - ua) * (nb / (na + nb));
}

// Block b owns rows [b rpb, (b + 1) rpb); thread (tx, ry) of it walks rows
// ry, ry + TY, ... of the run in row order.  part[b] = [mean | M2] of the run's
// z - z[0, c], and the mean of the run's z itself.
template <bool VEC>
__global__ __launch_bounds__(kBnThreads) void k_bn_stats(uint64_t rows, uint32_t F, uint32_t rpb,
                                                         uint32_t lx, const float* __restrict__ z,
                                                         uint64_t ldz, float* __restrict__ part) {
  using P = BnPiece<VEC>;
  constexpr int W = P::W;
  __shared__ float s_n[kBnThreads], s_m[kBnThreads * W], s_q[kBnThreads * W], s_u[kBnThreads * W];
  const uint32_t TX = 1u << lx, TY = kBnThreads >> lx;
  const uint32_t tx = threadIdx.x & (TX - 1), ry = threadIdx.x >> lx;
  const uint32_t c0 = (blockIdx.y * TX + tx) * W;
  const uint64_t r0 = (uint64_t)blockIdx.x * rpb, r1 = min(r0 + rpb, rows);
  float m[W], q[W], u[W];  // mean and M2 of z - z[0, c]; u: the mean of z itself
#pragma unroll
  for (int j = 0; j < W; ++j) m[j] = q[j] = u[j] = 0.f;
  uint32_t k = 0;
  if (c0 < F) {
    float sh[W];  // the column's first value: every block centres on the same one
    P::load(z + c0, sh);
#pragma unroll 4
    for (uint64_t r = r0 + ry; r < r1; r += TY) {
      float x[W];
      P::load(z + r * ldz + c0, x);
      const float inv = 1.0f / (float)++k;
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const float v = x[j] - sh[j], d = v - m[j];
        m[j] += d * inv;
        q[j] += d * (v - m[j]);
        u[j] += (x[j] - u[j]) * inv;
      }
    }
  }
  s_n[threadIdx.x] = (float)k;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    s_m[threadIdx.x * W + j] = m[j];
    s_q[threadIdx.x * W + j] = q[j];
    s_u[threadIdx.x * W + j] = u[j];
  }
  __syncthreads();
  if (ry != 0 || c0 >= F) return;
  float n[W];
#pragma unroll
  for (int j = 0; j < W; ++j) n[j] = (float)k;
  for (uint32_t t = 1; t < TY; ++t) {
    const uint32_t o = (t << lx) + tx;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      mean_merge(n[j], u[j], s_n[o], s_u[o * W + j]);
      chan_merge(n[j], m[j], q[j], s_n[o], s_m[o * W + j], s_q[o * W + j]);
    }
  }
  float* out = part + (uint64_t)blockIdx.x * 3 * F + c0;
  P::store(out, m);
  P::store(out + F, q);
  P::store(out + 2 * F, u);
}

// One thread per (column, segment of the blocks): the segment's partials merged
// in block order, then the segments in order by the column's first thread, which
// alone writes mean, rstd and (rows > 1) the column's running statistics.
__global__ __launch_bounds__(64 * kBnSegs) void k_bn_finish(
    const float* __restrict__ part, uint32_t nblk, uint32_t rpb, uint64_t rows, uint32_t F,
    const float* __restrict__ z, float eps, float momentum, float* __restrict__ mean,
    float* __restrict__ rstd, float* __restrict__ resid, float* __restrict__ running_mean,
    float* __restrict__ running_var) {
  __shared__ float s_n[kBnSegs][64], s_m[kBnSegs][64], s_q[kBnSegs][64], s_u[kBnSegs][64];
  const uint32_t lane = threadIdx.x & 63, seg = threadIdx.x / 64;
  const uint32_t c = blockIdx.x * 64 + lane;
  const uint32_t per = (nblk + kBnSegs - 1) / kBnSegs;
  const uint32_t b0 = min(seg * per, nblk), b1 = min(b0 + per, nblk);
  float n = 0.f, m = 0.f, q = 0.f, u = 0.f;
  if (c < F) {
#pragma unroll 4
    for (uint32_t b = b0; b < b1; ++b) {
      const float nb = (float)min((uint64_t)rpb, rows - (uint64_t)b * rpb);
      const float* p = part + (uint64_t)b * 3 * F + c;
      mean_merge(n, u, nb, p[2 * F]);
      chan_merge(n, m, q, nb, p[0], p[F]);
    }
  }
  s_n[seg][lane] = n, s_m[seg][lane] = m, s_q[seg][lane] = q, s_u[seg][lane] = u;
  __syncthreads();
  if (seg != 0 || c >= F) return;
#pragma unroll
  for (int k = 1; k < kBnSegs; ++k) {
    mean_merge(n, u, s_n[k][lane], s_u[k][lane]);
    chan_merge(n, m, q, s_n[k][lane], s_m[k][lane], s_q[k][lane]);
  }
  // The mean is z[0, c] + m, good to a few ulp of |m|, or u, good to a few ulp of
  // |u|: the one with the smaller magnitude to round in.  (Far from zero the
  // shifted one, with what the float sum drops kept in resid; for a column
  // centred near zero the plain one.)
  const float sh = z[c];
  float mu = sh + m, dm = m - (mu - sh);
  if (fabsf(u) < fabsf(m)) mu = u, dm = 0.f;
  mean[c] = mu;
  resid[c] = dm;
  // (one thread a column: the root and the quotients in double, rounded once)
  const double var = (double)q / (double)n;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean && rows > 1) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mu;
  if (running_var && rows > 1)
    running_var[c] = (1.0f - momentum) * running_var[c] +
                     momentum * (float)((double)q / ((double)n - 1.0));
}

// y = keep ? relu(gamma (z - mean) rstd + beta) scale : 0, rows strided over the grid
template <bool VEC>
__global__ __launch_bounds__(kBnThreads) void k_bn_apply(
    uint64_t rows, uint32_t F, uint32_t lx, const float* __restrict__ z, uint64_t ldz,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ resid, uint32_t keep_threshold, float scale, uint64_t seed,
    uint64_t offset, float* __restrict__ y, uint64_t ldy) {
  using P = BnPiece<VEC>;
  constexpr int W = P::W;
  const uint32_t TX = 1u << lx, TY = kBnThreads >> lx;
  const uint32_t tx = threadIdx.x & (TX - 1), ry = threadIdx.x >> lx;
  const uint32_t c0 = (blockIdx.y * TX + tx) * W;
  if (c0 >= F) return;
  float ga[W], be[W], mu[W], rs[W], dm[W];
  P::load(gamma + c0, ga);
  P::load(beta + c0, be);
  P::load(mean + c0, mu);
  P::load(rstd + c0, rs);
  P::load(resid + c0, dm);
  for (uint64_t r = (uint64_t)blockIdx.x * TY + ry; r < rows; r += (uint64_t)gridDim.x * TY) {
    float v[W];
    P::load(z + r * ldz + c0, v);
#pragma unroll
    for (int j = 0; j < W; j += 2) {  // one generator call per column pair
      uint32_t wd = 0;
      if (keep_threshold) {
        const uint4 rnd = dropout_words(r, c0 + j, seed, offset);
        const uint32_t k = (uint32_t)r & 3u;  // the row's word of the 4 x 2 block
        wd = k == 0 ? rnd.x : k == 1 ? rnd.y : k == 2 ? rnd.z : rnd.w;
      }
#pragma unroll
      for (int h = 0; h < (VEC ? 2 : 1); ++h) {
        const int e = j + h;
        const float a = ga[e] * (((v[e] - mu[e]) - dm[e]) * rs[e]) + be[e];
        v[e] = (dropout_bits(wd, c0 + e) >= keep_threshold && a > 0.f) ? a * scale : 0.f;
      }
    }
    P::store(y + r * ldy + c0, v);
  }
}

// y = relu(gamma (z - running_mean) / sqrt(running_var + eps) + beta)
template <bool VEC>
__global__ __launch_bounds__(kBnThreads) void k_bn_eval(
    uint64_t rows, uint32_t F, uint32_t lx, const float* __restrict__ z, uint64_t ldz,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ running_mean, const float* __restrict__ running_var, float eps,
    float* __restrict__ y, uint64_t ldy) {
  using P = BnPiece<VEC>;
  constexpr int W = P::W;
  const uint32_t TX = 1u << lx, TY = kBnThreads >> lx;
  const uint32_t tx = threadIdx.x & (TX - 1), ry = threadIdx.x >> lx;
  const uint32_t c0 = (blockIdx.y * TX + tx) * W;
  if (c0 >= F) return;
  float ga[W], be[W], mu[W], rs[W];
  P::load(gamma + c0, ga);
  P::load(beta + c0, be);
  P::load(running_mean + c0, mu);
  P::load(running_var + c0, rs);
#pragma unroll
  for (int j = 0; j < W; ++j) rs[j] = 1.0f / sqrtf(rs[j] + eps);
  for (uint64_t r = (uint64_t)blockIdx.x * TY + ry; r < rows; r += (uint64_t)gridDim.x * TY) {
    float v[W];
    P::load(z + r * ldz + c0, v);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float a = ga[j] * ((v[j] - mu[j]) * rs[j]) + be[j];
      v[j] = a > 0.f ? a : 0.f;
    }
    P::store(y + r * ldy + c0, v);
  }
}

// The statistics kernel's tiling: part[b] = [sum g (z - mean) rstd | sum g |
// sum (z - mean)] of block b's rows, each thread's rows summed in row order, the
// TY threads of a column in order.
template <bool VEC>
__global__ __launch_bounds__(kBnThreads) void k_bn_bwd_reduce(
    uint64_t rows, uint32_t F, uint32_t rpb, uint32_t lx, const float* __restrict__ dy,
    uint64_t lddy, const float* __restrict__ y, uint64_t ldy, const float* __restrict__ z,
    uint64_t ldz, const float* __restrict__ mean, const float* __restrict__ rstd, float scale,
    float* __restrict__ part) {
  using P = BnPiece<VEC>;
  constexpr int W = P::W;
  __shared__ float s_g[kBnThreads * W], s_b[kBnThreads * W], s_c[kBnThreads * W];
  const uint32_t TX = 1u << lx, TY = kBnThreads >> lx;
  const uint32_t tx = threadIdx.x & (TX - 1), ry = threadIdx.x >> lx;
  const uint32_t c0 = (blockIdx.y * TX + tx) * W;
  const uint64_t r0 = (uint64_t)blockIdx.x * rpb, r1 = min(r0 + rpb, rows);
  float dg[W], db[W], dc[W];
#pragma unroll
  for (int j = 0; j < W; ++j) dg[j] = db[j] = dc[j] = 0.f;
  if (c0 < F) {
    float mu[W], rs[W];
    P::load(mean + c0, mu);
    P::load(rstd + c0, rs);
#pragma unroll 2
    for (uint64_t r = r0 + ry; r < r1; r += TY) {
      float g[W], yv[W], x[W];
      P::load(dy + r * lddy + c0, g);
      P::load(y + r * ldy + c0, yv);
      P::load(z + r * ldz + c0, x);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const float gj = yv[j] > 0.f ? g[j] * scale : 0.f, v = x[j] - mu[j];
        db[j] += gj;
        dg[j] += gj * (v * rs[j]);
        dc[j] += v;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < W; ++j) {
    s_g[threadIdx.x * W + j] = dg[j];
    s_b[threadIdx.x * W + j] = db[j];
    s_c[threadIdx.x * W + j] = dc[j];
  }
  __syncthreads();
  if (ry != 0 || c0 >= F) return;
  for (uint32_t t = 1; t < TY; ++t) {
    const uint32_t o = ((t << lx) + tx) * W;
#pragma unroll
    for (int j = 0; j < W; ++j) dg[j] += s_g[o + j], db[j] += s_b[o + j], dc[j] += s_c[o + j];
  }
  float* out = part + (uint64_t)blockIdx.x * 3 * F + c0;
  P::store(out, dg);
  P::store(out + F, db);
  P::store(out + 2 * F, dc);
}

// k_ln_param_reduce's order over the three sums of a column (the blocks in
// kLnSegs contiguous segments, each summed in block order by one thread, the
// segments then added in order), then with d = mean_r (z - mean):
//   dbeta = sum g,  dgamma = sum g ((z - mean) - d) rstd,  resid = d.
__global__ __launch_bounds__(64 * kLnSegs) void k_bn_param_reduce(
    const float* __restrict__ part, uint32_t nblk, uint32_t F, float n,
    const float* __restrict__ rstd, float* __restrict__ dgamma, float* __restrict__ dbeta,
    float* __restrict__ resid) {
  __shared__ float s_seg[kLnSegs][3][64];
  const uint32_t lane = threadIdx.x & 63, seg = threadIdx.x / 64;
  const uint32_t c = blockIdx.x * 64 + lane;
  const uint32_t per = (nblk + kLnSegs - 1) / kLnSegs;
  const uint32_t b0 = min(seg * per, nblk), b1 = min(b0 + per, nblk);
  float s[3] = {0.f, 0.f, 0.f};
  if (c < F) {
#pragma unroll 4
    for (uint32_t b = b0; b < b1; ++b) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] += part[((uint64_t)b * 3 + k) * F + c];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) s_seg[seg][k][lane] = s[k];
  __syncthreads();
  if (seg != 0 || c >= F) return;
#pragma unroll
  for (int g = 1; g < kLnSegs; ++g) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += s_seg[g][k][lane];
  }
  const float d = s[2] / n;
  dbeta[c] = s[1];
  dgamma[c] = s[0] - (rstd[c] * d) * s[1];
  resid[c] = d;
}

// dz = gamma rstd (g - dbeta / n - xh dgamma / n), rows strided over the grid
template <bool VEC>
__global__ __launch_bounds__(kBnThreads) void k_bn_bwd_apply(
    uint64_t rows, uint32_t F, uint32_t lx, const float* __restrict__ dy, uint64_t lddy,
    const float* __restrict__ y, uint64_t ldy, const float* __restrict__ z, uint64_t ldz,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, float scale, const float* __restrict__ dgamma,
    const float* __restrict__ dbeta, const float* __restrict__ resid, float* __restrict__ dz,
    uint64_t lddz) {
  using P = BnPiece<VEC>;
  constexpr int W = P::W;
  const uint32_t TX = 1u << lx, TY = kBnThreads >> lx;
  const uint32_t tx = threadIdx.x & (TX - 1), ry = threadIdx.x >> lx;
  const uint32_t c0 = (blockIdx.y * TX + tx) * W;
  if (c0 >= F) return;
  float mu[W], rs[W], a[W], mg[W], mb[W], dm[W];
  P::load(resid + c0, dm);
  P::load(mean + c0, mu);
  P::load(rstd + c0, rs);
  P::load(gamma + c0, a);
  P::load(dgamma + c0, mg);
  P::load(dbeta + c0, mb);
  const float n = (float)rows;
#pragma unroll
  for (int j = 0; j < W; ++j) a[j] *= rs[j], mg[j] /= n, mb[j] /= n;
  for (uint64_t r = (uint64_t)blockIdx.x * TY + ry; r < rows; r += (uint64_t)gridDim.x * TY) {
    float g[W], yv[W], x[W];
    P::load(dy + r * lddy + c0, g);
    P::load(y + r * ldy + c0, yv);
    P::load(z + r * ldz + c0, x);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float gj = yv[j] > 0.f ? g[j] * scale : 0.f;
      g[j] = a[j] * ((gj - mb[j]) - (((x[j] - mu[j]) - dm[j]) * rs[j]) * mg[j]);
    }
    P::store(dz + r * lddz + c0, g);
  }
}

// The tile of a [rows, F] BatchNorm kernel: lx = log2 of the column threads,
// grid.y the chunks of TX pieces a row needs.
struct BnTile {
  uint32_t lx, gy, ty;
};
BnTile bn_tile(uint32_t F, bool vec) {
  const uint32_t pieces = vec ? F / 4 : F;
  const uint32_t lx = std::min<uint32_t>(ceil_log2(pieces), 8);
  return {lx, ceil_div(pieces, 1u << lx), (uint32_t)kBnThreads >> lx};
}
// blocks of an elementwise pass: every row tile once, or the memory-bound cap
uint32_t bn_apply_blocks(uint64_t rows, const BnTile& t) {
  return (uint32_t)std::min<uint64_t>((rows + t.ty - 1) / t.ty, std::max(1u, kMaxGrid / t.gy));
}

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

int nts_hip_bn_act_fwd(nts_hip_ctx* ctx, uint64_t rows, uint32_t feature_size, const float* z,
                       uint64_t ldz, const float* gamma, const float* beta, float eps,
                       float momentum, float p, uint64_t seed, uint64_t offset, float* y,
                       uint64_t ldy, float* mean, float* rstd, float* running_mean,
                       float* running_var) {
  NTS_CHECK_ARG(ctx && gamma && beta, "NULL argument");
  NTS_CHECK_ARG(feature_size >= 1 && feature_size <= kLnMaxF, "feature_size must be in [1, 1024]");
  NTS_CHECK_ARG((z && y && mean && rstd) || rows == 0, "NULL rows or statistics");
  NTS_CHECK_ARG(ldz >= feature_size && ldy >= feature_size, "leading dimension");
  NTS_CHECK_ARG(p >= 0.f && p <= 1.f, "dropout probability must be in [0, 1]");
  NTS_CHECK_ARG(eps > 0.f, "eps must be positive");
  NTS_CHECK_ARG(momentum >= 0.f && momentum <= 1.f, "momentum must be in [0, 1]");
  NTS_CHECK_ARG(rows <= (1ull << 40), "too many rows");
  if (rows == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const uint32_t F = feature_size;
  const uint32_t rpb = ln_rows_per_block(rows);
  const uint32_t nblk = (uint32_t)((rows + rpb - 1) / rpb);
  NTS_RET(ensure_scratch(ctx, ((size_t)nblk * 3 + 1) * F * sizeof(float)));
  float* part = reinterpret_cast<float*>(ctx->scratch);
  float* resid = part + (size_t)nblk * 3 * F;  // [F]: what the float mean dropped
  // (the partials are float4-stored too: F % 4 == 0 keeps them aligned)
  const bool vec = F % 4 == 0 && ldz % 4 == 0 && ldy % 4 == 0 && aligned16(z) && aligned16(y) &&
                   aligned16(gamma) && aligned16(beta) && aligned16(mean) && aligned16(rstd) &&
                   aligned16(part);
  const BnTile t = bn_tile(F, vec);
  const uint32_t thr = dropout_threshold(p);
  const float scale = p >= 1.f ? 0.f : 1.0f / (1.0f - p);
  const dim3 block(kBnThreads), sgrid(nblk, t.gy), agrid(bn_apply_blocks(rows, t), t.gy);
  if (vec)
    hipLaunchKernelGGL(k_bn_stats<true>, sgrid, block, 0, ctx->stream, rows, F, rpb, t.lx, z, ldz,
                       part);
  else
    hipLaunchKernelGGL(k_bn_stats<false>, sgrid, block, 0, ctx->stream, rows, F, rpb, t.lx, z, ldz,
                       part);
  NTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bn_finish, dim3(ceil_div(F, 64)), dim3(64 * kBnSegs), 0, ctx->stream, part,
                     nblk, rpb, rows, F, z, eps, momentum, mean, rstd, resid, running_mean,
                     running_var);
  NTS_LAUNCH_CHECK();
  if (vec)
    hipLaunchKernelGGL(k_bn_apply<true>, agrid, block, 0, ctx->stream, rows, F, t.lx, z, ldz, gamma,
                       beta, mean, rstd, resid, thr, scale, seed, offset, y, ldy);
  else
    hipLaunchKernelGGL(k_bn_apply<false>, agrid, block, 0, ctx->stream, rows, F, t.lx, z, ldz,
                       gamma, beta, mean, rstd, resid, thr, scale, seed, offset, y, ldy);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

int nts_hip_bn_act_eval(nts_hip_ctx* ctx, uint64_t rows, uint32_t feature_size, const float* z,
                        uint64_t ldz, const float* gamma, const float* beta,
                        const float* running_mean, const float* running_var, float eps, float* y,
                        uint64_t ldy) {
  NTS_CHECK_ARG(ctx && gamma && beta && running_mean && running_var, "NULL argument");
  NTS_CHECK_ARG(feature_size >= 1 && feature_size <= kLnMaxF, "feature_size must be in [1, 1024]");
  NTS_CHECK_ARG((z && y) || rows == 0, "NULL rows");
  NTS_CHECK_ARG(ldz >= feature_size && ldy >= feature_size, "leading dimension");
  NTS_CHECK_ARG(eps > 0.f, "eps must be positive");
  if (rows == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const uint32_t F = feature_size;
  const bool vec = F % 4 == 0 && ldz % 4 == 0 && ldy % 4 == 0 && aligned16(z) && aligned16(y) &&
                   aligned16(gamma) && aligned16(beta) && aligned16(running_mean) &&
                   aligned16(running_var);
  const BnTile t = bn_tile(F, vec);
  const dim3 block(kBnThreads), agrid(bn_apply_blocks(rows, t), t.gy);
  if (vec)
    hipLaunchKernelGGL(k_bn_eval<true>, agrid, block, 0, ctx->stream, rows, F, t.lx, z, ldz, gamma,
                       beta, running_mean, running_var, eps, y, ldy);
  else
    hipLaunchKernelGGL(k_bn_eval<false>, agrid, block, 0, ctx->stream, rows, F, t.lx, z, ldz, gamma,
                       beta, running_mean, running_var, eps, y, ldy);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

int nts_hip_bn_act_bwd(nts_hip_ctx* ctx, uint64_t rows, uint32_t feature_size, const float* dy,
                       uint64_t lddy, const float* y, uint64_t ldy, const float* z, uint64_t ldz,
                       const float* mean, const float* rstd, const float* gamma, float scale,
                       float* dz, uint64_t lddz, float* dgamma, float* dbeta) {
  NTS_CHECK_ARG(ctx && gamma && dgamma && dbeta, "NULL argument");
  NTS_CHECK_ARG(feature_size >= 1 && feature_size <= kLnMaxF, "feature_size must be in [1, 1024]");
  NTS_CHECK_ARG((dy && y && z && mean && rstd && dz) || rows == 0, "NULL rows");
  NTS_CHECK_ARG(lddy >= feature_size && ldy >= feature_size && ldz >= feature_size &&
                    lddz >= feature_size,
                "leading dimension");
  NTS_CHECK_ARG(rows <= (1ull << 40), "too many rows");
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const uint32_t F = feature_size;
  if (rows == 0) {
    NTS_HIP_TRY(hipMemsetAsync(dgamma, 0, F * sizeof(float), ctx->stream));
    NTS_HIP_TRY(hipMemsetAsync(dbeta, 0, F * sizeof(float), ctx->stream));
    return NTS_OK;
  }
  const uint32_t rpb = ln_rows_per_block(rows);
  const uint32_t nblk = (uint32_t)((rows + rpb - 1) / rpb);
  NTS_RET(ensure_scratch(ctx, ((size_t)nblk * 3 + 1) * F * sizeof(float)));
  float* part = reinterpret_cast<float*>(ctx->scratch);
  float* resid = part + (size_t)nblk * 3 * F;  // [F]: mean_r (z - mean)
  const bool vec = F % 4 == 0 && lddy % 4 == 0 && ldy % 4 == 0 && ldz % 4 == 0 && lddz % 4 == 0 &&
                   aligned16(dy) && aligned16(y) && aligned16(z) && aligned16(dz) &&
                   aligned16(gamma) && aligned16(mean) && aligned16(rstd) && aligned16(dgamma) &&
                   aligned16(dbeta) && aligned16(part);
  const BnTile t = bn_tile(F, vec);
  const dim3 block(kBnThreads), rgrid(nblk, t.gy), agrid(bn_apply_blocks(rows, t), t.gy);
  if (vec)
    hipLaunchKernelGGL(k_bn_bwd_reduce<true>, rgrid, block, 0, ctx->stream, rows, F, rpb, t.lx, dy,
                       lddy, y, ldy, z, ldz, mean, rstd, scale, part);
  else
    hipLaunchKernelGGL(k_bn_bwd_reduce<false>, rgrid, block, 0, ctx->stream, rows, F, rpb, t.lx, dy,
                       lddy, y, ldy, z, ldz, mean, rstd, scale, part);
  NTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bn_param_reduce, dim3(ceil_div(F, 64)), dim3(64 * kLnSegs), 0, ctx->stream,
                     part, nblk, F, (float)rows, rstd, dgamma, dbeta, resid);
  NTS_LAUNCH_CHECK();
  if (vec)
    hipLaunchKernelGGL(k_bn_bwd_apply<true>, agrid, block, 0, ctx->stream, rows, F, t.lx, dy, lddy,
                       y, ldy, z, ldz, mean, rstd, gamma, scale, dgamma, dbeta, resid, dz, lddz);
  else
    hipLaunchKernelGGL(k_bn_bwd_apply<false>, agrid, block, 0, ctx->stream, rows, F, t.lx, dy, lddy,
                       y, ldy, z, ldz, mean, rstd, gamma, scale, dgamma, dbeta, resid, dz, lddz);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

}  // extern "C"
