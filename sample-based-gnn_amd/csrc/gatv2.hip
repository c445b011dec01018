// Sampled GATv2 layer (Brody et al., "How Attentive are Graph Attention
// Networks?", ICLR 2022; no reference counterpart) fused into three kernels and
// a two-stage parameter reduction.
//
// Per head h of D columns, K heads, F = K D, on a sampled block:
//   Hs = X W_s [src_size, F]   the source rows, also the aggregated values
//   Hd = X[dst] W_d [v_size, F] one row per destination, in destination order
//   t_e   = leaky_relu(Hs[src_e] + Hd[d_e], 0.2)      F wide, never stored
//   u_e,h = t_e,h . att_h                              the score ([e, K], stored)
//   a_e,h = softmax over the edges of d of u_.,h       ([e, K], stored)
//   Z_h[d] = sum_e a~_e,h Hs[src_e]_h;  Y = relu(concat_h Z_h) or relu(mean_h Z_h)
// The lane / chunk layout, the per-head reductions (head_sums), the online
// softmax and the dropout forms are those of the multi-head GAT kernels
// (gat.hip, gat_common.hpp).  Backward, deterministic and without atomics:
//   k_gatv2_bwd_dst  per dst: GM = GY (.) [Y > 0] (scaled); pass 1 parks
//                    ga_e,h = GM_h . Hs[src_e]_h in du and sums a ga; pass 2
//                    re-reads the rows: du = a (ga - sum a ga),
//                    dHd[d] = sum_e q_e, q_e[c] = du_e,head(c) att[c] leaky'(Hs + Hd),
//                    and the block's share of datt[c] = sum_e du_e,head(c) t_e[c]
//   k_gatv2_datt_reduce  the blocks' shares of datt added in block order
//   k_gatv2_bwd_src  per src v over the CSR: dHs[v] = sum_e (a~_e GM[d_e] + q_e)
// leaky' is recomputed from Hs and Hd in both backward kernels.
#include "gat_common.hpp"

namespace nts_hip {

constexpr int kV2U = 2;          // rows in flight where two rows are gathered per edge
constexpr int kV2Blocks = 1024;  // most blocks of k_gatv2_bwd_dst (datt partials)
constexpr int kV2Segs = 4;       // k_gatv2_datt_reduce: segments of blocks

// t = leaky_relu(x + h) and w (.) leaky'(x + h), element by element
__device__ __forceinline__ float lk_sum(float x, float h) { return leaky(x + h); }
__device__ __forceinline__ float4 lk_sum(float4 x, float4 h) {
  return make_float4(leaky(x.x + h.x), leaky(x.y + h.y), leaky(x.z + h.z), leaky(x.w + h.w));
}
__device__ __forceinline__ float lk_grad(float x, float h, float w) {
  return x + h > 0.f ? w : 0.2f * w;
}
__device__ __forceinline__ float4 lk_grad(float4 x, float4 h, float4 w) {
  return make_float4(lk_grad(x.x, h.x, w.x), lk_grad(x.y, h.y, w.y), lk_grad(x.z, h.z, w.z),
                     lk_grad(x.w, h.w, w.w));
}

// ---- forward: one wave per destination ---------------------------------------------
template <int VEC, int NCH, int MODE, bool DROP = false, class... DR>
__global__ __launch_bounds__(kGatThreads) void k_gatv2_fwd(
    const uint32_t* __restrict__ co, const uint32_t* __restrict__ ri, uint32_t nv_dst,
    const float* __restrict__ Hs, uint64_t ldhs, const float* __restrict__ Hd, uint64_t ldhd,
    uint32_t nvec, uint32_t g, uint32_t heads, const float* __restrict__ att,
    float* __restrict__ u_out, float* __restrict__ a_out, float* __restrict__ Y, uint64_t ldy,
    int mean, DR... drs) {
  [[maybe_unused]] const GatDrop& dr = drop_of(drs...);
  using G = GV<VEC>;
  using T = typename G::T;
  // mean mode only (dynamic LDS, none in concat mode): the wave's normalised row
  extern __shared__ float4 gatv2_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  T* zrow = reinterpret_cast<T*>(gatv2_lds) + wave * (NCH * 64);
  const uint32_t d = blockIdx.x * (kGatThreads / 64) + wave;
  if (d >= nv_dst) return;
  const T* av = reinterpret_cast<const T*>(att);
  const T* hdr = reinterpret_cast<const T*>(Hd + (uint64_t)d * ldhd);
  T w[NCH], hd[NCH];
  uint32_t hc[NCH];
  bool lead[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    hc[c] = col / g;
    lead[c] = col < nvec && col == hc[c] * g;
    w[c] = col < nvec ? av[col] : G::zero();
    hd[c] = col < nvec ? hdr[col] : G::zero();
  }
  const uint32_t beg = co[d], end = co[d + 1];
  T acc[NCH];
  float M[NCH], S[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    acc[c] = G::zero();
    M[c] = -INFINITY;
    S[c] = 0.f;
  }
  for (uint32_t cb = beg; cb < end; cb += 64) {
    const uint32_t ne = min(end - cb, 64u);
    const uint32_t my_r = lane < (int)ne ? ri[cb + lane] : 0u;
    [[maybe_unused]] uint64_t kb[NCH];
    if constexpr (DROP) edge_keep_bits<NCH>(kb, cb + lane, heads, dr);
    for (uint32_t j0 = 0; j0 < ne; j0 += kGatU) {  // kGatU neighbour rows in flight
      T x[kGatU][NCH];
      float p1[kGatU][NCH];
#pragma unroll
      for (int u = 0; u < kGatU; ++u) {
        const bool ok = j0 + u < ne;
        const uint32_t r = chunk_get(my_r, j0 + u, ne);
        const T* hr = reinterpret_cast<const T*>(Hs + (uint64_t)r * ldhs);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const uint32_t col = lane + 64 * c;
          x[u][c] = (ok && col < nvec) ? hr[col] : G::zero();
          p1[u][c] = G::dot(lk_sum(x[u][c], hd[c]), w[c]);
        }
      }
      head_sums<MODE, NCH, kGatU>(p1, hc, g, heads);
#pragma unroll
      for (int u = 0; u < kGatU; ++u) {
        if (j0 + u >= ne) break;
        const uint64_t eb = (uint64_t)(cb + j0 + u) * heads;
        [[maybe_unused]] uint64_t kj[NCH];
        if constexpr (DROP) keep_bits_from<NCH>(kj, kb, (int)(j0 + u), heads);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const float m = p1[u][c];
          if (lead[c]) u_out[eb + hc[c]] = m;
          const float Mn = fmaxf(M[c], m);
          const float sc = expf(M[c] - Mn);  // 0 for the first edge (M = -inf)
          const float p = expf(m - Mn);
          S[c] = S[c] * sc + p;  // over all edges
          float pk = p;          // DROP: the accumulator takes the kept edges only
          if constexpr (DROP) pk = head_kept<NCH>(kj, hc[c], c) ? p : 0.f;
          acc[c] = G::axpy(G::scale(acc[c], sc), pk, x[u][c]);
          M[c] = Mn;
        }
      }
    }
  }
  float inv[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    inv[c] = S[c] > 0.f ? 1.f / S[c] : 0.f;
    float invy = inv[c];  // DROP: 1 / (1 - p_attn) folded in
    if constexpr (DROP) invy = inv[c] * dr.scale_attn;
    acc[c] = G::scale(acc[c], invy);
  }
  T* y = reinterpret_cast<T*>(Y + (uint64_t)d * ldy);
  if (!mean) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint32_t col = lane + 64 * c;
      if (col < nvec) {
        T o = G::relu(acc[c]);
        if constexpr (DROP)
          if (dr.thr_out) o = out_drop<VEC>(o, d, col, dr);
        y[col] = o;
      }
    }
  } else {  // Y[d] = relu(mean over heads), heads added in order
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint32_t col = lane + 64 * c;
      if (col < nvec) zrow[col] = acc[c];
    }
    // the row is the wave's own: its LDS writes are ordered before its reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float rk = 1.f / (float)heads;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint32_t col = lane + 64 * c;
      if (col < g) {
        T t = zrow[col];
        for (uint32_t h = 1; h < heads; ++h) t = G::axpy(t, 1.f, zrow[h * g + col]);
        T o = G::relu(G::scale(t, rk));
        if constexpr (DROP)
          if (dr.thr_out) o = out_drop<VEC>(o, d, col, dr);
        y[col] = o;
      }
    }
  }
  // attention coefficients (needed by the backward): each head's lead lane
  // reads back the scores it wrote
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    if (lead[c]) {
#pragma unroll 4
      for (uint32_t e = beg; e < end; ++e) {
        const uint64_t i = (uint64_t)e * heads + hc[c];
        a_out[i] = expf(u_out[i] - M[c]) * inv[c];
      }
    }
}

// ---- backward, per destination --------------------------------------------------
// Block b owns destinations [b rpb, (b + 1) rpb), wave w of it every fourth one
// from b rpb + w; a wave keeps its sum of datt over its destinations in
// registers, the block adds its waves in order and writes one partial row
// part[b][F] (k_gatv2_datt_reduce adds the rows).  rpb depends on v_size alone.
// DROP: as k_gat_bwd_dst_heads.
template <int VEC, int NCH, int MODE, bool DROP = false, class... DR>
__global__ __launch_bounds__(kGatThreads) void k_gatv2_bwd_dst(
    const uint32_t* __restrict__ co, const uint32_t* __restrict__ ri, uint32_t nv_dst,
    uint32_t rpb, const float* __restrict__ Hs, uint64_t ldhs, const float* __restrict__ Hd,
    uint64_t ldhd, uint32_t nvec, uint32_t g, uint32_t heads, const float* __restrict__ att,
    const float* __restrict__ a, const float* __restrict__ Y, uint64_t ldy,
    const float* __restrict__ GY, uint64_t ldg, float* du, float* __restrict__ GM, uint64_t ldm,
    float* __restrict__ dHd, uint64_t lddhd, float* __restrict__ part, int mean, DR... drs) {
  [[maybe_unused]] const GatDrop& dr = drop_of(drs...);
  using G = GV<VEC>;
  using T = typename G::T;
  __shared__ float4 s_acc4[NCH * 64 * VEC / 4];
  T* s_acc = reinterpret_cast<T*>(s_acc4);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const float rk = 1.f / (float)heads;
  const T* av = reinterpret_cast<const T*>(att);
  T w[NCH], dA[NCH];
  uint32_t hc[NCH];
  bool lead[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    hc[c] = col / g;
    lead[c] = col < nvec && col == hc[c] * g;
    w[c] = col < nvec ? av[col] : G::zero();
    dA[c] = G::zero();
  }
  const uint32_t d0 = blockIdx.x * rpb;
  const uint32_t d1 = min(d0 + rpb, nv_dst);
  for (uint32_t d = d0 + wave; d < d1; d += kGatThreads / 64) {
    const T* gy = reinterpret_cast<const T*>(GY + (uint64_t)d * ldg);
    const T* yy = reinterpret_cast<const T*>(Y + (uint64_t)d * ldy);
    T* gm = reinterpret_cast<T*>(GM + (uint64_t)d * ldm);
    const uint32_t beg = co[d], end = co[d + 1];
    float sag[NCH];
    {
      T gv[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const uint32_t col = lane + 64 * c;
        gv[c] = G::zero();
        sag[c] = 0.f;
        if (col < nvec) {
          // mean mode: every head gets GY / K under the mask of the D-wide Y
          const uint32_t q = mean ? col - hc[c] * g : col;
          gv[c] = G::mask(gy[q], yy[q]);
          if constexpr (DROP) gv[c] = G::scale(gv[c], dr.scale_out);
          if (mean) gv[c] = G::scale(gv[c], rk);
          gm[col] = gv[c];  // read per slot by k_gatv2_bwd_src
        }
      }
      // pass 1: ga[e, h] = g_h . Hs[src_e]_h, parked in du by the head's lead
      // lane; every lane of the head sums a ga in edge order (the same bits)
      for (uint32_t cb = beg; cb < end; cb += 64) {
        const uint32_t ne = min(end - cb, 64u);
        const uint32_t my_r = lane < (int)ne ? ri[cb + lane] : 0u;
        [[maybe_unused]] uint64_t kb[NCH];
        if constexpr (DROP) edge_keep_bits<NCH>(kb, cb + lane, heads, dr);
        for (uint32_t j0 = 0; j0 < ne; j0 += kGatU) {
          float p[kGatU][NCH], aa[kGatU][NCH];
#pragma unroll
          for (int u = 0; u < kGatU; ++u) {
            const bool ok = j0 + u < ne;
            const uint32_t r = chunk_get(my_r, j0 + u, ne);
            const T* hr = reinterpret_cast<const T*>(Hs + (uint64_t)r * ldhs);
            const uint64_t eb = (uint64_t)(cb + j0 + u) * heads;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
              const uint32_t col = lane + 64 * c;
              const bool in = ok && col < nvec;
              p[u][c] = in ? G::dot(gv[c], hr[col]) : 0.f;
              aa[u][c] = in ? a[eb + hc[c]] : 0.f;
            }
          }
          head_sums<MODE, NCH, kGatU>(p, hc, g, heads);
#pragma unroll
          for (int u = 0; u < kGatU; ++u) {
            if (j0 + u >= ne) break;
            const uint64_t eb = (uint64_t)(cb + j0 + u) * heads;
            [[maybe_unused]] uint64_t kj[NCH];
            if constexpr (DROP) keep_bits_from<NCH>(kj, kb, (int)(j0 + u), heads);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
              float ga = p[u][c];
              if constexpr (DROP) ga = head_kept<NCH>(kj, hc[c], c) ? ga * dr.scale_attn : 0.f;
              if (lead[c]) du[eb + hc[c]] = ga;
              sag[c] += aa[u][c] * ga;
            }
          }
        }
      }
    }
    // the parked ga is read below by every lane of its head: the wave's stores
    // are ordered before those loads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // pass 2: the rows again: du, dHd[d] and this destination's share of datt
    const T* hdr = reinterpret_cast<const T*>(Hd + (uint64_t)d * ldhd);
    T hd[NCH], dh[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint32_t col = lane + 64 * c;
      hd[c] = col < nvec ? hdr[col] : G::zero();
      dh[c] = G::zero();
    }
    for (uint32_t cb = beg; cb < end; cb += 64) {
      const uint32_t ne = min(end - cb, 64u);
      const uint32_t my_r = lane < (int)ne ? ri[cb + lane] : 0u;
      for (uint32_t j0 = 0; j0 < ne; j0 += kV2U) {
        T x[kV2U][NCH];
        float dv[kV2U][NCH];
        // every load of the group before its stores (the lead lane of a head
        // may sit in an earlier chunk than a lane that reads the head's ga)
#pragma unroll
        for (int u = 0; u < kV2U; ++u) {
          const bool ok = j0 + u < ne;
          const uint32_t r = chunk_get(my_r, j0 + u, ne);
          const T* hr = reinterpret_cast<const T*>(Hs + (uint64_t)r * ldhs);
          const uint64_t eb = (uint64_t)(cb + j0 + u) * heads;
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            const uint32_t col = lane + 64 * c;
            const bool in = ok && col < nvec;
            x[u][c] = in ? hr[col] : G::zero();
            const float ae = in ? a[eb + hc[c]] : 0.f;
            const float ga = in ? du[eb + hc[c]] : 0.f;
            dv[u][c] = ae * (ga - sag[c]);
          }
        }
#pragma unroll
        for (int u = 0; u < kV2U; ++u) {
          if (j0 + u >= ne) break;
          const uint64_t eb = (uint64_t)(cb + j0 + u) * heads;
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            if (lead[c]) du[eb + hc[c]] = dv[u][c];
            dh[c] = G::axpy(dh[c], dv[u][c], lk_grad(x[u][c], hd[c], w[c]));
            dA[c] = G::axpy(dA[c], dv[u][c], lk_sum(x[u][c], hd[c]));
          }
        }
      }
    }
    T* out = reinterpret_cast<T*>(dHd + (uint64_t)d * lddhd);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint32_t col = lane + 64 * c;
      if (col < nvec) out[col] = dh[c];
    }
  }
  // the block's partial: waves added in order
  for (int k = 0; k < kGatThreads / 64; ++k) {
    if (wave == k) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const uint32_t col = lane + 64 * c;
        if (col < nvec) s_acc[col] = k ? G::axpy(s_acc[col], 1.f, dA[c]) : dA[c];
      }
    }
    __syncthreads();
  }
  T* po = reinterpret_cast<T*>(part + (uint64_t)blockIdx.x * nvec * VEC);
  for (uint32_t col = threadIdx.x; col < nvec; col += kGatThreads) po[col] = s_acc[col];
}

// datt[c] = sum over blocks of part[b][c]: the blocks in kV2Segs contiguous
// segments, each summed in block order by one thread, the segments then added
// in order
__global__ __launch_bounds__(64 * kV2Segs) void k_gatv2_datt_reduce(
    const float* __restrict__ part, uint32_t nblk, uint32_t F, float* __restrict__ datt) {
  __shared__ float s_seg[kV2Segs][64];
  const uint32_t lane = threadIdx.x & 63, seg = threadIdx.x / 64;
  const uint32_t c = blockIdx.x * 64 + lane;
  const uint32_t per = (nblk + kV2Segs - 1) / kV2Segs;
  const uint32_t b0 = min(seg * per, nblk), b1 = min(b0 + per, nblk);
  float s = 0.f;
  if (c < F) {
#pragma unroll 8
    for (uint32_t b = b0; b < b1; ++b) s += part[(uint64_t)b * F + c];
  }
  s_seg[seg][lane] = s;
  __syncthreads();
  if (seg == 0 && c < F) {
    float t = s_seg[0][lane];
#pragma unroll
    for (int k = 1; k < kV2Segs; ++k) t += s_seg[k][lane];
    datt[c] = t;
  }
}

// ---- backward, per source (CSR) --------------------------------------------------
// Per slot the wave gathers GM[d] and Hd[d]; Hs[v] and att stay in registers.
// DROP: as k_gat_bwd_src_heads.
template <int VEC, int NCH, int = 0, bool DROP = false, class... DR>
__global__ __launch_bounds__(kGatThreads) void k_gatv2_bwd_src(
    const uint32_t* __restrict__ ro, const uint32_t* __restrict__ ci,
    const uint32_t* __restrict__ ceid, uint32_t nv_src, uint32_t nvec, uint32_t g, uint32_t heads,
    const float* __restrict__ a, const float* __restrict__ du, const float* __restrict__ att,
    const float* __restrict__ Hs, uint64_t ldhs, const float* __restrict__ Hd, uint64_t ldhd,
    const float* __restrict__ GM, uint64_t ldm, float* __restrict__ dHs, uint64_t lddhs,
    DR... drs) {
  [[maybe_unused]] const GatDrop& dr = drop_of(drs...);
  using G = GV<VEC>;
  using T = typename G::T;
  const int lane = threadIdx.x & 63;
  const uint32_t v = blockIdx.x * (kGatThreads / 64) + (threadIdx.x >> 6);
  if (v >= nv_src) return;
  const T* av = reinterpret_cast<const T*>(att);
  const T* hsr = reinterpret_cast<const T*>(Hs + (uint64_t)v * ldhs);
  uint32_t hc[NCH];
  T w[NCH], hs[NCH], acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    hc[c] = col / g;
    w[c] = col < nvec ? av[col] : G::zero();
    hs[c] = col < nvec ? hsr[col] : G::zero();
    acc[c] = G::zero();
  }
  const uint32_t beg = ro[v], end = ro[v + 1];
  for (uint32_t cb = beg; cb < end; cb += 64) {
    const uint32_t ne = min(end - cb, 64u);
    uint32_t my_d = 0, my_e = 0;
    if (lane < (int)ne) {
      my_e = ceid[cb + lane];
      my_d = ci[cb + lane];
    }
    [[maybe_unused]] uint64_t kb[NCH];
    if constexpr (DROP) edge_keep_bits<NCH>(kb, my_e, heads, dr);
    for (uint32_t j0 = 0; j0 < ne; j0 += kV2U) {
      T x[kV2U][NCH], y[kV2U][NCH];
      float wa[kV2U][NCH], uu[kV2U][NCH];
#pragma unroll
      for (int u = 0; u < kV2U; ++u) {
        const bool ok = j0 + u < ne;
        const int jj = (int)min(j0 + u, ne - 1);
        const uint32_t dd = chunk_get(my_d, j0 + u, ne);
        const uint64_t eb = (uint64_t)chunk_get(my_e, j0 + u, ne) * heads;
        const T* gm = reinterpret_cast<const T*>(GM + (uint64_t)dd * ldm);
        const T* hr = reinterpret_cast<const T*>(Hd + (uint64_t)dd * ldhd);
        [[maybe_unused]] uint64_t kj[NCH];
        if constexpr (DROP) keep_bits_from<NCH>(kj, kb, jj, heads);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const uint32_t col = lane + 64 * c;
          const bool in = ok && col < nvec;
          x[u][c] = in ? gm[col] : G::zero();
          y[u][c] = in ? hr[col] : G::zero();
          wa[u][c] = in ? a[eb + hc[c]] : 0.f;
          if constexpr (DROP)
            wa[u][c] = head_kept<NCH>(kj, hc[c], c) ? wa[u][c] * dr.scale_attn : 0.f;
          uu[u][c] = in ? du[eb + hc[c]] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < kV2U; ++u)
        if (j0 + u < ne) {  // slot order kept
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            acc[c] = G::axpy(acc[c], wa[u][c], x[u][c]);
            acc[c] = G::axpy(acc[c], uu[u][c], lk_grad(hs[c], y[u][c], w[c]));
          }
        }
    }
  }
  T* out = reinterpret_cast<T*>(dHs + (uint64_t)v * lddhs);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    if (col < nvec) out[col] = acc[c];
  }
}

// destinations of one k_gatv2_bwd_dst block: a function of v_size alone (a
// multiple of the block's waves), so datt's summation order never depends on
// the device
uint32_t gatv2_rows_per_block(uint32_t v_size) {
  const uint32_t waves = kGatThreads / 64;
  const uint32_t per = ceil_div(v_size, kV2Blocks);
  return std::max(waves, (per + waves - 1) / waves * waves);
}

}  // namespace nts_hip

using namespace nts_hip;

extern "C" {

int nts_hip_gatv2_forward(nts_hip_ctx* ctx, const uint32_t* column_offset,
                          const uint32_t* row_indices, uint32_t v_size, const float* Hs,
                          uint64_t ldhs, const float* Hd, uint64_t ldhd, uint32_t heads,
                          uint32_t D, const float* att, float* u_out, float* a_out, float* Y,
                          uint64_t ldy, int mean, float p_attn, float p_out, uint64_t seed,
                          uint64_t off_attn, uint64_t off_out) {
  const char* fn = __func__;
  GAT_CHECK(ctx && column_offset && row_indices && Hs && Hd && att && u_out && a_out && Y,
            "NULL argument");
  std::optional<GatDrop> drv;
  NTS_RET(gat_drop(fn, p_attn, p_out, seed, off_attn, off_out, &drv));
  NTS_RET(gat_heads_check(fn, heads, D));
  const uint32_t F = heads * D, FY = mean ? D : F;
  GAT_CHECK(ldhs >= F && ldhd >= F && ldy >= FY, "leading dimension");
  const bool v4 = gat_vec4(D, {{Hs, ldhs}, {Hd, ldhd}, {Y, ldy}, {att, 0}});
  HeadsShape hs;
  NTS_RET(gat_heads_shape(fn, heads, D, v4, &hs));
  if (v_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  return gat_dispatch(v4, hs.nch, hs.mode, [&](auto V, auto N, auto M) {
    return gat_launch(k_gatv2_fwd<V(), N(), M()>, k_gatv2_fwd<V(), N(), M(), true, GatDrop>,
                      gat_grid(v_size), gat_mean_lds(mean, hs.nch, v4), ctx->stream,
                      gat_drop_ptr(drv), column_offset, row_indices, v_size, Hs, ldhs, Hd, ldhd,
                      hs.nvec, hs.g, heads, att, u_out, a_out, Y, ldy, mean);
  });
}

int nts_hip_gatv2_backward(nts_hip_ctx* ctx, const uint32_t* column_offset,
                           const uint32_t* row_indices, uint32_t v_size,
                           const uint32_t* row_offset, const uint32_t* column_indices,
                           const uint32_t* csr_edge_id, uint32_t src_size, const float* Hs,
                           uint64_t ldhs, const float* Hd, uint64_t ldhd, uint32_t heads,
                           uint32_t D, const float* att, const float* a, const float* Y,
                           uint64_t ldy, const float* GY, uint64_t ldg, float* du, float* GM,
                           uint64_t ldm, float* dHs, uint64_t lddhs, float* dHd, uint64_t lddhd,
                           float* datt, int mean, float p_attn, float p_out, uint64_t seed,
                           uint64_t off_attn) {
  const char* fn = __func__;
  GAT_CHECK(ctx && column_offset && row_indices && row_offset && column_indices && csr_edge_id &&
                Hs && Hd && att && a && Y && GY && du && GM && dHs && dHd && datt,
            "NULL argument");
  std::optional<GatDrop> drv;
  NTS_RET(gat_drop(fn, p_attn, p_out, seed, off_attn, 0, &drv));
  const GatDrop* dr = gat_drop_ptr(drv);
  NTS_RET(gat_heads_check(fn, heads, D));
  const uint32_t F = heads * D, FY = mean ? D : F;
  GAT_CHECK(ldhs >= F && ldhd >= F && ldy >= FY && ldg >= FY && ldm >= F && lddhs >= F &&
                lddhd >= F,
            "leading dimension");
  const bool v4 = gat_vec4(D, {{Hs, ldhs}, {Hd, ldhd}, {Y, ldy}, {att, 0}, {GY, ldg}, {GM, ldm},
                               {dHs, lddhs}, {dHd, lddhd}});
  // a refused shape leaves every output as it was
  HeadsShape hs;
  NTS_RET(gat_heads_shape(fn, heads, D, v4, &hs));
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const hipStream_t st = ctx->stream;
  if (v_size == 0) {
    NTS_HIP_TRY(hipMemsetAsync(datt, 0, (size_t)F * sizeof(float), st));
  } else {
    const uint32_t rpb = gatv2_rows_per_block(v_size);
    const uint32_t nblk = ceil_div(v_size, rpb);
    NTS_RET(ensure_scratch(ctx, (size_t)nblk * F * sizeof(float)));
    float* part = reinterpret_cast<float*>(ctx->scratch);
    NTS_RET(gat_dispatch(v4, hs.nch, hs.mode, [&](auto V, auto N, auto M) {
      return gat_launch(k_gatv2_bwd_dst<V(), N(), M()>,
                        k_gatv2_bwd_dst<V(), N(), M(), true, GatDrop>, dim3(nblk), 0, st, dr,
                        column_offset, row_indices, v_size, rpb, Hs, ldhs, Hd, ldhd, hs.nvec, hs.g,
                        heads, att, a, Y, ldy, GY, ldg, du, GM, ldm, dHd, lddhd, part, mean);
    }));
    hipLaunchKernelGGL(k_gatv2_datt_reduce, dim3(ceil_div(F, 64)), dim3(64 * kV2Segs), 0, st, part,
                       nblk, F, datt);
    NTS_LAUNCH_CHECK();
  }
  if (src_size)
    NTS_RET(gat_dispatch(v4, hs.nch, [&](auto V, auto N) {
      return gat_launch(k_gatv2_bwd_src<V(), N(), 0>, k_gatv2_bwd_src<V(), N(), 0, true, GatDrop>,
                        gat_grid(src_size), 0, st, dr, row_offset, column_indices, csr_edge_id,
                        src_size, hs.nvec, hs.g, heads, a, du, att, Hs, ldhs, Hd, ldhd, GM, ldm, dHs,
                        lddhs);
    }));
  return NTS_OK;
}

}  // extern "C"
