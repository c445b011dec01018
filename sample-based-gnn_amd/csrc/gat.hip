// Sampled GAT layer (the reference's GAT_SAMPLE_ALL_GPU chain,
// toolkits/GAT_SAMPLE_ALL_GPU.hpp:308-391) fused into three kernels.
//
// Reference forward of one layer on a merged src/dst sampled block
// (core/ntsPushdownGraphOp.hpp:490-748, kernels cuda/ntsCUDADistKernel.cuh):
//   H     = X W                                   (Parameter::forward)
//   msg_e = [H[src_e], H[dst_local(d_e)]]         (BatchGPUSrcDstScatterOp)
//   m_e   = leaky_relu(msg_e . W_att, 0.2)        (edge NN, W_att [2F, 1])
//   a_e   = exp(m_e - max_d) / sum_d exp(...)     (BatchGPUEdgeSoftMax, :319-370)
//   Z_d   = sum_e a_e H[src_e]                    (e_msg * a, BatchGPUAggregateDst)
//   X'_d  = relu(Z_d)
// Here msg_e is never materialised: msg_e . W_att = H[src].a1 + H[dst].a2 with
// a1 = W_att[0:F], a2 = W_att[F:2F]; one wave per destination reads each
// neighbour row once and keeps an online softmax (running max / sum, the
// accumulator rescaled when the max grows).  Backward (all deterministic,
// no atomics):
//   k_gat_bwd_dst  per dst: g = G (.) [X' > 0] (stored: GM); ga_e = g . H[src_e];
//                  du_e = a_e (ga_e - sum a ga) * leaky'(m_e); ds2[dst_local(d)] = sum du_e
//   k_gat_bwd_src  per src v over the CSR: dH[v] = sum a_e g_{d_e} + ds1[v] a1 + ds2[v] a2,
//                  ds1[v] = sum du_e;  dS[v] = (ds1[v], ds2[v])
// and W_att.grad = H^T dS, W.grad = X^T dH, dX = dH W^T (layer GEMMs).
#include "gat_common.hpp"

namespace nts_hip {

// ---- forward -----------------------------------------------------------------
template <int VEC, int NCH, bool DROP = false, class... DR>
__global__ __launch_bounds__(kGatThreads) void k_gat_fwd(
    const uint32_t* __restrict__ co, const uint32_t* __restrict__ ri,
    const uint32_t* __restrict__ dl, uint32_t nv_dst, const float* __restrict__ H, uint64_t ldh,
    uint32_t nvec, const float* __restrict__ att, float* __restrict__ m_out,
    float* __restrict__ a_out, float* __restrict__ Y, uint64_t ldy, DR... drs) {
  [[maybe_unused]] const GatDrop& dr = drop_of(drs...);
  using G = GV<VEC>;
  using T = typename G::T;
  const int lane = threadIdx.x & 63;
  const uint32_t d = blockIdx.x * (kGatThreads / 64) + (threadIdx.x >> 6);
  if (d >= nv_dst) return;
  const T* a1 = reinterpret_cast<const T*>(att);
  const T* a2 = reinterpret_cast<const T*>(att + (uint64_t)nvec * VEC);
  T w1[NCH], w2[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    w1[c] = col < nvec ? a1[col] : G::zero();
    w2[c] = col < nvec ? a2[col] : G::zero();
  }
  // score of the destination's own row
  const T* hd = reinterpret_cast<const T*>(H + (uint64_t)dl[d] * ldh);
  float p2 = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    if (col < nvec) p2 += G::dot(hd[col], w2[c]);
  }
  const float s2 = wave_sum(p2);
  const uint32_t beg = co[d], end = co[d + 1];
  T acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) acc[c] = G::zero();
  float M = -INFINITY, S = 0.f;
  for (uint32_t cb = beg; cb < end; cb += 64) {
    const uint32_t ne = min(end - cb, 64u);
    const uint32_t my_r = lane < (int)ne ? ri[cb + lane] : 0u;
    float my_m = 0.f;
    // DROP: bit j = edge cb + j kept, drawn by the lane that owns the edge
    [[maybe_unused]] uint64_t kept = ~0ull;
    if constexpr (DROP) kept = __ballot(edge_kept(cb + lane, dr));
    for (uint32_t j0 = 0; j0 < ne; j0 += kGatU) {  // kGatU neighbour rows in flight
      T x[kGatU][NCH];
      float p1[kGatU];
#pragma unroll
      for (int u = 0; u < kGatU; ++u) {
        const bool ok = j0 + u < ne;
        const uint32_t r = chunk_get(my_r, j0 + u, ne);
        const T* hr = reinterpret_cast<const T*>(H + (uint64_t)r * ldh);
        p1[u] = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const uint32_t col = lane + 64 * c;
          x[u][c] = (ok && col < nvec) ? hr[col] : G::zero();
          p1[u] += G::dot(x[u][c], w1[c]);
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int u = 0; u < kGatU; ++u) p1[u] += __shfl_xor(p1[u], o, 64);
#pragma unroll
      for (int u = 0; u < kGatU; ++u) {
        if (j0 + u >= ne) break;
        const float m = leaky(p1[u] + s2);
        if (lane == (int)(j0 + u)) my_m = m;
        const float Mn = fmaxf(M, m);
        const float sc = expf(M - Mn);  // 0 for the first edge (M = -inf)
        const float p = expf(m - Mn);
        S = S * sc + p;  // over all edges
        float pk = p;    // DROP: the accumulator takes the kept edges only
        if constexpr (DROP) pk = ((kept >> (j0 + u)) & 1ull) ? p : 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] = G::axpy(G::scale(acc[c], sc), pk, x[u][c]);
        M = Mn;
      }
    }
    if (lane < (int)ne) m_out[cb + lane] = my_m;
  }
  const float inv = S > 0.f ? 1.f / S : 0.f;
  float invy = inv;  // DROP: 1 / (1 - p_attn) folded in
  if constexpr (DROP) invy = inv * dr.scale_attn;
  T* y = reinterpret_cast<T*>(Y + (uint64_t)d * ldy);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    if (col < nvec) {
      T o = G::relu(G::scale(acc[c], invy));
      if constexpr (DROP)
        if (dr.thr_out) o = out_drop<VEC>(o, d, col, dr);
      y[col] = o;
    }
  }
  // attention coefficients (needed by the backward)
  for (uint32_t e = beg + lane; e < end; e += 64) a_out[e] = expf(m_out[e] - M) * inv;
}


// ---- backward, per destination ------------------------------------------------
// DROP: GM = GY (.) [Y > 0] / (1 - p_out) (Y > 0 exactly where the row was
// relu-active and kept); the parked ga_e = (GM . H[src_e]) keep_e / (1 - p_attn)
// is dL/da_e, and du = a (ga - sum a ga) leaky' as without dropout.
template <int VEC, int NCH, bool DROP = false, class... DR>
__global__ __launch_bounds__(kGatThreads) void k_gat_bwd_dst(
    const uint32_t* __restrict__ co, const uint32_t* __restrict__ ri,
    const uint32_t* __restrict__ dl, uint32_t nv_dst, const float* __restrict__ H, uint64_t ldh,
    uint32_t nvec, const float* __restrict__ a, const float* __restrict__ m,
    const float* __restrict__ Y, uint64_t ldy, const float* __restrict__ GY, uint64_t ldg,
    float* __restrict__ du, float* __restrict__ ds2, float* __restrict__ GM, uint64_t ldm, DR... drs) {
  [[maybe_unused]] const GatDrop& dr = drop_of(drs...);
  using G = GV<VEC>;
  using T = typename G::T;
  const int lane = threadIdx.x & 63;
  const uint32_t d = blockIdx.x * (kGatThreads / 64) + (threadIdx.x >> 6);
  if (d >= nv_dst) return;
  const T* gy = reinterpret_cast<const T*>(GY + (uint64_t)d * ldg);
  const T* yy = reinterpret_cast<const T*>(Y + (uint64_t)d * ldy);
  T* gm = reinterpret_cast<T*>(GM + (uint64_t)d * ldm);
  T g[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    g[c] = col < nvec ? G::mask(gy[col], yy[col]) : G::zero();
    if constexpr (DROP) g[c] = G::scale(g[c], dr.scale_out);
    if (col < nvec) gm[col] = g[c];  // relu-masked gradient, read per edge by k_gat_bwd_src
  }
  const uint32_t beg = co[d], end = co[d + 1];
  // pass 1: ga_e = g . H[src_e] (kept by the lane owning e, chunk by chunk:
  // du needs sum_e a_e ga_e first, so ga is parked in du and rescaled below)
  float sag = 0.f;
  for (uint32_t cb = beg; cb < end; cb += 64) {
    const uint32_t ne = min(end - cb, 64u);
    const uint32_t my_r = lane < (int)ne ? ri[cb + lane] : 0u;
    float my_ga = 0.f;
    for (uint32_t j0 = 0; j0 < ne; j0 += kGatU) {
      float p[kGatU];
#pragma unroll
      for (int u = 0; u < kGatU; ++u) {
        const bool ok = j0 + u < ne;
        const uint32_t r = chunk_get(my_r, j0 + u, ne);
        const T* hr = reinterpret_cast<const T*>(H + (uint64_t)r * ldh);
        p[u] = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const uint32_t col = lane + 64 * c;
          if (ok && col < nvec) p[u] += G::dot(g[c], hr[col]);
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int u = 0; u < kGatU; ++u) p[u] += __shfl_xor(p[u], o, 64);
#pragma unroll
      for (int u = 0; u < kGatU; ++u)
        if (lane == (int)(j0 + u)) my_ga = p[u];
    }
    if (lane < (int)ne) {
      if constexpr (DROP) my_ga = edge_kept(cb + lane, dr) ? my_ga * dr.scale_attn : 0.f;
      du[cb + lane] = my_ga;
      sag += a[cb + lane] * my_ga;
    }
  }
  sag = wave_sum(sag);
  // pass 2: softmax and leaky_relu backward
  float s = 0.f;
  for (uint32_t e = beg + lane; e < end; e += 64) {
    const float dm = a[e] * (du[e] - sag);
    const float u = m[e] > 0.f ? dm : 0.2f * dm;
    du[e] = u;
    s += u;
  }
  s = wave_sum(s);
  if (lane == 0) ds2[dl[d]] = s;
}


// ---- backward, per source (CSR) ------------------------------------------------
// DROP: the weight of GM[d_e] is the dropped attention keep_e a_e / (1 - p_attn),
// the keep bit regenerated from the slot's CSC edge position
template <int VEC, int NCH, bool DROP = false, class... DR>
__global__ __launch_bounds__(kGatThreads) void k_gat_bwd_src(
    const uint32_t* __restrict__ ro, const uint32_t* __restrict__ ci,
    const uint32_t* __restrict__ ceid, uint32_t nv_src, uint32_t nvec,
    const float* __restrict__ a, const float* __restrict__ du, const float* __restrict__ ds2,
    const float* __restrict__ att, const float* __restrict__ GM, uint64_t ldm,
    float* __restrict__ dH, uint64_t lddh, float* __restrict__ dS, DR... drs) {
  [[maybe_unused]] const GatDrop& dr = drop_of(drs...);
  using G = GV<VEC>;
  using T = typename G::T;
  const int lane = threadIdx.x & 63;
  const uint32_t v = blockIdx.x * (kGatThreads / 64) + (threadIdx.x >> 6);
  if (v >= nv_src) return;
  const uint32_t beg = ro[v], end = ro[v + 1];
  T acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) acc[c] = G::zero();
  float s1 = 0.f;
  for (uint32_t cb = beg; cb < end; cb += 64) {
    const uint32_t ne = min(end - cb, 64u);
    uint32_t my_d = 0;
    float my_a = 0.f, my_u = 0.f;
    if (lane < (int)ne) {
      const uint32_t eid = ceid[cb + lane];
      my_d = ci[cb + lane];
      my_a = a[eid];
      my_u = du[eid];
      if constexpr (DROP) my_a = edge_kept(eid, dr) ? my_a * dr.scale_attn : 0.f;
    }
    s1 += my_u;
    for (uint32_t j0 = 0; j0 < ne; j0 += kGatU) {
      T x[kGatU][NCH];
      float w[kGatU];
#pragma unroll
      for (int u = 0; u < kGatU; ++u) {
        const bool ok = j0 + u < ne;
        const int jj = (int)min(j0 + u, ne - 1);
        const uint32_t dd = chunk_get(my_d, j0 + u, ne);
        w[u] = ok ? __shfl(my_a, jj, 64) : 0.f;
        const T* gm = reinterpret_cast<const T*>(GM + (uint64_t)dd * ldm);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const uint32_t col = lane + 64 * c;
          x[u][c] = (ok && col < nvec) ? gm[col] : G::zero();
        }
      }
#pragma unroll
      for (int u = 0; u < kGatU; ++u)
        if (j0 + u < ne) {  // edge order kept
#pragma unroll
          for (int c = 0; c < NCH; ++c) acc[c] = G::axpy(acc[c], w[u], x[u][c]);
        }
    }
  }
  s1 = wave_sum(s1);
  const float s2 = ds2[v];
  const T* a1 = reinterpret_cast<const T*>(att);
  const T* a2 = reinterpret_cast<const T*>(att + (uint64_t)nvec * VEC);
  T* out = reinterpret_cast<T*>(dH + (uint64_t)v * lddh);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    if (col < nvec) out[col] = G::axpy(G::axpy(acc[c], s1, a1[col]), s2, a2[col]);
  }
  if (lane == 0) {
    dS[2 * (uint64_t)v] = s1;
    dS[2 * (uint64_t)v + 1] = s2;
  }
}


// ---- multi-head layer -----------------------------------------------------------
// K heads of D columns, F = K D: head h owns columns [hD, (h+1)D) of H, a1 and
// a2, and has its own softmax over each destination's edges.  The F-wide
// neighbour row is still read once, by the same lane / chunk layout (vector
// col = lane + 64 c); D % VEC == 0, so every vector lies in one head: head of
// col = col / g with g = D / VEC lanes per head.  Each lane keeps one online
// softmax state (running max, running sum) per chunk, that of the head its
// vector of the chunk belongs to.  The per-head dot products are segmented
// wave reductions (head_sums), by the shape of g:
//   kHeadsPow2   g a power of two below 64: xor butterfly over o < g, log2(g)
//                steps give every head's score at once;
//   kHeadsChunk  g a multiple of 64: whole chunks belong to one head, the
//                chunks of a head are added and reduced over the wave;
//   kHeadsAny    anything else (heads that end inside a chunk): one masked
//                wave reduction per head.
// The per-edge arrays are edge-major ([e, K]); the lane holding the first
// vector of a head (lead) writes that head's entries.
// DROP: the lane that owns edge cb + lane of a chunk draws that edge's keep bits
// for every head (edge_keep_bits); they reach the lanes of head h with the
// edge's turn (keep_bits_from).
template <int VEC, int NCH, int MODE, bool DROP = false, class... DR>
__global__ __launch_bounds__(kGatThreads) void k_gat_fwd_heads(
    const uint32_t* __restrict__ co, const uint32_t* __restrict__ ri,
    const uint32_t* __restrict__ dl, uint32_t nv_dst, const float* __restrict__ H, uint64_t ldh,
    uint32_t nvec, uint32_t g, uint32_t heads, const float* __restrict__ att,
    float* __restrict__ m_out, float* __restrict__ a_out, float* __restrict__ Y, uint64_t ldy,
    int mean, DR... drs) {
  [[maybe_unused]] const GatDrop& dr = drop_of(drs...);
  using G = GV<VEC>;
  using T = typename G::T;
  // mean mode only (dynamic LDS, none in concat mode): the wave's normalised
  // row, NCH * 64 vectors, for the sum over heads
  extern __shared__ float4 gat_heads_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  T* zrow = reinterpret_cast<T*>(gat_heads_lds) + wave * (NCH * 64);
  const uint32_t d = blockIdx.x * (kGatThreads / 64) + wave;
  if (d >= nv_dst) return;
  const T* a1 = reinterpret_cast<const T*>(att);
  const T* a2 = reinterpret_cast<const T*>(att + (uint64_t)nvec * VEC);
  const T* hd = reinterpret_cast<const T*>(H + (uint64_t)dl[d] * ldh);
  T w1[NCH];
  uint32_t hc[NCH];
  bool lead[NCH];
  float s2[1][NCH];  // score of the destination's own row, per head
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    hc[c] = col / g;
    lead[c] = col < nvec && col == hc[c] * g;
    w1[c] = col < nvec ? a1[col] : G::zero();
    s2[0][c] = col < nvec ? G::dot(hd[col], a2[col]) : 0.f;
  }
  head_sums<MODE, NCH, 1>(s2, hc, g, heads);
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
        const uint32_t r = (uint32_t)__shfl((int)my_r, (int)min(j0 + u, ne - 1), 64);
        const T* hr = reinterpret_cast<const T*>(H + (uint64_t)r * ldh);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const uint32_t col = lane + 64 * c;
          x[u][c] = (ok && col < nvec) ? hr[col] : G::zero();
          p1[u][c] = G::dot(x[u][c], w1[c]);
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
          const float m = leaky(p1[u][c] + s2[0][c]);
          if (lead[c]) m_out[eb + hc[c]] = m;
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
        a_out[i] = expf(m_out[i] - M[c]) * inv[c];
      }
    }
}


// DROP: as k_gat_bwd_dst, per head
template <int VEC, int NCH, int MODE, bool DROP = false, class... DR>
__global__ __launch_bounds__(kGatThreads) void k_gat_bwd_dst_heads(
    const uint32_t* __restrict__ co, const uint32_t* __restrict__ ri,
    const uint32_t* __restrict__ dl, uint32_t nv_dst, const float* __restrict__ H, uint64_t ldh,
    uint32_t nvec, uint32_t g, uint32_t heads, const float* __restrict__ a,
    const float* __restrict__ m, const float* __restrict__ Y, uint64_t ldy,
    const float* __restrict__ GY, uint64_t ldg, float* __restrict__ du, float* __restrict__ ds2,
    float* __restrict__ GM, uint64_t ldm, int mean, DR... drs) {
  [[maybe_unused]] const GatDrop& dr = drop_of(drs...);
  using G = GV<VEC>;
  using T = typename G::T;
  const int lane = threadIdx.x & 63;
  const uint32_t d = blockIdx.x * (kGatThreads / 64) + (threadIdx.x >> 6);
  if (d >= nv_dst) return;
  const T* gy = reinterpret_cast<const T*>(GY + (uint64_t)d * ldg);
  const T* yy = reinterpret_cast<const T*>(Y + (uint64_t)d * ldy);
  T* gm = reinterpret_cast<T*>(GM + (uint64_t)d * ldm);
  const float rk = 1.f / (float)heads;
  T gv[NCH];
  uint32_t hc[NCH];
  bool lead[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    hc[c] = col / g;
    lead[c] = col < nvec && col == hc[c] * g;
    gv[c] = G::zero();
    if (col < nvec) {
      // mean mode: every head gets GY / K under the mask of the D-wide Y
      const uint32_t q = mean ? col - hc[c] * g : col;
      gv[c] = G::mask(gy[q], yy[q]);
      if constexpr (DROP) gv[c] = G::scale(gv[c], dr.scale_out);
      if (mean) gv[c] = G::scale(gv[c], rk);
      gm[col] = gv[c];  // read per edge by k_gat_bwd_src_heads
    }
  }
  const uint32_t beg = co[d], end = co[d + 1];
  // pass 1: ga[e, h] = g_h . H[src_e]_h, parked in du by the head's lead lane,
  // which also sums a ga in edge order
  float sag[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) sag[c] = 0.f;
  for (uint32_t cb = beg; cb < end; cb += 64) {
    const uint32_t ne = min(end - cb, 64u);
    const uint32_t my_r = lane < (int)ne ? ri[cb + lane] : 0u;
    [[maybe_unused]] uint64_t kb[NCH];
    if constexpr (DROP) edge_keep_bits<NCH>(kb, cb + lane, heads, dr);
    for (uint32_t j0 = 0; j0 < ne; j0 += kGatU) {
      float p[kGatU][NCH], av[kGatU][NCH];
#pragma unroll
      for (int u = 0; u < kGatU; ++u) {
        const bool ok = j0 + u < ne;
        const uint32_t r = chunk_get(my_r, j0 + u, ne);
        const T* hr = reinterpret_cast<const T*>(H + (uint64_t)r * ldh);
        const uint64_t eb = (uint64_t)(cb + j0 + u) * heads;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const uint32_t col = lane + 64 * c;
          p[u][c] = (ok && col < nvec) ? G::dot(gv[c], hr[col]) : 0.f;
          av[u][c] = (ok && lead[c]) ? a[eb + hc[c]] : 0.f;
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
          if (lead[c]) {
            du[eb + hc[c]] = ga;
            sag[c] += av[u][c] * ga;
          }
        }
      }
    }
  }
  // pass 2: softmax and leaky_relu backward, per head by its lead lane
  const uint64_t dd = (uint64_t)dl[d] * heads;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    if (lead[c]) {
      float s = 0.f;
#pragma unroll 4
      for (uint32_t e = beg; e < end; ++e) {
        const uint64_t i = (uint64_t)e * heads + hc[c];
        const float dm = a[i] * (du[i] - sag[c]);
        const float u = m[i] > 0.f ? dm : 0.2f * dm;
        du[i] = u;
        s += u;
      }
      ds2[dd + hc[c]] = s;
    }
}


// DROP: as k_gat_bwd_src, per head; the lane that owns CSR slot cb + lane
// draws the bits of that slot's CSC edge
template <int VEC, int NCH, int = 0, bool DROP = false, class... DR>  // (no reduction here: one form for every g)
__global__ __launch_bounds__(kGatThreads) void k_gat_bwd_src_heads(
    const uint32_t* __restrict__ ro, const uint32_t* __restrict__ ci,
    const uint32_t* __restrict__ ceid, uint32_t nv_src, uint32_t nvec, uint32_t g, uint32_t heads,
    const float* __restrict__ a, const float* __restrict__ du, const float* __restrict__ ds2,
    const float* __restrict__ att, const float* __restrict__ GM, uint64_t ldm,
    float* __restrict__ dH, uint64_t lddh, float* __restrict__ dS, DR... drs) {
  [[maybe_unused]] const GatDrop& dr = drop_of(drs...);
  using G = GV<VEC>;
  using T = typename G::T;
  const int lane = threadIdx.x & 63;
  const uint32_t v = blockIdx.x * (kGatThreads / 64) + (threadIdx.x >> 6);
  if (v >= nv_src) return;
  uint32_t hc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) hc[c] = (lane + 64 * c) / g;
  const uint32_t beg = ro[v], end = ro[v + 1];
  T acc[NCH];
  float s1[NCH];  // every lane sums its head's du in edge order: no reduction
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    acc[c] = G::zero();
    s1[c] = 0.f;
  }
  for (uint32_t cb = beg; cb < end; cb += 64) {
    const uint32_t ne = min(end - cb, 64u);
    uint32_t my_d = 0, my_e = 0;
    if (lane < (int)ne) {
      my_e = ceid[cb + lane];
      my_d = ci[cb + lane];
    }
    [[maybe_unused]] uint64_t kb[NCH];
    if constexpr (DROP) edge_keep_bits<NCH>(kb, my_e, heads, dr);
    for (uint32_t j0 = 0; j0 < ne; j0 += kGatU) {
      T x[kGatU][NCH];
      float w[kGatU][NCH], uu[kGatU][NCH];
#pragma unroll
      for (int u = 0; u < kGatU; ++u) {
        const bool ok = j0 + u < ne;
        const int jj = (int)min(j0 + u, ne - 1);
        const uint32_t dd = chunk_get(my_d, j0 + u, ne);
        const uint64_t eb = (uint64_t)chunk_get(my_e, j0 + u, ne) * heads;
        const T* gm = reinterpret_cast<const T*>(GM + (uint64_t)dd * ldm);
        [[maybe_unused]] uint64_t kj[NCH];
        if constexpr (DROP) keep_bits_from<NCH>(kj, kb, jj, heads);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const uint32_t col = lane + 64 * c;
          const bool in = ok && col < nvec;
          x[u][c] = in ? gm[col] : G::zero();
          w[u][c] = in ? a[eb + hc[c]] : 0.f;
          if constexpr (DROP) w[u][c] = head_kept<NCH>(kj, hc[c], c) ? w[u][c] * dr.scale_attn : 0.f;
          uu[u][c] = in ? du[eb + hc[c]] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < kGatU; ++u)
        if (j0 + u < ne) {  // edge order kept
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            acc[c] = G::axpy(acc[c], w[u][c], x[u][c]);
            s1[c] += uu[u][c];
          }
        }
    }
  }
  const T* a1 = reinterpret_cast<const T*>(att);
  const T* a2 = reinterpret_cast<const T*>(att + (uint64_t)nvec * VEC);
  T* out = reinterpret_cast<T*>(dH + (uint64_t)v * lddh);
  float* ds = dS + 2 * (uint64_t)v * heads;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint32_t col = lane + 64 * c;
    if (col < nvec) {
      const float s2 = ds2[(uint64_t)v * heads + hc[c]];
      out[col] = G::axpy(G::axpy(acc[c], s1[c], a1[col]), s2, a2[col]);
      if (col == hc[c] * g) {
        ds[hc[c]] = s1[c];
        ds[heads + hc[c]] = s2;
      }
    }
  }
}


// plain inverted dropout with the shared keep bits (the input pass of
// gat_feat_drop): thread = a 4-row x 2-column block, one generator call
__global__ void k_dropout(const float* x, uint64_t ldx, uint32_t rows, uint32_t F,
                          uint32_t keep_threshold, float scale, uint64_t seed, uint64_t offset,
                          float* y, uint64_t ldy) {
  const uint32_t cpairs = (F + 1) / 2;
  const uint64_t blocks = (uint64_t)((rows + 3) / 4) * cpairs;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < blocks;
       t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r4 = (uint32_t)(t / cpairs) * 4, c2 = (uint32_t)(t % cpairs) * 2;
    uint4 rnd = make_uint4(0u, 0u, 0u, 0u);
    if (keep_threshold) rnd = dropout_words(r4, c2, seed, offset);
    const uint32_t wd[4] = {rnd.x, rnd.y, rnd.z, rnd.w};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const uint32_t r = r4 + v;
      if (r >= rows) break;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t c = c2 + h;
        if (c >= F) break;
        const float a = x[(uint64_t)r * ldx + c];  // (y may be x: read before the write)
        y[(uint64_t)r * ldy + c] = dropout_bits(wd[v], c) >= keep_threshold ? a * scale : 0.f;
      }
    }
  }
}

}  // namespace nts_hip

using namespace nts_hip;

// at most 4 vectors per lane: 4 * 64 float4 or 4 * 64 floats a row
static const char kGatWidthMsg[] =
    "feature width too large (F <= 1024 on 16-byte aligned rows with pitches that are "
    "multiples of 4, F <= 256 otherwise)";

// ---- entry points: checks and dispatch ---------------------------------------------
// The plain and the _drop entry points share one checked implementation each:
// `fn` is the entry point's name for the error text, `dr` its dropout (none, or
// both rates 0: the plain kernels, the same launches as without the options).
namespace {

int gat_forward_heads_impl(const char* fn, nts_hip_ctx* ctx, const uint32_t* column_offset,
                           const uint32_t* row_indices, const uint32_t* dst_local_id,
                           uint32_t v_size, const float* H, uint64_t ldh, uint32_t heads,
                           uint32_t D, const float* att, float* m_out, float* a_out, float* Y,
                           uint64_t ldy, int mean, const GatDrop* dr) {
  GAT_CHECK(ctx && column_offset && row_indices && dst_local_id && H && att && m_out && a_out && Y,
            "NULL argument");
  NTS_RET(gat_heads_check(fn, heads, D));
  const uint32_t F = heads * D, FY = mean ? D : F;
  GAT_CHECK(ldh >= F && ldy >= FY, "leading dimension");
  const bool v4 = gat_vec4(D, {{H, ldh}, {Y, ldy}, {att, 0}});
  HeadsShape hs;
  NTS_RET(gat_heads_shape(fn, heads, D, v4, &hs));
  if (v_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  return gat_dispatch(v4, hs.nch, hs.mode, [&](auto V, auto N, auto M) {
    return gat_launch(k_gat_fwd_heads<V(), N(), M()>, k_gat_fwd_heads<V(), N(), M(), true, GatDrop>,
                      gat_grid(v_size), gat_mean_lds(mean, hs.nch, v4), ctx->stream, dr,
                      column_offset, row_indices, dst_local_id, v_size, H, ldh, hs.nvec, hs.g, heads,
                      att, m_out, a_out, Y, ldy, mean);
  });
}

int gat_backward_heads_impl(const char* fn, nts_hip_ctx* ctx, const uint32_t* column_offset,
                            const uint32_t* row_indices, const uint32_t* dst_local_id,
                            uint32_t v_size, const uint32_t* row_offset,
                            const uint32_t* column_indices, const uint32_t* csr_edge_id,
                            uint32_t src_size, const float* H, uint64_t ldh, uint32_t heads,
                            uint32_t D, const float* att, const float* a, const float* m,
                            const float* Y, uint64_t ldy, const float* GY, uint64_t ldg, float* du,
                            float* ds2, float* GM, uint64_t ldm, float* dH, uint64_t lddh,
                            float* dS, int mean, const GatDrop* dr) {
  GAT_CHECK(ctx && column_offset && row_indices && dst_local_id && row_offset && column_indices &&
                csr_edge_id && H && att && a && m && Y && GY && du && ds2 && GM && dH && dS,
            "NULL argument");
  NTS_RET(gat_heads_check(fn, heads, D));
  const uint32_t F = heads * D, FY = mean ? D : F;
  GAT_CHECK(ldm >= F, "leading dimension of GM");
  GAT_CHECK(ldh >= F && ldy >= FY && ldg >= FY && lddh >= F, "leading dimension");
  const bool v4 =
      gat_vec4(D, {{H, ldh}, {Y, ldy}, {att, 0}, {GY, ldg}, {dH, lddh}, {GM, ldm}});
  // a refused shape leaves every output as it was: checked before ds2 is cleared
  HeadsShape hs;
  NTS_RET(gat_heads_shape(fn, heads, D, v4, &hs));
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const hipStream_t st = ctx->stream;
  if (src_size)
    NTS_HIP_TRY(hipMemsetAsync(ds2, 0, (size_t)src_size * heads * sizeof(float), st));
  if (v_size)
    NTS_RET(gat_dispatch(v4, hs.nch, hs.mode, [&](auto V, auto N, auto M) {
      return gat_launch(k_gat_bwd_dst_heads<V(), N(), M()>,
                        k_gat_bwd_dst_heads<V(), N(), M(), true, GatDrop>, gat_grid(v_size), 0, st,
                        dr, column_offset, row_indices, dst_local_id, v_size, H, ldh, hs.nvec, hs.g,
                        heads, a, m, Y, ldy, GY, ldg, du, ds2, GM, ldm, mean);
    }));
  if (src_size)
    NTS_RET(gat_dispatch(v4, hs.nch, [&](auto V, auto N) {
      return gat_launch(k_gat_bwd_src_heads<V(), N(), 0>,
                        k_gat_bwd_src_heads<V(), N(), 0, true, GatDrop>, gat_grid(src_size), 0, st,
                        dr, row_offset, column_indices, csr_edge_id, src_size, hs.nvec, hs.g, heads,
                        a, du, ds2, att, GM, ldm, dH, lddh, dS);
    }));
  return NTS_OK;
}

int gat_forward_impl(const char* fn, nts_hip_ctx* ctx, const uint32_t* column_offset,
                     const uint32_t* row_indices, const uint32_t* dst_local_id, uint32_t v_size,
                     const float* H, uint64_t ldh, uint32_t F, const float* att, float* m_out,
                     float* a_out, float* Y, uint64_t ldy, const GatDrop* dr) {
  GAT_CHECK(ctx && column_offset && row_indices && dst_local_id && H && att && m_out && a_out && Y,
            "NULL argument");
  GAT_CHECK(ldh >= F && ldy >= F, "leading dimension");
  if (v_size == 0 || F == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const bool v4 = gat_vec4(F, {{H, ldh}, {Y, ldy}, {att, 0}});
  const uint32_t nvec = v4 ? F / 4 : F;
  const int nch = (int)((nvec + 63) / 64);
  GAT_CHECK(nch <= 4, kGatWidthMsg);
  return gat_dispatch(v4, nch, [&](auto V, auto N) {
    return gat_launch(k_gat_fwd<V(), N()>, k_gat_fwd<V(), N(), true, GatDrop>, gat_grid(v_size), 0,
                      ctx->stream, dr, column_offset, row_indices, dst_local_id, v_size, H, ldh,
                      nvec, att, m_out, a_out, Y, ldy);
  });
}

int gat_backward_impl(const char* fn, nts_hip_ctx* ctx, const uint32_t* column_offset,
                      const uint32_t* row_indices, const uint32_t* dst_local_id, uint32_t v_size,
                      const uint32_t* row_offset, const uint32_t* column_indices,
                      const uint32_t* csr_edge_id, uint32_t src_size, const float* H, uint64_t ldh,
                      uint32_t F, const float* att, const float* a, const float* m, const float* Y,
                      uint64_t ldy, const float* GY, uint64_t ldg, float* du, float* ds2, float* GM,
                      uint64_t ldm, float* dH, uint64_t lddh, float* dS, const GatDrop* dr) {
  GAT_CHECK(ctx && column_offset && row_indices && dst_local_id && row_offset && column_indices &&
                csr_edge_id && H && att && a && m && Y && GY && du && ds2 && GM && dH && dS,
            "NULL argument");
  GAT_CHECK(ldm >= F, "leading dimension of GM");
  GAT_CHECK(ldh >= F && ldy >= F && ldg >= F && lddh >= F, "leading dimension");
  if (F == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const hipStream_t st = ctx->stream;
  const bool v4 =
      gat_vec4(F, {{H, ldh}, {Y, ldy}, {att, 0}, {GY, ldg}, {dH, lddh}, {GM, ldm}});
  const uint32_t nvec = v4 ? F / 4 : F;
  const int nch = (int)((nvec + 63) / 64);
  // a refused width leaves every output as it was: checked before ds2 is cleared
  GAT_CHECK(nvec <= 256, kGatWidthMsg);
  if (src_size) NTS_HIP_TRY(hipMemsetAsync(ds2, 0, (size_t)src_size * sizeof(float), st));
  if (v_size)
    NTS_RET(gat_dispatch(v4, nch, [&](auto V, auto N) {
      return gat_launch(k_gat_bwd_dst<V(), N()>, k_gat_bwd_dst<V(), N(), true, GatDrop>,
                        gat_grid(v_size), 0, st, dr, column_offset, row_indices, dst_local_id,
                        v_size, H, ldh, nvec, a, m, Y, ldy, GY, ldg, du, ds2, GM, ldm);
    }));
  if (src_size)
    NTS_RET(gat_dispatch(v4, nch, [&](auto V, auto N) {
      return gat_launch(k_gat_bwd_src<V(), N()>, k_gat_bwd_src<V(), N(), true, GatDrop>,
                        gat_grid(src_size), 0, st, dr, row_offset, column_indices, csr_edge_id,
                        src_size, nvec, a, du, ds2, att, GM, ldm, dH, lddh, dS);
    }));
  return NTS_OK;
}

}  // namespace

extern "C" {

int nts_hip_gat_forward_heads(nts_hip_ctx* ctx, const uint32_t* column_offset,
                              const uint32_t* row_indices, const uint32_t* dst_local_id,
                              uint32_t v_size, const float* H, uint64_t ldh, uint32_t heads,
                              uint32_t D, const float* att, float* m_out, float* a_out, float* Y,
                              uint64_t ldy, int mean) {
  return gat_forward_heads_impl(__func__, ctx, column_offset, row_indices, dst_local_id, v_size, H,
                                ldh, heads, D, att, m_out, a_out, Y, ldy, mean, nullptr);
}

int nts_hip_gat_forward_heads_drop(nts_hip_ctx* ctx, const uint32_t* column_offset,
                                   const uint32_t* row_indices, const uint32_t* dst_local_id,
                                   uint32_t v_size, const float* H, uint64_t ldh, uint32_t heads,
                                   uint32_t D, const float* att, float* m_out, float* a_out,
                                   float* Y, uint64_t ldy, int mean, float p_attn, float p_out,
                                   uint64_t seed, uint64_t off_attn, uint64_t off_out) {
  std::optional<GatDrop> dr;
  NTS_RET(gat_drop(__func__, p_attn, p_out, seed, off_attn, off_out, &dr));
  return gat_forward_heads_impl(__func__, ctx, column_offset, row_indices, dst_local_id, v_size, H,
                                ldh, heads, D, att, m_out, a_out, Y, ldy, mean, gat_drop_ptr(dr));
}

int nts_hip_gat_backward_heads(nts_hip_ctx* ctx, const uint32_t* column_offset,
                               const uint32_t* row_indices, const uint32_t* dst_local_id,
                               uint32_t v_size, const uint32_t* row_offset,
                               const uint32_t* column_indices, const uint32_t* csr_edge_id,
                               uint32_t src_size, const float* H, uint64_t ldh, uint32_t heads,
                               uint32_t D, const float* att, const float* a, const float* m,
                               const float* Y, uint64_t ldy, const float* GY, uint64_t ldg,
                               float* du, float* ds2, float* GM, uint64_t ldm, float* dH,
                               uint64_t lddh, float* dS, int mean) {
  return gat_backward_heads_impl(__func__, ctx, column_offset, row_indices, dst_local_id, v_size,
                                 row_offset, column_indices, csr_edge_id, src_size, H, ldh, heads, D,
                                 att, a, m, Y, ldy, GY, ldg, du, ds2, GM, ldm, dH, lddh, dS, mean,
                                 nullptr);
}

int nts_hip_gat_backward_heads_drop(nts_hip_ctx* ctx, const uint32_t* column_offset,
                                    const uint32_t* row_indices, const uint32_t* dst_local_id,
                                    uint32_t v_size, const uint32_t* row_offset,
                                    const uint32_t* column_indices, const uint32_t* csr_edge_id,
                                    uint32_t src_size, const float* H, uint64_t ldh, uint32_t heads,
                                    uint32_t D, const float* att, const float* a, const float* m,
                                    const float* Y, uint64_t ldy, const float* GY, uint64_t ldg,
                                    float* du, float* ds2, float* GM, uint64_t ldm, float* dH,
                                    uint64_t lddh, float* dS, int mean, float p_attn, float p_out,
                                    uint64_t seed, uint64_t off_attn) {
  std::optional<GatDrop> dr;
  NTS_RET(gat_drop(__func__, p_attn, p_out, seed, off_attn, 0, &dr));
  return gat_backward_heads_impl(__func__, ctx, column_offset, row_indices, dst_local_id, v_size,
                                 row_offset, column_indices, csr_edge_id, src_size, H, ldh, heads, D,
                                 att, a, m, Y, ldy, GY, ldg, du, ds2, GM, ldm, dH, lddh, dS, mean,
                                 gat_drop_ptr(dr));
}

int nts_hip_gat_forward(nts_hip_ctx* ctx, const uint32_t* column_offset,
                        const uint32_t* row_indices, const uint32_t* dst_local_id,
                        uint32_t v_size, const float* H, uint64_t ldh, uint32_t F,
                        const float* att, float* m_out, float* a_out, float* Y, uint64_t ldy) {
  return gat_forward_impl(__func__, ctx, column_offset, row_indices, dst_local_id, v_size, H, ldh, F,
                          att, m_out, a_out, Y, ldy, nullptr);
}

int nts_hip_gat_forward_drop(nts_hip_ctx* ctx, const uint32_t* column_offset,
                             const uint32_t* row_indices, const uint32_t* dst_local_id,
                             uint32_t v_size, const float* H, uint64_t ldh, uint32_t F,
                             const float* att, float* m_out, float* a_out, float* Y, uint64_t ldy,
                             float p_attn, float p_out, uint64_t seed, uint64_t off_attn,
                             uint64_t off_out) {
  std::optional<GatDrop> dr;
  NTS_RET(gat_drop(__func__, p_attn, p_out, seed, off_attn, off_out, &dr));
  return gat_forward_impl(__func__, ctx, column_offset, row_indices, dst_local_id, v_size, H, ldh, F,
                          att, m_out, a_out, Y, ldy, gat_drop_ptr(dr));
}

int nts_hip_gat_backward(nts_hip_ctx* ctx, const uint32_t* column_offset,
                         const uint32_t* row_indices, const uint32_t* dst_local_id,
                         uint32_t v_size, const uint32_t* row_offset,
                         const uint32_t* column_indices, const uint32_t* csr_edge_id,
                         uint32_t src_size, const float* H, uint64_t ldh, uint32_t F,
                         const float* att, const float* a, const float* m, const float* Y,
                         uint64_t ldy, const float* GY, uint64_t ldg, float* du, float* ds2,
                         float* GM, uint64_t ldm, float* dH, uint64_t lddh, float* dS) {
  return gat_backward_impl(__func__, ctx, column_offset, row_indices, dst_local_id, v_size,
                           row_offset, column_indices, csr_edge_id, src_size, H, ldh, F, att, a, m, Y,
                           ldy, GY, ldg, du, ds2, GM, ldm, dH, lddh, dS, nullptr);
}

int nts_hip_gat_backward_drop(nts_hip_ctx* ctx, const uint32_t* column_offset,
                              const uint32_t* row_indices, const uint32_t* dst_local_id,
                              uint32_t v_size, const uint32_t* row_offset,
                              const uint32_t* column_indices, const uint32_t* csr_edge_id,
                              uint32_t src_size, const float* H, uint64_t ldh, uint32_t F,
                              const float* att, const float* a, const float* m, const float* Y,
                              uint64_t ldy, const float* GY, uint64_t ldg, float* du, float* ds2,
                              float* GM, uint64_t ldm, float* dH, uint64_t lddh, float* dS,
                              float p_attn, float p_out, uint64_t seed, uint64_t off_attn) {
  std::optional<GatDrop> dr;
  NTS_RET(gat_drop(__func__, p_attn, p_out, seed, off_attn, 0, &dr));
  return gat_backward_impl(__func__, ctx, column_offset, row_indices, dst_local_id, v_size,
                           row_offset, column_indices, csr_edge_id, src_size, H, ldh, F, att, a, m, Y,
                           ldy, GY, ldg, du, ds2, GM, ldm, dH, lddh, dS, gat_drop_ptr(dr));
}

int nts_hip_dropout_f32(nts_hip_ctx* ctx, uint32_t rows, uint32_t feature_size, const float* x,
                        uint64_t ldx, float p, uint64_t seed, uint64_t offset, float* y,
                        uint64_t ldy) {
  NTS_CHECK_ARG(ctx && x && y, "NULL argument");
  NTS_CHECK_ARG(ldx >= feature_size && ldy >= feature_size, "leading dimension");
  NTS_CHECK_ARG(gat_rate_ok(p), kGatRateMsg);
  if (rows == 0 || feature_size == 0) return NTS_OK;
  NTS_HIP_TRY(hipSetDevice(ctx->device));
  const uint64_t blocks = (uint64_t)((rows + 3) / 4) * ((feature_size + 1) / 2);
  const uint32_t gs = std::max(1u, std::min(ceil_div(blocks, 256), kMaxGrid));
  hipLaunchKernelGGL(k_dropout, dim3(gs), dim3(256), 0, ctx->stream, x, ldx, rows, feature_size,
                     dropout_threshold(p), p >= 1.f ? 0.f : 1.0f / (1.0f - p), seed, offset, y, ldy);
  NTS_LAUNCH_CHECK();
  return NTS_OK;
}

}  // extern "C"
