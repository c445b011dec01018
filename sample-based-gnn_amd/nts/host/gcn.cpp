// Model drivers: the GPU-sampled GCN / GraphSAGE toolkits.
//   GCN_SAMPLE_ALLGPU_impl   toolkits/GCN_SAMPLE_ALLGPU.hpp  (GPU sampler, 1 GPU)
//   GS_SAMPLE_ALLGPU         toolkits/GS_SAMPLE_ALLGPU.hpp   (same pipeline, Mean weights, :296)
//   GCN_SAMPLE_ALL_MULTI     toolkits/GCN_SAMPLE_ALL_MULTI.hpp (data parallel, grad SUM all-reduce)
// One class covers the three: the weight type and the optional communicator
// select the variant.  Per batch: sample_gpu_fast -> load_label_gpu ->
// [fused feature gather +] graph op -> vertexForward ... -> Loss ->
// self_backward -> Update (all-reduce + Adam) -> zero_grad.
#include "gcn.hpp"
#include "ops_util.hpp"
#include "options.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <random>
#include <cstdio>
#include <cstdlib>

namespace nts {

// cfg.feature_f16: the table as IEEE half with rows a lane can load 16 bytes
// of.  The pitch is the row rounded up to 8 halves; rows of 256 bytes and more
// are padded to a 128-byte multiple, the fp32 table's rule for its wide rows
// (a gathered row then spans the fewest cache lines).  An fp32 table is rounded
// to nearest even by the copy; a half table that already has such rows is used
// as given.  Values that are not finite as a half are refused.
static NtsVar half_feature_table(const NtsVar& t, int device) {
  const int64_t V = t.size(0), K = t.size(1);
  const int64_t ld = K >= 128 ? (K + 63) / 64 * 64 : (K + 7) / 8 * 8;
  NtsVar h = t;
  // (as given: also the last row's pitch padding, which a 16-byte load of a
  // partial last vector reads, must lie inside the tensor's storage)
  const int64_t K8 = (K + 7) / 8 * 8;
  const bool as_given =
      t.dtype() == torch::kFloat16 && t.stride(1) == 1 && t.stride(0) % 8 == 0 &&
      t.stride(0) >= K8 && (uintptr_t)t.data_ptr() % 16 == 0 &&
      (uint64_t)(t.storage_offset() + std::max<int64_t>(V - 1, 0) * t.stride(0) + K8) * 2 <=
          (uint64_t)t.storage().nbytes();
  if (!as_given) {
    h = torch::empty({V, ld}, torch::TensorOptions().dtype(torch::kFloat16).device(torch::kCUDA, device))
            .narrow(1, 0, K);
    h.copy_(t);
  }
  const NtsVar bad = torch::logical_not(torch::isfinite(h)).any(1);
  const int64_t rows = bad.sum().item<int64_t>();
  if (rows > 0) {
    const int64_t n = torch::logical_not(torch::isfinite(h)).sum().item<int64_t>();
    const int64_t first = bad.to(torch::kInt32).argmax().item<int64_t>();
    TORCH_CHECK(false, "feature_f16: ", n, " feature value(s) are not finite as IEEE half (the "
                "largest finite half is 65504); the first is in row ", first,
                ": scale the features or keep the fp32 table");
  }
  return h;
}

GCN_SAMPLE_ALLGPU_impl::GCN_SAMPLE_ALLGPU_impl(std::shared_ptr<FullyRepGraph> g, NtsVar feature,
                                               NtsVar label, std::vector<VertexId> train_nids,
                                               GCNConfig c, std::shared_ptr<Communicator> comm_)
    : graph(std::move(g)), F(std::move(feature)), L_GT(std::move(label)), cfg(std::move(c)),
      comm(std::move(comm_)) {
  check_driver_options(cfg, {F.scalar_type(), F.is_cuda(), F.dim() == 2 ? F.size(1) : -1,
                             L_GT.sizes().vec(), L_GT.is_cuda(),
                             (int64_t)graph->global_vertices, graph->edge_prob.defined()});
  // (derived after the check: the rules above read the caller's value)
  if (cfg.sample_gpu) cfg.deterministic_backward = true;  // the CSR exists for every backward
  // sampler_cus n > 0: the sampler's stream on n CUs, the training stream on
  // the others; n < 0: the sampler on |n| CUs, the training stream on all
  if (cfg.pipeline && cfg.sampler_cus > 0)
    cs = std::make_unique<NtsStream>(graph->device,
                                     cu_mask_spread(graph->device, cfg.sampler_cus, true),
                                     (uint64_t)cfg.seed);
  else
    cs = std::make_unique<NtsStream>(graph->device, nullptr, (uint64_t)cfg.seed,
                                     cfg.pipeline && cfg.sampler_priority < 0);
  NTS_CALL(nts_hip_ctx_set_gemm_mode, cs->ctx(), cfg.gemm_mode);
  // inputs were produced on other streams: order them before our stream
  TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "hipDeviceSynchronize");
  auto guard = cs->guard();
  // Wide feature rows are re-laid with a 128-byte aligned pitch (one copy,
  // +1% memory): a gathered row then spans the minimum number of cache lines
  // (19 instead of ~19.8 for 602 floats), ~2% less traffic in the bottom
  // aggregation, which reads every sampled row once per edge.
  // (feature_f16: the half table is laid out below, after the sampler is
  // built; nothing here touches the table before)
  const bool f16 = cfg.feature_f16;
  if (!f16 && cfg.pad_features && F.size(1) >= 256 && F.size(1) % 32 != 0 && F.stride(1) == 1) {
    NtsVar Fp = row_padded_empty(F.size(0), F.size(1), graph->device);
    Fp.copy_(F);
    F = Fp;
  }
  if (cfg.cache_rate >= 0.0 && !f16) {
    const uint64_t V = graph->global_vertices;
    const uint64_t n_cache = std::min<uint64_t>(V, (uint64_t)(cfg.cache_rate * (double)V));
    fcache = std::make_unique<FeatureCache>(*cs, *graph, F, n_cache);
    F = torch::empty({0, F.size(1)}, f32_opts(graph->device));  // HBM table released
  }
  if (cfg.shuffle) {  // shuffle_vec (toolkits/GCN_SAMPLE_GPU.hpp:175-180): mt19937(2000)
    std::mt19937 gen(2000);
    std::shuffle(train_nids.begin(), train_nids.end(), gen);
  }
  const int L = (int)cfg.fanout.size();
  // Bottom layer order: transform first when the first layer
  // narrows the rows — the aggregation then gathers F_out-wide rows of X W
  // (a table that stays in the Infinity Cache) instead of F_in-wide feature
  // rows, at the price of a GEMM over the src rows instead of the dst rows.
  const bool tf_ok = L >= 2 && !cfg.gat && !fcache && cfg.hip_gemm && cfg.fuse_activation &&
                     !cfg.pd_cache && !cfg.root_weight && !max_aggr() && !cfg.layer_norm &&
                     !cfg.batch_norm && !cfg.subgraph;
  // auto (-1): transform first where the first layer narrows the rows at
  // least 4x and its GEMMs run on the whole-row fp32-exact kernels
  // (csrc/gemmx3.hip, split-bf16) or the f16 pair tables (C2: 602 -> 128,
  // 0.93 vs 1.04 ms/step fp32-exact); the reference's order elsewhere
  tf_ = tf_ok && !f16 && (cfg.transform_first == 1 ||
                  (cfg.transform_first < 0 &&
                   (cfg.pair_table >= 3 || cfg.gemm_mode == NTS_GEMM_SPLIT3) &&
                   cfg.layer_size[0] >= 4 * cfg.layer_size[1]));
  if (tf_ && cfg.pair_table > 0) {
    // the feature table is static: its rows are split into f16 pairs once,
    // in ONE layout — planar where the planar kernels take the shape (both
    // GEMMs: every dW output row in one block, K <= 640, N % 128 == 0),
    // interleaved otherwise
    const int64_t V = F.size(0), K = F.size(1), Kp = (K + 31) / 32 * 32;
    const int64_t Nh = cfg.layer_size[1];
    pairs_ = std::make_unique<PairTable>();
    pairs_->rs = torch::empty({V}, f32_opts(graph->device));
    pairs_->tn = cfg.pair_table >= 2;
    if (cfg.pair_table >= 3 && Kp <= 640 && Nh % 128 == 0) {
      // rows padded to 2560 bytes where that leaves a tail for the row scale
      // (the four-stage forward GEMM reads it with the row); Q is the [V, 2 Kp]
      // view of the padded rows
      const int64_t ldq = 4 * Kp + 8 <= 2560 ? 1280 : 2 * Kp;
      pairs_->Q = torch::empty({V, ldq}, torch::TensorOptions().dtype(torch::kInt16).device(F.device()))
                      .narrow(1, 0, 2 * Kp);
      NTS_CALL(nts_hip_h2_split_rows_planar, cs->ctx(), (uint64_t)V, (uint32_t)K,
               F.data_ptr<float>(), (uint64_t)F.stride(0), (uint32_t)Kp,
               reinterpret_cast<uint16_t*>(pairs_->Q.data_ptr<int16_t>()), (uint64_t)ldq,
               pairs_->rs.data_ptr<float>());
    } else {
      pairs_->P = torch::empty({V, Kp}, torch::TensorOptions().dtype(torch::kInt32).device(F.device()));
      NTS_CALL(nts_hip_h2_split_rows, cs->ctx(), (uint64_t)V, (uint32_t)K, F.data_ptr<float>(),
               (uint64_t)F.stride(0), (uint32_t)Kp,
               reinterpret_cast<uint32_t*>(pairs_->P.data_ptr<int32_t>()), (uint64_t)Kp,
               pairs_->rs.data_ptr<float>());
    }
  }
  // CSR transposes only where a graph-op backward runs (every hop but the
  // outermost, whose backward the context skips — unless the bottom layer is
  // transform-first: its aggregation then has a backward, dH = A^T dZ)
  std::vector<bool> csr(L, cfg.deterministic_backward);
  csr[L - 1] = tf_;
  if (cfg.gat) csr.assign(L, true);  // every layer's backward runs over its CSR
  // Pipelined: three sampler slots.  Batch k+1 is sampled into the slot of
  // batch k-2, whose training finished before batch k-1's began, so the
  // sampling stream never waits on an unfinished event when its kernels are
  // launched (with two slots it waits on batch k-1's training, and ROCm then
  // blocks every launch on that stream in the host for ~60 us).
  nslots_ = cfg.pipeline ? kSlots : 1;
  sampler = std::make_unique<FastSampler>(graph, train_nids, L, cfg.batch_size, cfg.fanout,
                                          nslots_, csr,
                                          sample_weight() != WeightType::None || cfg.edge_weighted,
                                          cfg.gat || cfg.root_weight, max_aggr(),
                                          cfg.subgraph ? cfg.subgraph_walk : -1,
                                          (uint64_t)cfg.subgraph_edge_cap);
  sampler->rng_mode = cfg.rng_mode;
  sampler->weighted = cfg.weighted_sampling;
  sampler->coef = cfg.edge_weighted;
  sampler->up_degree = cfg.up_degree;
  if (cfg.root_weight)  // the inverse of dst_local_id, for every hop with a graph-op backward
    for (auto* q : sampler->ssgs)
      for (auto* s : q->sampled_sgs)
        if (s->has_csr)
          s->src_dst = torch::empty({std::max<int64_t>(s->s_cap, 1)}, u32_opts(graph->device));
  if (cfg.pipeline && cfg.sampler_cus != 0)
    ss = std::make_unique<NtsStream>(graph->device,
                                     cu_mask_spread(graph->device, std::abs(cfg.sampler_cus), false),
                                     (uint64_t)cfg.seed);
  else if (cfg.pipeline)
    ss = std::make_unique<NtsStream>(graph->device, nullptr, (uint64_t)cfg.seed,
                                     cfg.sampler_priority == 1 ||
                                         (cfg.sampler_priority == 2 && is_mt_mode(cfg.rng_mode)));
  // size the scratch arenas once so the training loop never allocates
  uint64_t items = graph->global_vertices;
  for (auto* s : sampler->ssg->sampled_sgs) items = std::max<uint64_t>({items, s->e_cap, s->v_cap});
  NTS_CALL(nts_hip_ctx_reserve, cs->ctx(), graph->global_vertices, items);
  if (ss) {
    NTS_CALL(nts_hip_ctx_reserve, ss->ctx(), graph->global_vertices, items);
    NTS_CALL(nts_hip_ctx_set_gemm_mode, ss->ctx(), cfg.gemm_mode);
  }
  // The bottom graph op Y_0 = A_0 X depends on the sampled graph and the
  // feature table only (not on the weights), so it is issued right behind the
  // sampling, on the sampling stream: with the pipeline it runs while the
  // previous batch trains (HBM-bound gather next to MFMA-bound GEMMs).
  early_ = cfg.early_aggregate && cfg.fused_gather && !cfg.gat && !tf_ && !cfg.pd_cache;
  sampler->rerun_ok = !early_;  // (an MT re-run would leave the early aggregation stale)
  if (cfg.pd_cache) {
    pd_cache_map_ = torch::full({(int64_t)graph->global_vertices}, -1, u32_opts(graph->device));
    pd_cache_loc_ = torch::zeros({(int64_t)graph->global_vertices}, u32_opts(graph->device));
  }
  if (f16) F = half_feature_table(F, graph->device);
  for (int i = 0; i < nslots_; ++i) {
    TORCH_CHECK(hipEventCreateWithFlags(&ready_[i], hipEventDisableTiming) == hipSuccess,
                "hipEventCreate");
    if (early_)
      pre_y_[i] = row_padded_empty((int64_t)sampler->ssgs[i]->sampled_sgs[L - 1]->v_cap,
                                   (cfg.root_weight ? 2 : 1) * F.size(1), graph->device);
    if (early_ && fcache)
      stage_[i] = torch::empty({(int64_t)std::max<uint32_t>(sampler->ssgs[i]->sampled_sgs[L - 1]->s_cap, 1),
                                (int64_t)fcache->ld},
                               f32_opts(graph->device));
  }
  correct_ = torch::zeros({1}, u32_opts(graph->device));
  if (cfg.multi_label) {  // the labels as bits, packed once; the [V, C] tensor is released
    label_bits_ = pack_label_bits(L_GT);
    L_GT = NtsVar();
    f1_ = torch::zeros({3}, u32_opts(graph->device));
  }
  init_nn();
  defer_ = comm && (cfg.overlap_allreduce == 1 || (cfg.overlap_allreduce < 0 && comm->nranks > 1));
  if (defer_) {
    TORCH_CHECK(hipStreamCreateWithFlags(&comm_stream_, hipStreamNonBlocking) == hipSuccess,
                "hipStreamCreate");
    TORCH_CHECK(hipEventCreateWithFlags(&grads_packed_, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&grads_reduced_, hipEventDisableTiming) == hipSuccess,
                "hipEventCreate");
  }
  if (cfg.pd_cache) {  // preSample on the device (the Python runner may replace it)
    auto hot = presample();
    set_presample(hot.first, hot.second);
  }
}

GCN_SAMPLE_ALLGPU_impl::~GCN_SAMPLE_ALLGPU_impl() {
  if (!tl_.empty()) {
    (void)hipDeviceSynchronize();
    const size_t from = tl_.size() > 80 ? tl_.size() - 80 : 0;
    for (size_t i = from; i < tl_.size(); ++i) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, tl_[from].second, tl_[i].second);
      fprintf(stderr, "[timeline] %s %9.1f us\n", tl_[i].first, ms * 1e3);
    }
    for (auto& e : tl_) (void)hipEventDestroy(e.second);
  }
  for (auto* e : ready_)
    if (e) (void)hipEventDestroy(e);
  if (defer_) {
    (void)hipDeviceSynchronize();
    (void)hipEventDestroy(grads_packed_);
    (void)hipEventDestroy(grads_reduced_);
    (void)hipStreamDestroy(comm_stream_);
  }
  for (auto* p : params()) delete p;
}

// Sampling of one batch into `slot` (sample_gpu_fast's device part), then —
// with early aggregation — the bottom graph op (fused feature gather +
// aggregation, SingleGPUAllSampleGraphOp::forward on the feature table) on
// the same stream.  Sizes are device-side: nothing here waits for the host.
// NTS_TIMELINE=1: timing events at the start/end of every sampling and
// training launch sequence, printed (relative to the first) at destruction —
// the unperturbed GPU timeline of the two streams (a profiler slows the host).
static bool timeline_on() {
  static const bool on = getenv("NTS_TIMELINE") != nullptr;
  return on;
}
void GCN_SAMPLE_ALLGPU_impl::mark(const char* what, NtsStream& st) {
  if (!timeline_on() || tl_.size() > 4000) return;
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return;
  (void)hipEventRecord(e, (hipStream_t)st.stream());
  tl_.push_back({what, e});
}

void GCN_SAMPLE_ALLGPU_impl::issue(int slot, NtsStream& st) {
  mark("S<", st);
  if (cfg.pd_cache) pd_issue(slot, st);
  sampler->issue_gpu_sample(cfg.batch_size, slot, st, sample_weight());
  sampler->omit_map = nullptr;
  if (cfg.root_weight)  // the backward's inverse maps, next to the sampling
    for (auto* s : sampler->ssgs[slot]->sampled_sgs)
      if (s->src_dst.defined())
        NTS_CALL(nts_hip_root_inverse_map, st.ctx(), s->dev_dst_local_id(), s->dev_v_size(),
                 s->v_cap, s->dev_src_size(), s->s_cap, dptr<uint32_t>(s->src_dst));
  if (!cfg.multi_label) {  // load_label_gpu for this batch, on the sampling stream next to its
     // subgraph (off the training stream; ordered by ready_[slot] below);
     // multi_label: the loss reads the packed table by the seeds' ids itself
    SampledSubgraph* q = sampler->ssgs[slot];
    const int64_t n = q->pending_batch;
    NtsVar& t = lbl_[slot];
    if (!t.defined() || t.size(0) < n)
      t = torch::empty({std::max<int64_t>(n, cfg.batch_size)},
                       torch::TensorOptions().dtype(torch::kInt64).device(torch::kCUDA, graph->device));
    if (n > 0)
      NTS_CALL(nts_hip_gather_labels, st.ctx(), L_GT.data_ptr<int64_t>(),
               q->sampled_sgs[0]->dev_dst(), nullptr, (uint32_t)n, t.data_ptr<int64_t>());
  }
  if (early_) {
    auto guard = st.guard();
    const int L = (int)P.size();
    sampCSC* s = sampler->ssgs[slot]->sampled_sgs[L - 1];
    if (cfg.profile) prof.begin(KernelProfiler::BOTTOM_AGG, (hipStream_t)st.stream());
    NtsVar& y = pre_y_[slot];
    if (fcache)
      fcache->aggregate(st.ctx(), s, dptr<uint32_t>(s->sizes), s->v_cap,
                        dptr<uint32_t>(s->sizes) + 2, s->s_cap, stage_[slot].data_ptr<float>(),
                        y.data_ptr<float>(), (uint64_t)y.stride(0));
    else  // from the table, sizes on the device; the bottom hop has no backward: no arg
      spmm_csc_fwd(st, agg_kind(), s, F, true, s->dev_v_size(), s->v_cap, y, nullptr, true);
    // bytes are added when the batch's sizes are known (train_batch)
    if (cfg.profile) prof.end(KernelProfiler::BOTTOM_AGG, (hipStream_t)st.stream(), 0.0);
  }
  TORCH_CHECK(hipEventRecord(ready_[slot], (hipStream_t)st.stream()) == hipSuccess,
              "hipEventRecord");
  mark("S>", st);
}

// compulsory bytes of the bottom aggregation: distinct src rows once, index +
// weight per edge, offsets, output rows (+ source map when fused)  
double GCN_SAMPLE_ALLGPU_impl::bottom_bytes(SampledSubgraph* sg, bool fused_map) const {
  sampCSC* s = sg->sampled_sgs[sg->layers - 1];
  const double Fd = (double)(fcache ? fcache->F : F.size(1));
  const double xb = fcache ? 4.0 : (double)F.element_size();  // 2 with feature_f16
  return Fd * xb * s->src_size + 8.0 * s->e_size + 4.0 * (s->v_size + 1) +
         Fd * 4.0 * s->v_size + (fused_map ? 4.0 * s->src_size : 0.0);
}

void GCN_SAMPLE_ALLGPU_impl::init_nn() {
  for (size_t i = 0; i + 1 < cfg.layer_size.size(); ++i) {
    // root_weight: the stacked [W_n; W_s]
    // gat_heads: the last layer's K heads of layer_size.back() columns each
    // gat_v2: the stacked [W_s | W_d] and the score vector att [F_{l+1}, 1]
    const int64_t out = gat_width((int)i);
    P.push_back(new Parameter((cfg.root_weight ? 2 : 1) * cfg.layer_size[i],
                              (cfg.gat_v2 ? 2 : 1) * out, cfg.learn_rate, cfg.beta1,
                              cfg.beta2, cfg.epsilon, cfg.weight_decay, graph->device,
                              cfg.seed + (int64_t)i));
    if (cfg.gat)  // attention vector W_att [2 F_{l+1}, 1] (GAT_SAMPLE_ALL_GPU.hpp:141-147)
      P.push_back(new Parameter((cfg.gat_v2 ? 1 : 2) * out, 1, cfg.learn_rate, cfg.beta1,
                                cfg.beta2, cfg.epsilon, cfg.weight_decay, graph->device,
                                cfg.seed + 1000 + (int64_t)i));
  }
  if (cfg.hip_gemm)
    for (auto* p : P) p->cs = cs.get();
  if (cfg.layer_norm || cfg.batch_norm)  // gamma = 1, beta = 0 per hidden layer; never decayed
    for (size_t i = 0; i + 2 < cfg.layer_size.size(); ++i)
      for (float init : {1.f, 0.f}) {
        auto* q = new Parameter(1, (size_t)cfg.layer_size[i + 1], cfg.learn_rate, cfg.beta1,
                                cfg.beta2, cfg.epsilon, 0.f, graph->device, cfg.seed);
        q->W = torch::full({(int64_t)cfg.layer_size[i + 1]}, init, f32_opts(graph->device))
                   .set_requires_grad(true);
        q->M = torch::zeros_like(q->W).set_requires_grad(false);
        q->V = torch::zeros_like(q->W).set_requires_grad(false);
        LN.push_back(q);
      }
  if (cfg.batch_norm)  // running_mean = 0, running_var = 1 per hidden layer
    for (size_t i = 0; i + 2 < cfg.layer_size.size(); ++i)
      for (float init : {0.f, 1.f})
        BN.push_back(torch::full({(int64_t)cfg.layer_size[i + 1]}, init, f32_opts(graph->device)));
  int64_t n = 0;
  for (auto* p : params()) n += p->W.numel();
  grad_bucket = torch::zeros({n}, f32_opts(graph->device));
  if (comm) {  // identical initial weights on every rank (init_parameter / Bcast)
    torch::NoGradGuard ng;
    // the initialisation ran on libtorch's current stream: order it before the
    // broadcast on the driver stream (construction time only)
    TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "hipDeviceSynchronize");
    for (auto* p : params())
      comm->broadcast(p->W.data_ptr<float>(), (uint64_t)p->W.numel(), 0, cs->stream());
  }
}

void GCN_SAMPLE_ALLGPU_impl::set_weights(const std::vector<NtsVar>& ws) {
  flush_update();
  auto guard = cs->guard();
  const auto all = params();
  TORCH_CHECK(ws.size() == all.size(), LN.empty() ? "one tensor per layer"
                                                  : "one tensor per layer, then gamma and beta "
                                                    "of every hidden layer (the list of weights())");
  torch::NoGradGuard ng;
  for (size_t i = 0; i < all.size(); ++i) all[i]->W.copy_(ws[i].view_as(all[i]->W));
}

std::vector<NtsVar> GCN_SAMPLE_ALLGPU_impl::weights() {
  flush_update();
  std::vector<NtsVar> out;
  for (auto* p : params()) out.push_back(p->W.detach().clone());
  return out;
}

std::vector<NtsVar> GCN_SAMPLE_ALLGPU_impl::norm_stats() {
  auto guard = cs->guard();
  std::vector<NtsVar> out;
  for (const auto& b : BN) out.push_back(b.clone());
  cs->synchronize();
  return out;
}

void GCN_SAMPLE_ALLGPU_impl::set_norm_stats(const std::vector<NtsVar>& stats) {
  auto guard = cs->guard();
  TORCH_CHECK(stats.size() == BN.size(), "running_mean and running_var of every hidden layer "
                                         "(the list of norm_stats(): ", BN.size(), " tensors), got ",
              stats.size());
  torch::NoGradGuard ng;
  for (size_t i = 0; i < BN.size(); ++i) BN[i].copy_(stats[i].view_as(BN[i]));
}

// vertexForward (toolkits/GCN_SAMPLE_GPU.hpp:252-266): hidden layers
// dropout(relu(XW)), the last layer log_softmax(XW).
NtsVar GCN_SAMPLE_ALLGPU_impl::vertexForward(int l, NtsVar& a) {
  const int L = (int)P.size();
  if (l == L - 1)  // multi_label: raw logits (the sigmoid is the loss's)
    return cfg.multi_label ? P[l]->forward(a) : P[l]->forward(a).log_softmax(1);
  if (cfg.layer_norm)  // the plain GEMM, then LayerNorm + relu + dropout in one pass
    return layer_norm_act(l, P[l]->forward(a), drop_rate(), dropout_calls_++);
  if (cfg.batch_norm)  // the plain GEMM, then BatchNorm + relu + dropout; eval draws no offset
    return batch_norm_act(l, P[l]->forward(a), drop_rate(),
                          ctx.is_train() ? dropout_calls_++ : 0);
  if (cfg.hip_gemm && cfg.fuse_activation)
    return hip_linear_act(a, P[l]->W, drop_rate(), dropout_key(), dropout_calls_++, cs.get(),
                          cfg.pair_table > 0);
  return torch::dropout(torch::relu(P[l]->forward(a)), cfg.drop_rate, ctx.is_train());
}

std::vector<NtsVar> GCN_SAMPLE_ALLGPU_impl::forward(SampledSubgraph* sg, bool keep,
                                                     const NtsVar* pre_y,
                                                     const NtsVar* loss_target) {
  const int L = (int)P.size();
  std::vector<NtsVar> acts;
  auto keep_pair = [&](const NtsVar& Y, const NtsVar& X) {  // a layer's aggregation and output
    if (!keep) return;
    acts.push_back(Y.detach());
    acts.push_back(X.detach());
  };
  NtsVar X0;
  if (!cfg.fused_gather && !tf_) {
    if (fcache)
      sampler->load_feature_gpu_cache(*cs, sg, X0, *fcache);
    else
      sampler->load_feature_gpu(*cs, sg, X0, F);
  }
  int l0 = 0;
  NtsVar X;
  if (pre_y) {  // bottom graph op already ran on the sampling stream (issue())
    NtsVar Y = pre_y->narrow(0, 0, (int64_t)sg->sampled_sgs[L - 1]->v_size);
    flush_update();
    X = ctx.runVertexForward([&](NtsVar& a) { return vertexForward(0, a); }, Y);
    keep_pair(Y, X);
    l0 = 1;
  } else {
    X = X0;
  }
  for (int l = l0; l < L; ++l) {
    const int hop = L - 1 - l;
    NtsVar Y;
    const bool bottom = (l == 0);
    if (bottom && tf_) {  // transform-first: H = X[src] W, X1 = act(A H) (one NN op)
      flush_update();
      sampCSC* s = sg->sampled_sgs[hop];
      const double p = drop_rate();
      NtsVar h;
      if (keep) h = torch::empty({(int64_t)std::max<uint32_t>(s->src_size, 1), P[0]->W.size(1)},
                                 f32_opts(graph->device));
      const uint64_t off = dropout_calls_++;
      X = ctx.runVertexForward(
          [&](NtsVar& t) {
            return hip_bottom_transform(t, P[0]->W, s, p, dropout_key(), off, cs.get(), profiler(),
                                        keep ? h.data_ptr<float>() : nullptr, pairs_.get());
          },
          F);
      // training: the graph op above applies this layer's relu/dropout
      // backward to its own backward output (one CSR pass instead of the CSR
      // gather + nts_hip_act_backward; same arithmetic)
      // (only over a CSR: with the atomic CSC backward the layer above has
      // none, and this layer then runs nts_hip_act_backward itself)
      const bool fuse = ctx.is_train() && hop >= 1 && sg->sampled_sgs[hop - 1]->has_csr;
      if (hop >= 1) {  // set, or cleared where an earlier batch in this slot left one
        FusedActBwd ab;
        if (fuse) {
          const bool bits = s->act_bits.defined() && nts_hip_act_bits_words((uint32_t)X.size(1));
          ab = {X.data_ptr<float>(), (uint64_t)X.stride(0),
                (float)keep_scale(p),
                bits ? reinterpret_cast<const uint32_t*>(s->act_bits.data_ptr<int32_t>()) : nullptr};
        }
        sg->sampled_sgs[hop - 1]->act_bwd = ab;
      }
      s->grad_premasked = fuse;
      if (keep) {
        acts.push_back(h.narrow(0, 0, (int64_t)s->src_size));
        acts.push_back(X.detach());
      }
      continue;
    }
    if (bottom && cfg.profile) prof.begin(KernelProfiler::BOTTOM_AGG, (hipStream_t)cs->stream());
    // the bottom op gathers its rows from the table; sample_gpu: the
    // reference's SingleGPUSampleGraphOp, whose backward insists on the CSR
    const bool gather = bottom && cfg.fused_gather;
    Y = ctx.runGraphOp<op::SingleGPUAllSampleGraphOp>(gather ? F : X, sg, graph.get(), hop,
                                                      cs.get(), gather,
                                                      gather ? fcache.get() : nullptr, agg_kind(),
                                                      cfg.sample_gpu);
    if (bottom && cfg.profile)
      prof.end(KernelProfiler::BOTTOM_AGG, (hipStream_t)cs->stream(),
               bottom_bytes(sg, cfg.fused_gather));
    // the previous step's all-reduce ran beside this bottom aggregation,
    // which does not read W; its optimizer step goes in here
    if (bottom) flush_update();
    if (bottom && pd_active_) {
      // GCN_SAMPLE_PD_CACHE::Forward (toolkits/GCN_SAMPLE_PD_CACHE.hpp:916-945):
      // Y W, the cached dsts' rows replaced by the super-batch's (A X) W
      // (load_share_embedding), then relu + dropout.  The omitted dsts have no
      // sampled edges, so their rows of Y are zero and add nothing to dW.
      sampCSC* s = sg->sampled_sgs[hop];
      const uint64_t off = dropout_calls_++;
      const double p = drop_rate();
      X = ctx.runVertexForward(
          [&](NtsVar& a) {
            NtsVar Z = P[0]->forward(a);
            NTS_CALL(nts_hip_pd_load_share, cs->ctx(), dptr<uint32_t>(s->omit_row), nullptr,
                     s->v_size, pd_share_.data_ptr<float>(), (uint64_t)pd_share_.stride(0),
                     (uint32_t)Z.size(1), Z.data_ptr<float>(), (uint64_t)Z.stride(0));
            if (l == L - 1) return Z.log_softmax(1);
            return hip_relu_dropout(Z, p, dropout_key(), off, cs.get());
          },
          Y);
      keep_pair(Y, X);
      continue;
    }
    if (loss_target && l == L - 1)  // vertexForward + Loss of the last layer, fused
      X = ctx.runVertexForward(
          [&](NtsVar& a) {
            if (cfg.multi_label)
              return hip_linear_bce(a, P[l]->W, *loss_target, sg->sampled_sgs[0]->dev_dst(),
                                    cs.get(), count_to_);
            return hip_linear_xent(a, P[l]->W, *loss_target, cs.get(), count_to_);
          },
          Y);
    else
      X = ctx.runVertexForward([&](NtsVar& a) { return vertexForward(l, a); }, Y);
    keep_pair(Y, X);
  }
  acts.push_back(X);
  return acts;
}

std::vector<NtsVar> GCN_SAMPLE_ALLGPU_impl::forward_gat(SampledSubgraph* sg) {
  flush_update();
  const int L = (int)sg->layers;
  NtsVar X;
  if (fcache)
    sampler->load_feature_gpu_cache(*cs, sg, X, *fcache);
  else
    sampler->load_feature_gpu(*cs, sg, X, F);
  // gat_attn_drop / gat_feat_drop (training mode only): every mask
  // takes the next dropout_calls_ in order of use — the input pass, then per
  // layer the attention draw and (hidden layers) the output draw.  With both
  // rates 0 no offset is drawn and the layers run the plain entry points.
  const double q = ctx.is_train() ? cfg.gat_attn_drop : 0.0;
  const double p = ctx.is_train() ? cfg.gat_feat_drop : 0.0;
  if (p > 0.0) X = hip_dropout(X, p, dropout_key(), dropout_calls_++, cs.get());
  std::vector<NtsVar> acts;
  for (int l = 0; l < L; ++l) {
    const int hop = L - 1 - l;  // X_{l+1} = relu(attention aggregate of X_l W_l)
    GatDropout drop;
    drop.seed = dropout_key();
    if (q > 0.0) {
      drop.p_attn = q;
      drop.off_attn = dropout_calls_++;
    }
    if (p > 0.0 && l < L - 1) {
      drop.p_out = p;
      drop.off_out = dropout_calls_++;
    }
    const auto layer = cfg.gat_v2 ? hip_gatv2_layer : hip_gat_layer;
    X = layer(X, P[2 * l]->W, P[2 * l + 1]->W, sg->sampled_sgs[hop], cs.get(), profiler(),
              gat_heads(l), l == L - 1 && gat_heads(l) > 1, drop);
    acts.push_back(X);
  }
  return acts;
}

void GCN_SAMPLE_ALLGPU_impl::Loss(NtsVar& left, NtsVar& right) {
  if (cfg.multi_label) {  // left: raw logits, right: float 0/1 targets
    loss = torch::binary_cross_entropy_with_logits(left, right);
    if (ctx.training) ctx.appendNNOp(left, loss);
    return;
  }
  NtsVar a = left.log_softmax(1);
  loss = torch::nll_loss(a, right);
  if (ctx.training) ctx.appendNNOp(left, loss);
}

void GCN_SAMPLE_ALLGPU_impl::Update() {
  // GCN_SAMPLE_ALL_MULTI::Update (toolkits/GCN_SAMPLE_ALL_MULTI.hpp:367-377):
  // SUM all-reduce of every W.grad — one fused RCCL call over a flat bucket.
  if (defer_) {
    // pack on the training stream, reduce on the comm stream; the Adam step
    // runs in flush_update() once the next batch first needs W
    TORCH_CHECK(!pending_update_, "deferred update still pending");
    torch::NoGradGuard ng;
    int64_t off = 0;
    for (auto* p : params()) {
      const int64_t n = p->W.numel();
      grad_bucket.narrow(0, off, n).copy_(p->W.grad().reshape({-1}));
      off += n;
    }
    TORCH_CHECK(hipEventRecord(grads_packed_, (hipStream_t)cs->stream()) == hipSuccess &&
                    hipStreamWaitEvent(comm_stream_, grads_packed_, 0) == hipSuccess,
                "hipEventRecord/hipStreamWaitEvent");
    comm->allreduce_sum(grad_bucket.data_ptr<float>(), (uint64_t)grad_bucket.numel(), comm_stream_);
    TORCH_CHECK(hipEventRecord(grads_reduced_, comm_stream_) == hipSuccess, "hipEventRecord");
    pending_update_ = true;
    return;
  }
  if (comm) {  // also at one rank: the same bucket, all-reduce and unpack run
    torch::NoGradGuard ng;
    int64_t off = 0;
    for (auto* p : params()) {
      const int64_t n = p->W.numel();
      grad_bucket.narrow(0, off, n).copy_(p->W.grad().reshape({-1}));
      off += n;
    }
    comm->allreduce_sum(grad_bucket.data_ptr<float>(), (uint64_t)grad_bucket.numel(), cs->stream());
    off = 0;
    for (auto* p : params()) {
      const int64_t n = p->W.numel();
      p->W.mutable_grad().copy_(grad_bucket.narrow(0, off, n).view(p->W.sizes()));
      off += n;
    }
  }
  for (auto* p : params()) {
    if (cfg.bias_correction) p->learnC2C_with_decay_Adam(*cs);
    else p->learn_local_with_decay_Adam(*cs);
    p->next();
  }
}

void GCN_SAMPLE_ALLGPU_impl::flush_update() {
  if (!pending_update_) return;
  pending_update_ = false;
  auto guard = cs->guard();
  TORCH_CHECK(hipStreamWaitEvent((hipStream_t)cs->stream(), grads_reduced_, 0) == hipSuccess,
              "hipStreamWaitEvent");
  int64_t off = 0;
  for (auto* p : params()) {
    p->adam_from(*cs, grad_bucket.data_ptr<float>() + off, cfg.bias_correction != 0);
    p->next();
    off += p->W.numel();
  }
}

float GCN_SAMPLE_ALLGPU_impl::train_batch() {
  auto guard = cs->guard();
  double t0 = now_s();
  if (cfg.profile) prof.next_step();  // (one kernel class timed per step)
  NtsStream& sst = ss ? *ss : *cs;
  // set_diag_reuse_sample (diagnostic only, not a valid measurement): sample
  // once and train every step on that batch — the training stream's time
  // without the sampler beside it
  const bool diag_reuse = diag_reuse_;
  int slot;
  SampledSubgraph* sg;
  if (diag_reuse && reuse_slot_ >= 0) {
    slot = reuse_slot_;
    sg = sampler->ssgs[slot];
  } else {
    if (prefetched_ >= 0) {
      slot = prefetched_;
      prefetched_ = -1;
    } else {
      slot = next_slot_;
      issue(slot, sst);
    }
    sg = sampler->finish_gpu_sample(slot);
    if (diag_reuse) {
      reuse_slot_ = slot;
    } else if (ss) {
      next_slot_ = (slot + 1) % nslots_;
      if (cfg.sampler_gate > 0 && tf_) {
        // issued from the bottom layer's forward GEMM hook (below), behind it
        deferred_issue_ = [this] { prefetch_next(); };
      } else {
        prefetch_next();
      }
    }
  }
  if (deferred_issue_) {
    if (!gate_ev_)
      TORCH_CHECK(hipEventCreateWithFlags(&gate_ev_, hipEventDisableTiming) == hipSuccess,
                  "hipEventCreate");
    set_bottom_gemm_hooks(
        [this] {
          if (!deferred_issue_) return;
          TORCH_CHECK(hipEventRecord(gate_ev_, (hipStream_t)cs->stream()) == hipSuccess &&
                          hipStreamWaitEvent((hipStream_t)ss->stream(), gate_ev_, 0) == hipSuccess,
                      "hipEventRecord/hipStreamWaitEvent");
          auto f = std::move(deferred_issue_);
          deferred_issue_ = nullptr;
          f();
        },
        cfg.sampler_gate >= 2
            ? std::function<void()>([this] {
                if (gated_slot_ >= 0)
                  TORCH_CHECK(hipStreamWaitEvent((hipStream_t)cs->stream(), ready_[gated_slot_], 0) ==
                                  hipSuccess,
                              "hipStreamWaitEvent");
              })
            : std::function<void()>());
  }
  fresh_pass_ = false;
  last_sg = sg;
  TORCH_CHECK(hipStreamWaitEvent((hipStream_t)cs->stream(), ready_[slot], 0) == hipSuccess,
              "hipStreamWaitEvent");
  double t1 = now_s();
  if (cfg.pd_cache) pd_train(slot);
  mark("T<", *cs);
  if (!cfg.multi_label) target = lbl_[slot].narrow(0, 0, (int64_t)sg->sampled_sgs[0]->v_size);
  ctx.train();
  if (early_ && cfg.profile) prof.add_units(KernelProfiler::BOTTOM_AGG, bottom_bytes(sg, true));
  const int L = (int)P.size();
  if (cfg.gat) {  // GAT_SAMPLE_ALL_GPU::Loss + loss.backward() (toolkits/GAT_SAMPLE_ALL_GPU.hpp:393-399)
    auto acts = forward_gat(sg);
    loss = torch::nll_loss(acts.back().log_softmax(1), target);
    count_correct(acts.back(), target);
    loss.backward();
    ctx.reset();
  } else if (cfg.multi_label) {
    const bool fuse_loss = fuse_bce();
    count_to_ = dptr<uint32_t>(f1_);
    auto acts = forward(sg, false, early_ ? &pre_y_[slot] : nullptr,
                        fuse_loss ? &label_bits_ : nullptr);
    count_to_ = nullptr;
    if (fuse_loss) {
      loss = acts.back();
    } else {  // the libtorch chain: matmul, binary_cross_entropy_with_logits
      NtsVar out = acts.back();
      target = batch_targets(sg);
      count_f1(f1_, out, target);
      Loss(out, target);
    }
    ctx.self_backward(false);
  } else {
    const bool fuse_loss = cfg.fuse_loss && cfg.hip_gemm && L >= 2 &&
                           hip_linear_xent_supported(P[L - 1]->W.size(0), P[L - 1]->W.size(1));
    count_to_ = dptr<uint32_t>(correct_);
    auto acts = forward(sg, false, early_ ? &pre_y_[slot] : nullptr, fuse_loss ? &target : nullptr);
    count_to_ = nullptr;
    if (fuse_loss) {
      loss = acts.back();
    } else {
      NtsVar out = acts.back();
      count_correct(out, target);
      Loss(out, target);
    }
    ctx.self_backward(false);
  }
  pd_active_ = false;
  if (deferred_issue_) {  // (the hook did not run: issue behind the step's kernels so far)
    auto f = std::move(deferred_issue_);
    deferred_issue_ = nullptr;
    f();
  }
  set_bottom_gemm_hooks(nullptr, nullptr);
  gated_slot_ = -1;
  Update();
  for (auto* p : params()) p->zero_grad();
  TORCH_CHECK(hipEventRecord(sg->consumed, (hipStream_t)cs->stream()) == hipSuccess,
              "hipEventRecord");
  mark("T>", *cs);
  double t2 = now_s();
  sample_time += t1 - t0;
  train_time += t2 - t1;
  for (int l = 0; l < sg->layers; ++l) batch_edges += sg->sampled_sgs[l]->e_size;
  ++batches;
  return 0.f;  // the loss stays on the device (no per-step host sync)
}

// the pipelined sampler's next batch (issued behind the batch being trained)
void GCN_SAMPLE_ALLGPU_impl::prefetch_next() {
  if (!pass_done_ && sampler->sample_not_finished()) {
    issue(next_slot_, *ss);  // prefetch the next batch behind this one
    prefetched_ = next_slot_;
    gated_slot_ = next_slot_;
  } else if (!pass_done_) {
    // last batch of the pass: sample the first batch of the next pass now
    // (same seeds, same stream position as after restart()), so the
    // pipeline does not drain at every pass boundary
    sampler->restart();
    issue(next_slot_, *ss);
    carry_ = next_slot_;
    gated_slot_ = next_slot_;
    pass_done_ = true;
  }
}

void GCN_SAMPLE_ALLGPU_impl::restart() {
  if (fresh_pass_) return;  // nothing trained since the last restart
  fresh_pass_ = true;
  if (carry_ >= 0) {  // the next pass's first batch is already in flight
    TORCH_CHECK(prefetched_ < 0, "pipeline state");
    prefetched_ = carry_;
    carry_ = -1;
    pass_done_ = false;
    return;
  }
  pass_done_ = false;
  if (prefetched_ >= 0) {  // drop a prefetched batch of the previous pass
    sampler->finish_gpu_sample(prefetched_);
    prefetched_ = -1;
  }
  sampler->restart();
}

float GCN_SAMPLE_ALLGPU_impl::run_epoch() {
  restart();
  float l = 0;
  while (has_batch()) l = train_batch();
  return l;
}

// An evaluation's sampler over `ids`: sampled like training (weights, merged
// layers, RNG mode), one slot, CSRs only where the forward reads them (GAT).
std::unique_ptr<FastSampler> GCN_SAMPLE_ALLGPU_impl::eval_sampler(const std::vector<VertexId>& ids,
                                                                  int batch, uint64_t batch_seq) {
  const int L = (int)cfg.fanout.size();
  auto s = std::make_unique<FastSampler>(graph, ids, L, batch, cfg.fanout, 1,
                                         std::vector<bool>(L, cfg.gat),
                                         sample_weight() != WeightType::None || cfg.edge_weighted,
                                         cfg.gat || cfg.root_weight, false,
                                         cfg.subgraph ? cfg.subgraph_walk : -1,
                                         (uint64_t)cfg.subgraph_edge_cap);
  s->rng_mode = cfg.rng_mode;
  s->weighted = cfg.weighted_sampling;
  s->coef = cfg.edge_weighted;
  s->up_degree = cfg.up_degree;
  s->batch_seq = batch_seq;
  return s;
}

std::vector<NtsVar> GCN_SAMPLE_ALLGPU_impl::forward_eval(const std::vector<VertexId>& seeds,
                                                         uint64_t batch_seq) {
  flush_update();
  auto guard = cs->guard();
  auto s = eval_sampler(seeds, (int)seeds.size(), batch_seq);
  SampledSubgraph* sg = s->sample_gpu_fast((int)seeds.size(), 0, *cs, sample_weight());
  ctx.eval();
  torch::NoGradGuard ng;
  std::vector<NtsVar> acts;
  if (cfg.gat) {
    acts = forward_gat(sg);
  } else {
    acts = forward(sg, true);
    acts.pop_back();
  }
  ctx.train();
  cs->synchronize();
  return acts;
}

void GCN_SAMPLE_ALLGPU_impl::count_correct(const NtsVar& out, const NtsVar& tgt) {
  torch::NoGradGuard ng;
  correct_.add_(out.argmax(1).eq(tgt).sum().to(torch::kInt32));
}

uint64_t GCN_SAMPLE_ALLGPU_impl::train_correct() {
  cs->synchronize();
  return (uint64_t)(uint32_t)correct_.cpu().item<int32_t>();
}

void GCN_SAMPLE_ALLGPU_impl::reset_correct() {
  auto guard = cs->guard();
  correct_.zero_();
  if (f1_.defined()) f1_.zero_();
}

// ---- multi_label ----
bool GCN_SAMPLE_ALLGPU_impl::fuse_bce() const {
  const size_t L = P.size();
  return cfg.fuse_loss && cfg.hip_gemm && L >= 2 &&
         hip_linear_bce_supported(P[L - 1]->W.size(0), P[L - 1]->W.size(1));
}

NtsVar GCN_SAMPLE_ALLGPU_impl::batch_targets(SampledSubgraph* sg) const {
  sampCSC* s0 = sg->sampled_sgs[0];
  NtsVar ids = s0->destination.narrow(0, 0, (int64_t)s0->v_size).to(torch::kInt64);
  return unpack_label_bits(label_bits_.index_select(0, ids), cfg.layer_size.back());
}

void GCN_SAMPLE_ALLGPU_impl::count_f1(NtsVar& counts, const NtsVar& logits, const NtsVar& targets) {
  torch::NoGradGuard ng;
  NtsVar pos = logits.gt(0), t = targets.gt(0.5);
  counts.add_(torch::stack({pos.logical_and(t).sum(), pos.logical_and(t.logical_not()).sum(),
                            pos.logical_not().logical_and(t).sum()})
                  .to(torch::kInt32));
}

double GCN_SAMPLE_ALLGPU_impl::micro_f1(const NtsVar& counts) {
  NtsVar c = counts.cpu();
  const auto* p = reinterpret_cast<const uint32_t*>(c.data_ptr<int32_t>());
  const double tp = p[0], den = 2.0 * p[0] + (double)p[1] + (double)p[2];
  return den > 0.0 ? 2.0 * tp / den : 0.0;
}

std::vector<uint64_t> GCN_SAMPLE_ALLGPU_impl::f1_counts() {
  TORCH_CHECK(cfg.multi_label, "f1_counts: a multi_label driver's counters");
  cs->synchronize();
  NtsVar c = f1_.cpu();
  const auto* p = reinterpret_cast<const uint32_t*>(c.data_ptr<int32_t>());
  return {p[0], p[1], p[2]};
}

double GCN_SAMPLE_ALLGPU_impl::evaluate(const std::vector<VertexId>& nids) {
  flush_update();
  if (nids.empty()) return 0.0;
  auto guard = cs->guard();
  const int L = (int)cfg.fanout.size();
  const WeightType wt = sample_weight();
  auto sp = eval_sampler(nids, cfg.batch_size, eval_seq);
  FastSampler& s = *sp;
  NtsVar correct = torch::zeros({cfg.multi_label ? 3 : 1}, u32_opts(graph->device));
  const bool fuse_loss = cfg.multi_label
                             ? fuse_bce()
                             : !cfg.gat && cfg.fuse_loss && cfg.hip_gemm && L >= 2 &&
                                   hip_linear_xent_supported(P[L - 1]->W.size(0), P[L - 1]->W.size(1));
  ctx.eval();
  {
    torch::NoGradGuard ng;
    NtsVar tgt;
    while (s.sample_not_finished()) {
      SampledSubgraph* sg = s.sample_gpu_fast(cfg.batch_size, 0, *cs, wt);
      if (cfg.multi_label) {
        if (fuse_loss) {  // the loss kernel counts tp, fp, fn as it goes
          count_to_ = dptr<uint32_t>(correct);
          forward(sg, false, nullptr, &label_bits_);
          count_to_ = nullptr;
        } else {
          auto acts = forward(sg, false);
          count_f1(correct, acts.back(), batch_targets(sg));
        }
        TORCH_CHECK(hipEventRecord(sg->consumed, (hipStream_t)cs->stream()) == hipSuccess,
                    "hipEventRecord");
        continue;
      }
      s.load_label_gpu(*cs, sg, tgt, L_GT);
      if (cfg.gat) {
        auto acts = forward_gat(sg);
        correct.add_(acts.back().argmax(1).eq(tgt).sum().to(torch::kInt32));
      } else if (fuse_loss) {
        count_to_ = dptr<uint32_t>(correct);
        forward(sg, false, nullptr, &tgt);
        count_to_ = nullptr;
      } else {
        auto acts = forward(sg, false);
        correct.add_(acts.back().argmax(1).eq(tgt).sum().to(torch::kInt32));
      }
      // the sampler slot is reused by the next batch: order it behind this forward
      TORCH_CHECK(hipEventRecord(sg->consumed, (hipStream_t)cs->stream()) == hipSuccess,
                  "hipEventRecord");
    }
  }
  ctx.train();
  eval_seq = s.batch_seq;
  cs->synchronize();
  if (cfg.multi_label) return micro_f1(correct);
  return (double)(uint32_t)correct.cpu().item<int32_t>() / (double)nids.size();
}

// Full-neighbour layer-wise inference: each layer is one O(E) aggregation over
// the global CSC plus one GEMM over all V rows, on the narrower side of the
// layer.  Peak activation footprint V (F_l + F_{l+1}) 4 bytes.
NtsVar GCN_SAMPLE_ALLGPU_impl::infer_full() {
  TORCH_CHECK(!cfg.gat, "infer_full: GAT layers are not supported (GCN / GraphSAGE only); a GAT "
                        "driver has infer_full_gat() / evaluate_full_gat()");
  TORCH_CHECK(!cfg.up_degree,
              "infer_full: UP_DEGREE weights are a property of a sample, not of the whole graph");
  TORCH_CHECK(max_aggr() || cfg.weight_type != WeightType::MeanSampled,
              "infer_full: MeanSampled weights are a property of a sample, not of the whole graph");
  TORCH_CHECK(!fcache, "infer_full: needs the whole feature table in HBM (cache_rate < 0)");
  flush_update();
  auto guard = cs->guard();
  const int L = (int)P.size();
  const int64_t V = (int64_t)graph->global_vertices;
  const int wt = cfg.weight_type == WeightType::Sum    ? NTS_WEIGHT_SUM
                 : cfg.weight_type == WeightType::Mean ? NTS_WEIGHT_MEAN
                                                       : NTS_WEIGHT_NONE;
  const nts_graph_dev g = graph->dev();
  hipStream_t st = (hipStream_t)cs->stream();
  std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
  // root_weight: the aggregation fills the left half of a [V, 2 F] buffer and
  // the rows themselves are copied into the right half
  auto aggregate = [&](const NtsVar& x, bool relu) {
    NtsVar xr = row_major(x);
    NtsVar y = row_padded_empty(V, (cfg.root_weight ? 2 : 1) * xr.size(1), graph->device);
    if (cfg.root_weight) y.narrow(1, xr.size(1), xr.size(1)).copy_(xr);
    if (cfg.profile) {
      hipEvent_t a, b;
      TORCH_CHECK(hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess,
                  "hipEventCreate");
      evs.push_back({a, b});
      (void)hipEventRecord(a, st);
    }
    const float* coef = cfg.edge_weighted ? dptr<float>(graph->edge_prob) : nullptr;
    if (coef && xr.dtype() == torch::kFloat16)  // edge_weighted: the _coef siblings
      NTS_CALL(nts_hip_spmm_graph_fwd_coef_h, cs->ctx(), &g, coef, 0, (uint64_t)V, wt, relu ? 1 : 0,
               dptr<const uint16_t>(xr), (uint64_t)xr.stride(0), (uint32_t)xr.size(1),
               y.data_ptr<float>(), (uint64_t)y.stride(0));
    else if (coef)
      NTS_CALL(nts_hip_spmm_graph_fwd_coef, cs->ctx(), &g, coef, 0, (uint64_t)V, wt, relu ? 1 : 0,
               xr.data_ptr<float>(), (uint64_t)xr.stride(0), (uint32_t)xr.size(1),
               y.data_ptr<float>(), (uint64_t)y.stride(0));
    else if (xr.dtype() == torch::kFloat16)  // feature_f16: layer 0 reads the half table
      NTS_CALL(nts_hip_spmm_graph_fwd_h, cs->ctx(), &g, 0, (uint64_t)V, wt, relu ? 1 : 0,
               dptr<const uint16_t>(xr), (uint64_t)xr.stride(0), (uint32_t)xr.size(1),
               y.data_ptr<float>(), (uint64_t)y.stride(0));
    else if (max_aggr())
      NTS_CALL(nts_hip_spmm_graph_fwd_max, cs->ctx(), &g, 0, (uint64_t)V, relu ? 1 : 0,
               xr.data_ptr<float>(), (uint64_t)xr.stride(0), (uint32_t)xr.size(1),
               y.data_ptr<float>(), (uint64_t)y.stride(0));
    else
      NTS_CALL(nts_hip_spmm_graph_fwd, cs->ctx(), &g, 0, (uint64_t)V, wt, relu ? 1 : 0,
               xr.data_ptr<float>(), (uint64_t)xr.stride(0), (uint32_t)xr.size(1),
               y.data_ptr<float>(), (uint64_t)y.stride(0));
    if (cfg.profile) (void)hipEventRecord(evs.back().second, st);
    return y;
  };
  ctx.eval();
  NtsVar X = F;
  {
    torch::NoGradGuard ng;
    for (int l = 0; l < L; ++l) {
      const bool last = l == L - 1;
      const NtsVar& W = P[l]->W;
      // layer_norm: the hidden layer's activation is the fused LayerNorm pass
      // over A X W, whichever way the (linear) product was formed
      // batch_norm: the eval pass on the running statistics, in the same places
      const bool ln = (cfg.layer_norm || cfg.batch_norm) && !last;
      auto norm_act = [&](const NtsVar& Z) {
        return cfg.batch_norm ? batch_norm_act(l, Z, 0.0, 0) : layer_norm_act(l, Z, 0.0, 0);
      };
      // (feature_f16: layer 0 aggregates first, from the half table: no fp32 copy of it)
      const bool half_in = X.dtype() == torch::kFloat16;
      if (!cfg.root_weight && !max_aggr() && !half_in && W.size(0) > W.size(1)) {  // transform first: act(A (X W)), the relu in the kernel
        NtsVar H = P[l]->forward(X);
        NtsVar Y = aggregate(H, !last && !ln);
        X = ln ? norm_act(Y) : last && !cfg.multi_label ? Y.log_softmax(1) : Y;
      } else {  // aggregate first: act((A X) W)
        NtsVar Y = aggregate(X, false);
        if (last)
          X = cfg.multi_label ? P[l]->forward(Y) : P[l]->forward(Y).log_softmax(1);
        else if (ln)
          X = norm_act(P[l]->forward(Y));
        else if (cfg.hip_gemm && cfg.fuse_activation)  // p = 0: no mask, no offset drawn
          X = hip_linear_act(Y, W, 0.0, 0, 0, cs.get(), false);
        else
          X = torch::relu(P[l]->forward(Y));
      }
    }
  }
  ctx.train();
  cs->synchronize();
  full_agg_ms.clear();
  for (auto& e : evs) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e.first, e.second);
    full_agg_ms.push_back((double)ms);
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  return X;
}

double GCN_SAMPLE_ALLGPU_impl::evaluate_full(const std::vector<VertexId>& nids) {
  NtsVar out = infer_full();
  if (nids.empty()) return 0.0;
  for (VertexId v : nids)
    TORCH_CHECK((uint64_t)v < graph->global_vertices, "evaluate_full: vertex id ", v,
                " >= vertex count ", graph->global_vertices);
  auto guard = cs->guard();
  torch::NoGradGuard ng;
  NtsVar idx = torch::from_blob((void*)nids.data(), {(int64_t)nids.size()}, torch::kInt32)
                   .to(torch::Device(torch::kCUDA, graph->device))
                   .to(torch::kInt64);
  if (cfg.multi_label) {
    NtsVar counts = torch::zeros({3}, u32_opts(graph->device));
    count_f1(counts, out.index_select(0, idx),
             unpack_label_bits(label_bits_.index_select(0, idx), cfg.layer_size.back()));
    return micro_f1(counts);
  }
  // labels gathered and rows counted on the device; one scalar comes back
  NtsVar n_ok = out.index_select(0, idx).argmax(1).eq(L_GT.index_select(0, idx)).sum();
  const int64_t correct = n_ok.cpu().item<int64_t>();
  return (double)correct / (double)nids.size();
}

// Full-neighbour inference of a GAT driver: per layer one GEMM
// H = X W over all V rows, the per-vertex scores S = H [a1 | a2] once, and one
// fused attention pass over the global CSC (nts_hip_gat_graph_fwd: online
// softmax per row, nothing E-sized written).  Footprint V (F_l + F_{l+1} + 2 K)
// floats, plus V F_{l+1} in the last layer's mean mode.
NtsVar GCN_SAMPLE_ALLGPU_impl::infer_full_gat() {
  TORCH_CHECK(cfg.gat, "infer_full_gat: attention layers only; a GCN / GraphSAGE driver has "
                       "infer_full() / evaluate_full()");
  TORCH_CHECK(!cfg.gat_v2, "infer_full_gat: full-neighbour inference for GATv2 (gat_v2) is not "
                           "built; use evaluate() on sampled neighbourhoods");
  TORCH_CHECK(!fcache, "infer_full_gat: needs the whole feature table in HBM (cache_rate < 0)");
  flush_update();
  auto guard = cs->guard();
  const int L = (int)P.size() / 2;
  const int64_t V = (int64_t)graph->global_vertices;
  const nts_graph_dev g = graph->dev();
  hipStream_t st = (hipStream_t)cs->stream();
  std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
  ctx.eval();
  NtsVar X = F;
  {
    torch::NoGradGuard ng;
    for (int l = 0; l < L; ++l) {
      const int64_t K = gat_heads(l);
      const bool mean = l == L - 1 && K > 1;
      NtsVar H = row_major(P[2 * l]->forward(X));
      NtsVar A = P[2 * l + 1]->W.contiguous();
      const int64_t Fl = H.size(1), D = Fl / K;
      TORCH_CHECK(D * K == Fl && A.numel() == 2 * Fl, "infer_full_gat: layer ", l, " shapes");
      NtsVar S = torch::empty({V, 2 * K}, f32_opts(graph->device));
      NtsVar Y = row_padded_empty(V, mean ? D : Fl, graph->device);
      if (cfg.profile) {
        hipEvent_t a, b;
        TORCH_CHECK(hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess,
                    "hipEventCreate");
        evs.push_back({a, b});
        (void)hipEventRecord(a, st);
      }
      NTS_CALL(nts_hip_gat_scores, cs->ctx(), H.data_ptr<float>(), (uint64_t)H.stride(0),
               (uint64_t)V, (uint32_t)K, (uint32_t)D, A.data_ptr<float>(), S.data_ptr<float>());
      NTS_CALL(nts_hip_gat_graph_fwd, cs->ctx(), &g, 0, (uint64_t)V, H.data_ptr<float>(),
               (uint64_t)H.stride(0), (uint32_t)K, (uint32_t)D, S.data_ptr<float>(),
               Y.data_ptr<float>(), (uint64_t)Y.stride(0), mean ? 1 : 0);
      if (cfg.profile) (void)hipEventRecord(evs.back().second, st);
      X = Y;
    }
    X = X.log_softmax(1);  // what Loss() applies to the last layer's relu'd output
  }
  ctx.train();
  cs->synchronize();
  full_agg_ms.clear();
  for (auto& e : evs) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e.first, e.second);
    full_agg_ms.push_back((double)ms);
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  return X;
}

double GCN_SAMPLE_ALLGPU_impl::evaluate_full_gat(const std::vector<VertexId>& nids) {
  NtsVar out = infer_full_gat();
  if (nids.empty()) return 0.0;
  for (VertexId v : nids)
    TORCH_CHECK((uint64_t)v < graph->global_vertices, "evaluate_full_gat: vertex id ", v,
                " >= vertex count ", graph->global_vertices);
  auto guard = cs->guard();
  torch::NoGradGuard ng;
  NtsVar idx = torch::from_blob((void*)nids.data(), {(int64_t)nids.size()}, torch::kInt32)
                   .to(torch::Device(torch::kCUDA, graph->device))
                   .to(torch::kInt64);
  // labels gathered and rows counted on the device; one scalar comes back
  NtsVar n_ok = out.index_select(0, idx).argmax(1).eq(L_GT.index_select(0, idx)).sum();
  const int64_t correct = n_ok.cpu().item<int64_t>();
  return (double)correct / (double)nids.size();
}

// ---------------------------------------------------------------------------
// PD cache
std::pair<std::vector<uint32_t>, std::vector<uint32_t>> GCN_SAMPLE_ALLGPU_impl::presample() {
  auto guard = cs->guard();
  const std::vector<VertexId>& ids = sampler->sample_nids;  // shuffled like training
  const uint64_t sbs = (uint64_t)cfg.batch_size * (uint64_t)cfg.pd_super_batch;
  const uint64_t n_sb = (ids.size() + sbs - 1) / sbs;
  const uint64_t V = graph->global_vertices;
  NtsVar seeds = torch::empty({(int64_t)std::max<size_t>(ids.size(), 1)}, u32_opts(graph->device));
  if (!ids.empty())
    seeds.narrow(0, 0, (int64_t)ids.size())
        .copy_(torch::from_blob((void*)ids.data(), {(int64_t)ids.size()}, torch::kInt32));
  NtsVar counts = torch::empty({(int64_t)V}, u32_opts(graph->device));
  NtsVar tmp = torch::empty({(int64_t)V}, u32_opts(graph->device));
  NtsVar out = torch::empty({(int64_t)V}, u32_opts(graph->device));
  NtsVar n_dev = torch::empty({1}, u32_opts(graph->device));
  const nts_graph_dev g = graph->dev();
  std::vector<uint32_t> cnt(n_sb), all;
  // get_most_neighbor over `layers` = the number of GNN layers (the driver's
  // gnnctx->layer_size.size() - 1, toolkits/GCN_SAMPLE_PD_CACHE.hpp:989)
  const int layers = (int)cfg.fanout.size();
  for (uint64_t b = 0; b < n_sb; ++b) {
    const uint64_t beg = b * sbs, n = std::min<uint64_t>(sbs, ids.size() - beg);
    NTS_CALL(nts_hip_presample_counts, cs->ctx(), &g, dptr<uint32_t>(seeds) + beg, (uint32_t)n,
             layers, dptr<uint32_t>(counts), dptr<uint32_t>(tmp));
    NTS_CALL(nts_hip_presample_select, cs->ctx(), dptr<uint32_t>(counts), V, (float)cfg.pd_rate,
             dptr<uint32_t>(out), dptr<uint32_t>(n_dev));
    cs->synchronize();
    cnt[b] = (uint32_t)n_dev.cpu().item<int32_t>();
    auto h = out.narrow(0, 0, (int64_t)cnt[b]).cpu();
    const uint32_t* hp = reinterpret_cast<const uint32_t*>(h.data_ptr<int32_t>());
    all.insert(all.end(), hp, hp + cnt[b]);
  }
  return {cnt, all};
}

void GCN_SAMPLE_ALLGPU_impl::set_presample(const std::vector<uint32_t>& counts,
                                           const std::vector<uint32_t>& ids) {
  TORCH_CHECK(cfg.pd_cache, "set_presample needs the PD cache (cfg.pd_cache)");
  auto guard = cs->guard();
  TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "hipDeviceSynchronize");
  pd_counts_ = counts;
  pd_offset_.assign(counts.size() + 1, 0);
  for (size_t i = 0; i < counts.size(); ++i) pd_offset_[i + 1] = pd_offset_[i] + counts[i];
  TORCH_CHECK(pd_offset_.back() == ids.size(), "PD cache: ids must hold sum(counts) vertices");
  // the ids index cache_map / cache_location on the device: a stale or
  // mismatched PRE_SAMPLE_FILE must not write past them
  for (uint32_t id : ids)
    TORCH_CHECK(id < graph->global_vertices, "PD cache: hot vertex id ", id,
                " >= vertex count ", graph->global_vertices, " (stale PRE_SAMPLE_FILE?)");
  uint32_t mx = 1;
  for (uint32_t c : counts) mx = std::max(mx, c);
  std::vector<VertexId> hot(ids.begin(), ids.end());
  if (hot.empty()) hot.push_back(0);  // a sampler needs a non-empty id list
  const int L = (int)cfg.fanout.size();
  // CPU side of the reference (:740-745): a 1-layer sampler over the hot ids
  // with the bottom layer's fanout, consumed super-batch by super-batch
  pd_sampler_ = std::make_unique<FastSampler>(graph, hot, 1, (int)mx,
                                              std::vector<int>{cfg.fanout[L - 1]}, kPdRing,
                                              std::vector<bool>{false},
                                              cfg.weight_type != WeightType::None, false);
  pd_sampler_->rng_mode = cfg.rng_mode;
  pd_sampler_->batch_seq = uint64_t(1) << 48;  // a PHILOX stream of its own
  const int64_t Fin = cfg.layer_size[0];
  for (int i = 0; i < kPdRing; ++i) {
    pd_y_[i] = torch::empty({(int64_t)mx, Fin}, f32_opts(graph->device));
    if (fcache)  // the hot rows' neighbours may be spilled to the host table
      pd_stage_[i] = torch::empty(
          {(int64_t)std::max<uint32_t>(pd_sampler_->ssgs[i]->sampled_sgs[0]->s_cap, 1),
           (int64_t)fcache->ld},
          f32_opts(graph->device));
  }
  pd_share_ = torch::empty({(int64_t)mx, (int64_t)cfg.layer_size[1]}, f32_opts(graph->device));
  pd_ids_ = torch::empty({(int64_t)std::max<size_t>(ids.size(), 1)}, u32_opts(graph->device));
  if (!ids.empty())
    pd_ids_.narrow(0, 0, (int64_t)ids.size())
        .copy_(torch::from_blob((void*)ids.data(), {(int64_t)ids.size()}, torch::kInt32));
  TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "hipDeviceSynchronize");
}

// At sampling time, for a batch that opens a super-batch: its hot vertices get
// the next key in cache_map / cache_location (set_cache_index), their
// 1-layer neighbourhoods are sampled and aggregated (PushDownBatchOp: the
// reference's CPU thread; here the fused gather on the sampling stream).  Every
// batch then samples its bottom layer with the super-batch's key omitted.
void GCN_SAMPLE_ALLGPU_impl::pd_issue(int slot, NtsStream& st) {
  const uint64_t bip = (sampler->work_offset - sampler->work_range[0]) / (uint64_t)cfg.batch_size;
  const int sb = (int)(bip / (uint64_t)cfg.pd_super_batch);
  const bool first = bip % (uint64_t)cfg.pd_super_batch == 0;
  TORCH_CHECK(sb < (int)pd_counts_.size(), "PD cache: more super-batches than preSampled");
  if (first) {
    pd_next_key_++;
    const uint32_t n = pd_counts_[sb];
    auto guard = st.guard();
    NTS_CALL(nts_hip_pd_set_cache, st.ctx(), dptr<uint32_t>(pd_ids_) + pd_offset_[sb], n,
             pd_next_key_, dptr<uint32_t>(pd_cache_map_), dptr<uint32_t>(pd_cache_loc_));
    if (n) {
      const int ring = (int)(pd_next_key_ % kPdRing);
      pd_sampler_->work_offset = (VertexId)pd_offset_[sb];
      pd_sampler_->issue_gpu_sample((int)n, ring, st, cfg.weight_type);
      sampCSC* h = pd_sampler_->ssgs[ring]->sampled_sgs[0];
      NtsVar& y = pd_y_[ring];
      if (fcache)  // two-tier table: cached rows from HBM, the rest staged once from the host
        fcache->aggregate(st.ctx(), h, dptr<uint32_t>(h->sizes), h->v_cap,
                          dptr<uint32_t>(h->sizes) + 2, h->s_cap, pd_stage_[ring].data_ptr<float>(),
                          y.data_ptr<float>(), (uint64_t)y.stride(0));
      else
        hip_check(nts_hip_spmm_csc_fwd(st.ctx(), h->dev_c_o(), h->dev_r_i(), h->dev_e_w_f(),
                                       dptr<uint32_t>(h->sizes), h->v_cap, F.data_ptr<float>(),
                                       (uint64_t)F.stride(0), h->dev_src(), (uint32_t)F.size(1),
                                       y.data_ptr<float>(), (uint64_t)y.stride(0)),
                  "nts_hip_spmm_csc_fwd(pd)");
    }
  }
  pd_slot_key_[slot] = (int)pd_next_key_;
  pd_slot_sb_[slot] = sb;
  pd_slot_first_[slot] = first;
  sampler->omit_map = dptr<uint32_t>(pd_cache_map_);
  sampler->omit_key = pd_next_key_;
  sampler->omit_loc = dptr<uint32_t>(pd_cache_loc_);
}

// Before the forward of a batch: at the super-batch's first batch, the shared
// embedding = (A X) W with the current weights (the reference's CPU GEMM with
// the W of shared_W_queue, :821-840); later batches of the super-batch reuse it.
void GCN_SAMPLE_ALLGPU_impl::pd_train(int slot) {
  flush_update();
  pd_key_ = (uint32_t)pd_slot_key_[slot];
  pd_active_ = true;
  if (!pd_slot_first_[slot]) return;
  const int sb = pd_slot_sb_[slot];
  const uint32_t n = pd_counts_[sb];
  if (n == 0) return;
  const int ring = (int)(pd_key_ % kPdRing);
  pd_sampler_->finish_gpu_sample(ring);  // its sizes (the batch's own sync already covered it)
  auto guard = cs->guard();
  torch::NoGradGuard ng;
  NtsVar Wc = P[0]->W.contiguous();
  gemm(*cs, 0, fmat(pd_y_[ring]).top(n), Wc, fmat(pd_share_).top(n), "pd share");
  TORCH_CHECK(hipEventRecord(pd_sampler_->ssgs[ring]->consumed, (hipStream_t)cs->stream()) ==
                  hipSuccess,
              "hipEventRecord");
}

void GCN_SAMPLE_ALLGPU_impl::reset_stats() {
  prof.reset();
  sample_time = train_time = 0;
  batch_edges = 0;
  batches = 0;
}

SamplerRate sampler_throughput(std::shared_ptr<FullyRepGraph> g, const std::vector<VertexId>& seeds,
                               int batch_size, const std::vector<int>& fanout, WeightType w,
                               int rng_mode, int n_batches, const std::vector<bool>& csr_layers,
                               bool weighted, bool coef) {
  TORCH_CHECK(!(weighted || coef) || g->edge_prob.defined(),
              "weighted / coef: the graph has no edge_prob");
  constexpr int kS = 3;
  TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "hipDeviceSynchronize");
  NtsStream st(g->device, nullptr, 2000);
  auto guard = st.guard();
  const int L = (int)fanout.size();
  FastSampler s(g, seeds, L, batch_size, fanout, kS, csr_layers, w != WeightType::None || coef,
                false);
  s.rng_mode = rng_mode;
  s.weighted = weighted;
  s.coef = coef;
  uint64_t items = g->global_vertices;
  for (auto* x : s.ssg->sampled_sgs) items = std::max<uint64_t>({items, x->e_cap, x->v_cap});
  NTS_CALL(nts_hip_ctx_reserve, st.ctx(), g->global_vertices, items);
  SamplerRate r;
  auto run = [&](int n, bool count) {
    int pending[kS] = {0, 0, 0};
    for (int i = 0; i < n + kS; ++i) {
      const int slot = i % kS;
      if (pending[slot]) {
        // (no consumer: the slot is free once its sizes are read.  Recording
        // `consumed` here, at the stream's tail, made the next issue into the
        // slot wait for every batch in flight — one batch at a time, the GPU
        // idle while the host issued the next: 5.7 G edges/s)
        SampledSubgraph* sg = s.finish_gpu_sample(slot);
        pending[slot] = 0;
        if (count) {
          for (auto* x : sg->sampled_sgs) r.edges += x->e_size;
          ++r.batches;
        }
      }
      if (i >= n) continue;
      if (!s.sample_not_finished()) s.restart();
      s.issue_gpu_sample(batch_size, slot, st, w);
      pending[slot] = 1;
    }
  };
  run(std::min(n_batches, 4), false);  // warm-up (first-touch, code objects)
  st.synchronize();
  const auto t0 = std::chrono::steady_clock::now();
  run(n_batches, true);
  st.synchronize();
  r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return r;
}

}  // namespace nts
