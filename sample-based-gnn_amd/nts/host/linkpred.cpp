// LinkPredictor: link prediction composed from the NtsContext ops.
#include "linkpred.hpp"
#include "ops_util.hpp"

#include <algorithm>
#include <random>

namespace nts {

namespace {
constexpr uint64_t kEvalSeq = uint64_t(1) << 40;  // the evaluation stream, as in the GCN driver

// int64 [2, n] host edges -> (heads, tails) as int32 device tensors
std::pair<NtsVar, NtsVar> edges_to_device(const NtsVar& edges, int64_t n_vertices, int device,
                                          const std::vector<int64_t>* order) {
  TORCH_CHECK(edges.defined() && !edges.is_cuda() && edges.dim() == 2 && edges.size(0) == 2 &&
                  edges.size(1) >= 1 && edges.scalar_type() == torch::kInt64,
              "edges must be int64 [2, n] on the host, n >= 1");
  NtsVar e = edges.contiguous();
  TORCH_CHECK(e.min().item<int64_t>() >= 0 && e.max().item<int64_t>() < n_vertices,
              "edge endpoints must be vertex ids in [0, V)");
  if (order) e = e.index_select(1, torch::from_blob((void*)order->data(), {(int64_t)order->size()},
                                                    torch::kInt64));
  NtsVar d = e.to(torch::kInt32).to(torch::Device(torch::kCUDA, device));
  return {d[0].contiguous(), d[1].contiguous()};
}
}  // namespace

void LpBatch::alloc(int64_t b_cap, int K_, int device, bool exclude) {
  counters = torch::zeros({2}, u32_opts(device));
  if (exclude) {
    excl_keys = torch::empty({2 * b_cap}, torch::TensorOptions().dtype(torch::kInt64).device(
                                               torch::kCUDA, device));
    n_keys = torch::zeros({1}, u32_opts(device));
  }
  const int64_t P = b_cap * (1 + (int64_t)K_);
  pos_src = torch::empty({b_cap}, u32_opts(device));
  pos_dst = torch::empty({b_cap}, u32_opts(device));
  destination = torch::empty({2 * P}, u32_opts(device));
  v_size = torch::zeros({1}, u32_opts(device));
  pair_u = torch::empty({P}, u32_opts(device));
  pair_v = torch::empty({P}, u32_opts(device));
  score = torch::empty({P}, f32_opts(device));
  inc_offset = torch::empty({2 * P + 1}, u32_opts(device));
  inc_slot = torch::empty({2 * P}, u32_opts(device));
  K = (uint32_t)K_;
}

LinkPredictor::LinkPredictor(std::shared_ptr<FullyRepGraph> g, NtsVar feature,
                             const NtsVar& train_edges, GCNConfig c)
    : graph(std::move(g)), F(std::move(feature)), cfg(std::move(c)) {
  check_link_pred_options(cfg, {F.scalar_type(), F.is_cuda(), F.dim() == 2 ? F.size(1) : -1,
                                train_edges.sizes().vec(), !train_edges.is_cuda(),
                                (int64_t)graph->global_vertices, graph->edge_prob.defined()});
  cs = std::make_unique<NtsStream>(graph->device, nullptr, (uint64_t)cfg.seed);
  NTS_CALL(nts_hip_ctx_set_gemm_mode, cs->ctx(), cfg.gemm_mode);
  // inputs were produced on other streams: order them before our stream
  TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "hipDeviceSynchronize");
  auto guard = cs->guard();
  n_train_ = train_edges.size(1);
  std::vector<int64_t> order((size_t)n_train_);
  for (int64_t i = 0; i < n_train_; ++i) order[(size_t)i] = i;
  if (cfg.shuffle) {  // shuffle_vec's generator, as the GCN driver shuffles its seeds
    std::mt19937 gen(2000);
    std::shuffle(order.begin(), order.end(), gen);
  }
  std::tie(train_src_, train_dst_) =
      edges_to_device(train_edges, (int64_t)graph->global_vertices, graph->device, &order);
  if (cfg.lp_filter_neg) ensure_sorted_rows();
  sampler = make_sampler();
  batch.alloc(cfg.batch_size, cfg.neg_per_pos, graph->device, cfg.lp_exclude != 0);
  // size the scratch arena once so the training loop never allocates
  const uint64_t pairs_cap = (uint64_t)cfg.batch_size * (1 + (uint64_t)cfg.neg_per_pos);
  uint64_t items = std::max<uint64_t>(graph->global_vertices, 8 * pairs_cap);
  for (auto* s : sampler->ssg->sampled_sgs) items = std::max<uint64_t>({items, s->e_cap, s->v_cap});
  NTS_CALL(nts_hip_ctx_reserve, cs->ctx(), graph->global_vertices, items);
  for (size_t i = 0; i + 1 < cfg.layer_size.size(); ++i) {
    P.push_back(new Parameter((size_t)cfg.layer_size[i], (size_t)cfg.layer_size[i + 1],
                                    cfg.learn_rate, cfg.beta1, cfg.beta2, cfg.epsilon,
                                    cfg.weight_decay, graph->device, cfg.seed + (int64_t)i));
    if (cfg.hip_gemm) P.back()->cs = cs.get();
  }
  cs->synchronize();
}

LinkPredictor::~LinkPredictor() {
  for (auto* p : P) delete p;
}

// row_indices ascending within each destination's segment: one sort of the
// (dst << 32 | src) keys (the callers' option rules: V <= 2^31, so they are
// non-negative int64)
void LinkPredictor::ensure_sorted_rows() {
  if (sorted_rows_.defined()) return;
  const auto dev = torch::Device(torch::kCUDA, graph->device);
  NtsVar deg = graph->column_offset.narrow(0, 1, (int64_t)graph->global_vertices) -
               graph->column_offset.narrow(0, 0, (int64_t)graph->global_vertices);
  NtsVar dst = torch::repeat_interleave(
      torch::arange((int64_t)graph->global_vertices, torch::TensorOptions().dtype(torch::kInt64).device(dev)),
      deg, 0, (int64_t)graph->global_edges);
  NtsVar src = graph->row_indices.to(torch::kInt64).bitwise_and(0xFFFFFFFFll);
  NtsVar keys = std::get<0>(torch::sort(dst * (int64_t(1) << 32) + src));
  sorted_rows_ = keys.bitwise_and(0xFFFFFFFFll).to(torch::kInt32).contiguous();
}

// one slot whose layer-0 capacity is the most endpoints a batch can have;
// CSR transposes where a graph-op backward runs (every hop but the outermost)
std::unique_ptr<FastSampler> LinkPredictor::make_sampler() const {
  const int L = (int)cfg.fanout.size();
  const int64_t P = (int64_t)cfg.batch_size * (1 + (int64_t)cfg.neg_per_pos);
  std::vector<bool> csr(L, true);
  csr[L - 1] = false;
  auto s = std::make_unique<FastSampler>(graph, std::vector<VertexId>(), L, (int)(2 * P), cfg.fanout,
                                         1, csr,
                                         cfg.weight_type != WeightType::None || cfg.edge_weighted ||
                                             cfg.lp_exclude != 0);
  s->rng_mode = cfg.rng_mode;
  s->weighted = cfg.weighted_sampling;
  s->coef = cfg.edge_weighted;
  s->up_degree = cfg.up_degree;
  return s;
}

SampledSubgraph* LinkPredictor::build(LpBatch& b, FastSampler& s, const NtsVar& src,
                                      const NtsVar& dst, int64_t off, int64_t B, uint64_t seq) {
  b.B = (uint32_t)B;
  b.batch_seq = seq;
  b.pos_src.narrow(0, 0, B).copy_(src.narrow(0, off, B));
  b.pos_dst.narrow(0, 0, B).copy_(dst.narrow(0, off, B));
  uint32_t* counters = dptr<uint32_t>(b.counters);
  if (cfg.lp_filter_neg || cfg.lp_exclude)
    TORCH_CHECK(hipMemsetAsync(counters, 0, 2 * sizeof(uint32_t), (hipStream_t)cs->stream()) ==
                    hipSuccess,
                "hipMemsetAsync");
  if (cfg.lp_filter_neg) {
    const nts_graph_dev g = graph->dev();
    NTS_CALL(nts_hip_lp_batch_filtered, cs->ctx(), dptr<uint32_t>(b.pos_src),
             dptr<uint32_t>(b.pos_dst), b.B, b.K, graph->global_vertices, seq,
             (uint32_t)b.destination.numel(), dptr<uint32_t>(b.destination),
             dptr<uint32_t>(b.v_size), dptr<uint32_t>(b.pair_u), dptr<uint32_t>(b.pair_v),
             dptr<uint32_t>(b.inc_offset), dptr<uint32_t>(b.inc_slot), &g,
             dptr<uint32_t>(sorted_rows_), counters + 1);
  } else {
    NTS_CALL(nts_hip_lp_batch, cs->ctx(), dptr<uint32_t>(b.pos_src), dptr<uint32_t>(b.pos_dst), b.B,
             b.K, graph->global_vertices, seq, (uint32_t)b.destination.numel(),
             dptr<uint32_t>(b.destination), dptr<uint32_t>(b.v_size), dptr<uint32_t>(b.pair_u),
             dptr<uint32_t>(b.pair_v), dptr<uint32_t>(b.inc_offset), dptr<uint32_t>(b.inc_slot));
  }
  if (cfg.lp_exclude)
    NTS_CALL(nts_hip_lp_exclude_keys, cs->ctx(), dptr<uint32_t>(b.pos_src),
             dptr<uint32_t>(b.pos_dst), b.B, cfg.lp_exclude == 2, graph->global_vertices,
             (uint32_t)b.excl_keys.numel(),
             reinterpret_cast<uint64_t*>(b.excl_keys.data_ptr<int64_t>()),
             dptr<uint32_t>(b.n_keys));
  b.pairs = {dptr<uint32_t>(b.pair_u),   dptr<uint32_t>(b.pair_v), dptr<uint32_t>(b.inc_offset),
             dptr<uint32_t>(b.inc_slot), dptr<uint32_t>(b.v_size), b.B,
             b.K};
  const uint64_t P = (uint64_t)b.B * (1 + (uint64_t)b.K);
  s.batch_seq = seq;
  s.issue_gpu_sample_dev(b.destination, b.v_size, (VertexId)(2 * P), 0, *cs, cfg.weight_type);
  if (cfg.lp_exclude) {
    // behind the layers on the same stream: the target edges' coefficients to
    // 0 in every block; the blocks' structure stays the sampler's
    const bool had = cfg.weight_type != WeightType::None || cfg.edge_weighted;
    for (sampCSC* l : s.ssg->sampled_sgs) {
      nts_sampcsc_dev o{};
      o.v_cap = l->v_cap;
      o.e_cap = l->e_cap;
      o.s_cap = l->s_cap;
      o.destination = dptr<uint32_t>(l->destination);
      o.sample_ans = dptr<uint32_t>(l->sample_ans);
      o.edge_dst = dptr<uint32_t>(l->edge_dst);
      o.source = dptr<uint32_t>(l->source);
      o.edge_weight_forward = dptr<float>(l->edge_weight_forward);
      if (l->has_csr) {
        o.row_offset = dptr<uint32_t>(l->row_offset);
        o.column_indices = dptr<uint32_t>(l->column_indices);
        o.edge_weight_backward = dptr<float>(l->edge_weight_backward);
      }
      o.sizes = dptr<uint32_t>(l->sizes);
      NTS_CALL(nts_hip_lp_mask_block, cs->ctx(), &o,
               reinterpret_cast<const uint64_t*>(b.excl_keys.data_ptr<int64_t>()),
               dptr<uint32_t>(b.n_keys), had, counters);
    }
  }
  return s.finish_gpu_sample(0);
}

NtsVar LinkPredictor::forward(SampledSubgraph* sg, LpBatch& b, float* mrr, NtsVar* emb) {
  const int L = (int)P.size();
  const double p = ctx.is_train() ? (double)cfg.drop_rate : 0.0;
  NtsVar X, out;
  for (int l = 0; l < L; ++l) {
    const int hop = L - 1 - l;
    const bool bottom = l == 0;  // gathers its rows from the feature table
    NtsVar Y = ctx.runGraphOp<op::SingleGPUAllSampleGraphOp>(bottom ? F : X, sg, graph.get(), hop,
                                                             cs.get(), bottom, nullptr, AggKind{},
                                                             false);
    if (l < L - 1) {
      const uint64_t off = ctx.is_train() ? dropout_calls_++ : 0;
      X = ctx.runVertexForward(
          [&](NtsVar& a) {
            if (cfg.hip_gemm && cfg.fuse_activation)
              return hip_linear_act(a, P[l]->W, p, dropout_key(), off, cs.get(), false);
            return hip_relu_dropout(P[l]->forward(a), p, dropout_key(), off, cs.get());
          },
          Y);
    } else {  // the embedding and the pairs' loss, one autograd segment
      out = ctx.runVertexForward(
          [&](NtsVar& a) {
            NtsVar h = P[l]->forward(a);
            if (emb) *emb = h;
            return hip_lp_bce(h, b.pairs, b.score, cs.get(), mrr);
          },
          Y);
    }
  }
  return out;
}

float LinkPredictor::train_batch() {
  auto guard = cs->guard();
  TORCH_CHECK(has_batch(), "train_batch: the pass is over (restart())");
  const int64_t B = std::min<int64_t>(cfg.batch_size, n_train_ - offset_);
  SampledSubgraph* sg = build(batch, *sampler, train_src_, train_dst_, offset_, B, train_seq);
  offset_ += B;
  ++train_seq;
  last_sg = sg;
  ctx.train();
  loss = forward(sg, batch, nullptr);
  ctx.self_backward(false);
  for (auto* p : P) {
    if (cfg.bias_correction) p->learnC2C_with_decay_Adam(*cs);
    else p->learn_local_with_decay_Adam(*cs);
    p->next();
  }
  for (auto* p : P) p->zero_grad();
  TORCH_CHECK(hipEventRecord(sg->consumed, (hipStream_t)cs->stream()) == hipSuccess,
              "hipEventRecord");
  ++batches;
  return loss.item<float>();
}

float LinkPredictor::run_epoch() {
  double sum = 0;
  int64_t n = 0;
  while (has_batch()) {
    sum += train_batch();
    ++n;
  }
  return n ? (float)(sum / (double)n) : 0.f;
}

std::vector<NtsVar> LinkPredictor::weights() {
  auto guard = cs->guard();
  std::vector<NtsVar> out;
  for (auto* p : P) out.push_back(p->W.detach().clone());
  cs->synchronize();
  return out;
}

void LinkPredictor::set_weights(const std::vector<NtsVar>& ws) {
  auto guard = cs->guard();
  TORCH_CHECK(ws.size() == P.size(), "one tensor per layer");
  torch::NoGradGuard ng;
  for (size_t i = 0; i < P.size(); ++i) P[i]->W.copy_(ws[i].view_as(P[i]->W));
  cs->synchronize();
}

int64_t LinkPredictor::excluded_edges() {
  auto guard = cs->guard();
  cs->synchronize();
  return (int64_t)(uint32_t)batch.counters.cpu()[0].item<int32_t>();
}

int64_t LinkPredictor::unresolved_negatives() {
  auto guard = cs->guard();
  cs->synchronize();
  return (int64_t)(uint32_t)batch.counters.cpu()[1].item<int32_t>();
}

double LinkPredictor::evaluate(const NtsVar& edges) {
  auto guard = cs->guard();
  NtsVar src, dst;
  std::tie(src, dst) = edges_to_device(edges, (int64_t)graph->global_vertices, graph->device, nullptr);
  const int64_t m = src.size(0);
  // a sampler and a batch of their own: the training slot, its batch_seq and
  // last_batch() stay as the last training step left them
  auto es = make_sampler();
  LpBatch eb;
  eb.alloc(cfg.batch_size, cfg.neg_per_pos, graph->device, cfg.lp_exclude != 0);
  NtsVar counter = torch::zeros({2}, f32_opts(graph->device));
  const bool was_train = ctx.is_train();
  ctx.eval();
  double rr = 0, n = 0;
  {
    torch::NoGradGuard ng;
    uint64_t seq = kEvalSeq;
    for (int64_t off = 0; off < m; off += cfg.batch_size, ++seq) {
      const int64_t B = std::min<int64_t>(cfg.batch_size, m - off);
      SampledSubgraph* sg = build(eb, *es, src, dst, off, B, seq);
      counter.zero_();
      forward(sg, eb, counter.data_ptr<float>());
      TORCH_CHECK(hipEventRecord(sg->consumed, (hipStream_t)cs->stream()) == hipSuccess,
                  "hipEventRecord");
      NtsVar h = counter.cpu();  // per batch: the fp32 sums stay short, the total is a double
      rr += (double)h[0].item<float>();
      n += (double)h[1].item<float>();
    }
  }
  cs->synchronize();
  if (was_train) ctx.train();
  return n > 0 ? rr / n : 0.0;
}

std::pair<NtsVar, NtsVar> LinkPredictor::embed_sampled(const NtsVar& edges) {
  auto guard = cs->guard();
  NtsVar src, dst;
  std::tie(src, dst) = edges_to_device(edges, (int64_t)graph->global_vertices, graph->device, nullptr);
  auto es = make_sampler();
  LpBatch eb;
  eb.alloc(cfg.batch_size, cfg.neg_per_pos, graph->device, cfg.lp_exclude != 0);
  const bool was_train = ctx.is_train();
  ctx.eval();
  NtsVar emb, ids;
  {
    torch::NoGradGuard ng;
    const int64_t B = std::min<int64_t>(cfg.batch_size, src.size(0));
    SampledSubgraph* sg = build(eb, *es, src, dst, 0, B, kEvalSeq);
    forward(sg, eb, nullptr, &emb);
    const int64_t v = sg->sampled_sgs[0]->v_size;
    ids = eb.destination.narrow(0, 0, v).clone();
    emb = emb.narrow(0, 0, v).clone();
  }
  cs->synchronize();
  if (was_train) ctx.train();
  return {ids, emb};
}

// Each layer is one O(E) aggregation over the global CSC plus one GEMM over
// all V rows (DESIGN §8d's pass with the link predictor's layers).
NtsVar LinkPredictor::embed_full() {
  check_link_pred_full(cfg, (int64_t)graph->global_vertices, false);
  auto guard = cs->guard();
  const int L = (int)P.size();
  const int64_t V = (int64_t)graph->global_vertices;
  const int wt = cfg.weight_type == WeightType::Sum    ? NTS_WEIGHT_SUM
                 : cfg.weight_type == WeightType::Mean ? NTS_WEIGHT_MEAN
                                                       : NTS_WEIGHT_NONE;
  const nts_graph_dev g = graph->dev();
  auto aggregate = [&](const NtsVar& x, bool relu) {
    NtsVar xr = row_major(x);
    NtsVar y = row_padded_empty(V, xr.size(1), graph->device);
    if (cfg.edge_weighted)
      NTS_CALL(nts_hip_spmm_graph_fwd_coef, cs->ctx(), &g, dptr<float>(graph->edge_prob), 0,
               (uint64_t)V, wt, relu ? 1 : 0, xr.data_ptr<float>(), (uint64_t)xr.stride(0),
               (uint32_t)xr.size(1), y.data_ptr<float>(), (uint64_t)y.stride(0));
    else
      NTS_CALL(nts_hip_spmm_graph_fwd, cs->ctx(), &g, 0, (uint64_t)V, wt, relu ? 1 : 0,
               xr.data_ptr<float>(), (uint64_t)xr.stride(0), (uint32_t)xr.size(1),
               y.data_ptr<float>(), (uint64_t)y.stride(0));
    return y;
  };
  const bool was_train = ctx.is_train();
  ctx.eval();
  NtsVar X = F;
  {
    torch::NoGradGuard ng;
    for (int l = 0; l < L; ++l) {
      const NtsVar& W = P[l]->W;
      if (l == L - 1) {  // the embedding: (A X) W, no activation
        X = P[l]->forward(aggregate(X, false));
      } else if (W.size(0) > W.size(1)) {  // relu(A (X W)), the relu in the kernel
        X = aggregate(P[l]->forward(X), true);
      } else {  // relu((A X) W)
        NtsVar Y = aggregate(X, false);
        if (cfg.hip_gemm && cfg.fuse_activation)  // p = 0: no mask, no offset drawn
          X = hip_linear_act(Y, W, 0.0, 0, 0, cs.get(), false);
        else
          X = torch::relu(P[l]->forward(Y));
      }
    }
  }
  if (was_train) ctx.train();
  cs->synchronize();
  return X;
}

std::vector<std::pair<std::string, double>> LinkPredictor::evaluate_full(
    const NtsVar& edges, const std::vector<int64_t>& ks, bool filtered, bool both_sides,
    const NtsVar& candidates) {
  const int64_t V = (int64_t)graph->global_vertices;
  check_link_pred_full(cfg, V, filtered);
  for (int64_t k : ks) TORCH_CHECK(k >= 1, "evaluate_full: hits@k needs k >= 1, got ", k);
  NtsVar H = embed_full();
  auto guard = cs->guard();
  torch::NoGradGuard ng;
  const auto dev = torch::Device(torch::kCUDA, graph->device);
  NtsVar src, dst;
  std::tie(src, dst) = edges_to_device(edges, V, graph->device, nullptr);
  NtsVar cand;
  if (candidates.defined()) {
    TORCH_CHECK(!candidates.is_cuda() && candidates.dim() == 1 && candidates.size(0) >= 1 &&
                    candidates.scalar_type() == torch::kInt64,
                "evaluate_full: candidates must be int64 [n] on the host, n >= 1");
    TORCH_CHECK(candidates.min().item<int64_t>() >= 0 && candidates.max().item<int64_t>() < V,
                "evaluate_full: candidates must be vertex ids in [0, V)");
    cand = candidates.to(torch::kInt32).to(dev).contiguous();
  }
  if (filtered) ensure_sorted_rows();
  const nts_graph_dev g = graph->dev();
  const int64_t m = src.size(0), total = both_sides ? 2 * m : m;
  NtsVar counts = torch::empty({3, total}, u32_opts(graph->device));  // greater | equal | n_valid
  uint32_t* cg = dptr<uint32_t>(counts);
  for (int side = 0; side < (both_sides ? 2 : 1); ++side) {
    const NtsVar& heads = side ? dst : src;
    const NtsVar& tails = side ? src : dst;
    for (int64_t off = 0; off < m; off += cfg.batch_size) {
      const int64_t B = std::min<int64_t>(cfg.batch_size, m - off);
      uint32_t* out = cg + side * m + off;
      NTS_CALL(nts_hip_lp_rank, cs->ctx(), H.data_ptr<float>(), (uint64_t)H.stride(0),
               (uint32_t)H.size(1), (uint32_t)V, dptr<uint32_t>(heads) + off,
               dptr<uint32_t>(tails) + off, (uint32_t)B,
               cand.defined() ? dptr<uint32_t>(cand) : nullptr,
               cand.defined() ? (uint64_t)cand.numel() : 0, filtered ? g.column_offset : nullptr,
               filtered ? dptr<uint32_t>(sorted_rows_) : nullptr, out, out + total,
               out + 2 * total);
    }
  }
  // the metrics on the device, in double; one small tensor comes back
  NtsVar c = counts.to(torch::kInt64).bitwise_and(0xFFFFFFFFll).to(torch::kFloat64);
  NtsVar rank = c[0] + c[1] + 1.0, rank_opt = c[0] + 1.0;
  std::vector<NtsVar> vals = {rank.reciprocal().mean(), rank_opt.reciprocal().mean(), rank.mean()};
  for (int64_t k : ks) vals.push_back(rank.le((double)k).to(torch::kFloat64).mean());
  vals.push_back(c[1].sum());
  NtsVar h = torch::stack(vals).cpu();
  cs->synchronize();
  const double* p = h.data_ptr<double>();
  std::vector<std::pair<std::string, double>> out = {
      {"mrr", p[0]}, {"mrr_optimistic", p[1]}, {"mean_rank", p[2]}};
  for (size_t i = 0; i < ks.size(); ++i) out.push_back({"hits@" + std::to_string(ks[i]), p[3 + i]});
  out.push_back({"n", (double)total});
  out.push_back({"ties", p[3 + ks.size()]});
  return out;
}

}  // namespace nts
