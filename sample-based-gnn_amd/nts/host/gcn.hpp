#pragma once
#include <hip/hip_runtime_api.h>

#include "nts_host.hpp"

namespace nts {

struct GCNConfig {
  std::vector<int> layer_size;  // LAYERS, e.g. 602-128-41
  std::vector<int> fanout;      // FANOUT, layer 0 = nearest the seeds
  int batch_size = 1024;        // BATCH_SIZE
  float learn_rate = 0.01f, weight_decay = 1e-4f, drop_rate = 0.5f;
  float beta1 = 0.9f, beta2 = 0.999f, epsilon = 1e-9f;  // toolkits/GCN_SAMPLE_GPU.hpp:115-117
  // NTS_RNG_PHILOX (default), the MT19937 modes (the reference's stream), or
  // NTS_RNG_PHILOX_SHARED: one variate per source vertex, every destination
  // keeps its `fanout` neighbours with the smallest variates (fixed-size LABOR,
  // DESIGN §8o) — the same per-destination distribution, a smaller frontier.
  // Not with sample_gpu or pd_cache.
  int rng_mode = NTS_RNG_PHILOX;
  // GCN_SAMPLE_GPU (toolkits/GCN_SAMPLE_GPU.hpp:289-394): the CPU sampler's
  // blocks (sample_fast: the reference's mt19937 stream, here replayed on the
  // device, NTS_RNG_MT19937_LEMIRE) through SingleGPUSampleGraphOp, whose
  // backward always runs over the sampled CSR (Gather_By_Src_From_Dst_Spmm)
  bool sample_gpu = false;
  WeightType weight_type = WeightType::Sum;  // GraphSAGE toolkits: Mean
  bool up_degree = false;             // UP_DEGREE cfg key (core/GraphSegment.cpp:273-276)
  bool gat = false;                   // GAT_SAMPLE_ALL_GPU model (attention layers)
  // Multi-head attention (gat only; no reference counterpart): one head count
  // per layer, bottom first; empty = 1 everywhere.  A hidden layer with K heads
  // splits its layer_size[l+1] columns into K heads of layer_size[l+1] / K and
  // concatenates them, so the widths of layer_size keep their meaning.  The
  // last layer with K > 1 averages K heads of layer_size.back() columns: its W
  // is [F_in, K C] and its W_att [2 K C, 1].  Every layer's K D must be within
  // the kernels' width limit (1024 when D % 4 == 0, else 256).
  std::vector<int> gat_heads;
  // GATv2 attention (gat only; no reference counterpart; Brody et al., ICLR
  // 2022): every layer scores an edge with
  //   att_h . leaky_relu(W_s x_src + W_d x_dst, 0.2)_h
  // instead of GAT's leaky_relu(a1 . W x_src + a2 . W x_dst), so the ranking of
  // a destination's neighbours depends on the destination.  P[2l] is then the
  // stacked [F_in, 2 gat_width(l)] = [W_s | W_d] and P[2l+1] the score vector
  // [gat_width(l), 1]; gat_heads, gat_attn_drop and gat_feat_drop keep their
  // meaning.  infer_full_gat() / evaluate_full_gat() are not built for it.
  bool gat_v2 = false;
  // GAT dropout (gat only, training mode only; no reference counterpart: the
  // reference's GAT stores drop_rate and never uses it, and drop_rate stays
  // ignored by a GAT driver).  gat_attn_drop: the normalised attention
  // coefficients of every layer, a~ = keep ? a / (1 - q) : 0, the softmax still
  // over all edges.  gat_feat_drop: the input of every layer — the gathered
  // feature rows of layer 0 (no relu) and the relu'd output of every hidden
  // layer (DGL's feat_drop / attn_drop, PyG's GATConv(dropout=)).  Both in
  // [0, 1), fused into the GAT kernels; 0 = off: no launch, Philox
  // offset or output differs from a build without the options.
  double gat_attn_drop = 0.0, gat_feat_drop = 0.0;
  bool fused_gather = true;          // gather features inside the bottom aggregation
  bool bias_correction = false;       // false: learn_local_with_decay_Adam (GPU drivers)
  bool deterministic_backward = true; // CSR transpose gather instead of atomics
  bool hip_gemm = true;               // layer GEMMs on the hand-written MFMA kernels
  bool pipeline = true;               // sample batch i+1 on its own stream while i trains
  bool fuse_activation = true;        // hidden layers: relu + dropout in the MFMA GEMM
  bool fuse_loss = true;              // training: output layer + log_softmax x2 + nll in 2 kernels
  // Multi-label node classification (no reference counterpart): the label
  // tensor is [V, layer_size.back()] of 0/1, the top layer gives raw logits,
  // the loss is the mean sigmoid binary cross-entropy over all entries (fused:
  // nts_hip_linear_bce_*), and evaluate() / evaluate_full() return the
  // micro-F1 of the prediction z > 0.  GCN / GraphSAGE layers only.
  bool multi_label = false;
  // GraphSAGE root weight (SAGEConv; no reference counterpart): every layer is
  // X' = act([A X | X_dst] W) with one stacked W = [W_n; W_s] of
  // [2 layer_size[l], layer_size[l+1]].  The sampler merges the dsts into each
  // frontier (with the weights of weight_type); aggregate-first only.  Not with
  // gat, pd_cache, sample_gpu, transform_first = 1, pair_table, cache_rate >= 0
  // or fused_gather = false.
  bool root_weight = false;
  // Aggregator of every layer's graph op: 0 = the weighted sum of weight_type
  // (the default), 1 = max (GraphSAGE's max aggregator, SAGEConv(aggr="max");
  // no reference counterpart): Y[d] = max over d's sampled edges of X[src] per
  // column, ties to the earliest CSC edge, an empty column 0.  weight_type is
  // ignored (the sampler builds no edge weights, the CSRs carry their edge
  // ids), every layer is aggregate-first (a maximum does not commute with W:
  // transform_first = -1 resolves to 0) and infer_full() takes the maximum
  // over all in-edges.  Not with gat, pd_cache, sample_gpu, transform_first =
  // 1, pair_table > 0, cache_rate >= 0, fused_gather = false,
  // deterministic_backward = false or up_degree.
  int aggregator = 0;
  // LayerNorm on every hidden layer (no reference counterpart): layer l < L-1 is
  // X' = dropout(relu(LayerNorm((A X) W_l; gamma_l, beta_l))) in one fused pass
  // over the plain GEMM's output (nts_hip_ln_act_*; fuse_activation has no
  // effect there); the last layer is unchanged.  gamma_l (ones) and beta_l
  // (zeros) are [layer_size[l+1]] parameters that take Adam steps without
  // weight decay.  Aggregate-first only (LayerNorm does not commute with A:
  // transform_first = -1 resolves to 0).  Not with gat, pd_cache,
  // transform_first = 1, pair_table > 0 or a hidden width above 1024.
  bool layer_norm = false;
  float layer_norm_eps = 1e-5f;
  // BatchNorm on every hidden layer (no reference counterpart),
  // torch.nn.BatchNorm1d's semantics: layer l < L-1 is
  // X' = dropout(relu(BatchNorm((A X) W_l; gamma_l, beta_l))) over the plain
  // GEMM's output (nts_hip_bn_act_*; fuse_activation has no effect there), the
  // statistics taken over the rows of the layer's block in this batch; the
  // last layer is unchanged.  gamma_l (ones) and beta_l (zeros) are parameters
  // as under layer_norm (Adam steps without weight decay, after the W's in
  // weights()); running_mean_l (zeros) and running_var_l (ones) are buffers
  // (norm_stats()) that training moves by batch_norm_momentum and that
  // evaluate(), forward_eval() and infer_full() read without updating.  Per
  // rank under data parallelism (no SyncBatchNorm; nothing joins the
  // all-reduce).  Aggregate-first only (transform_first = -1 resolves to 0).
  // Not with gat, pd_cache, transform_first = 1, pair_table > 0, layer_norm or
  // a hidden width above 1024.
  bool batch_norm = false;
  float batch_norm_eps = 1e-5f;
  float batch_norm_momentum = 0.1f;
  // f16 feature table: the table is kept in HBM as IEEE half and
  // every gather of it (the bottom aggregation, early or in the step; the row
  // gather of fused_gather = false; infer_full()'s layer 0) widens the rows to
  // fp32 as it reads them — f16 storage, fp32 arithmetic, so the driver
  // computes, bit for bit, what a driver without the option computes on
  // table.half().float() with an aggregate-first bottom layer.  The
  // constructor takes a kFloat32 table (rounded to nearest even on the device,
  // the fp32 tensor released) or a kFloat16 one (used as given where its rows
  // allow 16-byte loads); a value that is not finite as a half is refused.
  // Aggregate-first only (transform_first = -1 resolves to 0).  Not with gat,
  // pd_cache, transform_first = 1, pair_table > 0, cache_rate >= 0,
  // root_weight or aggregator = max.
  bool feature_f16 = false;
  // Edge-weighted neighbour selection (DGL prob=, PyG
  // weight_attr=): a destination with more neighbours than its fanout keeps
  // `fanout` of them by successive sampling without replacement with
  // probability proportional to the graph's edge_prob (Efraimidis-Spirakis
  // keys on a Philox stream of their own).  Only the draw changes: counts,
  // frontier, CSR and the weight_type weights are the default sampler's; the
  // option alone does not make edge_prob an aggregation coefficient
  // (edge_weighted does).  Every sampler the driver builds
  // (training, evaluate, forward_eval) uses it.  Needs a graph with edge_prob;
  // not with an MT19937 rng_mode, NTS_RNG_PHILOX_SHARED, pd_cache or sample_gpu.
  bool weighted_sampling = false;
  // Edge weights as aggregation coefficients (DGL
  // GraphConv(edge_weight=), PyG GCNConv(x, ei, edge_weight)): every layer's
  // graph op is Y[d] = sum_e fl32(c(e) a_e) X[src(e)], a = the graph's edge_prob
  // and c the weight of weight_type (WeightType::None: the coefficient alone, for
  // a caller's own normalisation such as gcn_norm).  Every sampler the driver
  // builds calls nts_hip_sample_layer_coef, and infer_full() / evaluate_full()
  // the _coef graph kernels.  With or without weighted_sampling, either
  // bottom-layer order, feature_f16, layer_norm, multi_label, PHILOX or
  // PHILOX_SHARED, pipelined or not, data parallel.  Needs a graph with
  // edge_prob; not with gat, aggregator = max, root_weight, pd_cache,
  // sample_gpu, up_degree, an MT19937 rng_mode, cache_rate >= 0 or
  // deterministic_backward = false.
  bool edge_weighted = false;
  // pipelined sampler's stream priority: 1 = sampler stream high, 0 = both
  // normal, -1 = the training stream high (the sampler's blocks dispatched
  // after the training stream's), 2 = auto: high for the MT19937 stream (its
  // chain is the step's critical path), normal for Philox (its ~0.2 ms of
  // kernels a batch fit beside the training step: C2 0.819-0.823 vs
  // 0.830-0.832 ms/step with the sampler high)
  int sampler_priority = 2;
  // CUs of the pipelined sampler's stream: n > 0 reserves n CUs for it (the
  // training stream on the rest), n < 0 confines it to |n| CUs and leaves the
  // training stream on all; 0: no CU masks
  int sampler_cus = 0;
  // pipelined sampler, transform-first bottom layer: 0 = the next batch's
  // sampling is issued ahead of the training step; 1 = behind the forward
  // gather GEMM (it starts once that GEMM ends); 2 = also the backward gather
  // GEMM waits for it (neither GEMM shares CUs with the sampler)
  int sampler_gate = 0;
  bool pad_features = true;           // copy wide feature tables to a 128-byte row pitch
  bool early_aggregate = true;        // bottom aggregation issued with the sampling (see issue())
  // bottom layer order: 1 = transform first, A (X W) (rows narrowed before the
  // aggregation), 0 = aggregate first, (A X) W (the reference's order),
  // -1 = auto: transform first where F_in >= 4 F_out and the split-bf16
  // (fp32-exact) or pair-table GEMMs apply, aggregate first elsewhere
  int transform_first = -1;
  // layer GEMM arithmetic (nts_hip_ctx_set_gemm_mode): NTS_GEMM_F32 (fp32-input
  // MFMA) or NTS_GEMM_SPLIT3 (fp32-accurate three-piece bf16 split)
  int gemm_mode = NTS_GEMM_SPLIT3;
  // transform-first GEMMs on the feature table's f16 pair table (csrc/gemmh2.hip,
  // built once at construction; 22-bit significand inputs, narrower than
  // fp32: opt-in): 0 = off (gemm_mode: fp32-exact split-bf16), 1 = the
  // forward GEMM, 2 = the forward and the weight-gradient GEMMs, 3 = 2 with
  // the weight gradient on the planar table's whole-row kernel where the
  // shape allows
  int pair_table = 0;
  // data parallel: the gradient all-reduce of step k runs on a stream of its
  // own and the optimizer step waits for it only where step k+1 first reads
  // W (after its bottom aggregation, which does not depend on W): -1 = on with
  // more than one rank, 1 = always (also at one rank, for tests), 0 = off
  int overlap_allreduce = -1;
  bool shuffle = true;
  bool profile = false;               // HIP events around the bottom aggregation
  // CACHE_RATE in [0, 1): the feature table moves to pinned host memory and
  // the rows of the cache_rate * V highest-degree vertices stay in HBM
  // (GS_SAMPLE_PD_CACHE's placement); < 0: the whole table in HBM
  double cache_rate = -1.0;
  // NeutronOrch PD cache (GCN_SAMPLE_PD_CACHE): training seeds in
  // super-batches of pd_super_batch mini-batches (PIPELINE_NUM); per
  // super-batch the hot vertices (preSample, rate pd_rate = CACHE_RATE) get
  // their bottom-layer embedding (A X) W once, at the super-batch's first
  // batch, and every batch of the super-batch skips sampling their bottom
  // neighbourhoods and takes those rows instead.  Training only; aggregate-first.
  bool pd_cache = false;
  double pd_rate = 0.2;
  int pd_super_batch = 4;
  int64_t seed = 2000;
  // LinkPredictor only (nts/host/linkpred.hpp): uniform negatives
  // drawn per positive edge of a batch.  No node-classification driver reads it.
  int neg_per_pos = 1;
  // LinkPredictor only.  lp_exclude: 0 = none, 1 = self: every
  // sampled edge of a batch's blocks that is one of the batch's positive edges
  // (src = head, dst = tail) aggregates with coefficient 0; 2 = reverse: the
  // positives turned round as well.  After selection: a destination above its
  // fanout may aggregate fewer than fanout neighbours.  lp_filter_neg: a
  // negative that is a self pair or a graph edge in either direction is drawn
  // again, up to 16 times.
  int lp_exclude = 0;
  bool lp_filter_neg = false;
  // Subgraph-sampled training (GraphSAINT node / random-walk
  // samplers, random-partition Cluster-GCN): per batch ONE vertex set S is
  // drawn — the batch's seeds and subgraph_walk steps of a random walk over
  // in-neighbours from each — and every layer runs on the subgraph S induces
  // (nts_hip_random_walk + nts_hip_induced_layer in every sampler the driver
  // builds).  Layer 0 has the seeds as destinations and S as sources; layers
  // >= 1 are the square block S x S.  The loss rows are the seeds.  Every
  // fanout must be -1.  subgraph_edge_cap: the edge capacity of every block
  // (0 = min(E, s_cap * 4 * ceil(E / V)) with s_cap = batch_size * (1 +
  // subgraph_walk)); a block above it raises the capacity error.  weight_type
  // (all four), up_degree and root_weight are taken; not with gat, aggregator =
  // max, pd_cache, sample_gpu, an MT19937 rng_mode, NTS_RNG_PHILOX_SHARED,
  // weighted_sampling, edge_weighted, cache_rate >= 0, layer_norm, batch_norm,
  // multi_label, feature_f16, transform_first = 1 (-1 resolves to 0),
  // pair_table > 0, fused_gather = false or deterministic_backward = false.
  // LinkPredictor does not read these fields.
  bool subgraph = false;
  int subgraph_walk = 0;
  int64_t subgraph_edge_cap = 0;
};

// Sampler-only throughput of the GPU sampler (SURVEY §8d "sampler-only"
// sampled-edges/s): FastSampler::sample_gpu_fast over `n_batches` batches of
// `seeds` on its own stream, three slots in flight (issue / finish as the
// pipelined driver does), nothing else on the device.  csr_layers as the
// training driver builds them.
struct SamplerRate {
  double seconds = 0;
  uint64_t edges = 0, batches = 0;
};
SamplerRate sampler_throughput(std::shared_ptr<FullyRepGraph> g, const std::vector<VertexId>& seeds,
                               int batch_size, const std::vector<int>& fanout, WeightType w,
                               int rng_mode, int n_batches, const std::vector<bool>& csr_layers,
                               bool weighted = false, bool coef = false);

class GCN_SAMPLE_ALLGPU_impl {
 public:
  GCN_SAMPLE_ALLGPU_impl(std::shared_ptr<FullyRepGraph> g, NtsVar feature, NtsVar label,
                         std::vector<VertexId> train_nids, GCNConfig cfg,
                         std::shared_ptr<Communicator> comm = nullptr);
  ~GCN_SAMPLE_ALLGPU_impl();

  void init_nn();
  float train_batch();
  float run_epoch();
  // Diagnostic (bench.py's training-stream-alone probe, never the headline):
  // on = sample one batch and train every later step on it, so the training
  // stream runs without the sampler beside it; off = back to sampling.
  void set_diag_reuse_sample(bool on) {
    diag_reuse_ = on;
    reuse_slot_ = -1;
  }
  bool has_batch() const {
    return prefetched_ >= 0 || (!pass_done_ && sampler->sample_not_finished());
  }
  void restart();
  // eval-mode forward over a given seed batch: [Y_0, X_1, Y_1, X_2, ...]
  std::vector<NtsVar> forward_eval(const std::vector<VertexId>& seeds, uint64_t batch_seq);
  // one tensor per layer; with cfg.layer_norm the list of weights()
  void set_weights(const std::vector<NtsVar>& ws);
  // Accuracy (getCorrect / Test, toolkits/GCN_SAMPLE_ALLGPU.hpp:166-213,361-383):
  // training batches count their correct rows on the device as they train
  // (no per-batch sync); train_correct() reads the count (synchronises).
  uint64_t train_correct();
  void reset_correct();
  // multi_label: (tp, fp, fn) of the training batches since reset_correct()
  // (counted on the device as they train; synchronises)
  std::vector<uint64_t> f1_counts();
  // Forward(eval_sampler, 1/2): eval mode over `nids` in batches of the
  // training batch size, sampled like training (the reference's eval/test
  // samplers); returns correct / |nids| (multi_label: the micro-F1
  // 2 tp / (2 tp + fp + fn) over those batches, 0 when nothing is positive).
  double evaluate(const std::vector<VertexId>& nids);
  // Full-neighbour layer-wise inference over the whole graph (no sampling; the
  // reference has no counterpart): [V, C] log-softmax rows of every vertex in
  // eval mode, layer by layer — hidden layers relu((A X) W), the last
  // log_softmax((A X) W), A = nts_hip_spmm_graph_fwd under cfg.weight_type,
  // each layer aggregated on its narrower side (multi_label: the raw logits,
  // no log_softmax).  Deterministic: no RNG stream,
  // sampler slot, eval_seq or dropout offset is touched.  Not for GAT,
  // UP_DEGREE or a spilled feature table (cache_rate >= 0).
  NtsVar infer_full();
  // correct / |nids| of infer_full()'s argmax rows (counted on the device);
  // multi_label: the micro-F1 of its logits > 0 over the rows `nids`
  double evaluate_full(const std::vector<VertexId>& nids);
  // The same for a GAT driver (infer_full() refuses one): per layer H = X W
  // over all V rows, the per-vertex scores (nts_hip_gat_scores) and one fused
  // attention pass over the global CSC (nts_hip_gat_graph_fwd), gat_heads as in
  // training (the last layer the mean over its heads); returns log_softmax of
  // the last layer's relu'd output, what Loss() applies in training.  The same
  // contract: nothing of the sampler, eval_seq or the dropout offsets is
  // touched.  Not for a GCN / GraphSAGE driver or a spilled feature table.
  NtsVar infer_full_gat();
  // correct / |nids| of infer_full_gat()'s argmax rows (counted on the device)
  double evaluate_full_gat(const std::vector<VertexId>& nids);
  // cfg.profile: device ms of each layer's aggregation in the last infer_full()
  // (infer_full_gat(): scores + attention pass)
  std::vector<double> full_agg_ms;
  // PD cache: the hot vertices of every super-batch (preSample on the device,
  // per super-batch counts + their concatenated ids, the PRE_SAMPLE_FILE
  // layout), or replace them (e.g. read from a PRE_SAMPLE_FILE)
  std::pair<std::vector<uint32_t>, std::vector<uint32_t>> presample();
  void set_presample(const std::vector<uint32_t>& counts, const std::vector<uint32_t>& ids);
  uint64_t pd_hits = 0;  // bottom-layer dsts served from the PD cache (host count, sampled batches)
  // [W_0 .. W_{L-1}], then with cfg.layer_norm or cfg.batch_norm
  // [gamma_0, beta_0, gamma_1, beta_1, ...]
  std::vector<NtsVar> weights();
  // cfg.batch_norm: the running statistics of the hidden layers,
  // [running_mean_0, running_var_0, running_mean_1, ...] (copies; empty without
  // the option), and their replacement by a list of the same shapes
  std::vector<NtsVar> norm_stats();
  void set_norm_stats(const std::vector<NtsVar>& stats);
  void reset_stats();
  void resolve_profile() { prof.resolve(); }

  std::shared_ptr<FullyRepGraph> graph;
  NtsVar F, L_GT, target, loss, grad_bucket;
  GCNConfig cfg;
  std::shared_ptr<Communicator> comm;
  std::unique_ptr<NtsStream> cs;  // training stream
  std::unique_ptr<NtsStream> ss;  // sampling stream (pipeline) — own scratch arena
  std::unique_ptr<FastSampler> sampler;
  std::unique_ptr<FeatureCache> fcache;  // two-tier feature table (cache_rate)
  std::vector<Parameter*> P;
  // cfg.layer_norm or cfg.batch_norm: gamma_0, beta_0, gamma_1, beta_1, ... of
  // the hidden layers (apart from P, whose size is the layer count)
  std::vector<Parameter*> LN;
  // cfg.batch_norm: running_mean_0, running_var_0, running_mean_1, ... (buffers:
  // no gradient, no Adam step, not in the gradient bucket or the all-reduce)
  std::vector<NtsVar> BN;
  ctx::NtsContext ctx;
  // statistics
  double sample_time = 0, train_time = 0;
  uint64_t batch_edges = 0, batches = 0;
  KernelProfiler prof;  // device time of the bottom-layer kernels (cfg.profile)
  bool transform_first() const { return tf_; }
  uint64_t eval_seq = uint64_t(1) << 40;  // PHILOX stream of the evaluation batches

  SampledSubgraph* last_sg = nullptr;  // the batch the last train_batch() trained on
  // finish a deferred optimizer step (overlap_allreduce); every public entry
  // that reads or writes the weights calls it
  void flush_update();
  void sync() {
    flush_update();
    cs->synchronize();
  }

 private:
  NtsVar vertexForward(int l, NtsVar& a);
  // with `loss_target` (the batch's targets; multi_label: the packed label
  // table), the last element is the fused scalar loss
  std::vector<NtsVar> forward(SampledSubgraph* sg, bool keep, const NtsVar* pre_y = nullptr,
                              const NtsVar* loss_target = nullptr);
  void issue(int slot, NtsStream& st);
  // GAT_SAMPLE_ALL_GPU::Forward (toolkits/GAT_SAMPLE_ALL_GPU.hpp:308-391)
  std::vector<NtsVar> forward_gat(SampledSubgraph* sg);
  double bottom_bytes(SampledSubgraph* sg, bool fused_map) const;
  KernelProfiler* profiler() { return cfg.profile ? &prof : nullptr; }
  void Loss(NtsVar& left, NtsVar& right);
  // every trained tensor, in the order of weights() and of grad_bucket: the W's, then LN
  std::vector<Parameter*> params() const {
    std::vector<Parameter*> all(P);
    all.insert(all.end(), LN.begin(), LN.end());
    return all;
  }
  // hidden layer l's LayerNorm + relu + dropout (p = 0, offset 0: no mask drawn)
  NtsVar layer_norm_act(int l, const NtsVar& Z, double p, uint64_t offset) {
    return hip_ln_act(Z, LN[2 * (size_t)l]->W, LN[2 * (size_t)l + 1]->W, cfg.layer_norm_eps, p,
                      dropout_key(), offset, cs.get());
  }
  // hidden layer l's BatchNorm + relu + dropout: in training mode the batch's
  // statistics (and the buffers move), otherwise the running statistics
  NtsVar batch_norm_act(int l, const NtsVar& Z, double p, uint64_t offset) {
    return hip_bn_act(Z, LN[2 * (size_t)l]->W, LN[2 * (size_t)l + 1]->W, BN[2 * (size_t)l],
                      BN[2 * (size_t)l + 1], ctx.is_train(), cfg.batch_norm_eps,
                      cfg.batch_norm_momentum, p, dropout_key(), offset, cs.get());
  }
  void Update();
  bool defer_ = false;            // overlap_allreduce in effect
  bool pending_update_ = false;   // an all-reduce is in flight, its Adam not yet run
  hipStream_t comm_stream_ = nullptr;
  hipEvent_t grads_packed_ = nullptr, grads_reduced_ = nullptr;
  std::pair<hipEvent_t, hipEvent_t>& next_events();
  void mark(const char* what, NtsStream& st);
  void count_correct(const NtsVar& out, const NtsVar& tgt);  // non-fused output layers
  NtsVar correct_;        // int32 [1]: correct rows of the training batches since reset
  uint32_t* count_to_ = nullptr;  // where forward's fused loss adds its correct count
  // ---- multi_label ----
  NtsVar label_bits_;     // int32 [V, ceil(C / 32)]: the packed 0/1 labels of every vertex
  NtsVar f1_;             // int32 [3]: tp, fp, fn of the training batches since reset
  bool fuse_bce() const;  // the fused BCE kernels take this model's top layer
  // float [n, C] targets of a sampled batch's seeds (the libtorch chain)
  NtsVar batch_targets(SampledSubgraph* sg) const;
  // counts[0..2] += tp, fp, fn of logits > 0 against float 0/1 targets
  static void count_f1(NtsVar& counts, const NtsVar& logits, const NtsVar& targets);
  static double micro_f1(const NtsVar& counts);
  // ---- PD cache state ----
  static constexpr int kPdRing = 4;  // super-batches in flight (sampler lookahead)
  void pd_issue(int slot, NtsStream& st);  // per batch, at sampling time
  void pd_train(int slot);                 // per batch, before its forward
  std::vector<uint32_t> pd_counts_;   // hot vertices per super-batch
  std::vector<uint64_t> pd_offset_;   // their offsets in the concatenated id list
  NtsVar pd_ids_, pd_cache_map_, pd_cache_loc_;  // device: ids; u32 [V] map / location
  std::unique_ptr<FastSampler> pd_sampler_;      // 1 layer (bottom fanout) over the hot ids
  NtsVar pd_y_[kPdRing];              // their aggregation A X, per ring slot
  NtsVar pd_stage_[kPdRing];          // spilled feature rows of that aggregation (feature cache)
  NtsVar pd_share_;                   // (A X) W of the current super-batch
  uint32_t pd_next_key_ = 0;
  int pd_slot_key_[3] = {0, 0, 0};    // per sampler slot (kSlots): its super-batch key
  int pd_slot_sb_[3] = {-1, -1, -1};  // ... its super-batch index in the pass
  bool pd_slot_first_[3] = {false, false, false};
  uint32_t pd_key_ = 0;               // key of the batch being trained (forward)
  bool pd_active_ = false;
  std::vector<std::pair<const char*, hipEvent_t>> tl_;  // NTS_TIMELINE events
  bool tf_ = false;  // transform-first bottom layer (cfg.transform_first)
  // cfg.aggregator: the max graph op, and the weights the samplers then build (none)
  bool max_aggr() const { return cfg.aggregator == 1; }
  AggKind agg_kind() const { return {max_aggr(), cfg.root_weight}; }  // every layer's graph op
  // the fused dropout masks: their Philox key, and the rate (none in eval mode)
  uint64_t dropout_key() const { return (uint64_t)cfg.seed * 0x9E3779B97F4A7C15ull + 1; }
  double drop_rate() const { return ctx.is_train() ? cfg.drop_rate : 0.0; }
  // forward_eval's and evaluate()'s sampler: batches of `batch` over `ids`
  std::unique_ptr<FastSampler> eval_sampler(const std::vector<VertexId>& ids, int batch,
                                            uint64_t batch_seq);
  // cfg.gat_heads: layer l's head count, and the width of its W (the last
  // layer's heads are averaged, so its W holds K heads of layer_size.back())
  int gat_heads(int l) const { return cfg.gat_heads.empty() ? 1 : cfg.gat_heads[(size_t)l]; }
  int64_t gat_width(int l) const {
    const bool last = (size_t)l + 2 == cfg.layer_size.size();
    return (last ? gat_heads(l) : 1) * (int64_t)cfg.layer_size[(size_t)l + 1];
  }
  WeightType sample_weight() const {
    return cfg.gat || max_aggr() ? WeightType::None : cfg.weight_type;
  }
  std::unique_ptr<PairTable> pairs_;  // the feature table's f16 pair table (cfg.pair_table)
  // early aggregation: per sampler slot, the bottom graph op's output and the
  // event after which it (and the slot's sampled graph) is ready
  static constexpr int kSlots = 3;  // sampler slots when pipelined (see the constructor)
  int nslots_ = 1;
  NtsVar pre_y_[kSlots];
  NtsVar lbl_[kSlots];  // each slot's batch labels, gathered on the sampling stream
  NtsVar stage_[kSlots];  // early aggregation + feature cache: staged spill rows
  hipEvent_t ready_[kSlots] = {nullptr, nullptr, nullptr};
  bool early_ = false;
  uint64_t dropout_calls_ = 0;  // Philox offset of the fused dropout masks
  int prefetched_ = -1;  // slot holding an issued, not yet trained batch
  int next_slot_ = 0;
  bool diag_reuse_ = false;
  int reuse_slot_ = -1;  // set_diag_reuse_sample
  // pass boundary: the next pass's first batch is issued behind the current
  // pass's last one (carry_), handed over by restart()
  int carry_ = -1;
  bool pass_done_ = false;
  bool fresh_pass_ = true;
  // cfg.sampler_gate: the next batch's issue, deferred to the bottom layer's
  // forward GEMM hook, and the event it waits on
  std::function<void()> deferred_issue_;
  hipEvent_t gate_ev_ = nullptr;
  int gated_slot_ = -1;
  void prefetch_next();
};

}  // namespace nts
