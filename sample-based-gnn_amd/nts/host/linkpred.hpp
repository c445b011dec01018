// Link prediction on sampled blocks (no reference counterpart: the
// semantics of DGL's as_edge_prediction_sampler + negative_sampler.Uniform and
// PyG's LinkNeighborLoader).  A batch is B positive edges and K Philox
// negatives per positive (nts_hip_lp_batch); the seeds of the sampled blocks
// are the batch's distinct endpoints, known on the device only
// (FastSampler::issue_gpu_sample_dev); the model is L GCN / GraphSAGE layers
// with the sum aggregator, X' = dropout(relu((A X) W_l)), the last (A X) W
// without activation: its layer_size.back() columns are the embedding; the
// loss is the mean sigmoid BCE of the pairs' dot products (nts_hip_lp_bce_*).
// Adam as in the GCN driver.  One sampler slot, no pipeline.
#pragma once
#include "gcn.hpp"
#include "options.hpp"

namespace nts {

// the device arrays of one batch (nts_hip_lp_batch's outputs), sized for
// b_cap positives
struct LpBatch {
  NtsVar pos_src, pos_dst;             // int32 [b_cap]
  NtsVar destination, v_size;          // int32 [2 P_cap], [1]
  NtsVar pair_u, pair_v, score;        // [P_cap]
  NtsVar inc_offset, inc_slot;         // int32 [2 P_cap + 1], [2 P_cap]
  uint32_t B = 0, K = 0;               // the live batch
  uint64_t batch_seq = 0;
  LpPairs pairs{};                     // the raw pointers the loss op takes
  // the excluded edges' sorted key table (int64 [2 b_cap], with
  // lp_exclude), its live count, and the batch's counters {CSC edges excluded
  // over all blocks, negatives still a true edge after 16 draws}
  NtsVar excl_keys, n_keys, counters;
  void alloc(int64_t b_cap, int K, int device, bool exclude = false);
};

class LinkPredictor {
 public:
  // feature: fp32 [V, layer_size[0]] on the GPU; train_edges: int64 [2, n] on
  // the host (row 0 the heads, row 1 the tails)
  LinkPredictor(std::shared_ptr<FullyRepGraph> g, NtsVar feature, const NtsVar& train_edges,
                GCNConfig cfg);
  ~LinkPredictor();

  float train_batch();  // returns the batch's loss (synchronises to read it)
  float run_epoch();    // the remaining batches of the pass; the mean loss
  bool has_batch() const { return offset_ < n_train_; }
  void restart() { offset_ = 0; }
  std::vector<NtsVar> weights();
  void set_weights(const std::vector<NtsVar>& ws);
  // Eval mode over `edges` (int64 [2, m], host) in batches of the training
  // batch size: negatives and sampling keyed by the evaluation stream, batch
  // j of every call at batch_seq (1 << 40) + j, so two calls on the same
  // edges see the same negatives and blocks.  Returns the MRR over all m
  // positives (each ranked against its own K negatives).  Nothing of the
  // training stream (batch_seq, position in the pass, dropout offsets) moves.
  double evaluate(const NtsVar& edges);
  // DESIGN §8v.  The model's own embedding of EVERY vertex, fp32 [V,
  // layer_size.back()]: layer by layer over the whole graph with the
  // whole-graph aggregation (nts_hip_spmm_graph_fwd, _coef with edge_weighted)
  // and the driver's GEMMs; hidden layers relu on the narrower side of the
  // layer, the last (A X) W without activation.  Eval mode, no
  // grad, no random stream; nothing of the training state moves (train_seq,
  // the position in the pass, the dropout offsets, the sampler slot, `batch`).
  // Refuses mean-sampled weights and up_degree (check_link_pred_full).
  NtsVar embed_full();
  // One embed_full(), then every edge of `edges` (int64 [2, m], host) ranked
  // against all V tails (or `candidates`, int64 ids on the host; undefined:
  // all) by nts_hip_lp_rank in chunks of at most batch_size queries; with
  // both_sides a second pass ranks the heads (heads and tails swapped).
  // filtered: a candidate that is the head or its neighbour in either
  // direction is dropped (sorted_rows_ is built on demand).  The metrics are
  // formed on the device from the three count arrays, one small tensor comes
  // back: {mrr, mrr_optimistic, mean_rank, hits@k for each k, n, ties}, rank =
  // 1 + greater + equal (ties count against the positive), optimistic 1 +
  // greater, ties = sum of equal.
  std::vector<std::pair<std::string, double>> evaluate_full(const NtsVar& edges,
                                                            const std::vector<int64_t>& ks,
                                                            bool filtered, bool both_sides,
                                                            const NtsVar& candidates);
  // Eval mode, the first min(batch_size, m) edges of `edges` as one batch of
  // the evaluation stream: {the batch's distinct endpoints (global ids), their
  // embedding rows from the sampled blocks} (tests compare them with
  // embed_full()).  Nothing of the training state moves.
  std::pair<NtsVar, NtsVar> embed_sampled(const NtsVar& edges);
  void synchronize() { cs->synchronize(); }
  // of the last training batch, read back on request only: the
  // sampled edges, over all its blocks, that lp_exclude set to 0, and the
  // negatives lp_filter_neg could not resolve in 16 draws
  int64_t excluded_edges();
  int64_t unresolved_negatives();

  std::shared_ptr<FullyRepGraph> graph;
  NtsVar F, loss;
  GCNConfig cfg;
  std::unique_ptr<NtsStream> cs;
  std::unique_ptr<FastSampler> sampler;
  std::vector<Parameter*> P;
  ctx::NtsContext ctx;
  LpBatch batch;                       // the last training step's batch
  SampledSubgraph* last_sg = nullptr;  // and its sampled blocks
  uint64_t train_seq = 0;              // batch_seq of the next training batch
  uint64_t batches = 0;

 private:
  // pairs + seed set + sampled blocks of edges [off, off + B) of (src, dst)
  SampledSubgraph* build(LpBatch& b, FastSampler& s, const NtsVar& src, const NtsVar& dst,
                         int64_t off, int64_t B, uint64_t seq);
  // the embedding of the batch's endpoints, then the loss (and, training, its
  // recorded backward); mrr: the device counter pair (evaluation)
  // emb (nullable): receives the embedding rows
  NtsVar forward(SampledSubgraph* sg, LpBatch& b, float* mrr, NtsVar* emb = nullptr);
  std::unique_ptr<FastSampler> make_sampler() const;
  void ensure_sorted_rows();  // sorted_rows_, once
  uint64_t dropout_key() const { return (uint64_t)cfg.seed * 0x9E3779B97F4A7C15ull + 1; }
  NtsVar train_src_, train_dst_;  // int32 [n] on the device, in training order
  NtsVar sorted_rows_;            // lp_filter_neg: row_indices sorted within each destination
  int64_t n_train_ = 0, offset_ = 0;
  uint64_t dropout_calls_ = 0;
};

}  // namespace nts
