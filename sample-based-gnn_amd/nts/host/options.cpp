#include "options.hpp"

namespace nts {

namespace {

// One row of a refusal table: where `hit` holds the job is refused with the
// table's lead followed by `why`.  The conditions of one table are evaluated
// together, so a table holds only rows that are safe to evaluate whatever
// the rows above them say.
struct Refusal {
  bool hit;
  std::string why;
};

void refuse(const char* lead, const std::vector<Refusal>& rows) {
  for (const auto& r : rows) TORCH_CHECK(!r.hit, lead, r.why);
}

// what root_weight and aggregator = max both refuse, in the order it is
// reported; tf_why: the option's own reason inside the transform_first text
std::vector<Refusal> aggregate_first_refusals(const GCNConfig& cfg, const char* tf_why) {
  return {
      {cfg.gat, " is not supported with gat (GCN / GraphSAGE layers only)"},
      {cfg.pd_cache, " is not supported with pd_cache"},
      {cfg.sample_gpu, " is not supported with sample_gpu"},
      {cfg.transform_first == 1, std::string(" is not supported with transform_first = 1 (") +
                                     tf_why + "aggregate-first only)"},
      {cfg.pair_table > 0, " is not supported with pair_table > 0"},
      {!(cfg.cache_rate < 0.0), " is not supported with cache_rate >= 0"},
      {!cfg.fused_gather, " is not supported with fused_gather = false"},
      {!cfg.deterministic_backward, " needs deterministic_backward (its backward runs over the CSR)"},
  };
}

}  // namespace

// (each check needs the ones above it, a head count >= 1 before it divides: no table)
void check_gat_heads(const std::vector<int>& layer_size, bool gat, const std::vector<int>& heads) {
  if (heads.empty()) return;
  const size_t nl = layer_size.empty() ? 0 : layer_size.size() - 1;
  TORCH_CHECK(gat, "gat_heads is not supported without gat (attention layers only)");
  TORCH_CHECK(heads.size() == nl, "gat_heads needs one entry per layer (", nl, "), got ",
              heads.size());
  for (size_t l = 0; l < nl; ++l) {
    const int64_t K = heads[l], w = layer_size[l + 1];
    TORCH_CHECK(K >= 1, "gat_heads[", l, "] must be >= 1, got ", K);
    const bool last = l + 1 == nl;
    TORCH_CHECK(last || w % K == 0, "gat_heads[", l, "] = ", K, " does not divide layer width ", w);
    const int64_t D = last ? w : w / K, Fl = K * D;
    TORCH_CHECK(K == 1 || Fl <= (D % 4 == 0 ? 1024 : 256), "gat_heads[", l, "] = ", K, " heads of ",
                D, " columns: K D = ", Fl, " is outside the kernels' width limit (1024 when D is a "
                "multiple of 4, else 256)");
  }
}

void check_gat_v2(bool gat_v2, bool gat) {
  refuse("", {{gat_v2 && !gat, "gat_v2 is not supported without gat (attention layers only)"}});
}

void check_gat_drop(const char* name, double rate, bool gat) {
  refuse(name, {{!(rate >= 0.0 && rate < 1.0), c10::str(" must be in [0, 1), got ", rate)},
                {!(rate == 0.0 || gat), " is not supported without gat (attention layers only)"}});
}

void check_driver_options(const GCNConfig& cfg, const DriverInputs& in) {
  const bool max = cfg.aggregator == 1, mt = is_mt_mode(cfg.rng_mode);
  const bool half = in.feature_dtype == torch::kFloat16;
  const size_t rank = in.label_shape.size();
  refuse("", {{cfg.layer_size.size() < 2, "need at least one layer"},
              {cfg.fanout.size() != cfg.layer_size.size() - 1, "fanout per layer"}});
  const int L = (int)cfg.fanout.size();
  refuse("", {{half && !cfg.feature_f16,
               "a float16 feature table needs feature_f16 (FEATURE_F16:1): without it the driver "
               "takes an fp32 table"},
              {!(in.feature_on_gpu && (in.feature_dtype == torch::kFloat32 || half) &&
                 in.feature_cols == cfg.layer_size[0]),
               "feature table must be fp32 [V, layer_size[0]] on the GPU"}});
  if (cfg.multi_label)
    refuse("", {{cfg.gat, "multi_label is not supported with GAT layers (GCN / GraphSAGE only)"},
                {rank != 2, c10::str("multi_label needs a 2-D label tensor [V, C] of 0/1, got ", rank,
                                     "-D")},
                {!(rank == 2 && in.label_on_gpu && in.label_shape[0] == in.n_vertices &&
                   in.label_shape[1] == cfg.layer_size.back()),
                 "multi_label: labels must be [V, layer_size.back()] on the GPU"}});
  else
    refuse("", {{rank != 1, "labels must be int64 [V] (a [V, C] 0/1 label tensor needs multi_label)"}});
  if (cfg.root_weight) refuse("root_weight", aggregate_first_refusals(cfg, ""));
  refuse("", {{cfg.aggregator != 0 && cfg.aggregator != 1, "aggregator must be 0 (sum) or 1 (max)"}});
  if (max) {
    auto rows = aggregate_first_refusals(cfg, "a maximum does not commute with W: ");
    rows.push_back({cfg.up_degree, " is not supported with up_degree (it takes no edge weights)"});
    refuse("aggregator = max", rows);
  }
  check_gat_heads(cfg.layer_size, cfg.gat, cfg.gat_heads);
  check_gat_v2(cfg.gat_v2, cfg.gat);
  if (cfg.layer_norm) {
    std::vector<Refusal> rows = {
        {cfg.gat, "gat (GCN / GraphSAGE layers only)"},
        {cfg.pd_cache, "pd_cache"},
        {cfg.transform_first == 1,
         "transform_first = 1 (LayerNorm does not commute with A: aggregate-first only)"},
        {cfg.pair_table > 0, "pair_table > 0"},
    };
    for (size_t l = 1; l + 1 < cfg.layer_size.size(); ++l)
      rows.push_back({cfg.layer_size[l] > 1024, c10::str("a hidden width above 1024 (layer ", l - 1,
                                                         ": ", cfg.layer_size[l], ")")});
    refuse("layer_norm is not supported with ", rows);
  }
  check_gat_drop("gat_attn_drop", cfg.gat_attn_drop, cfg.gat);
  check_gat_drop("gat_feat_drop", cfg.gat_feat_drop, cfg.gat);
  if (cfg.sample_gpu)
    refuse("", {{cfg.gat || cfg.pd_cache, "GCN_SAMPLE_GPU: GCN / GraphSAGE layers"},
                {cfg.rng_mode == NTS_RNG_PHILOX, "GCN_SAMPLE_GPU samples with the reference's "
                                                 "mt19937 stream (rng_mode MT19937)"}});
  // the feature cache is built for cache_rate >= 0 unless the table is kept as half
  const bool fcache = cfg.cache_rate >= 0.0 && !cfg.feature_f16;
  const bool tf_ok = L >= 2 && !cfg.gat && !fcache && cfg.hip_gemm && cfg.fuse_activation &&
                     !cfg.pd_cache && !cfg.root_weight && !max && !cfg.layer_norm;
  refuse("", {{fcache && !(cfg.cache_rate <= 1.0), "cache_rate must be in [0, 1]"},
              {cfg.transform_first == 1 && !tf_ok,
               "transform_first needs >= 2 layers, the MFMA GEMMs with the fused activation, no "
               "GAT and no feature cache"},
              {cfg.pd_cache && !(!cfg.gat && L >= 2 && cfg.hip_gemm && cfg.pd_super_batch >= 1 &&
                                 cfg.pd_rate >= 0.0),
               "PD cache: GCN/GraphSAGE with >= 2 layers on the MFMA GEMMs"}});
  if (cfg.rng_mode == NTS_RNG_PHILOX_SHARED)
    refuse("shared sampling is not supported with ",
           {{cfg.sample_gpu, "sample_gpu (the reference's mt19937 stream)"},
            {cfg.pd_cache, "pd_cache"}});
  if (cfg.feature_f16)
    refuse("feature_f16 is not supported with ",
           {{cfg.gat, "gat (GCN / GraphSAGE layers only)"},
            {cfg.pd_cache, "pd_cache"},
            {cfg.transform_first == 1,
             "transform_first = 1 (the transform-first GEMMs gather fp32 rows: aggregate-first only)"},
            {cfg.pair_table > 0, "pair_table > 0"},
            {!(cfg.cache_rate < 0.0), "cache_rate >= 0"},
            {cfg.root_weight, "root_weight"},
            {max, "aggregator = max"}});
  if (cfg.weighted_sampling)
    refuse("weighted_sampling ",
           {{!in.has_edge_prob, "needs a graph with edge_prob (from_edges(..., edge_weight) or "
                                "from_csc(..., edge_prob))"},
            {mt, "is not supported with an MT19937 rng_mode (it draws from a Philox stream of its "
                 "own)"},
            {cfg.rng_mode == NTS_RNG_PHILOX_SHARED,
             "is not supported with rng_mode NTS_RNG_PHILOX_SHARED (shared_sampling)"},
            {cfg.pd_cache, "is not supported with pd_cache"},
            {cfg.sample_gpu, "is not supported with sample_gpu (the reference's mt19937 stream)"}});
  if (cfg.edge_weighted)
    refuse("edge_weighted is not supported with ",
           {{!in.has_edge_prob,
             "a graph without edge_prob (from_edges(..., edge_weight) or from_csc(..., edge_prob))"},
            {cfg.gat, "gat (attention layers use no edge weights)"},
            {max, "aggregator = max (it uses no edge weights)"},
            {cfg.root_weight, "root_weight"},
            {cfg.pd_cache, "pd_cache"},
            {cfg.sample_gpu, "sample_gpu (the reference's mt19937 stream)"},
            {cfg.up_degree, "up_degree"},
            {mt, "an MT19937 rng_mode"},
            {!(cfg.cache_rate < 0.0), "cache_rate >= 0"},
            {!cfg.deterministic_backward,
             "deterministic_backward = false (the backward reads the CSR's weights)"}});
  // (transform_first = 1 passes the tf_ok row above: this table's own text reports it)
  if (cfg.batch_norm) {
    std::vector<Refusal> rows = {
        {cfg.gat, "gat (GCN / GraphSAGE layers only)"},
        {cfg.pd_cache, "pd_cache"},
        {cfg.transform_first == 1,
         "transform_first = 1 (BatchNorm does not commute with A: aggregate-first only)"},
        {cfg.pair_table > 0, "pair_table > 0"},
        {cfg.layer_norm, "layer_norm (one normalisation per hidden layer)"},
    };
    for (size_t l = 1; l + 1 < cfg.layer_size.size(); ++l)
      rows.push_back({cfg.layer_size[l] > 1024, c10::str("a hidden width above 1024 (layer ", l - 1,
                                                         ": ", cfg.layer_size[l], ")")});
    refuse("batch_norm is not supported with ", rows);
  }
  // subgraph-sampled training
  if (cfg.subgraph) {
    bool all_fanout = true;
    for (int f : cfg.fanout) all_fanout &= f == -1;
    refuse("subgraph ",
           {{!all_fanout, "needs every fanout = -1 (all induced neighbours; other values are "
                          "kept for a fanout-capped meaning)"},
            {cfg.subgraph_walk < 0 || cfg.subgraph_walk > 64,
             c10::str("needs subgraph_walk in [0, 64], got ", cfg.subgraph_walk)},
            {cfg.subgraph_edge_cap < 0 || cfg.subgraph_edge_cap > 0xFFFFFFFFll,
             c10::str("needs subgraph_edge_cap in [0, 2^32) (0 = the default), got ",
                      cfg.subgraph_edge_cap)},
            {cfg.gat, "is not supported with gat (GCN / GraphSAGE layers only)"},
            {max, "is not supported with aggregator = max"},
            {cfg.pd_cache, "is not supported with pd_cache"},
            {cfg.sample_gpu, "is not supported with sample_gpu (the reference's mt19937 stream)"},
            {mt, "is not supported with an MT19937 rng_mode (the walks draw from a Philox stream "
                 "of their own)"},
            {cfg.rng_mode == NTS_RNG_PHILOX_SHARED,
             "is not supported with rng_mode NTS_RNG_PHILOX_SHARED (shared_sampling): an induced "
             "block selects nothing"},
            {cfg.weighted_sampling, "is not supported with weighted_sampling (the walks are uniform)"},
            {cfg.edge_weighted, "is not supported with edge_weighted"},
            {!(cfg.cache_rate < 0.0), "is not supported with cache_rate >= 0"},
            {cfg.layer_norm, "is not supported with layer_norm"},
            {cfg.batch_norm, "is not supported with batch_norm"},
            {cfg.multi_label, "is not supported with multi_label"},
            {cfg.feature_f16, "is not supported with feature_f16"},
            {cfg.transform_first == 1,
             "is not supported with transform_first = 1 (aggregate-first only)"},
            {cfg.pair_table > 0, "is not supported with pair_table > 0"},
            {!cfg.fused_gather, "is not supported with fused_gather = false"},
            {!cfg.deterministic_backward, "is not supported with deterministic_backward = false"}});
  }
}

void check_link_pred_options(const GCNConfig& cfg, const LinkPredInputs& in) {
  refuse("", {{cfg.layer_size.size() < 2, "need at least one layer"},
              {cfg.fanout.size() != cfg.layer_size.size() - 1, "fanout per layer"}});
  refuse("link prediction ",
         {{cfg.neg_per_pos < 1, c10::str("needs neg_per_pos >= 1, got ", cfg.neg_per_pos)},
          {cfg.batch_size < 1, c10::str("needs batch_size >= 1, got ", cfg.batch_size)},
          {cfg.gat, "is not supported with gat (GCN / GraphSAGE layers only)"},
          {cfg.aggregator != 0, "is not supported with aggregator = max (the sum aggregator only)"},
          {cfg.root_weight, "is not supported with root_weight"},
          {cfg.pd_cache, "is not supported with pd_cache"},
          {cfg.sample_gpu, "is not supported with sample_gpu (the reference's mt19937 stream)"},
          {is_mt_mode(cfg.rng_mode),
           "is not supported with an MT19937 rng_mode (the seeds are device-side: Philox and "
           "Philox-shared only)"},
          {!(cfg.cache_rate < 0.0), "is not supported with cache_rate >= 0"},
          {cfg.multi_label, "is not supported with multi_label (it has no label tensor)"},
          {cfg.layer_norm, "is not supported with layer_norm"},
          {cfg.batch_norm, "is not supported with batch_norm"},
          {cfg.feature_f16, "is not supported with feature_f16"},
          {cfg.transform_first == 1,
           "is not supported with transform_first = 1 (aggregate-first only)"},
          {cfg.pair_table > 0, "is not supported with pair_table > 0"},
          {cfg.layer_size.back() > 1024,
           c10::str("takes an embedding width of at most 1024, got ", cfg.layer_size.back())},
          {(cfg.weighted_sampling || cfg.edge_weighted) && !in.has_edge_prob,
           "with weighted_sampling / edge_weighted needs a graph with edge_prob"}});
  // target-edge exclusion
  refuse("lp_exclude ",
         {{cfg.lp_exclude < 0 || cfg.lp_exclude > 2,
           c10::str("must be 0 (none), 1 (self) or 2 (reverse), got ", cfg.lp_exclude)},
          {cfg.lp_exclude != 0 && cfg.weight_type == WeightType::MeanSampled,
           "is not supported with the mean-sampled weights (their normaliser counts the sampled "
           "edges, the excluded one among them)"},
          {cfg.lp_exclude != 0 && cfg.up_degree,
           "is not supported with up_degree (its degrees count the sampled edges, the excluded "
           "one among them)"}});
  refuse("lp_filter_neg ",
         {{cfg.lp_filter_neg && in.n_vertices > (int64_t(1) << 31),
           "takes a graph of at most 2^31 vertices (its sorted adjacency is built from signed "
           "64-bit keys)"}});
  refuse("", {{!(in.feature_on_gpu && in.feature_dtype == torch::kFloat32 &&
                 in.feature_cols == cfg.layer_size[0]),
               "feature table must be fp32 [V, layer_size[0]] on the GPU"},
              {!(in.edges_on_host && in.edge_shape.size() == 2 && in.edge_shape[0] == 2 &&
                 in.edge_shape[1] >= 1),
               "train_edges must be int64 [2, n] on the host, n >= 1"},
              {(int64_t)cfg.batch_size * (1 + (int64_t)std::max(cfg.neg_per_pos, 1)) > (1ll << 28),
               "link prediction: batch_size x (1 + neg_per_pos) above 2^28 pairs"}});
}

// (infer_full()'s wording for the two weight rules, lp_filter_neg's for the key width)
void check_link_pred_full(const GCNConfig& cfg, int64_t n_vertices, bool filtered) {
  refuse("embed_full: ",
         {{cfg.up_degree, "UP_DEGREE weights are a property of a sample, not of the whole graph"},
          {cfg.weight_type == WeightType::MeanSampled,
           "MeanSampled weights are a property of a sample, not of the whole graph"}});
  refuse("evaluate_full: filtered ",
         {{filtered && n_vertices > (int64_t(1) << 31),
           "takes a graph of at most 2^31 vertices (its sorted adjacency is built from signed "
           "64-bit keys)"}});
}

}  // namespace nts
