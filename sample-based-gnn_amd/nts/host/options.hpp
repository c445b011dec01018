// The driver's option and shape rules, in one pass that touches no device:
// GCN_SAMPLE_ALLGPU_impl's constructor runs it before it builds anything, and
// the bindings expose it, so every rule can be checked without a GPU.
#pragma once
#include "gcn.hpp"

namespace nts {

// what the rules read of the constructor's inputs, and nothing else
struct DriverInputs {
  torch::ScalarType feature_dtype = torch::kFloat32;
  bool feature_on_gpu = true;
  int64_t feature_cols = 0;          // -1: the table is not 2-D
  std::vector<int64_t> label_shape;  // its size is the label tensor's rank
  bool label_on_gpu = true;
  int64_t n_vertices = 0;
  bool has_edge_prob = false;
};

// Every refusal of a (cfg, inputs) pair, first one wins, as a c10::Error whose
// first line is the rule's text.  A new option's refusals are one more table
// at the end of the pass: the report order is the source order.
void check_driver_options(const GCNConfig& cfg, const DriverInputs& in);

// Link prediction (LinkPredictor): what its rules read of the
// constructor's inputs, and every refusal of a (cfg, inputs) pair before
// anything is built.  This first version takes GCN / GraphSAGE layers with the
// sum aggregator on an fp32 table; each option it does not take has a text of
// its own.  check_driver_options is not involved.
struct LinkPredInputs {
  torch::ScalarType feature_dtype = torch::kFloat32;
  bool feature_on_gpu = true;
  int64_t feature_cols = 0;         // -1: the table is not 2-D
  std::vector<int64_t> edge_shape;  // train_edges' sizes: [2, n]
  bool edges_on_host = true;
  int64_t n_vertices = 0;
  bool has_edge_prob = false;
};
void check_link_pred_options(const GCNConfig& cfg, const LinkPredInputs& in);
// what LinkPredictor::embed_full() / evaluate_full(filtered) refuse of a
// predictor that was built
void check_link_pred_full(const GCNConfig& cfg, int64_t n_vertices, bool filtered);

// the rules nts.host.gcn_config also applies, each at its place in the pass
void check_gat_heads(const std::vector<int>& layer_size, bool gat, const std::vector<int>& heads);
void check_gat_v2(bool gat_v2, bool gat);
void check_gat_drop(const char* name, double rate, bool gat);

}  // namespace nts
