// C++ host layer (libtorch-ROCm) over the C-ABI in include/nts_hip.h.
//
// Mirrors the reference's operator / sampler surface so a toolkit written
// against it reads the same:
//   FullyRepGraph           core/FullyRepGraph.hpp:682-798   (HBM-resident here)
//   sampCSC / SampledSubgraph core/coocsc.hpp:24-462, core/FullyRepGraph.hpp:30-681
//   FastSampler             core/ntsFastSampler.hpp:28-1326  (GPU ctor + sample_gpu_fast)
//   nts::op::ntsGraphOp     core/ntsBaseOp.hpp:28-45
//   SingleGPUAllSampleGraphOp / SingleGPUSampleGraphOp  core/ntsSingleGPUSampleGraphOp.hpp:50-294
//     (one implementation: AggKind selects the sum / max aggregator and the
//      root-weight self term, spmm_csc_fwd launches its forward kernel)
//   nts::ctx::NtsContext    core/ntsContext.hpp:95-680
//   Parameter               core/NtsScheduler.hpp:680-1029
//   Cuda_Stream             cuda/ntsCUDA.hpp:177-595  -> NtsStream (one nts_hip_ctx)
// Errors from the C-ABI throw std::runtime_error (the reference aborts).
#pragma once

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/torch.h>

#include <functional>
#include <memory>
#include <stack>
#include <string>
#include <deque>
#include <vector>

#include "nts_hip.h"

typedef uint32_t VertexId;
typedef float ValueType;
typedef torch::Tensor NtsVar;

// Sum / Mean / None: core/ntsFastSampler.hpp:27.  MeanSampled: the reference GPU
// kernel get_mean_weight's formula (NTS_WEIGHT_MEAN_SAMPLED, nts_hip.h).
enum class WeightType { Sum, Mean, None, MeanSampled };

namespace nts {

void hip_check(int rc, const char* what);

// torch dtype used to store uint32 vertex ids (bit pattern kept)
inline torch::TensorOptions u32_opts(int device) {
  return torch::TensorOptions().dtype(torch::kInt32).device(torch::kCUDA, device);
}
inline torch::TensorOptions f32_opts(int device) {
  return torch::TensorOptions().dtype(torch::kFloat32).device(torch::kCUDA, device);
}
template <typename T>
inline T* dptr(const torch::Tensor& t) {
  return t.defined() ? reinterpret_cast<T*>(t.data_ptr()) : nullptr;
}

// ---------------------------------------------------------------------------
// Cuda_Stream equivalent: one C-ABI context bound to one HIP stream.
// ---------------------------------------------------------------------------
class NtsStream {
 public:
  // stream == nullptr: a dedicated stream from torch's pool; torch work that
  // must be ordered with our kernels runs under guard() (the reference binds
  // a pool stream per pipeline thread, toolkits/GCN_SAMPLE_GPU.hpp:444-466).
  // high_priority: the pool's high-priority stream (the pipelined sampler:
  // its short, latency-bound kernels are dispatched ahead of the training
  // stream's long ones, which fill the remaining CU slots)
  NtsStream(int device, void* stream, uint64_t seed, bool high_priority = false);
  // an owned stream restricted to the CUs set in `cu_mask` (one bit per CU,
  // hipExtStreamCreateWithCUMask): partitions the device between streams
  NtsStream(int device, const std::vector<uint32_t>& cu_mask, uint64_t seed);
  ~NtsStream();
  NtsStream(const NtsStream&) = delete;
  NtsStream& operator=(const NtsStream&) = delete;
  void setNewStream(void* stream);  // Cuda_Stream::setNewStream
  void* stream() const;
  nts_hip_ctx* ctx() const { return ctx_; }
  int device() const { return device_; }
  void synchronize() const;
  // make this stream torch's current stream for the guard's lifetime
  c10::hip::HIPStreamGuard guard() const { return c10::hip::HIPStreamGuard(torch_stream_); }
  c10::hip::HIPStream torch_stream() const { return torch_stream_; }

 private:
  nts_hip_ctx* ctx_ = nullptr;
  hipStream_t owned_ = nullptr;
  int device_ = 0;
  c10::hip::HIPStream torch_stream_;
};

// ---------------------------------------------------------------------------
// FullyRepGraph: replicated global CSC + degrees in HBM.
// ---------------------------------------------------------------------------
class FullyRepGraph {
 public:
  VertexId global_vertices = 0;
  uint64_t global_edges = 0;
  int device = 0;
  torch::Tensor column_offset;  // int64 [V+1]
  torch::Tensor row_indices;    // int32 [E]
  torch::Tensor in_degree;      // int32 [V]  in_degree_for_backward
  torch::Tensor out_degree;     // int32 [V]  out_degree_for_backward
  // float32 [E] in CSC order, or undefined: the edges' sampling weights
  // (weighted_sampling), every value finite and in [2^-60, 2^60]
  torch::Tensor edge_prob;

  // GenerateAll/ReadRepGraphFromRawFile from an edge list already on the device
  // (src/dst int32 tensors in file order), degrees from the same list.
  // edge_weight (optional, float32 [E]): value i belongs to file edge i and is
  // moved to that edge's CSC position (edge_prob).
  static std::shared_ptr<FullyRepGraph> from_edges(NtsStream& cs, const torch::Tensor& src,
                                                   const torch::Tensor& dst, VertexId vertices,
                                                   const torch::Tensor& edge_weight = {});
  // Wrap an existing device CSC (+ degrees, + edge_prob in CSC order).
  static std::shared_ptr<FullyRepGraph> from_csc(torch::Tensor column_offset,
                                                 torch::Tensor row_indices,
                                                 torch::Tensor in_degree, torch::Tensor out_degree,
                                                 torch::Tensor edge_prob = {});
  nts_graph_dev dev() const;
};

// An activation backward fused into a graph-op backward: the op's output rows
// are multiplied by [mask > 0] * scale (mask = the activation's output, row
// pitch ld; bits = the same keep mask packed, where the width has a bits
// kernel).  mask == nullptr: none.
struct FusedActBwd {
  const float* mask = nullptr;
  uint64_t ld = 0;
  float scale = 1.f;
  const uint32_t* bits = nullptr;
};

// ---------------------------------------------------------------------------
// sampCSC: one sampled layer, device arrays sized by capacity (the
// reference's dev_* mirrors + its global_data_buffer arena in one).
// ---------------------------------------------------------------------------
class sampCSC {
 public:
  VertexId v_size = 0, e_size = 0, src_size = 0;  // live sizes (host copy)
  VertexId v_cap = 0, e_cap = 0, s_cap = 0;
  bool has_csr = false;
  torch::Tensor destination, column_offset, row_indices, sample_ans, edge_dst, source,
      edge_weight_forward, row_offset, column_indices, edge_weight_backward, sizes;
  // is_merge_src_dst (GAT): dst d is local src dst_local_id[d]; CSR slot j is
  // CSC edge csr_edge_id[j] (both undefined unless set_merge_src_dst();
  // set_edge_ids() asks for csr_edge_id alone: the max aggregator's backward)
  torch::Tensor dst_local_id, csr_edge_id;
  // root weight: src_dst[s] = the dst whose dst_local_id is s, else
  // NTS_NOT_CACHED (nts_hip_root_inverse_map, built next to the sampling)
  torch::Tensor src_dst;
  // PD cache (sampled with an omit map): per dst its cache row or NTS_NOT_CACHED
  torch::Tensor omit_row;
  // transform-first training: this layer's graph-op backward also applies the
  // bottom layer's relu/dropout backward to its output (act_bwd, set on the
  // layer above the bottom one), and the bottom layer then receives dZ
  // instead of dX1 (grad_premasked on it).  The driver's forward sets both.
  FusedActBwd act_bwd;
  torch::Tensor act_bits;  // transform-first bottom layer: its output's keep mask as bits
  bool grad_premasked = false;

  sampCSC(int device, VertexId v_cap, VertexId e_cap, VertexId s_cap, bool csr, bool weights);
  void set_merge_src_dst();  // core/coocsc.hpp:405-411
  void set_edge_ids();       // csr_edge_id where the layer has a CSR, without merging
  VertexId* dev_dst_local_id() const { return dptr<VertexId>(dst_local_id); }
  // the reference accessor names
  VertexId* dev_dst() const { return dptr<VertexId>(destination); }
  VertexId* dev_src() const { return dptr<VertexId>(source); }
  VertexId* dev_c_o() const { return dptr<VertexId>(column_offset); }
  VertexId* dev_r_i() const { return dptr<VertexId>(row_indices); }
  VertexId* dev_r_o() const { return dptr<VertexId>(row_offset); }
  VertexId* dev_c_i() const { return dptr<VertexId>(column_indices); }
  ValueType* dev_e_w_f() const { return dptr<ValueType>(edge_weight_forward); }
  ValueType* dev_e_w_b() const { return dptr<ValueType>(edge_weight_backward); }
  ValueType* dev_e_w() const { return dptr<ValueType>(edge_weight_forward); }
  const VertexId* dev_v_size() const { return dptr<VertexId>(sizes); }
  const VertexId* dev_e_size() const { return dptr<VertexId>(sizes) + 1; }
  const VertexId* dev_src_size() const { return dptr<VertexId>(sizes) + 2; }
  // host copies (debug / tests): destination(), src(), c_o(), r_i(), ...
  std::vector<VertexId> host_u32(const torch::Tensor& t, size_t n) const;
};

class SampledSubgraph {
 public:
  std::vector<sampCSC*> sampled_sgs;
  int layers = 0;
  std::vector<int> fanout;
  torch::Tensor dev_sizes;   // device u32 [layers*4]: the layers' sizes (views)
  // int32 [layers*4] in mapped, coherent host memory: each layer's last
  // kernel stores its sizes words there (nts_sampcsc_dev::sizes_host)
  int32_t* host_sizes = nullptr;
  uint32_t* host_sizes_dev = nullptr;  // its device-visible address
  hipEvent_t sampled = nullptr;   // recorded after the last issue's kernels
  hipEvent_t consumed = nullptr;  // recorded by the trainer once it is done with the slot
  int pending_batch = 0;          // seeds of the issued, not yet finished batch
  // subgraph_walk >= 0: the capacities of a subgraph-sampled batch
  SampledSubgraph(int device, int layers, const std::vector<int>& fanout, VertexId batch,
                  VertexId vertices, uint64_t edges, const std::vector<bool>& csr,
                  bool weights,
                  bool merge = false, bool edge_ids = false, int subgraph_walk = -1,
                  uint64_t subgraph_edge_cap = 0);
  ~SampledSubgraph();
  SampledSubgraph(const SampledSubgraph&) = delete;
  SampledSubgraph& operator=(const SampledSubgraph&) = delete;
};

// ---------------------------------------------------------------------------
// HBM feature cache + host-pinned spill (GS_SAMPLE_PD_CACHE:
// determine_cache_node_idx / cache_high_degree / mark_cache_node /
// gater_cpu_cache_feature_and_trans_to_gpu, toolkits/GS_SAMPLE_PD_CACHE.hpp:1019-1112).
// The full table moves to pinned host memory (device-mapped, zero-copy reads);
// the rows of the n_cache highest-out-degree vertices stay in HBM.
// ---------------------------------------------------------------------------
class FeatureCache {
 public:
  // table: fp32 [V, F] on the GPU (any row pitch); n_cache <= V rows cached
  FeatureCache(NtsStream& cs, const FullyRepGraph& g, const NtsVar& table, uint64_t n_cache);
  ~FeatureCache();
  FeatureCache(const FeatureCache&) = delete;
  FeatureCache& operator=(const FeatureCache&) = delete;
  uint64_t n_vertices = 0, n_cache = 0;
  int64_t F = 0;
  uint64_t ld = 0;               // row pitch (floats) of both tiers
  float* host = nullptr;         // pinned host table [V, ld] (owned)
  const float* host_dev = nullptr;  // its device-visible address
  NtsVar cache;                  // HBM [n_cache, F] (pitch ld), undefined when n_cache == 0
  NtsVar cache_map;              // u32 [V]: slot or NTS_NOT_CACHED
  NtsVar cache_ids;              // u32 [n_cache]
  const float* cache_ptr() const { return cache.defined() ? cache.data_ptr<float>() : nullptr; }
  // the fused bottom graph op on the two-tier table: the layer's non-cached
  // source rows are staged once into `stage` ([s_cap, ld] floats, HBM), then
  // Y = A X reads cached rows from the cache and the others from the stage.
  // v_dev / s_dev: device v_size / src_size (NULL: v_cap / s_cap are exact).
  void aggregate(nts_hip_ctx* ctx, const sampCSC* s, const uint32_t* v_dev, uint32_t v_cap,
                 const uint32_t* s_dev, uint32_t s_cap, float* stage, float* y,
                 uint64_t ldy) const;
};

// ---------------------------------------------------------------------------
// FastSampler (GPU form): sample_gpu_fast runs every hop on the device, with
// one D2H copy of the layer sizes per batch.
// ---------------------------------------------------------------------------
// the modes that replay the reference's sequential generator (stream ring,
// checkpoints, re-runs); PHILOX and PHILOX_SHARED keep no generator state
inline bool is_mt_mode(int rng_mode) {
  return rng_mode == NTS_RNG_MT19937_LEMIRE || rng_mode == NTS_RNG_MT19937_DIV;
}

class FastSampler {
 public:
  std::shared_ptr<FullyRepGraph> whole_graph;
  VertexId work_range[2] = {0, 0};
  VertexId work_offset = 0;
  int layer = 0;
  std::vector<int> fanout;
  std::vector<VertexId> sample_nids;
  SampledSubgraph* ssg = nullptr;
  std::vector<SampledSubgraph*> ssgs;
  int rng_mode = NTS_RNG_PHILOX;
  // edge-weighted selection (nts_hip_sample_layer_weighted with
  // whole_graph->edge_prob) in place of rng_mode's draw
  bool weighted = false;
  // edge_prob as aggregation coefficients too (nts_hip_sample_layer_coef,
  // DESIGN §8r): the weights are built under WeightType::None as well
  bool coef = false;
  bool up_degree = false;  // UP_DEGREE: weights from each sampled layer's own degrees
  uint64_t batch_seq = 0;  // keys the PHILOX / PHILOX_SHARED streams (one per sampled batch)
  // Subgraph mode, fixed at construction: subgraph_walk >= 0 and a
  // batch is ONE vertex set S — its seeds and subgraph_walk random-walk steps
  // from each (nts_hip_random_walk, keyed by batch_seq) — with every layer the
  // block S induces (nts_hip_induced_layer): layer 0 seeds x S, layers >= 1
  // S x S (each rebuilt: the slots' arrays are per layer).  Capacities: s_cap =
  // min(V, batch (1 + walk)), v_cap of layers >= 1 the same, e_cap =
  // subgraph_edge_cap (0: min(E, s_cap 4 ceil(E / V))).  rng_mode must be
  // NTS_RNG_PHILOX; weighted, coef and omit_map are refused at issue.
  int subgraph_walk() const { return subgraph_walk_; }
  // sample_gpu_fast_omit (core/ntsFastSampler.hpp:711-915): when set, the
  // bottom layer skips the dsts with omit_map[d] == omit_key
  const uint32_t* omit_map = nullptr;
  uint32_t omit_key = 0;
  const uint32_t* omit_loc = nullptr;  // cache rows; recorded in the layer's omit_row
  double all_time = 0;     // sampler wall time (reference `all_time`)
  uint64_t sampled_edges = 0;

  // GPU ctor (core/ntsFastSampler.hpp:125-176).  csr_layers: which hops need
  // the CSR transpose (backward); empty = all.
  FastSampler(std::shared_ptr<FullyRepGraph> g, const std::vector<VertexId>& index, int layers,
              int batch_size, const std::vector<int>& fanout, int pipeline_num = 1,
              std::vector<bool> csr_layers = {}, bool weights = true,
              bool merge_src_dst = false, bool edge_ids = false, int subgraph_walk = -1,
              uint64_t subgraph_edge_cap = 0);
  ~FastSampler();

  SampledSubgraph* sample_gpu_fast(int batch_size, int ssg_id, NtsStream& cs,
                                   WeightType w = WeightType::Sum);
  // Split form for pipelining (the reference overlaps with PIPELINE_NUM host
  // threads, toolkits/GCN_SAMPLE_GPU.hpp:289-394): issue enqueues every hop
  // and the size copy on `cs` without blocking; finish waits for that batch
  // and publishes v/e/src sizes.  A slot is reused only after its `consumed`
  // event (recorded by the trainer) — issue makes `cs` wait for it.
  void issue_gpu_sample(int batch_size, int ssg_id, NtsStream& cs, WeightType w);
  SampledSubgraph* finish_gpu_sample(int ssg_id);
  // The issue path with the layer-0 destinations in the caller's device
  // buffers (link prediction): `dest` int32 [>= hint] holds the
  // ids, v_size_dev[0] their live count, both produced by work enqueued on
  // `cs` before the call; v_cap_live_hint bounds that count (<= the sampler's
  // batch capacity).  finish_gpu_sample publishes the live count as layer 0's
  // v_size.  Philox and Philox-shared draws, weighted and coefficient draws as
  // issue_gpu_sample; refuses the MT19937 modes and omit_map.  sample_nids and
  // work_offset are neither read nor moved; batch_seq advances by one.
  void issue_gpu_sample_dev(const torch::Tensor& dest, const torch::Tensor& v_size_dev,
                            VertexId v_cap_live_hint, int ssg_id, NtsStream& cs, WeightType w);
  // MT19937 modes: a batch whose word stream fell short is sampled again
  // from its checkpoint with larger bounds (finish_gpu_sample does it; the
  // batches issued behind it are re-run too).  rerun_ok = false when work
  // chained to the sampled batches on the sampler stream (the driver's early
  // aggregation) would have to be re-done as well: then a short stream throws.
  bool rerun_ok = true;
  uint64_t mt_reruns = 0;  // batches re-run so far (tests)
  bool sample_not_finished() const { return work_offset < work_range[1]; }
  void restart() { work_offset = work_range[0]; }
  void set_sample_nids(const std::vector<VertexId>& ids);

  // load_feature_gpu / load_label_gpu (core/ntsFastSampler.hpp:244-261, 414-426)
  void load_feature_gpu(NtsStream& cs, SampledSubgraph* sg, NtsVar& local_feature,
                        const NtsVar& global_feature);
  void load_label_gpu(NtsStream& cs, SampledSubgraph* sg, NtsVar& local_label,
                      const NtsVar& global_label);
  // load_feature_gpu_cache (core/ntsFastSampler.hpp:263-317): cached rows from
  // HBM, the rest zero-copy from the pinned host table, in one kernel
  void load_feature_gpu_cache(NtsStream& cs, SampledSubgraph* sg, NtsVar& local_feature,
                              const FeatureCache& cache);
  // MT19937 modes: every later layer's word bound x scale (tests force a short
  // first stream with a small one; each re-run multiplies it by 4)
  void set_mt_budget_scale(NtsStream& cs, double scale);
  double mt_budget_scale() const { return mt_budget_; }

 private:
  struct IssueRec {  // one pending batch per slot: what a re-run needs
    VertexId offset = 0, actual = 0;
    uint64_t batch_seq = 0;
    int wt = 0;
    const uint32_t* omit_map = nullptr;
    uint32_t omit_key = 0;
    const uint32_t* omit_loc = nullptr;
    NtsStream* cs = nullptr;
    torch::Tensor mt_ckpt;  // device u32 [625]: the generator before the batch
    torch::Tensor dev_dest, dev_vsz;  // issue_gpu_sample_dev: the caller's layer-0 ids and count
  };
  std::vector<IssueRec> recs_;
  std::deque<int> issued_;  // slots issued and not yet finished, in issue order
  double mt_budget_ = 1.0;
  void enqueue_layers(int ssg_id, const IssueRec& r);
  void rerun_from(int ssg_id);
  torch::Tensor dev_nids_;  // device copy of sample_nids
  torch::Tensor dev_iota_;  // 0, 1, ..., batch_cap: device scalars for the layer-0 v_size
  int subgraph_walk_ = -1;  // >= 0: subgraph mode
  torch::Tensor dev_walkn_;             // k (1 + walk), k = 0..batch_cap: the walk set's live count
  std::vector<torch::Tensor> walk_;     // per slot: the walks' ids [batch_cap (1 + walk)]
  void enqueue_subgraph(int ssg_id, const IssueRec& r);
  VertexId batch_cap_ = 0;
};

// ---------------------------------------------------------------------------
// graph operators
// ---------------------------------------------------------------------------
// What a sampled graph op aggregates: the weighted sum (default) or the
// per-column maximum, alone or with the dst's own row beside it (root weight).
struct AggKind {
  bool max = false, root = false;
};
// The sampled forward aggregation of `kind` over layer `s`: y = A x, max x or
// [. | x[self rows]] on nts_hip_spmm_csc_fwd / _max / _root.  gather: x is the
// global table and rows go through the layer's `source` (self rows:
// `destination`), else x holds the layer's source rows (self rows:
// dst_local_id).  v_dev / v_rows: the device row count, or NULL and the exact
// one.  arg: the max kernel's winners (nullable).  early: the driver's launch
// behind the sampling (the error label says so).  A kFloat16 x is the f16
// feature table (gather, the plain sum): nts_hip_spmm_csc_fwd_h, y stays fp32.
void spmm_csc_fwd(NtsStream& cs, AggKind kind, const sampCSC* s, const NtsVar& x, bool gather,
                  const uint32_t* v_dev, uint32_t v_rows, NtsVar& y, uint32_t* arg = nullptr,
                  bool early = false);

namespace op {

class ntsGraphOp {
 public:
  virtual ~ntsGraphOp() = default;
  virtual NtsVar forward(NtsVar& f_input) = 0;
  virtual NtsVar forward(NtsVar& f_input, std::vector<VertexId> cacheflag) {
    (void)cacheflag;
    return forward(f_input);
  }
  virtual NtsVar backward(NtsVar& output_grad) = 0;
  bool output_requires_grad = true;
};

// SingleGPUAllSampleGraphOp (core/ntsSingleGPUSampleGraphOp.hpp:195-294):
// forward Y = A^T X over the sampled CSC (hand kernel instead of cuSPARSE);
// backward through the CSR transpose when the sampler built it
// (deterministic), otherwise the atomic CSC scatter (Push_From_Dst_To_Src).
// With `gather_from_table`, f_input is the global feature table and rows are
// fetched through the layer's `source` (fused load_feature_gpu + aggregate).
// `kind` (no reference counterpart) selects the GraphSAGE variants, all of
// them CSR-only in the backward:
//   root: Ycat = [A X | X[dst rows]] in one launch over a merged src/dst layer
//         (dst_local_id; with gather_from_table the self rows are the table's
//         `destination` rows); backward dX = A^T dYcat[:, :F] + dYcat[src_dst, F:]
//         over the CSR and the layer's inverse map.
//   max:  Y[d] = max over d's sampled edges of X[src] per column, in CSC edge
//         order (ties to the earliest edge), the winning edge kept in `arg`
//         where a backward follows; backward routes each dY[d, c] to the
//         source of that edge over the CSR and its csr_edge_id.
class SingleGPUAllSampleGraphOp : public ntsGraphOp {
 public:
  // feature_cache: with gather_from_table, rows come from the two-tier table
  // (HBM cache + host spill) instead of f_input (the plain sum only)
  SingleGPUAllSampleGraphOp(SampledSubgraph* subgraphs, FullyRepGraph* graph, int layer,
                            NtsStream* cs, bool gather_from_table = false,
                            const FeatureCache* feature_cache = nullptr, AggKind kind = {},
                            bool csr_only = false);
  NtsVar forward(NtsVar& f_input) override;
  NtsVar backward(NtsVar& f_output_grad) override;

  SampledSubgraph* subgraphs;
  int layer;
  NtsStream* cuda_stream;
  bool gather_from_table;
  const FeatureCache* feature_cache;
  AggKind kind;
  bool csr_only;      // SingleGPUSampleGraphOp: the backward refuses a layer without a CSR
  torch::Tensor arg;  // max: u32 [v_size, F], forward to backward
};

// SingleGPUSampleGraphOp (core/ntsSingleGPUSampleGraphOp.hpp:50-176): same
// forward; backward always through the CSR (row_offset/column_indices/e_w_b).
class SingleGPUSampleGraphOp : public SingleGPUAllSampleGraphOp {
 public:
  SingleGPUSampleGraphOp(SampledSubgraph* subgraphs, FullyRepGraph* graph, int layer,
                         NtsStream* cs, bool gather_from_table = false,
                         const FeatureCache* feature_cache = nullptr)
      : SingleGPUAllSampleGraphOp(subgraphs, graph, layer, cs, gather_from_table, feature_cache,
                                  AggKind{}, true) {}
};

}  // namespace op

// ---------------------------------------------------------------------------
// autodiff context (core/ntsContext.hpp)
// ---------------------------------------------------------------------------
namespace ctx {

enum OpType { NNOP = 0, GRAPHOP = 1 };

class NtsContext {
 public:
  NtsContext();
  ~NtsContext();

  template <typename GOPT, typename... Args>
  NtsVar runGraphOp(NtsVar& f_input, Args&&... args) {
    auto* curr = new GOPT(std::forward<Args>(args)...);
    // The bottom graph op's input never needs a gradient (its backward is
    // skipped, core/ntsContext.hpp:443-444); its output then needs none either,
    // which spares autograd the dense dY of the first GEMM.
    curr->output_requires_grad = !(training && count == 0);
    NtsVar f_output = curr->forward(f_input);
    push_graph_op(curr, f_input, f_output);
    return f_output;
  }
  NtsVar runVertexForward(const std::function<NtsVar(NtsVar&, NtsVar&)>& fn, NtsVar& nbr_input,
                          NtsVar& vtx_input);
  NtsVar runVertexForward(const std::function<NtsVar(NtsVar&)>& fn, NtsVar& nbr_input);
  void appendNNOp(NtsVar& input_t, NtsVar& output_t);
  void self_backward(bool retain_graph = true);
  void reset();
  void train() { training = true; }
  void eval() { training = false; }
  bool is_train() const { return training; }

  bool training = true;
  int count = 0;

 private:
  struct Entry {
    OpType type;
    op::ntsGraphOp* op;  // owned (GRAPHOP)
    NtsVar input, output, output_grad;
    void* in_id;
    void* out_id;
  };
  void push_graph_op(op::ntsGraphOp* op, NtsVar& in, NtsVar& out);
  void pop_one_op();
  std::vector<Entry> ops_;
};

}  // namespace ctx

// ---------------------------------------------------------------------------
// Parameter (core/NtsScheduler.hpp:680-1029), Adam via the fused HIP kernel.
// ---------------------------------------------------------------------------
// x.matmul(W) on the MFMA fp32 kernels (nts_hip_gemm_f32) with its own
// backward: dW = x^T dZ (split-reduction, deterministic), dx = dZ W^T.
NtsVar hip_linear(const NtsVar& x, const NtsVar& W, NtsStream* cs);
// one GAT layer (H = X W, attention softmax over each dst's sampled edges,
// relu(sum a H[src])) on a merged src/dst layer: [src_size, F_in] -> [v_size, F].
// heads > 1: W's F columns are `heads` heads of F / heads columns, each with
// its own softmax; the output is their concatenation [v_size, F], or with
// `mean` the mean over the heads [v_size, F / heads] (relu in both).
// GatDropout: p_attn drops the attention coefficients, p_out the
// layer's output, with the shared keep bits under key `seed` at the two
// offsets; both rates 0 (the default) run the plain entry points.
class KernelProfiler;
struct GatDropout {
  double p_attn = 0.0, p_out = 0.0;
  uint64_t seed = 0, off_attn = 0, off_out = 0;
  bool on() const { return p_attn > 0.0 || p_out > 0.0; }
};
NtsVar hip_gat_layer(const NtsVar& x, const NtsVar& W, const NtsVar& Watt, sampCSC* sg,
                     NtsStream* cs, KernelProfiler* prof = nullptr, int heads = 1,
                     bool mean = false, const GatDropout& drop = GatDropout());
// one GATv2 layer: W [F_in, 2F] = [W_s | W_d] stacked, att [F, 1];
// Hs = X W_s over the source rows, Hd = X[dst_local_id] W_d over the
// destination rows, score att_h . leaky_relu(Hs[src] + Hd[dst])_h per head,
// softmax over each dst's sampled edges, relu(sum a Hs[src]).  heads, mean and
// GatDropout as hip_gat_layer.
NtsVar hip_gatv2_layer(const NtsVar& x, const NtsVar& W, const NtsVar& att, sampCSC* sg,
                       NtsStream* cs, KernelProfiler* prof = nullptr, int heads = 1,
                       bool mean = false, const GatDropout& drop = GatDropout());
// plain inverted dropout with the shared keep bits (nts_hip_dropout_f32), no
// backward: the input pass of gat_feat_drop over untrained features
NtsVar hip_dropout(const NtsVar& x, double p, uint64_t seed, uint64_t offset, NtsStream* cs);
// CU masks splitting the device: `n` CUs spread evenly over the chip
// (every (total/n)-th CU) and the complement
std::vector<uint32_t> cu_mask_spread(int device, int n, bool complement);
// training output layer + loss: nll_loss(log_softmax(log_softmax(y W)), target)
// in two fused kernels (nts_hip_linear_xent_fwd/bwd); returns the scalar loss
// Persistent fp32 scalar 1 on `dev` (the loss-backward seed).
const NtsVar& unit_scalar(const torch::Device& dev);
bool hip_linear_xent_supported(int64_t K, int64_t C);
// correct != NULL: *correct += rows whose argmax is the target (getCorrect)
NtsVar hip_linear_xent(const NtsVar& y, const NtsVar& W, const NtsVar& target, NtsStream* cs,
                       uint32_t* correct = nullptr);
// Multi-label output layer + loss: binary_cross_entropy_with_logits(y W, T)
// (mean) in the fused kernels nts_hip_linear_bce_fwd/train.  label_bits: the
// packed targets of every vertex, int32 [V, wpr] (pack_label_bits); index:
// device ids of y's rows (the batch's seeds), n = y.size(0).  counts != NULL:
// counts[0..2] += tp, fp, fn of the prediction z > 0.
bool hip_linear_bce_supported(int64_t K, int64_t C);
NtsVar hip_linear_bce(const NtsVar& y, const NtsVar& W, const NtsVar& label_bits,
                      const VertexId* index, NtsStream* cs, uint32_t* counts = nullptr);
// [V, C] 0/1 labels (uint8, bool or int64) -> int32 [V, ceil(C / 32)]: label c
// is bit c & 31 of word c >> 5; and rows of that table back to float [n, C]
NtsVar pack_label_bits(const NtsVar& labels);
NtsVar unpack_label_bits(const NtsVar& words, int64_t C);
// row-major fp32 views the HIP GEMMs take without a copy (unit column stride)
NtsVar row_major(const NtsVar& x);
// [rows, F] with 128-byte aligned rows when F >= 64 (padded leading dimension)
NtsVar row_padded_empty(int64_t rows, int64_t F, int device);
// dropout(relu(x W), p) in one MFMA GEMM (activation in the epilogue, Philox
// mask of (seed, offset)); autograd: dW = x^T (dX ⊙ [X > 0] / (1-p)) fused.
// pair_split: narrow inputs (K <= 128, N 128 | 256) may use the in-kernel f16
// pair split (nts_hip_gemm_h2d_act) instead of the GEMM mode's kernel.
NtsVar hip_linear_act(const NtsVar& x, const NtsVar& W, double p, uint64_t seed, uint64_t offset,
                      NtsStream* cs, bool pair_split);

// Device time of selected kernels on the stream that launches them (HIP
// events; resolve() synchronises — call outside timed regions).  `units` are
// the algorithmic bytes (aggregations) or flops (GEMMs) of one launch.
// One kernel class per step is timed, rotating over the classes the driver
// has launched (next_step() per training step): each event pair costs the
// training stream ~4-5 us of gap, so timing every class every step added ~36
// us to a 0.9 ms step; a quarter of the launches of each class is the sample.
class KernelProfiler {
 public:
  enum Id { BOTTOM_AGG = 0, GATHER_GEMM, GATHER_GEMM_TN, BOTTOM_BWD, GAT_FWD, kCount };
  struct Stat {
    double ms = 0, units = 0;
    uint64_t calls = 0;
  };
  KernelProfiler() { for (int& o : open_) o = -1; }
  ~KernelProfiler();
  KernelProfiler(const KernelProfiler&) = delete;
  KernelProfiler& operator=(const KernelProfiler&) = delete;
  void begin(Id id, hipStream_t st);
  void end(Id id, hipStream_t st, double units);
  void resolve();
  void reset();
  void add_units(Id id, double units) {
    if (active(id)) stat[id].units += units;
  }
  // a new step: its timed class is the (step % #seen)-th of the classes seen
  // in the steps before it, frozen for the whole step (a class
  // first seen mid-step no longer changes the choice between begin, add_units
  // and end of one step); before any class was seen, the step's first caller
  void next_step() {
    ++step_;
    sel_ = -1;
    if (seen_) {
      uint32_t m = seen_;
      for (int k = (int)(step_ % (uint64_t)__builtin_popcount(seen_)); k > 0; --k) m &= m - 1;
      sel_ = __builtin_ctz(m);
    }
  }
  static const char* name(int id);
  Stat stat[kCount];

 private:
  bool active(Id id) {
    seen_ |= 1u << id;
    if (sel_ < 0) sel_ = (int)id;
    return sel_ == (int)id;
  }
  uint32_t seen_ = 0;
  uint64_t step_ = 0;
  int sel_ = -1;  // this step's timed class
  struct Slot {
    Id id = BOTTOM_AGG;
    hipEvent_t a = nullptr, b = nullptr;
    double units = 0;
  };
  std::vector<Slot> pool_;
  size_t used_ = 0;
  int open_[kCount];
};

// dropout(relu(x), p) as its own autograd op (the GEMM epilogue's mask keys)
NtsVar hip_relu_dropout(const NtsVar& x, double p, uint64_t seed, uint64_t offset, NtsStream* cs);
// dropout(relu(LayerNorm(z; gamma, beta, eps)), p) as one autograd op
// (nts_hip_ln_act_fwd / _bwd, the same mask keys): gradients for z, gamma [F]
// and beta [F]; saves z, y, mean, rstd and gamma when a backward can follow,
// nothing otherwise (eval / inference)
NtsVar hip_ln_act(const NtsVar& z, const NtsVar& gamma, const NtsVar& beta, double eps, double p,
                  uint64_t seed, uint64_t offset, NtsStream* cs);
// dropout(relu(BatchNorm(z; gamma, beta, eps)), p) as one autograd op
// (nts_hip_bn_act_*, the same mask keys).  train: the batch's statistics, the
// running buffers [F] updated in place by `momentum`, and z, y, mean, rstd and
// gamma saved for the backward (gradients for z, gamma and beta).  Otherwise
// the eval kernel on the running buffers: no dropout, nothing saved or updated.
NtsVar hip_bn_act(const NtsVar& z, const NtsVar& gamma, const NtsVar& beta,
                  const NtsVar& running_mean, const NtsVar& running_var, bool train, double eps,
                  double momentum, double p, uint64_t seed, uint64_t offset, NtsStream* cs);

// Transform-first bottom layer (nts_hip.h): X1 = dropout(relu(A (X[source] W)))
// on the layer's sampled block `sg` (its CSR is needed for the backward);
// autograd returns dW = X[source]^T (A^T (dX1 ⊙ mask)).  h_out != NULL: H =
// X[source] W is written there ([src_size, F_out], eval / tests).
// pairs != NULL: the table's f16 pair table (nts_hip_h2_split_rows, built once
// by the driver) — the forward GEMM runs on it, and the weight-gradient GEMM
// too when pairs->tn.
struct PairTable {
  NtsVar P;   // int32 [V, Kp] pair words
  NtsVar rs;  // fp32 [V] row scales
  bool tn = true;
  NtsVar Q;   // int16 [V, 2 Kp] planar form (defined: the weight gradient on k_h2_tn3)
  // the tables as the C-ABI takes them, and Kp of the one that is there
  const uint16_t* q_ptr() const { return reinterpret_cast<const uint16_t*>(Q.data_ptr<int16_t>()); }
  const uint32_t* p_ptr() const { return reinterpret_cast<const uint32_t*>(P.data_ptr<int32_t>()); }
  int kp() const { return (int)(Q.defined() ? Q.size(1) / 2 : P.size(1)); }
};
// Stream-phase hooks of the transform-first bottom layer (the driver's
// sampler gating, GCNConfig::sampler_gate): called on the host right after
// the forward gather GEMM is enqueued, and right before the backward one.
void set_bottom_gemm_hooks(std::function<void()> after_fwd_gemm,
                           std::function<void()> before_bwd_gemm);
NtsVar hip_bottom_transform(const NtsVar& table, const NtsVar& W, sampCSC* sg, double p,
                            uint64_t seed, uint64_t offset, NtsStream* cs, KernelProfiler* prof,
                            float* h_out = nullptr, const PairTable* pairs = nullptr);

// Link-prediction loss (nts_hip_lp_bce_fwd / _train): the mean
// sigmoid BCE of the dot-product scores of h's rows over the pairs of a batch
// built by nts_hip_lp_batch.  h [rows, D] holds one row per distinct endpoint
// (rows == the batch's live v_size).  Under grad mode with h requiring grad the
// training entry runs and autograd returns its gathered dH.  score [P] receives
// the scores; mrr != NULL: the device counter pair of nts_hip_lp_bce_fwd.
struct LpPairs {
  const uint32_t *pair_u, *pair_v, *inc_offset, *inc_slot, *v_size;
  uint32_t B, K;
};
NtsVar hip_lp_bce(const NtsVar& h, const LpPairs& pairs, NtsVar& score, NtsStream* cs,
                  float* mrr = nullptr);

struct Parameter {
  NtsVar W, M, V;
  NtsStream* cs = nullptr;  // set -> forward runs on the hand-written MFMA GEMM
  int row, col;
  ValueType alpha, beta1, beta2, epsilon, weight_decay;
  ValueType beta1_t, beta2_t;
  int curr_epoch = 0;
  Parameter(size_t w, size_t h, ValueType alpha, ValueType beta1, ValueType beta2,
            ValueType epsilon, ValueType weight_decay, int device, int64_t init_seed);
  NtsVar forward(const NtsVar& x) const { return cs ? hip_linear(x, W, cs) : x.matmul(W); }
  // Parameter::learnC2C_with_decay_Adam (bias-corrected, CPU driver semantics)
  void learnC2C_with_decay_Adam(NtsStream& cs);
  // Parameter::learn_local_with_decay_Adam (GPU drivers, no bias correction)
  void learn_local_with_decay_Adam(NtsStream& cs);
  // either variant with the gradient taken from `grad` (a reduced bucket slice)
  void adam_from(NtsStream& cs, const float* grad, bool bias_correction);
  void next();
  void zero_grad();
};

// RCCL communicator (NCCL_Communicator replacement) — one per process.
// Host transport for the same two collectives (tests and the one-GPU
// rehearsal of the multi-rank path): called with a tensor viewing the device
// buffer after its stream is synchronised; op 0 = SUM all-reduce in place,
// op 1 = broadcast from `root`.  The result must be in the buffer when it
// returns.
using HostCollective = std::function<void(torch::Tensor, int op, int root)>;

class Communicator {
 public:
  Communicator(int nranks, int rank, const std::vector<uint8_t>& uid, int device);
  Communicator(int nranks, int rank, HostCollective host);
  ~Communicator();
  void allreduce_sum(float* buf, uint64_t n, void* stream);
  void broadcast(float* buf, uint64_t n, int root, void* stream);
  static std::vector<uint8_t> unique_id();
  bool host_transport() const { return (bool)host_; }
  // (ranks, this rank) as RCCL reports them (ncclCommCount / ncclCommUserRank);
  // (-1, -1) for the host transport
  std::pair<int, int> rccl_count() const;
  int nranks, rank;
  // Per-call timing of allreduce_sum (bench.py's allreduce_us_per_step):
  // RCCL — a HIP event pair (no system fence) around the call on the stream it
  // is enqueued on; host transport — the host wall time of the blocking call.
  // timing_stats() synchronises the events: call outside timed regions.
  void set_timing(bool on) { timing_ = on; }
  void timing_reset();
  // (mean microseconds per call, calls, "hip-events" | "host-wall")
  std::tuple<double, uint64_t, std::string> timing_stats();

 private:
  void host_call(float* buf, uint64_t n, void* stream, int op, int root);
  nts_hip_comm* comm_ = nullptr;
  HostCollective host_;
  bool timing_ = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> tev_;
  size_t tused_ = 0;
  double host_us_ = 0;
  uint64_t host_calls_ = 0;
};

}  // namespace nts
