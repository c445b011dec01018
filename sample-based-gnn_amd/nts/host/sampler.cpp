// C++ host layer, sampler side: the replicated graph, sampled layers, the GPU
// sampler, the two-tier feature cache and the feature / label loads.
#include <algorithm>
#include <cstring>

#include "ops_util.hpp"

namespace nts {

// ---------------------------------------------------------------------------
// The sampling weights of a graph, checked once at load: float32 [E] on the
// graph's device, every value finite and in [2^-60, 2^60] (the range keeps
// every selection key a normal positive float).  The check runs on
// the device and is read once; `name` is the caller's argument.
static torch::Tensor checked_edge_prob(const torch::Tensor& w, uint64_t edges, int device,
                                       const char* name) {
  TORCH_CHECK(w.is_cuda() && w.device().index() == device && w.dtype() == torch::kFloat32 &&
                  w.dim() == 1 && (uint64_t)w.numel() == edges,
              name, ": a float32 CUDA tensor with one value per edge (", edges, "), got ",
              w.numel(), " value(s) of ", w.dtype());
  auto p = w.contiguous();
  if (edges == 0) return p;
  const float lo = 0x1p-60f, hi = 0x1p60f;
  // (a NaN fails both comparisons; +-inf fail one of them)
  const auto bad = torch::logical_not(torch::logical_and(p >= lo, p <= hi));
  const auto first = bad.to(torch::kInt32).argmax();
  const auto rep = torch::stack({bad.sum().to(torch::kFloat64), first.to(torch::kFloat64),
                                 p.index_select(0, first.reshape({1}))[0].to(torch::kFloat64)})
                       .cpu();
  const int64_t n = (int64_t)rep[0].item<double>();
  TORCH_CHECK(n == 0, name, ": ", n, " value(s) are not finite and in [2^-60, 2^60] (zero, "
              "negative, NaN, inf and out-of-range weights are refused); the first is edge ",
              (int64_t)rep[1].item<double>(), " with value ", rep[2].item<double>());
  return p;
}

std::shared_ptr<FullyRepGraph> FullyRepGraph::from_edges(NtsStream& cs, const torch::Tensor& src,
                                                         const torch::Tensor& dst,
                                                         VertexId vertices,
                                                         const torch::Tensor& edge_weight) {
  TORCH_CHECK(src.is_cuda() && dst.is_cuda() && src.dtype() == torch::kInt32 &&
                  dst.dtype() == torch::kInt32 && src.numel() == dst.numel(),
              "from_edges: src/dst must be int32 CUDA tensors of equal length");
  hip_rt(hipDeviceSynchronize(), "hipDeviceSynchronize");  // inputs may come from any stream
  auto guard = cs.guard();
  auto g = std::make_shared<FullyRepGraph>();
  g->device = cs.device();
  g->global_vertices = vertices;
  g->global_edges = (uint64_t)src.numel();
  auto s = src.contiguous(), d = dst.contiguous();
  g->column_offset = torch::empty({(int64_t)vertices + 1},
                                  torch::TensorOptions().dtype(torch::kInt64).device(torch::kCUDA, g->device));
  g->row_indices = torch::empty({(int64_t)std::max<uint64_t>(g->global_edges, 1)}, u32_opts(g->device));
  g->in_degree = torch::empty({(int64_t)vertices}, u32_opts(g->device));
  g->out_degree = torch::empty({(int64_t)vertices}, u32_opts(g->device));
  NTS_CALL(nts_hip_build_csc, cs.ctx(), dptr<uint32_t>(s), dptr<uint32_t>(d), g->global_edges,
           vertices, dptr<uint64_t>(g->column_offset), dptr<uint32_t>(g->row_indices));
  NTS_CALL(nts_hip_degrees, cs.ctx(), dptr<uint32_t>(s), dptr<uint32_t>(d), g->global_edges,
           vertices, dptr<uint32_t>(g->out_degree), dptr<uint32_t>(g->in_degree));
  if (edge_weight.defined()) {
    // file edge i -> its CSC position: nts_hip_build_csc keeps the file order
    // within a destination, which is the stable order by destination (load
    // time: a libtorch sort is enough)
    const auto w = checked_edge_prob(edge_weight, g->global_edges, g->device, "edge_weight");
    const auto key = d.to(torch::kInt64).bitwise_and(0xFFFFFFFFll);  // ids are uint32
    g->edge_prob = w.index_select(0, torch::argsort(key, /*stable=*/true, 0, false));
  }
  cs.synchronize();
  return g;
}

std::shared_ptr<FullyRepGraph> FullyRepGraph::from_csc(torch::Tensor column_offset,
                                                       torch::Tensor row_indices,
                                                       torch::Tensor in_degree,
                                                       torch::Tensor out_degree,
                                                       torch::Tensor edge_prob) {
  auto g = std::make_shared<FullyRepGraph>();
  TORCH_CHECK(column_offset.dtype() == torch::kInt64 && row_indices.dtype() == torch::kInt32,
              "from_csc: column_offset int64, row_indices int32");
  g->device = column_offset.device().index();
  g->global_vertices = (VertexId)(column_offset.numel() - 1);
  g->global_edges = (uint64_t)row_indices.numel();
  g->column_offset = column_offset.contiguous();
  g->row_indices = row_indices.contiguous();
  g->in_degree = in_degree.contiguous();
  g->out_degree = out_degree.contiguous();
  if (edge_prob.defined())
    g->edge_prob = checked_edge_prob(edge_prob, g->global_edges, g->device, "edge_prob");
  return g;
}

nts_graph_dev FullyRepGraph::dev() const {
  nts_graph_dev d;
  d.n_vertices = global_vertices;
  d.n_edges = global_edges;
  d.column_offset = dptr<uint64_t>(column_offset);
  d.row_indices = dptr<uint32_t>(row_indices);
  d.in_degree = dptr<uint32_t>(in_degree);
  d.out_degree = dptr<uint32_t>(out_degree);
  return d;
}

// ---------------------------------------------------------------------------
void sampCSC::set_merge_src_dst() {
  dst_local_id = torch::empty({std::max<int64_t>(v_cap, 1)}, u32_opts(column_offset.device().index()));
  if (has_csr)
    csr_edge_id = torch::empty({std::max<int64_t>(e_cap, 1)}, u32_opts(column_offset.device().index()));
}

void sampCSC::set_edge_ids() {
  if (has_csr && !csr_edge_id.defined())
    csr_edge_id = torch::empty({std::max<int64_t>(e_cap, 1)}, u32_opts(column_offset.device().index()));
}

sampCSC::sampCSC(int device, VertexId vc, VertexId ec, VertexId sc, bool csr, bool weights)
    : v_cap(vc), e_cap(ec), s_cap(sc), has_csr(csr) {
  auto U = u32_opts(device);
  auto F = f32_opts(device);
  const int64_t e1 = std::max<int64_t>(ec, 1), s1 = std::max<int64_t>(sc, 1);
  column_offset = torch::empty({(int64_t)vc + 1}, U);
  row_indices = torch::empty({e1}, U);
  sample_ans = torch::empty({e1}, U);
  edge_dst = torch::empty({e1}, U);
  source = torch::empty({s1}, U);
  sizes = torch::zeros({4}, U);
  if (weights) edge_weight_forward = torch::empty({e1}, F);
  if (csr) {
    row_offset = torch::empty({(int64_t)sc + 1}, U);
    column_indices = torch::empty({e1}, U);
    if (weights) edge_weight_backward = torch::empty({e1}, F);
  }
}

std::vector<VertexId> sampCSC::host_u32(const torch::Tensor& t, size_t n) const {
  auto c = t.narrow(0, 0, (int64_t)n).cpu();
  std::vector<VertexId> out(n);
  if (n) std::memcpy(out.data(), c.data_ptr(), n * 4);
  return out;
}

static std::vector<std::array<uint64_t, 3>> layer_caps(VertexId batch,
                                                       const std::vector<int>& fanout,
                                                       VertexId V, uint64_t E, bool merge,
                                                       int subgraph_walk = -1,
                                                       uint64_t subgraph_edge_cap = 0) {
  std::vector<std::array<uint64_t, 3>> caps;
  if (subgraph_walk >= 0) {
    // one vertex set per batch: the seeds and `walk` steps from each; every
    // block holds at most e_cap of the graph's edges (the default's factor 4
    // over the mean degree is a guess)
    const uint64_t s = std::min<uint64_t>((uint64_t)batch * (1 + (uint64_t)subgraph_walk), V);
    const uint64_t mean_deg = V ? (E + V - 1) / V : 0;
    const uint64_t e = subgraph_edge_cap ? std::min<uint64_t>(subgraph_edge_cap, E)
                                         : std::min<uint64_t>(E, s * 4 * mean_deg);
    TORCH_CHECK(e <= 0xFFFFFFFFull, "sampled layer exceeds 2^32 edges");
    for (size_t l = 0; l < fanout.size(); ++l) caps.push_back({l == 0 ? (uint64_t)batch : s, e, s});
    return caps;
  }
  uint64_t v = batch;
  for (int f : fanout) {
    uint64_t e = f < 0 ? E : std::min<uint64_t>(v * (uint64_t)f, E);
    uint64_t s = std::min<uint64_t>(e + (merge ? v : 0), V);
    TORCH_CHECK(e <= 0xFFFFFFFFull, "sampled layer exceeds 2^32 edges");
    caps.push_back({v, e, s});
    v = s;
  }
  return caps;
}

SampledSubgraph::SampledSubgraph(int device, int layers_, const std::vector<int>& fanout_,
                                 VertexId batch, VertexId vertices, uint64_t edges,
                                 const std::vector<bool>& csr, bool weights, bool merge,
                                 bool edge_ids, int subgraph_walk, uint64_t subgraph_edge_cap)
    : layers(layers_), fanout(fanout_) {
  auto caps = layer_caps(batch, fanout, vertices, edges, merge, subgraph_walk, subgraph_edge_cap);
  for (int l = 0; l < layers; ++l) {
    bool c = csr.empty() ? true : (bool)csr[l];
    sampled_sgs.push_back(new sampCSC(device, (VertexId)caps[l][0], (VertexId)caps[l][1],
                                      (VertexId)caps[l][2], c, weights));
    if (merge) sampled_sgs.back()->set_merge_src_dst();
    if (edge_ids) sampled_sgs.back()->set_edge_ids();
  }
  // every layer's sizes[4] as a view of one device array: one D2H per batch
  dev_sizes = torch::zeros({std::max(layers, 1) * 4}, u32_opts(device));
  for (int l = 0; l < layers; ++l) sampled_sgs[l]->sizes = dev_sizes.narrow(0, 4 * l, 4);
  void* hs = nullptr;
  hip_rt(hipHostMalloc(&hs, 16 * (size_t)std::max(layers, 1), hipHostMallocMapped | hipHostMallocCoherent),
         "hipHostMalloc(sizes)");
  host_sizes = static_cast<int32_t*>(hs);
  std::fill(host_sizes, host_sizes + 4 * std::max(layers, 1), 0);
  void* hd = nullptr;
  hip_rt(hipHostGetDevicePointer(&hd, hs, 0), "hipHostGetDevicePointer(sizes)");
  host_sizes_dev = static_cast<uint32_t*>(hd);
  hip_rt(hipEventCreateWithFlags(&sampled, hipEventDisableTiming), "hipEventCreate");
  hip_rt(hipEventCreateWithFlags(&consumed, hipEventDisableTiming), "hipEventCreate");
}

SampledSubgraph::~SampledSubgraph() {
  for (auto* s : sampled_sgs) delete s;
  (void)hipHostFree(host_sizes);
  (void)hipEventDestroy(sampled);
  (void)hipEventDestroy(consumed);
}

// ---------------------------------------------------------------------------
FastSampler::FastSampler(std::shared_ptr<FullyRepGraph> g, const std::vector<VertexId>& index,
                         int layers, int batch_size, const std::vector<int>& fanout_,
                         int pipeline_num, std::vector<bool> csr_layers, bool weights,
                         bool merge_src_dst, bool edge_ids, int subgraph_walk,
                         uint64_t subgraph_edge_cap)
    : whole_graph(g), layer(layers), fanout(fanout_), batch_cap_((VertexId)batch_size),
      subgraph_walk_(subgraph_walk) {
  TORCH_CHECK((int)fanout.size() == layers, "fanout size != layers");
  if (pipeline_num < 1) pipeline_num = 1;
  if (subgraph_walk_ >= 0)
    for (int f : fanout)
      TORCH_CHECK(f == -1, "subgraph mode needs every fanout = -1 (all induced neighbours)");
  for (int i = 0; i < pipeline_num; ++i)
    ssgs.push_back(new SampledSubgraph(g->device, layers, fanout, batch_cap_, g->global_vertices,
                                       g->global_edges, csr_layers, weights, merge_src_dst,
                                       edge_ids, subgraph_walk, subgraph_edge_cap));
  if (subgraph_walk_ > 0) {  // (walk 0: the set is the seeds themselves, no walk buffer)
    const int64_t w1 = 1 + (int64_t)subgraph_walk_;
    dev_walkn_ = torch::arange((int64_t)batch_cap_ + 1, u32_opts(g->device)) * w1;
    for (int i = 0; i < pipeline_num; ++i)
      walk_.push_back(torch::empty({std::max<int64_t>((int64_t)batch_cap_ * w1, 1)},
                                   u32_opts(g->device)));
  }
  ssg = ssgs[0];
  recs_.resize(ssgs.size());
  set_sample_nids(index);
  dev_iota_ = torch::arange((int64_t)batch_cap_ + 1, u32_opts(g->device));
}

FastSampler::~FastSampler() {
  for (auto* s : ssgs) delete s;
}

void FastSampler::set_sample_nids(const std::vector<VertexId>& ids) {
  sample_nids = ids;
  work_range[0] = 0;
  work_range[1] = (VertexId)sample_nids.size();
  work_offset = 0;
  dev_nids_ = torch::empty({(int64_t)std::max<size_t>(ids.size(), 1)}, u32_opts(whole_graph->device));
  if (!ids.empty()) {
    auto h = torch::from_blob((void*)sample_nids.data(), {(int64_t)ids.size()}, torch::kInt32);
    dev_nids_.narrow(0, 0, (int64_t)ids.size()).copy_(h);
  }
}

SampledSubgraph* FastSampler::sample_gpu_fast(int batch_size, int ssg_id, NtsStream& cs,
                                              WeightType w) {
  issue_gpu_sample(batch_size, ssg_id, cs, w);
  return finish_gpu_sample(ssg_id);
}

void FastSampler::issue_gpu_sample(int batch_size, int ssg_id, NtsStream& cs, WeightType w) {
  double t0 = now_s();
  TORCH_CHECK(work_offset < work_range[1], "sample_gpu_fast: no work left");
  TORCH_CHECK((VertexId)batch_size <= batch_cap_, "batch larger than the sampler's capacity");
  TORCH_CHECK(ssg_id >= 0 && ssg_id < (int)ssgs.size(), "ssg_id out of range");
  ssg = ssgs[ssg_id];
  const VertexId actual = std::min<VertexId>((VertexId)batch_size, work_range[1] - work_offset);
  hipStream_t st = (hipStream_t)cs.stream();
  // The slot's previous batch must be trained before it is overwritten.  With
  // several slots (pipelined sampler on its own stream) wait for that on the
  // host: ROCm blocks every kernel launch on a stream whose queue waits on an
  // unfinished event of another stream (~60 us each here), which would stall
  // the whole issue loop; the event is normally complete already.
  if (ssgs.size() > 1) hip_rt(hipEventSynchronize(ssg->consumed), "hipEventSynchronize");
  hip_rt(hipStreamWaitEvent(st, ssg->consumed, 0), "hipStreamWaitEvent");
  int wt = w == WeightType::Sum           ? NTS_WEIGHT_SUM
           : w == WeightType::Mean        ? NTS_WEIGHT_MEAN
           : w == WeightType::MeanSampled ? NTS_WEIGHT_MEAN_SAMPLED
                                          : NTS_WEIGHT_NONE;
  if (up_degree && wt != NTS_WEIGHT_NONE) wt |= NTS_WEIGHT_UP_DEGREE;
  // what a re-run of this batch needs (MT19937 modes: a short word stream)
  IssueRec& r = recs_[ssg_id];
  r.offset = work_offset;
  r.actual = actual;
  r.batch_seq = batch_seq;
  r.wt = wt;
  r.omit_map = omit_map;
  r.omit_key = omit_key;
  r.omit_loc = omit_loc;
  r.cs = &cs;
  if (is_mt_mode(rng_mode)) {
    if (!r.mt_ckpt.defined())
      r.mt_ckpt = torch::empty({625}, u32_opts(whole_graph->device));
    // the generator state before the batch's first layer (stream order)
    NTS_CALL(nts_hip_mt_checkpoint, cs.ctx(), dptr<uint32_t>(r.mt_ckpt));
  }
  TORCH_CHECK(subgraph_walk_ < 0 || (rng_mode == NTS_RNG_PHILOX && !weighted && !coef && !omit_map),
              "subgraph mode draws its walks from a Philox stream of its own and selects nothing: "
              "rng_mode NTS_RNG_PHILOX without weighted, coef or omit_map");
  issued_.push_back(ssg_id);
  enqueue_layers(ssg_id, r);
  if (host_profile()) fprintf(stderr, "[host] issue total: %.1f us\n", (now_s() - t0) * 1e6);
  ssg->pending_batch = (int)actual;
  work_offset += actual;
  ++batch_seq;
  all_time += now_s() - t0;
}

// The same issue with the layer-0 destinations taken from the caller's device
// buffers: `dest` holds the ids and *v_size_dev their count, both written by
// work already enqueued on `cs` (a link-prediction batch's distinct endpoints,
// nts_hip_lp_batch).  Nothing of sample_nids / work_offset is read or moved.
void FastSampler::issue_gpu_sample_dev(const torch::Tensor& dest, const torch::Tensor& v_size_dev,
                                       VertexId v_cap_live_hint, int ssg_id, NtsStream& cs,
                                       WeightType w) {
  double t0 = now_s();
  TORCH_CHECK(!is_mt_mode(rng_mode), "issue_gpu_sample_dev: the MT19937 modes replay a host-ordered "
              "stream (Philox and Philox-shared only)");
  TORCH_CHECK(!omit_map, "issue_gpu_sample_dev is not supported with omit_map");
  TORCH_CHECK(subgraph_walk_ < 0, "issue_gpu_sample_dev is not supported in subgraph mode");
  TORCH_CHECK(ssg_id >= 0 && ssg_id < (int)ssgs.size(), "ssg_id out of range");
  TORCH_CHECK(dest.defined() && dest.is_cuda() && dest.scalar_type() == torch::kInt32 &&
                  dest.is_contiguous() && v_size_dev.defined() && v_size_dev.is_cuda() &&
                  v_size_dev.scalar_type() == torch::kInt32 && v_size_dev.numel() >= 1,
              "issue_gpu_sample_dev: dest and v_size must be int32 device tensors");
  TORCH_CHECK(v_cap_live_hint >= 1 && v_cap_live_hint <= batch_cap_ &&
                  (int64_t)v_cap_live_hint <= dest.numel(),
              "issue_gpu_sample_dev: the destination bound must be in 1..min(capacity, dest size)");
  ssg = ssgs[ssg_id];
  hipStream_t st = (hipStream_t)cs.stream();
  if (ssgs.size() > 1) hip_rt(hipEventSynchronize(ssg->consumed), "hipEventSynchronize");
  hip_rt(hipStreamWaitEvent(st, ssg->consumed, 0), "hipStreamWaitEvent");
  int wt = w == WeightType::Sum           ? NTS_WEIGHT_SUM
           : w == WeightType::Mean        ? NTS_WEIGHT_MEAN
           : w == WeightType::MeanSampled ? NTS_WEIGHT_MEAN_SAMPLED
                                          : NTS_WEIGHT_NONE;
  if (up_degree && wt != NTS_WEIGHT_NONE) wt |= NTS_WEIGHT_UP_DEGREE;
  IssueRec& r = recs_[ssg_id];
  r.offset = 0;
  r.actual = v_cap_live_hint;
  r.batch_seq = batch_seq;
  r.wt = wt;
  r.omit_map = nullptr;
  r.omit_key = 0;
  r.omit_loc = nullptr;
  r.cs = &cs;
  r.dev_dest = dest;
  r.dev_vsz = v_size_dev;
  issued_.push_back(ssg_id);
  enqueue_layers(ssg_id, r);
  r.dev_dest = torch::Tensor();  // (the layer keeps its own view; nothing re-runs a Philox batch)
  r.dev_vsz = torch::Tensor();
  ssg->pending_batch = (int)v_cap_live_hint;
  ++batch_seq;
  all_time += now_s() - t0;
}

// the batch's sampling kernels (every layer) on the record's stream
void FastSampler::enqueue_layers(int ssg_id, const IssueRec& r) {
  if (subgraph_walk_ >= 0) return enqueue_subgraph(ssg_id, r);
  ssg = ssgs[ssg_id];
  NtsStream& cs = *r.cs;
  hipStream_t st = (hipStream_t)cs.stream();
  const nts_graph_dev g = whole_graph->dev();
  const int wt = r.wt;
  const VertexId actual = r.actual;
  const uint64_t bseq = r.batch_seq;
  const bool from_dev = r.dev_dest.defined();  // issue_gpu_sample_dev
  const VertexId* dst = from_dev ? dptr<VertexId>(r.dev_dest) : dptr<VertexId>(dev_nids_) + r.offset;
  sampCSC* s0 = ssg->sampled_sgs[0];
  // layer-0 v_size as a device scalar without a per-batch memset: entry
  // `actual` of the device table 0..batch_cap
  (void)s0;
  const VertexId* vsz = from_dev ? dptr<VertexId>(r.dev_vsz) : dptr<VertexId>(dev_iota_) + actual;
  for (int l = 0; l < layer; ++l) {
    sampCSC* s = ssg->sampled_sgs[l];
    nts_sampcsc_dev o{};
    o.v_cap = s->v_cap;
    o.e_cap = s->e_cap;
    o.s_cap = s->s_cap;
    o.destination = dst;
    o.v_size = vsz;
    o.column_offset = dptr<uint32_t>(s->column_offset);
    o.row_indices = dptr<uint32_t>(s->row_indices);
    o.sample_ans = dptr<uint32_t>(s->sample_ans);
    o.edge_dst = dptr<uint32_t>(s->edge_dst);
    o.source = dptr<uint32_t>(s->source);
    o.edge_weight_forward =
        wt == NTS_WEIGHT_NONE && !coef ? nullptr : dptr<float>(s->edge_weight_forward);
    o.row_offset = s->has_csr ? dptr<uint32_t>(s->row_offset) : nullptr;
    o.column_indices = s->has_csr ? dptr<uint32_t>(s->column_indices) : nullptr;
    o.edge_weight_backward =
        (s->has_csr && (wt != NTS_WEIGHT_NONE || coef)) ? dptr<float>(s->edge_weight_backward)
                                                        : nullptr;
    o.sizes = dptr<uint32_t>(s->sizes);
    o.dst_local_id = dptr<uint32_t>(s->dst_local_id);  // undefined (NULL) unless merged
    o.csr_edge_id = dptr<uint32_t>(s->csr_edge_id);
    o.sizes_host = ssg->host_sizes_dev + 4 * l;
    if (l == layer - 1 && r.omit_map) {
      if (!s->omit_row.defined())
        s->omit_row = torch::empty({std::max<int64_t>(s->v_cap, 1)}, u32_opts(whole_graph->device));
      o.omit_map = r.omit_map;
      o.omit_key = r.omit_key;
      o.omit_loc = r.omit_loc;
      o.omit_row = dptr<uint32_t>(s->omit_row);
    }
    const double tl = now_s();
    if (coef)
      NTS_CALL(nts_hip_sample_layer_coef, cs.ctx(), &g,
               weighted ? dptr<float>(whole_graph->edge_prob) : nullptr,
               dptr<float>(whole_graph->edge_prob), fanout[l], l, bseq, rng_mode, wt, &o);
    else if (weighted)
      NTS_CALL(nts_hip_sample_layer_weighted, cs.ctx(), &g, dptr<float>(whole_graph->edge_prob),
               fanout[l], l, bseq, wt, &o);
    else
      NTS_CALL(nts_hip_sample_layer, cs.ctx(), &g, fanout[l], l, bseq, rng_mode, wt, &o);
    if (host_profile()) fprintf(stderr, "[host] sample_layer %d: %.1f us\n", l, (now_s() - tl) * 1e6);
    // the reference keeps the destination as a view of the previous source
    if (l == 0)
      s->destination = from_dev ? r.dev_dest
                                : dev_nids_.narrow(0, r.offset, std::max<int64_t>(actual, 0));
    else
      s->destination = ssg->sampled_sgs[l - 1]->source;
    dst = o.source;
    vsz = o.sizes + 2;
  }
  // the layers' sizes reach host_sizes from their last kernels (the reference
  // syncs twice per layer; a D2H copy here cost a blit kernel per batch)
  hip_rt(hipEventRecord(ssg->sampled, st), "hipEventRecord");
}

// Subgraph mode: the batch's vertex set S (the seeds, and the walks from them)
// and the blocks it induces, every kernel on the record's stream.  Layer 0:
// destinations the seeds, set = the walks' ids (duplicates and all); layers
// >= 1: destinations and set both the previous layer's source, which is S.
void FastSampler::enqueue_subgraph(int ssg_id, const IssueRec& r) {
  ssg = ssgs[ssg_id];
  NtsStream& cs = *r.cs;
  hipStream_t st = (hipStream_t)cs.stream();
  const nts_graph_dev g = whole_graph->dev();
  const VertexId actual = r.actual;
  const VertexId* dst = dptr<VertexId>(dev_nids_) + r.offset;
  const VertexId* vsz = dptr<VertexId>(dev_iota_) + actual;
  const VertexId* set = dst;
  const VertexId* set_n = vsz;
  uint32_t set_cap = batch_cap_;
  if (subgraph_walk_ > 0) {
    VertexId* w = dptr<VertexId>(walk_[ssg_id]);
    NTS_CALL(nts_hip_random_walk, cs.ctx(), &g, dst, vsz, batch_cap_, subgraph_walk_, r.batch_seq, w);
    set = w;
    set_n = dptr<VertexId>(dev_walkn_) + actual;
    set_cap = (uint32_t)walk_[ssg_id].numel();
  }
  for (int l = 0; l < layer; ++l) {
    sampCSC* s = ssg->sampled_sgs[l];
    nts_sampcsc_dev o{};
    o.v_cap = s->v_cap;
    o.e_cap = s->e_cap;
    o.s_cap = s->s_cap;
    o.destination = dst;
    o.v_size = vsz;
    o.column_offset = dptr<uint32_t>(s->column_offset);
    o.row_indices = dptr<uint32_t>(s->row_indices);
    o.sample_ans = dptr<uint32_t>(s->sample_ans);
    o.edge_dst = dptr<uint32_t>(s->edge_dst);
    o.source = dptr<uint32_t>(s->source);
    o.edge_weight_forward = r.wt == NTS_WEIGHT_NONE ? nullptr : dptr<float>(s->edge_weight_forward);
    o.row_offset = s->has_csr ? dptr<uint32_t>(s->row_offset) : nullptr;
    o.column_indices = s->has_csr ? dptr<uint32_t>(s->column_indices) : nullptr;
    o.edge_weight_backward =
        (s->has_csr && r.wt != NTS_WEIGHT_NONE) ? dptr<float>(s->edge_weight_backward) : nullptr;
    o.sizes = dptr<uint32_t>(s->sizes);
    o.dst_local_id = dptr<uint32_t>(s->dst_local_id);  // undefined (NULL) unless merged
    o.csr_edge_id = dptr<uint32_t>(s->csr_edge_id);
    o.sizes_host = ssg->host_sizes_dev + 4 * l;
    NTS_CALL(nts_hip_induced_layer, cs.ctx(), &g, set, set_n, set_cap, r.wt, &o);
    if (l == 0)
      s->destination = dev_nids_.narrow(0, r.offset, std::max<int64_t>(actual, 0));
    else
      s->destination = ssg->sampled_sgs[l - 1]->source;
    dst = set = o.source;
    vsz = set_n = o.sizes + 2;
    set_cap = o.s_cap;
  }
  hip_rt(hipEventRecord(ssg->sampled, st), "hipEventRecord");
}

void FastSampler::set_mt_budget_scale(NtsStream& cs, double scale) {
  mt_budget_ = scale;
  NTS_CALL(nts_hip_mt_budget_scale, cs.ctx(), scale);
}

// MT19937 modes: a layer's draws passed the words generated for it (its
// bound, nts_hip_mt_budget_scale).  That layer left the generator where it
// began, so every layer after it — of this batch and of the batches issued
// behind it — read the stream from the wrong word.  Re-run from the batch's
// checkpoint with every bound scaled up: the batch and each one issued after
// it, in order (the same stream, so the same, reference-exact sets).
void FastSampler::rerun_from(int ssg_id) {
  TORCH_CHECK(is_mt_mode(rng_mode), "only the MT19937 modes can fall short");
  TORCH_CHECK(rerun_ok, "a short MT19937 stream with work chained to the sampled batches "
              "(early aggregation): cannot re-run");
  auto it = std::find(issued_.begin(), issued_.end(), ssg_id);
  TORCH_CHECK(it != issued_.end(), "re-run of a batch that is not pending");
  IssueRec& r0 = recs_[ssg_id];
  NtsStream& cs = *r0.cs;
  TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "hipDeviceSynchronize");
  mt_budget_ = std::min(mt_budget_ * 4.0, 1e4);
  NTS_CALL(nts_hip_mt_budget_scale, cs.ctx(), mt_budget_);
  NTS_CALL(nts_hip_mt_rewind, cs.ctx(), dptr<uint32_t>(r0.mt_ckpt));
  ++mt_reruns;
  for (auto j = it; j != issued_.end(); ++j) {
    IssueRec& r = recs_[*j];
    NTS_CALL(nts_hip_mt_checkpoint, r.cs->ctx(), dptr<uint32_t>(r.mt_ckpt));
    enqueue_layers(*j, r);
  }
  TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "hipDeviceSynchronize");
}

SampledSubgraph* FastSampler::finish_gpu_sample(int ssg_id) {
  double t0 = now_s();
  ssg = ssgs[ssg_id];
  TORCH_CHECK(ssg->pending_batch > 0, "finish_gpu_sample without a pending issue");
  hip_rt(hipEventSynchronize(ssg->sampled), "hipEventSynchronize");
  if (host_profile()) fprintf(stderr, "[host] finish wait: %.1f us\n", (now_s() - t0) * 1e6);
  const volatile int32_t* hs = ssg->host_sizes;
  for (int attempt = 0;; ++attempt) {
    bool short_stream = false;
    for (int l = 0; l < layer; ++l) short_stream |= (hs[4 * l + 3] & 4) != 0;
    if (!short_stream) break;
    TORCH_CHECK(attempt < 8, "the MT19937 word stream fell short ", attempt + 1,
                " times for one batch (bound scale ", mt_budget_, ")");
    rerun_from(ssg_id);  // synchronises (and moves `ssg` to the last slot it re-ran)
    ssg = ssgs[ssg_id];
  }
  ssg->pending_batch = 0;
  issued_.erase(std::find(issued_.begin(), issued_.end(), ssg_id));
  for (int l = 0; l < layer; ++l) {
    sampCSC* s = ssg->sampled_sgs[l];
    s->v_size = (VertexId)hs[4 * l];
    s->e_size = (VertexId)hs[4 * l + 1];
    s->src_size = (VertexId)hs[4 * l + 2];
    TORCH_CHECK(hs[4 * l + 3] == 0, "sampled layer ", l, " exceeded its capacity",
                subgraph_walk_ >= 0 ? " (subgraph_edge_cap)" : "");
    sampled_edges += s->e_size;
  }
  all_time += now_s() - t0;
  return ssg;
}

void FastSampler::load_feature_gpu(NtsStream& cs, SampledSubgraph* sg, NtsVar& local_feature,
                                   const NtsVar& global_feature) {
  sampCSC* top = sg->sampled_sgs[layer - 1];
  const int64_t F = global_feature.size(1);
  if (!local_feature.defined() || local_feature.size(0) != (int64_t)top->src_size ||
      local_feature.size(1) != F)  // 128-byte row pitch: float4 rows for the GEMMs
    local_feature = row_padded_empty((int64_t)top->src_size, F, whole_graph->device);
  if (global_feature.dtype() == torch::kFloat16) {  // the f16 table: widened as it is gathered
    NTS_CALL(nts_hip_gather_rows_h, cs.ctx(), dptr<const uint16_t>(global_feature),
             (uint64_t)global_feature.stride(0), top->dev_src(), nullptr, top->src_size,
             (uint32_t)F, local_feature.data_ptr<float>(), (uint64_t)local_feature.stride(0));
    return;
  }
  NTS_CALL(nts_hip_gather_rows, cs.ctx(), global_feature.data_ptr<float>(),
           (uint64_t)global_feature.stride(0), top->dev_src(), nullptr, top->src_size, (uint32_t)F,
           local_feature.data_ptr<float>(), (uint64_t)local_feature.stride(0));
}

void FastSampler::load_feature_gpu_cache(NtsStream& cs, SampledSubgraph* sg,
                                         NtsVar& local_feature, const FeatureCache& fc) {
  sampCSC* top = sg->sampled_sgs[layer - 1];
  if (!local_feature.defined() || local_feature.size(0) != (int64_t)top->src_size ||
      local_feature.size(1) != fc.F)
    local_feature = torch::empty({(int64_t)top->src_size, fc.F}, f32_opts(whole_graph->device));
  NTS_CALL(nts_hip_gather_rows_cached, cs.ctx(), fc.cache_ptr(), fc.ld,
           dptr<uint32_t>(fc.cache_map), fc.host_dev, fc.ld, top->dev_src(), nullptr, top->src_size,
           (uint32_t)fc.F, local_feature.data_ptr<float>(), (uint64_t)local_feature.stride(0));
}

FeatureCache::FeatureCache(NtsStream& cs, const FullyRepGraph& g, const NtsVar& table,
                           uint64_t n_cache_)
    : n_vertices(g.global_vertices), n_cache(n_cache_), F(table.size(1)) {
  TORCH_CHECK(table.is_cuda() && table.dtype() == torch::kFloat32 && table.dim() == 2 &&
                  table.stride(1) == 1 && (uint64_t)table.size(0) == n_vertices,
              "feature table must be fp32 [V, F] on the GPU");
  TORCH_CHECK(n_cache <= n_vertices, "n_cache > V");
  ld = (uint64_t)(F + 31) / 32 * 32;  // 128-byte rows in both tiers
  void* hp = nullptr;
  NTS_CALL(nts_hip_host_alloc, n_vertices * ld * sizeof(float), &hp);
  host = static_cast<float*>(hp);
  void* dp = nullptr;
  NTS_CALL(nts_hip_host_device_pointer, hp, &dp);
  host_dev = static_cast<const float*>(dp);
  // spill: the whole table to the host (the reference's pinned
  // local_feature, core/ntsDataloador.hpp:483), then the hot rows back to HBM
  TORCH_CHECK(hipMemcpy2DAsync(host, ld * sizeof(float), table.data_ptr<float>(),
                               (size_t)table.stride(0) * sizeof(float), (size_t)F * sizeof(float),
                               (size_t)n_vertices, hipMemcpyDeviceToHost,
                               (hipStream_t)cs.stream()) == hipSuccess,
              "hipMemcpy2DAsync");
  cache_map = torch::empty({(int64_t)n_vertices}, u32_opts(g.device));
  if (n_cache) {
    cache_ids = torch::empty({(int64_t)n_cache}, u32_opts(g.device));
    cache = torch::empty({(int64_t)n_cache, (int64_t)ld}, f32_opts(g.device)).narrow(1, 0, F);
  }
  NTS_CALL(nts_hip_cache_select, cs.ctx(), dptr<uint32_t>(g.out_degree), n_vertices, n_cache,
           dptr<uint32_t>(cache_map), dptr<uint32_t>(cache_ids));
  if (n_cache)  // gater_cpu_cache_feature_and_trans_to_gpu
    NTS_CALL(nts_hip_gather_rows, cs.ctx(), table.data_ptr<float>(), (uint64_t)table.stride(0),
             dptr<uint32_t>(cache_ids), nullptr, (uint32_t)n_cache, (uint32_t)F,
             cache.data_ptr<float>(), ld);
  cs.synchronize();
}

void FeatureCache::aggregate(nts_hip_ctx* ctx, const sampCSC* s, const uint32_t* v_dev,
                             uint32_t v_cap, const uint32_t* s_dev, uint32_t s_cap, float* stage,
                             float* y, uint64_t ldy) const {
  NTS_CALL(nts_hip_stage_uncached_rows, ctx, dptr<uint32_t>(cache_map), host_dev, ld, s->dev_src(),
           s_dev, s_cap, (uint32_t)F, stage, ld);
  NTS_CALL(nts_hip_spmm_csc_fwd_cached, ctx, s->dev_c_o(), s->dev_r_i(), s->dev_e_w_f(), v_dev,
           v_cap, cache_ptr(), ld, dptr<uint32_t>(cache_map), stage, ld, 1, s->dev_src(),
           (uint32_t)F, y, ldy);
}

FeatureCache::~FeatureCache() {
  if (host) (void)nts_hip_host_free(host);
}

void FastSampler::load_label_gpu(NtsStream& cs, SampledSubgraph* sg, NtsVar& local_label,
                                 const NtsVar& global_label) {
  sampCSC* s0 = sg->sampled_sgs[0];
  if (!local_label.defined() || local_label.size(0) != (int64_t)s0->v_size)
    local_label = torch::empty({(int64_t)s0->v_size},
                               torch::TensorOptions().dtype(torch::kInt64).device(torch::kCUDA, whole_graph->device));
  NTS_CALL(nts_hip_gather_labels, cs.ctx(), global_label.data_ptr<int64_t>(), s0->dev_dst(),
           nullptr, s0->v_size, local_label.data_ptr<int64_t>());
}

}  // namespace nts
