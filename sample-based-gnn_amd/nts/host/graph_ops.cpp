// C++ host layer, graph side: the sampled aggregation dispatch, the graph
// operators and the autodiff context.
#include <algorithm>
#include <map>
#include <mutex>

#include "ops_util.hpp"

namespace nts {

// ---------------------------------------------------------------------------
void spmm_csc_fwd(NtsStream& cs, AggKind kind, const sampCSC* s, const NtsVar& x, bool gather,
                  const uint32_t* v_dev, uint32_t v_rows, NtsVar& y, uint32_t* arg, bool early) {
  const uint64_t ldx = (uint64_t)x.stride(0), ldy = (uint64_t)y.stride(0);
  const uint32_t F = (uint32_t)x.size(1);
  const VertexId* map = gather ? s->dev_src() : nullptr;
  if (x.dtype() == torch::kFloat16) {  // the f16 feature table: half rows in, fp32 sums out
    TORCH_CHECK(gather && !kind.max && !kind.root,
                "a half table is gathered by the sum aggregation only");
    hip_check(nts_hip_spmm_csc_fwd_h(cs.ctx(), s->dev_c_o(), s->dev_r_i(), s->dev_e_w_f(), v_dev,
                                     v_rows, dptr<const uint16_t>(x), ldx, map, F, y.data_ptr<float>(), ldy),
              early ? "nts_hip_spmm_csc_fwd_h(early)" : "nts_hip_spmm_csc_fwd_h");
    return;
  }
  const float* xp = x.data_ptr<float>();
  const VertexId* self = !kind.root ? nullptr : gather ? s->dev_dst() : s->dev_dst_local_id();
  if (kind.max)
    hip_check(nts_hip_spmm_csc_fwd_max(cs.ctx(), s->dev_c_o(), s->dev_r_i(), v_dev, v_rows, xp,
                                       ldx, map, self, F, y.data_ptr<float>(), ldy, arg),
              early ? "nts_hip_spmm_csc_fwd_max(early)" : "nts_hip_spmm_csc_fwd_max");
  else if (kind.root)  // [A X | X[self rows]], one launch
    hip_check(nts_hip_spmm_csc_fwd_root(cs.ctx(), s->dev_c_o(), s->dev_r_i(), s->dev_e_w_f(),
                                        v_dev, v_rows, xp, ldx, map, self, F,
                                        y.data_ptr<float>(), ldy),
              early ? "nts_hip_spmm_csc_fwd_root(early)" : "nts_hip_spmm_csc_fwd_root");
  else
    hip_check(nts_hip_spmm_csc_fwd(cs.ctx(), s->dev_c_o(), s->dev_r_i(), s->dev_e_w_f(), v_dev,
                                   v_rows, xp, ldx, map, F, y.data_ptr<float>(), ldy),
              early ? "nts_hip_spmm_csc_fwd(early)" : "nts_hip_spmm_csc_fwd");
}

namespace op {

SingleGPUAllSampleGraphOp::SingleGPUAllSampleGraphOp(SampledSubgraph* sgs, FullyRepGraph* graph,
                                                     int layer_, NtsStream* cs, bool gather,
                                                     const FeatureCache* fc, AggKind kind_,
                                                     bool csr_only_)
    : subgraphs(sgs), layer(layer_), cuda_stream(cs), gather_from_table(gather),
      feature_cache(fc), kind(kind_), csr_only(csr_only_) {
  (void)graph;
  TORCH_CHECK(!fc || gather, "a feature cache needs gather_from_table");
  TORCH_CHECK(!fc || !(kind.max || kind.root),
              "a feature cache takes the sum aggregator without root weight");
}

NtsVar SingleGPUAllSampleGraphOp::forward(NtsVar& f_input) {
  sampCSC* sg = subgraphs->sampled_sgs[layer];
  const int dev = cuda_stream->device();
  NtsVar f_output;
  if (feature_cache) {  // two-tier table: f_input only carries the width
    const FeatureCache& fc = *feature_cache;
    f_output = row_padded_empty((int64_t)sg->v_size, fc.F, dev);
    NtsVar stage = torch::empty({(int64_t)std::max<uint32_t>(sg->src_size, 1), (int64_t)fc.ld},
                                f32_opts(dev));
    fc.aggregate(cuda_stream->ctx(), sg, nullptr, sg->v_size, nullptr, sg->src_size,
                 stage.data_ptr<float>(), f_output.data_ptr<float>(), (uint64_t)f_output.stride(0));
  } else {
    TORCH_CHECK(!kind.root || sg->dst_local_id.defined(),
                "root weight needs a merged src/dst layer");
    // (the f16 feature table is the one half input: gathered rows, no backward)
    const bool half_table = gather_from_table && f_input.dtype() == torch::kFloat16;
    TORCH_CHECK(f_input.is_cuda() && (f_input.dtype() == torch::kFloat32 || half_table) &&
                    f_input.dim() == 2 && f_input.stride(1) == 1,
                "graph op input must be a row-major fp32 CUDA matrix");
    TORCH_CHECK(gather_from_table || f_input.size(0) >= (int64_t)sg->src_size,
                "graph op input has fewer rows than src_size");
    const int64_t F = f_input.size(1);
    f_output = row_padded_empty((int64_t)sg->v_size, (kind.root ? 2 : 1) * F, dev);
    // max: the winners only where a backward will read them (never the bottom hop)
    if (kind.max && output_requires_grad && sg->has_csr) {
      TORCH_CHECK(sg->csr_edge_id.defined(), "max aggregator backward needs csr_edge_id");
      arg = torch::empty({std::max<int64_t>(sg->v_size, 1), F}, u32_opts(dev));
    }
    // (the sum kernel takes the exact host row count, the other two also the device's)
    spmm_csc_fwd(*cuda_stream, kind, sg, f_input, gather_from_table,
                 kind.max || kind.root ? sg->dev_v_size() : nullptr, sg->v_size, f_output,
                 dptr<uint32_t>(arg));
  }
  if (output_requires_grad) f_output.set_requires_grad(true);
  return f_output;
}

NtsVar SingleGPUAllSampleGraphOp::backward(NtsVar& g) {
  sampCSC* sg = subgraphs->sampled_sgs[layer];
  nts_hip_ctx* c = cuda_stream->ctx();
  TORCH_CHECK(!csr_only || sg->has_csr, "SingleGPUSampleGraphOp needs the CSR transpose");
  if (kind.max) {
    TORCH_CHECK(sg->has_csr && sg->csr_edge_id.defined() && arg.defined(),
                "max aggregator backward needs the CSR transpose, its edge ids and the forward's arg");
    TORCH_CHECK(!kind.root || sg->src_dst.defined(), "root weight backward needs the inverse map");
  } else if (kind.root) {
    TORCH_CHECK(sg->has_csr && sg->src_dst.defined(),
                "root weight backward needs the CSR transpose and the inverse map");
  }
  NtsVar go = g.contiguous();
  const bool rows_ok = go.size(0) == (int64_t)sg->v_size;
  const int64_t ldg = go.size(1);
  const int64_t F = kind.max ? arg.size(1) : kind.root ? ldg / 2 : ldg;
  if (kind.max) {
    TORCH_CHECK(rows_ok && ldg == (kind.root ? 2 : 1) * F,
                "output grad must be [v_size, F] ([v_size, 2 F] under root weight)");
  } else if (kind.root) {
    TORCH_CHECK(rows_ok && ldg % 2 == 0, "output grad must be [v_size, 2 F]");
  } else {
    TORCH_CHECK(rows_ok, "output grad rows != v_size");
  }
  const float* gp = go.data_ptr<float>();
  const FusedActBwd& ab = sg->act_bwd;
  if (!sg->has_csr) {  // (the plain sum alone gets here)
    TORCH_CHECK(!ab.mask, "a fused activation backward needs the CSR backward");
    NtsVar gi = torch::zeros({(int64_t)sg->src_size, F}, f32_opts(cuda_stream->device()));
    NTS_CALL(nts_hip_spmm_csc_bwd_atomic, c, sg->dev_c_o(), sg->dev_r_i(), sg->dev_e_w_f(), nullptr,
             sg->v_size, gp, (uint64_t)F, (uint32_t)F, gi.data_ptr<float>(), (uint64_t)F);
    return gi;
  }
  NtsVar gi = torch::empty({(int64_t)sg->src_size, F}, f32_opts(cuda_stream->device()));
  float* ip = gi.data_ptr<float>();
  if (kind.max)
    NTS_CALL(nts_hip_spmm_csr_bwd_max, c, sg->dev_r_o(), sg->dev_c_i(),
             dptr<uint32_t>(sg->csr_edge_id), sg->dev_src_size(), sg->src_size, gp, (uint64_t)ldg,
             dptr<uint32_t>(arg), kind.root ? dptr<uint32_t>(sg->src_dst) : nullptr, ab.mask, ab.ld,
             ab.scale, (uint32_t)F, ip, (uint64_t)F);
  else if (kind.root)
    NTS_CALL(nts_hip_spmm_csr_bwd_root, c, sg->dev_r_o(), sg->dev_c_i(), sg->dev_e_w_b(),
             sg->dev_src_size(), sg->src_size, gp, (uint64_t)(2 * F), dptr<uint32_t>(sg->src_dst),
             ab.mask, ab.ld, ab.scale, (uint32_t)F, ip, (uint64_t)F);
  else if (ab.bits)  // the transform-first bottom layer's activation backward fused, its mask as bits
    NTS_CALL(nts_hip_spmm_csr_bwd_postmask_bits, c, sg->dev_r_o(), sg->dev_c_i(), sg->dev_e_w_b(),
             nullptr, sg->src_size, gp, (uint64_t)F, ab.bits, ab.scale, (uint32_t)F, ip,
             (uint64_t)F);
  else if (ab.mask)  // the same, the mask read from the activation's rows
    NTS_CALL(nts_hip_spmm_csr_bwd_postmask, c, sg->dev_r_o(), sg->dev_c_i(), sg->dev_e_w_b(),
             nullptr, sg->src_size, gp, (uint64_t)F, ab.mask, ab.ld, ab.scale, (uint32_t)F, ip,
             (uint64_t)F);
  else
    NTS_CALL(nts_hip_spmm_csr_bwd, c, sg->dev_r_o(), sg->dev_c_i(), sg->dev_e_w_b(), nullptr,
             sg->src_size, gp, (uint64_t)F, (uint32_t)F, ip, (uint64_t)F);
  return gi;
}

}  // namespace op

// ---------------------------------------------------------------------------
// A persistent fp32 scalar 1 per device: the seed gradient of a scalar loss.
// Kernels that precompute their backward for d loss = 1 recognise it by
// identity (HipLinearXentFn); no fill kernel per step.
const NtsVar& unit_scalar(const torch::Device& dev) {
  static std::mutex mu;
  static std::map<std::string, NtsVar> units;
  std::lock_guard<std::mutex> lk(mu);
  NtsVar& u = units[dev.str()];
  if (!u.defined()) u = torch::ones({}, torch::TensorOptions().dtype(torch::kFloat32).device(dev));
  return u;
}

namespace ctx {

NtsContext::NtsContext() {}
NtsContext::~NtsContext() { reset(); }

void NtsContext::push_graph_op(op::ntsGraphOp* op, NtsVar& in, NtsVar& out) {
  if (!training) {  // eval: ops are not recorded (and not leaked, unlike the reference)
    delete op;
    return;
  }
  ops_.push_back(Entry{GRAPHOP, op, in, out, NtsVar(), in.data_ptr(), out.data_ptr()});
  ++count;
}

NtsVar NtsContext::runVertexForward(const std::function<NtsVar(NtsVar&, NtsVar&)>& fn,
                                    NtsVar& nbr_input, NtsVar& vtx_input) {
  NtsVar out = fn(nbr_input, vtx_input);
  if (training) appendNNOp(nbr_input, out);
  return out;
}

NtsVar NtsContext::runVertexForward(const std::function<NtsVar(NtsVar&)>& fn, NtsVar& nbr_input) {
  NtsVar out = fn(nbr_input);
  if (training) appendNNOp(nbr_input, out);
  return out;
}

// core/ntsContext.hpp:384-405: consecutive NN ops are chained (libtorch
// handles their backward), so only the segment's last output is kept.
void NtsContext::appendNNOp(NtsVar& input_t, NtsVar& output_t) {
  TORCH_CHECK(training, "appendNNOp in eval mode");
  if (count > 0 && ops_.back().type == NNOP) {
    ops_.back().output = output_t;
    ops_.back().out_id = output_t.data_ptr();
  } else {
    ops_.push_back(Entry{NNOP, nullptr, input_t, output_t, NtsVar(), input_t.data_ptr(),
                         output_t.data_ptr()});
    ++count;
  }
}

void NtsContext::pop_one_op() {
  delete ops_.back().op;
  ops_.pop_back();
  --count;
}

// core/ntsContext.hpp:436-508: loss backward through libtorch, then walk the
// stack alternating graph-op backward and libtorch backward; the bottom graph
// op's backward is skipped.
void NtsContext::self_backward(bool retain_graph) {
  TORCH_CHECK(training && count > 0, "self_backward outside training");
  Entry& top = ops_.back();
  const bool unit = top.output.dim() == 0 && top.output.scalar_type() == torch::kFloat32;
  top.output.backward(unit ? unit_scalar(top.output.device()) : torch::ones_like(top.output), {},
                      retain_graph);
  if (count >= 2) ops_[count - 2].output_grad = top.input.grad();
  pop_one_op();
  while (count > 1 || (count == 1 && ops_.back().type == NNOP)) {
    Entry& e = ops_.back();
    const int t = count - 1;
    if (e.type == GRAPHOP) {
      if (!e.output_grad.defined()) e.output_grad = e.output.grad();
      int pre = t;
      for (; pre >= 0; --pre)
        if (ops_[pre].out_id == e.in_id) break;
      TORCH_CHECK(pre >= 0, "graph op input has no producer on the stack");
      ops_[pre].output_grad = e.op->backward(e.output_grad);
      pop_one_op();
    } else {
      if (!e.output_grad.defined()) e.output_grad = e.output.grad();
      if (e.output_grad.defined() && e.output_grad.dim() > 1)
        e.output.backward(e.output_grad, {}, retain_graph);
      pop_one_op();
    }
  }
  reset();
}

void NtsContext::reset() {
  while (!ops_.empty()) pop_one_op();
  count = 0;
}

}  // namespace ctx

}  // namespace nts
