// C++ host layer, attention: the GAT and GATv2 layers and their dropout.
#include <algorithm>

#include "ops_util.hpp"

namespace nts {

namespace {
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

// What the two attention layers take besides their tensors.  Built once by the
// public wrapper (on a merged src/dst layer only; one head is the single-head
// layer in both modes), handed to forward as one handle, kept for backward in
// saved_data.
struct GatArgs {
  sampCSC* sg;
  NtsStream* cs;
  KernelProfiler* prof;
  int64_t heads;
  bool mean;
  GatDropout drop;
  bool x_grad = false;  // forward: the input wants a gradient

  GatArgs(const char* who, sampCSC* sg_, NtsStream* cs_, KernelProfiler* prof_, int heads_,
          bool mean_, const GatDropout& drop_)
      : sg(sg_), cs(cs_), prof(prof_), heads(heads_), mean(mean_ && heads_ != 1), drop(drop_) {
    TORCH_CHECK(sg->dst_local_id.defined() && sg->csr_edge_id.defined(), who,
                " needs a merged src/dst layer with its CSR (set_merge_src_dst)");
  }
  void save(AutogradContext* ctx) const {
    ctx->saved_data["heads"] = heads;
    ctx->saved_data["mean"] = mean;
    ctx->saved_data["sg"] = to_handle(sg);
    ctx->saved_data["cs"] = to_handle(cs);
    ctx->saved_data["x_grad"] = x_grad;
    ctx->saved_data["p_attn"] = drop.p_attn;
    ctx->saved_data["p_out"] = drop.p_out;
    ctx->saved_data["seed"] = (int64_t)drop.seed;
    ctx->saved_data["off_attn"] = (int64_t)drop.off_attn;
  }
  explicit GatArgs(AutogradContext* ctx)  // backward: what save() kept
      : sg(from_handle<sampCSC>(ctx->saved_data["sg"])),
        cs(from_handle<NtsStream>(ctx->saved_data["cs"])),
        prof(nullptr),
        heads(ctx->saved_data["heads"].toInt()),
        mean(ctx->saved_data["mean"].toBool()),
        x_grad(ctx->saved_data["x_grad"].toBool()) {
    drop.p_attn = ctx->saved_data["p_attn"].toDouble();
    drop.p_out = ctx->saved_data["p_out"].toDouble();
    drop.seed = (uint64_t)ctx->saved_data["seed"].toInt();
    drop.off_attn = (uint64_t)ctx->saved_data["off_attn"].toInt();
  }
};
}  // namespace

// GAT layer on a merged src/dst sampled block (GAT_SAMPLE_ALL_GPU's chain,
// toolkits/GAT_SAMPLE_ALL_GPU.hpp:322-388): H = X W on the MFMA GEMM, then
// the fused attention/softmax/aggregation/relu kernel; the backward runs the
// two deterministic GAT backward passes and three GEMMs (dW = X^T dH,
// dW_att = H^T dS, dX = dH W^T).
// heads > 1: the multi-head entry points (K heads of D = F / K columns; Y is
// their concatenation, or with `mean` their mean, D wide).  dW_att is then the
// same TN GEMM with N = 2K, T = H^T dS [F, 2K], of which head h's rows keep
// columns h and K + h (the other columns, products of one head's rows with
// another head's dS, are dropped): the GEMM is the MFMA kernel that is there,
// deterministic, and at K <= 8 its 2K columns still fill one 16-column tile.
// The _drop entry points take the rates as they are: with both 0 they run the
// plain kernels; p_attn / p_out > 0 adds attention and output dropout in the
// same kernels (the backward regenerates the attention keep bits from
// (seed, off_attn) and reads the output mask off Y > 0).
struct HipGATLayerFn : public torch::autograd::Function<HipGATLayerFn> {
  static NtsVar forward(AutogradContext* ctx, NtsVar X, NtsVar W, NtsVar Watt, int64_t args) {
    GatArgs arg = *from_handle<const GatArgs>(args);
    sampCSC* sg = arg.sg;
    NtsStream* cs = arg.cs;
    KernelProfiler* prof = arg.prof;
    const GatDropout& drop = arg.drop;
    const int64_t K = arg.heads;
    const bool mean = arg.mean;
    TORCH_CHECK(K >= 1 && W.size(1) % K == 0, "GAT layer: ", K, " heads do not divide width ",
                W.size(1));
    const int64_t D = W.size(1) / K;
    NtsVar Xc = row_major(X), Wc = W.contiguous(), Ac = Watt.contiguous();
    const int64_t s = sg->src_size, v = sg->v_size, e = sg->e_size;
    const int64_t Fin = Xc.size(1), F = Wc.size(1);
    TORCH_CHECK(Xc.size(0) == s && Wc.size(0) == Fin && Ac.numel() == 2 * F, "GAT layer shapes");
    const int dev = cs->device();
    NtsVar H = torch::empty({s, F}, f32_opts(dev));
    gemm(*cs, 0, Xc, Wc, H, "H");
    NtsVar m = torch::empty({std::max<int64_t>(e, 1) * K}, f32_opts(dev));
    NtsVar a = torch::empty({std::max<int64_t>(e, 1) * K}, f32_opts(dev));
    const int64_t FY = mean ? D : F;
    NtsVar Y = torch::empty({v, FY}, f32_opts(dev));
    hipStream_t st = (hipStream_t)cs->stream();
    if (prof) prof->begin(KernelProfiler::GAT_FWD, st);
    if (K == 1)
      NTS_CALL(nts_hip_gat_forward_drop, cs->ctx(), sg->dev_c_o(), sg->dev_r_i(),
               sg->dev_dst_local_id(), (uint32_t)v, H.data_ptr<float>(), (uint64_t)F, (uint32_t)F,
               Ac.data_ptr<float>(), m.data_ptr<float>(), a.data_ptr<float>(), Y.data_ptr<float>(),
               (uint64_t)F, (float)drop.p_attn, (float)drop.p_out, drop.seed, drop.off_attn,
               drop.off_out);
    else
      NTS_CALL(nts_hip_gat_forward_heads_drop, cs->ctx(), sg->dev_c_o(), sg->dev_r_i(),
               sg->dev_dst_local_id(), (uint32_t)v, H.data_ptr<float>(), (uint64_t)F, (uint32_t)K,
               (uint32_t)D, Ac.data_ptr<float>(), m.data_ptr<float>(), a.data_ptr<float>(),
               Y.data_ptr<float>(), (uint64_t)FY, mean ? 1 : 0, (float)drop.p_attn,
               (float)drop.p_out, drop.seed, drop.off_attn, drop.off_out);
    // compulsory bytes: H rows once, offsets, row index + score + weight per
    // edge, dst local ids, W_att, output rows
    if (prof)
      prof->end(KernelProfiler::GAT_FWD, st,
                4.0 * F * s + 4.0 * (v + 1) + (4.0 + 8.0 * K) * e + 4.0 * v + 8.0 * F +
                    4.0 * FY * v);
    ctx->save_for_backward({Xc, Wc, Ac, H, Y, m, a});
    arg.x_grad = X.requires_grad();
    arg.save(ctx);
    return Y;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto v_ = ctx->get_saved_variables();
    NtsVar X = v_[0], W = v_[1], A = v_[2], H = v_[3], Y = v_[4], m = v_[5], a = v_[6];
    const GatArgs arg(ctx);
    sampCSC* sg = arg.sg;
    NtsStream* cs = arg.cs;
    const GatDropout& drop = arg.drop;
    NtsVar GY = grads[0].contiguous();
    const int64_t s = H.size(0), F = H.size(1), Fin = X.size(1), v = Y.size(0);
    const int64_t e = sg->e_size;
    const int64_t K = arg.heads, D = F / K;
    const bool mean = arg.mean;
    const int64_t FY = mean ? D : F;
    const int dev = cs->device();
    auto guard = cs->guard();
    NtsVar du = torch::empty({std::max<int64_t>(e, 1) * K}, f32_opts(dev));
    NtsVar ds2 = torch::empty({std::max<int64_t>(s, 1) * K}, f32_opts(dev));
    NtsVar dH = torch::empty({s, F}, f32_opts(dev));
    NtsVar dS = torch::empty({s, 2 * K}, f32_opts(dev));
    NtsVar GM = torch::empty({std::max<int64_t>(v, 1), F}, f32_opts(dev));
    if (K > 1)
      NTS_CALL(nts_hip_gat_backward_heads_drop, cs->ctx(), sg->dev_c_o(), sg->dev_r_i(),
               sg->dev_dst_local_id(), (uint32_t)v, sg->dev_r_o(), sg->dev_c_i(),
               dptr<uint32_t>(sg->csr_edge_id), (uint32_t)s, H.data_ptr<float>(), (uint64_t)F,
               (uint32_t)K, (uint32_t)D, A.data_ptr<float>(), a.data_ptr<float>(),
               m.data_ptr<float>(), Y.data_ptr<float>(), (uint64_t)FY, GY.data_ptr<float>(),
               (uint64_t)FY, du.data_ptr<float>(), ds2.data_ptr<float>(), GM.data_ptr<float>(),
               (uint64_t)F, dH.data_ptr<float>(), (uint64_t)F, dS.data_ptr<float>(), mean ? 1 : 0,
               (float)drop.p_attn, (float)drop.p_out, drop.seed, drop.off_attn);
    else
      NTS_CALL(nts_hip_gat_backward_drop, cs->ctx(), sg->dev_c_o(), sg->dev_r_i(),
               sg->dev_dst_local_id(), (uint32_t)v, sg->dev_r_o(), sg->dev_c_i(),
               dptr<uint32_t>(sg->csr_edge_id), (uint32_t)s, H.data_ptr<float>(), (uint64_t)F,
               (uint32_t)F, A.data_ptr<float>(), a.data_ptr<float>(), m.data_ptr<float>(),
               Y.data_ptr<float>(), (uint64_t)F, GY.data_ptr<float>(), (uint64_t)F,
               du.data_ptr<float>(), ds2.data_ptr<float>(), GM.data_ptr<float>(), (uint64_t)F,
               dH.data_ptr<float>(), (uint64_t)F, dS.data_ptr<float>(), (float)drop.p_attn,
               (float)drop.p_out, drop.seed, drop.off_attn);
    NtsVar dW = torch::empty({Fin, F}, f32_opts(dev));
    gemm(*cs, 1, X, dH, dW, "dW");
    NtsVar T = torch::empty({F, 2 * K}, f32_opts(dev));
    gemm(*cs, 1, H, dS, T, "dW_att");
    if (K > 1) {  // row hD + j keeps columns h (a1) and K + h (a2)
      NtsVar h = torch::arange(F, torch::TensorOptions().dtype(torch::kInt64).device(T.device()))
                     .floor_divide(D);
      T = T.gather(1, torch::stack({h, h + K}, 1));
    }
    NtsVar dA = T.t().contiguous().view({2 * F, 1});  // [a1 | a2] as W_att's rows
    NtsVar dX;
    if (arg.x_grad) {
      NtsVar Wt = W.t().contiguous();
      dX = torch::empty({s, Fin}, f32_opts(dev));
      gemm(*cs, 0, dH, Wt, dX, "dX");
    }
    return no_grads({dX, dW, dA.view(A.sizes())}, 1);
  }
};

NtsVar hip_gat_layer(const NtsVar& x, const NtsVar& W, const NtsVar& Watt, sampCSC* sg,
                     NtsStream* cs, KernelProfiler* prof, int heads, bool mean,
                     const GatDropout& drop) {
  const GatArgs args("GAT", sg, cs, prof, heads, mean, drop);
  return HipGATLayerFn::apply(x, W, Watt, to_handle(&args));
}

// GATv2 layer (no reference counterpart) on a merged src/dst
// sampled block.  W is the stacked parameter [F_in, 2F] = [W_s | W_d]:
// Hs = X W_s over all source rows, Hd = X[dst_local_id] W_d over the v
// destination rows only (s is several times v), both on the MFMA GEMM, then
// the fused score / softmax / aggregation / relu kernel.  The backward runs the
// two deterministic kernels (datt comes straight from them) and four GEMMs:
// dW = [X^T dHs | X[dst]^T dHd], dX = dHs W_s^T, plus dHd W_d^T added at the
// rows dst_local_id (the map is injective: no two rows meet).
struct HipGATv2LayerFn : public torch::autograd::Function<HipGATv2LayerFn> {
  static NtsVar forward(AutogradContext* ctx, NtsVar X, NtsVar W, NtsVar Watt, int64_t args) {
    GatArgs arg = *from_handle<const GatArgs>(args);
    sampCSC* sg = arg.sg;
    NtsStream* cs = arg.cs;
    KernelProfiler* prof = arg.prof;
    const GatDropout& drop = arg.drop;
    const int64_t K = arg.heads;
    const bool mean = arg.mean;
    TORCH_CHECK(W.size(1) % 2 == 0, "GATv2 layer: W must be [F_in, 2 F] = [W_s | W_d]");
    const int64_t F = W.size(1) / 2;
    TORCH_CHECK(K >= 1 && F % K == 0, "GATv2 layer: ", K, " heads do not divide width ", F);
    const int64_t D = F / K;
    NtsVar Xc = row_major(X), Ac = Watt.contiguous();
    NtsVar Ws = W.narrow(1, 0, F).contiguous(), Wd = W.narrow(1, F, F).contiguous();
    const int64_t s = sg->src_size, v = sg->v_size, e = sg->e_size;
    const int64_t Fin = Xc.size(1);
    TORCH_CHECK(Xc.size(0) == s && W.size(0) == Fin && Ac.numel() == F, "GATv2 layer shapes");
    const int dev = cs->device();
    NtsVar idx = sg->dst_local_id.narrow(0, 0, v).to(torch::kInt64);
    NtsVar Xd = Xc.index_select(0, idx);
    NtsVar Hs = torch::empty({s, F}, f32_opts(dev));
    NtsVar Hd = torch::empty({std::max<int64_t>(v, 1), F}, f32_opts(dev));
    gemm(*cs, 0, Xc, Ws, Hs, "Hs");
    if (v) gemm(*cs, 0, Xd, Wd, Hd, "Hd");
    NtsVar u = torch::empty({std::max<int64_t>(e, 1) * K}, f32_opts(dev));
    NtsVar a = torch::empty({std::max<int64_t>(e, 1) * K}, f32_opts(dev));
    const int64_t FY = mean ? D : F;
    NtsVar Y = torch::empty({v, FY}, f32_opts(dev));
    hipStream_t st = (hipStream_t)cs->stream();
    if (prof) prof->begin(KernelProfiler::GAT_FWD, st);
    NTS_CALL(nts_hip_gatv2_forward, cs->ctx(), sg->dev_c_o(), sg->dev_r_i(), (uint32_t)v,
             Hs.data_ptr<float>(), (uint64_t)F, Hd.data_ptr<float>(), (uint64_t)F, (uint32_t)K,
             (uint32_t)D, Ac.data_ptr<float>(), u.data_ptr<float>(), a.data_ptr<float>(),
             Y.data_ptr<float>(), (uint64_t)FY, mean ? 1 : 0, (float)drop.p_attn,
             (float)drop.p_out, drop.seed, drop.off_attn, drop.off_out);
    // compulsory bytes: Hs and Hd rows once, offsets, row index + score + weight
    // per edge, att, output rows
    if (prof)
      prof->end(KernelProfiler::GAT_FWD, st,
                4.0 * F * s + 4.0 * F * v + 4.0 * (v + 1) + (4.0 + 8.0 * K) * e + 4.0 * F +
                    4.0 * FY * v);
    ctx->save_for_backward({Xc, Xd, Ws, Wd, Ac, Hs, Hd, Y, a, idx});
    arg.x_grad = X.requires_grad();
    arg.save(ctx);
    return Y;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto v_ = ctx->get_saved_variables();
    NtsVar X = v_[0], Xd = v_[1], Ws = v_[2], Wd = v_[3], A = v_[4], Hs = v_[5], Hd = v_[6],
           Y = v_[7], a = v_[8], idx = v_[9];
    const GatArgs arg(ctx);
    sampCSC* sg = arg.sg;
    NtsStream* cs = arg.cs;
    const GatDropout& drop = arg.drop;
    NtsVar GY = grads[0].contiguous();
    const int64_t s = Hs.size(0), F = Hs.size(1), Fin = X.size(1), v = Y.size(0);
    const int64_t e = sg->e_size;
    const int64_t K = arg.heads, D = F / K;
    const bool mean = arg.mean;
    const int64_t FY = mean ? D : F;
    const int dev = cs->device();
    auto guard = cs->guard();
    NtsVar du = torch::empty({std::max<int64_t>(e, 1) * K}, f32_opts(dev));
    NtsVar GM = torch::empty({std::max<int64_t>(v, 1), F}, f32_opts(dev));
    NtsVar dHs = torch::empty({s, F}, f32_opts(dev));
    NtsVar dHd = torch::empty({std::max<int64_t>(v, 1), F}, f32_opts(dev));
    NtsVar dA = torch::empty({F}, f32_opts(dev));
    NTS_CALL(nts_hip_gatv2_backward, cs->ctx(), sg->dev_c_o(), sg->dev_r_i(), (uint32_t)v,
             sg->dev_r_o(), sg->dev_c_i(), dptr<uint32_t>(sg->csr_edge_id), (uint32_t)s,
             Hs.data_ptr<float>(), (uint64_t)F, Hd.data_ptr<float>(), (uint64_t)F, (uint32_t)K,
             (uint32_t)D, A.data_ptr<float>(), a.data_ptr<float>(), Y.data_ptr<float>(),
             (uint64_t)FY, GY.data_ptr<float>(), (uint64_t)FY, du.data_ptr<float>(),
             GM.data_ptr<float>(), (uint64_t)F, dHs.data_ptr<float>(), (uint64_t)F,
             dHd.data_ptr<float>(), (uint64_t)F, dA.data_ptr<float>(), mean ? 1 : 0,
             (float)drop.p_attn, (float)drop.p_out, drop.seed, drop.off_attn);
    NtsVar dWs = torch::empty({Fin, F}, f32_opts(dev));
    NtsVar dWd = torch::zeros({Fin, F}, f32_opts(dev));
    gemm(*cs, 1, X, dHs, dWs, "dW_s");
    if (v) gemm(*cs, 1, Xd, dHd, dWd, "dW_d");
    NtsVar dW = torch::cat({dWs, dWd}, 1);
    NtsVar dX;
    if (arg.x_grad) {
      NtsVar Wst = Ws.t().contiguous(), Wdt = Wd.t().contiguous();
      dX = torch::empty({s, Fin}, f32_opts(dev));
      gemm(*cs, 0, dHs, Wst, dX, "dX");
      if (v) {
        NtsVar dXd = torch::empty({v, Fin}, f32_opts(dev));
        gemm(*cs, 0, dHd, Wdt, dXd, "dX_d");
        dX.index_add_(0, idx, dXd);  // injective: one addend per row
      }
    }
    return no_grads({dX, dW, dA.view(A.sizes())}, 1);
  }
};

NtsVar hip_gatv2_layer(const NtsVar& x, const NtsVar& W, const NtsVar& att, sampCSC* sg,
                       NtsStream* cs, KernelProfiler* prof, int heads, bool mean,
                       const GatDropout& drop) {
  const GatArgs args("GATv2", sg, cs, prof, heads, mean, drop);
  return HipGATv2LayerFn::apply(x, W, att, to_handle(&args));
}

NtsVar hip_dropout(const NtsVar& x, double p, uint64_t seed, uint64_t offset, NtsStream* cs) {
  NtsVar xc = row_major(x);
  NtsVar y = torch::empty({xc.size(0), xc.size(1)}, xc.options());
  NTS_CALL(nts_hip_dropout_f32, cs->ctx(), (uint32_t)xc.size(0), (uint32_t)xc.size(1),
           xc.data_ptr<float>(), (uint64_t)xc.stride(0), (float)p, seed, offset,
           y.data_ptr<float>(), (uint64_t)y.size(1));
  return y;
}

}  // namespace nts
