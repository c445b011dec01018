// C++ host layer, dense side: the autograd functions of the linear layers,
// the transform-first bottom layer, the activations and norms, and the fused
// output-layer losses.
#include <algorithm>

#include "ops_util.hpp"

namespace nts {

// ---------------------------------------------------------------------------
// Row-major with unit column stride (rows may be padded); copies otherwise.
NtsVar row_major(const NtsVar& x) {
  return (x.dim() == 2 && x.stride(1) == 1 && x.stride(0) >= x.size(1)) ? x : x.contiguous();
}

// [rows, F] fp32 whose rows start on 128-byte boundaries for wide F (the
// bottom aggregation output: aligned row writes, 16-byte A loads in the
// GEMMs that consume it).
NtsVar row_padded_empty(int64_t rows, int64_t F, int device) {
  // (F >= 64: whole 32-float k-steps for k_x3_tn's row reads, C3 / C4's F = 100)
  const int64_t ld = F >= 64 ? (F + 31) / 32 * 32 : F;
  if (ld == F) return torch::empty({rows, F}, f32_opts(device));
  return torch::empty_strided({rows, F}, {ld, 1}, f32_opts(device));
}

namespace {
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

struct HipLinearFn : public torch::autograd::Function<HipLinearFn> {
  static NtsVar forward(AutogradContext* ctx, NtsVar x, NtsVar W, int64_t cs_ptr) {
    auto* cs = from_handle<NtsStream>(cs_ptr);
    NtsVar xc = row_major(x), Wc = W.contiguous();
    const int64_t M = xc.size(0), K = xc.size(1), N = Wc.size(1);
    TORCH_CHECK(Wc.size(0) == K, "hip_linear: shape mismatch");
    NtsVar Z = torch::empty({M, N}, xc.options());
    gemm(*cs, 0, xc, Wc, Z, "nn");
    ctx->save_for_backward({xc, Wc});
    ctx->saved_data["cs"] = cs_ptr;
    return Z;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    NtsVar x = saved[0], W = saved[1];
    auto* cs = from_handle<NtsStream>(ctx->saved_data["cs"]);
    NtsVar g = grads[0].contiguous();
    NtsVar dx, dW;
    if (ctx->needs_input_grad(1)) {
      dW = torch::empty({x.size(1), W.size(1)}, W.options());
      gemm(*cs, 1, x, g, dW, "tn");
    }
    if (ctx->needs_input_grad(0)) dx = g.matmul(W.t());
    return no_grads({dx, dW}, 1);
  }
};
// dropout(relu(x W)) with the activation in the GEMM epilogue and its
// backward in the weight-gradient GEMM's operand load (nts_hip.h).
struct HipLinearActFn : public torch::autograd::Function<HipLinearActFn> {
  static NtsVar forward(AutogradContext* ctx, NtsVar x, NtsVar W, double p, int64_t seed,
                        int64_t offset, int64_t cs_ptr, bool pair_split) {
    auto* cs = from_handle<NtsStream>(cs_ptr);
    NtsVar xc = row_major(x), Wc = W.contiguous();
    const int64_t M = xc.size(0), K = xc.size(1), N = Wc.size(1);
    TORCH_CHECK(Wc.size(0) == K, "hip_linear_act: shape mismatch");
    NtsVar X = torch::empty({M, N}, xc.options());
    // a narrow input (K <= 128, N 128 or 256: the products / papers-shaped
    // aggregate-first bottom layer) on the in-kernel f16 pair split
    // (nts_hip_gemm_h2d_act) when the config allows pair-split
    // arithmetic (GCNConfig::pair_table > 0); otherwise the GEMM mode's kernel
    if (pair_split && K <= 128 && K % 4 == 0 && (N == 128 || N == 256) && xc.stride(0) % 4 == 0 &&
        (uintptr_t)xc.data_ptr<float>() % 16 == 0)
      NTS_CALL(nts_hip_gemm_h2d_act, cs->ctx(), 1, (int)M, (int)N, (int)K, xc.data_ptr<float>(),
               (uint64_t)xc.stride(0), Wc.data_ptr<float>(), (uint64_t)N, X.data_ptr<float>(),
               (uint64_t)N, (float)p, (uint64_t)seed, (uint64_t)offset, nullptr, 0, nullptr);
    else
      NTS_CALL(nts_hip_gemm_relu_dropout_f32, cs->ctx(), (int)M, (int)N, (int)K,
               xc.data_ptr<float>(), (uint64_t)xc.stride(0), Wc.data_ptr<float>(), (uint64_t)N,
               X.data_ptr<float>(), (uint64_t)N, (float)p, (uint64_t)seed, (uint64_t)offset);
    ctx->save_for_backward({xc, Wc, X});
    ctx->saved_data["cs"] = cs_ptr;
    ctx->saved_data["scale"] = keep_scale(p);
    return X;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    NtsVar x = saved[0], W = saved[1], X = saved[2];
    auto* cs = from_handle<NtsStream>(ctx->saved_data["cs"]);
    const float scale = (float)ctx->saved_data["scale"].toDouble();
    NtsVar g = grads[0].contiguous();
    const int64_t M = x.size(0), K = x.size(1), N = W.size(1);
    NtsVar dx, dW;
    if (ctx->needs_input_grad(1)) {
      dW = torch::empty({K, N}, W.options());
      NTS_CALL(nts_hip_gemm_tn_masked_f32, cs->ctx(), (int)K, (int)N, (int)M, x.data_ptr<float>(),
               (uint64_t)x.stride(0), g.data_ptr<float>(), (uint64_t)N, X.data_ptr<float>(),
               (uint64_t)N, scale, dW.data_ptr<float>(), (uint64_t)N);
    }
    if (ctx->needs_input_grad(0)) {
      // dx = (g ⊙ [X > 0] / (1-p)) W^T: the activation backward
      // (nts_hip_act_backward) and the layer GEMM, not three torch
      // elementwise kernels and a library GEMM
      NtsVar dZ = torch::empty({M, N}, g.options());
      act_backward(*cs, g, X, scale, dZ);
      NtsVar Wt = W.t().contiguous();
      dx = torch::empty({M, K}, g.options());
      gemm(*cs, 0, dZ, Wt, dx, "dx");
    }
    return no_grads({dx, dW}, 5);
  }
};

// Transform-first bottom layer (nts_hip.h):
//   H = X[source] W      (row-gathered MFMA GEMM: load_feature_gpu fused away)
//   X1 = dropout(relu(A H))  (the graph op over F_out-wide rows, activation in
//                             the epilogue with the GEMM epilogue's mask keys)
// backward: dH = A^T (dX1 ⊙ [X1 > 0] / (1-p)) over the CSR, dW = X[source]^T dH.
// Recorded as one NN op whose input is the feature table (the bottom graph
// op has no backward, core/ntsContext.hpp:443-444).
std::function<void()> g_after_fwd_gemm, g_before_bwd_gemm;  // set_bottom_gemm_hooks

struct HipBottomTFFn : public torch::autograd::Function<HipBottomTFFn> {
  static NtsVar forward(AutogradContext* ctx, NtsVar table, NtsVar W, int64_t sg_ptr,
                        int64_t cs_ptr, double p, int64_t seed, int64_t offset, int64_t prof_ptr,
                        int64_t h_out, int64_t pairs_ptr) {
    const auto* pairs = from_handle<const PairTable>(pairs_ptr);
    auto* cs = from_handle<NtsStream>(cs_ptr);
    auto* sg = from_handle<sampCSC>(sg_ptr);
    auto* prof = from_handle<KernelProfiler>(prof_ptr);
    NtsVar Wc = W.contiguous();
    const int64_t F = table.size(1), N = Wc.size(1);
    const int64_t s = sg->src_size, v = sg->v_size, e = sg->e_size;
    TORCH_CHECK(Wc.size(0) == F && table.stride(1) == 1, "transform-first: shape mismatch");
    const int dev = cs->device();
    hipStream_t st = (hipStream_t)cs->stream();
    NtsVar H = h_out ? NtsVar() : torch::empty({std::max<int64_t>(s, 1), N}, f32_opts(dev));
    float* hp = h_out ? from_handle<float>(h_out) : H.data_ptr<float>();
    if (prof) prof->begin(KernelProfiler::GATHER_GEMM, st);
    if (pairs && pairs->Q.defined())
      NTS_CALL(nts_hip_gemm_h2p_gather, cs->ctx(), 0, (int)s, (int)N, pairs->kp(),
               pairs->q_ptr(), (uint64_t)pairs->Q.stride(0), pairs->rs.data_ptr<float>(),
               sg->dev_src(), Wc.data_ptr<float>(), (uint64_t)N, (int)F, hp, (uint64_t)N, 0.f, 0,
               0);
    else if (pairs && pairs->P.defined())
      NTS_CALL(nts_hip_gemm_h2_gather, cs->ctx(), 0, (int)s, (int)N, pairs->kp(),
               pairs->p_ptr(), (uint64_t)pairs->P.stride(0), pairs->rs.data_ptr<float>(),
               sg->dev_src(), Wc.data_ptr<float>(), (uint64_t)N, (int)F, hp, (uint64_t)N, 0.f, 0,
               0);
    else
      NTS_CALL(nts_hip_gemm_gather_f32, cs->ctx(), (int)s, (int)N, (int)F, table.data_ptr<float>(),
               (uint64_t)table.stride(0), sg->dev_src(), Wc.data_ptr<float>(), (uint64_t)N, hp,
               (uint64_t)N);
    if (prof) prof->end(KernelProfiler::GATHER_GEMM, st, 2.0 * (double)s * F * N);
    if (g_after_fwd_gemm) g_after_fwd_gemm();
    NtsVar X1 = torch::empty({v, N}, f32_opts(dev));
    if (prof) prof->begin(KernelProfiler::BOTTOM_AGG, st);
    // the keep mask [X1 > 0] also as bits (16 B a 128-float row), which the
    // graph op above reads in its fused activation backward instead of X1
    const uint32_t words = nts_hip_act_bits_words((uint32_t)N);
    if (words) {
      const int64_t need = std::max<int64_t>((int64_t)sg->v_cap, 1) * words;
      if (!sg->act_bits.defined() || sg->act_bits.numel() < need)
        sg->act_bits = torch::empty({need}, torch::TensorOptions().dtype(torch::kInt32).device(
                                                torch::kCUDA, dev));
      NTS_CALL(nts_hip_spmm_csc_fwd_act_bits, cs->ctx(), sg->dev_c_o(), sg->dev_r_i(),
               sg->dev_e_w_f(), nullptr, (uint32_t)v, hp, (uint64_t)N, (uint32_t)N,
               X1.data_ptr<float>(), (uint64_t)N, (float)p, (uint64_t)seed, (uint64_t)offset,
               dptr<uint32_t>(sg->act_bits));
    } else {
      NTS_CALL(nts_hip_spmm_csc_fwd_act, cs->ctx(), sg->dev_c_o(), sg->dev_r_i(), sg->dev_e_w_f(),
               nullptr, (uint32_t)v, hp, (uint64_t)N, (uint32_t)N, X1.data_ptr<float>(),
               (uint64_t)N, (float)p, (uint64_t)seed, (uint64_t)offset);
    }
    // compulsory bytes: each H row once, index + weight per edge, offsets, output
    if (prof)
      prof->end(KernelProfiler::BOTTOM_AGG, st,
                4.0 * N * s + 8.0 * e + 4.0 * (v + 1) + 4.0 * N * v);
    ctx->save_for_backward({table, Wc, X1});
    ctx->saved_data["sg"] = sg_ptr;
    ctx->saved_data["cs"] = cs_ptr;
    ctx->saved_data["prof"] = prof_ptr;
    ctx->saved_data["pairs"] = pairs_ptr;
    ctx->saved_data["scale"] = keep_scale(p);
    return X1;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    NtsVar table = saved[0], W = saved[1], X1 = saved[2];
    auto* cs = from_handle<NtsStream>(ctx->saved_data["cs"]);
    auto* sg = from_handle<sampCSC>(ctx->saved_data["sg"]);
    auto* prof = from_handle<KernelProfiler>(ctx->saved_data["prof"]);
    TORCH_CHECK(sg->has_csr, "transform-first backward needs the bottom layer's CSR");
    NtsVar g = grads[0].contiguous();
    const int64_t F = table.size(1), N = W.size(1), s = sg->src_size, v = sg->v_size;
    const int dev = cs->device();
    hipStream_t st = (hipStream_t)cs->stream();
    NtsVar dH = torch::empty({std::max<int64_t>(s, 1), N}, f32_opts(dev));
    const float scale = (float)ctx->saved_data["scale"].toDouble();
    const auto* pairs = from_handle<const PairTable>(ctx->saved_data["pairs"]);
    const PairTable* pairs_q = pairs && pairs->tn && pairs->Q.defined() ? pairs : nullptr;
    NtsVar colmax;  // dH's per-part column maxima (int32 bits), when the gather produced them
    uint32_t rpp = 0;
    // dZ = dX1 ⊙ mask once per dst row, then the plain CSR gather (measured
    // faster than applying the mask to every gathered row:
    // nts_hip_spmm_csr_bwd_masked reads two rows per edge); premasked: the
    // graph op above applied the activation backward already (its act_bwd)
    NtsVar dZ = sg->grad_premasked ? g : torch::empty({std::max<int64_t>(v, 1), N}, f32_opts(dev));
    if (!sg->grad_premasked)
      act_backward(*cs, g, X1, scale, dZ);
    if (prof) prof->begin(KernelProfiler::BOTTOM_BWD, st);
    // the planar-table TN GEMM takes dH's column maxima per part of rows
    // from this gather's epilogue (one read of dH instead of two)
    // (its float4 rows need 16-byte aligned dZ / dH rows: else the plain gather)
    const bool cm_rows = N <= 512 && N % 4 == 0 && (uintptr_t)dZ.data_ptr<float>() % 16 == 0 &&
                         (uintptr_t)dH.data_ptr<float>() % 16 == 0;
    if (pairs_q && cm_rows) {
      rpp = nts_hip_csr_bwd_colmax_rows_per_part((uint32_t)N);
      const int64_t nparts = (std::max<int64_t>(s, 1) + rpp - 1) / rpp;
      colmax = torch::empty({nparts, N}, torch::TensorOptions().dtype(torch::kInt32).device(torch::kCUDA, dev));
      NTS_CALL(nts_hip_spmm_csr_bwd_colmax, cs->ctx(), sg->dev_r_o(), sg->dev_c_i(),
               sg->dev_e_w_b(), nullptr, (uint32_t)s, dZ.data_ptr<float>(), (uint64_t)N,
               (uint32_t)N, dH.data_ptr<float>(), (uint64_t)N,
               dptr<uint32_t>(colmax), pairs_q->rs.data_ptr<float>(), sg->dev_src());
    } else {
      NTS_CALL(nts_hip_spmm_csr_bwd, cs->ctx(), sg->dev_r_o(), sg->dev_c_i(), sg->dev_e_w_b(),
               nullptr, (uint32_t)s, dZ.data_ptr<float>(), (uint64_t)N, (uint32_t)N,
               dH.data_ptr<float>(), (uint64_t)N);
    }
    if (prof)
      prof->end(KernelProfiler::BOTTOM_BWD, st,
                4.0 * N * v + 8.0 * sg->e_size + 4.0 * (s + 1) + 4.0 * N * s);
    NtsVar dW = torch::empty({F, N}, W.options());
    if (g_before_bwd_gemm) g_before_bwd_gemm();
    if (prof) prof->begin(KernelProfiler::GATHER_GEMM_TN, st);
    if (pairs_q && colmax.defined())
      NTS_CALL(nts_hip_gemm_h2p_tn_gather_cm, cs->ctx(), (int)F, (int)N, (int)s,
               pairs->q_ptr(), (uint64_t)pairs->Q.stride(0), pairs->kp(),
               pairs->rs.data_ptr<float>(), sg->dev_src(), dH.data_ptr<float>(), (uint64_t)N,
               dW.data_ptr<float>(), (uint64_t)N,
               dptr<const uint32_t>(colmax), rpp);
    else if (pairs_q)
      NTS_CALL(nts_hip_gemm_h2p_tn_gather, cs->ctx(), (int)F, (int)N, (int)s,
               pairs->q_ptr(), (uint64_t)pairs->Q.stride(0), pairs->kp(),
               pairs->rs.data_ptr<float>(), sg->dev_src(), dH.data_ptr<float>(), (uint64_t)N,
               dW.data_ptr<float>(), (uint64_t)N);
    else if (pairs && pairs->tn && pairs->P.defined())
      NTS_CALL(nts_hip_gemm_h2_tn_gather, cs->ctx(), (int)F, (int)N, (int)s,
               pairs->p_ptr(), (uint64_t)pairs->P.stride(0), pairs->rs.data_ptr<float>(),
               sg->dev_src(), dH.data_ptr<float>(), (uint64_t)N, nullptr, 0, 1.f,
               dW.data_ptr<float>(), (uint64_t)N);
    else
      NTS_CALL(nts_hip_gemm_tn_gather_f32, cs->ctx(), (int)F, (int)N, (int)s,
               table.data_ptr<float>(), (uint64_t)table.stride(0), sg->dev_src(),
               dH.data_ptr<float>(), (uint64_t)N, dW.data_ptr<float>(), (uint64_t)N);
    if (prof) prof->end(KernelProfiler::GATHER_GEMM_TN, st, 2.0 * (double)s * F * N);
    return no_grads({NtsVar(), dW}, 8);
  }
};
// Output layer + loss in fused kernels (nts_hip.h).  Under grad mode the
// forward runs the training kernel: loss, dY and dW for d loss = 1 in one pass
// over Y; the backward returns them when the upstream gradient is the unit
// seed of self_backward (exactly 1), and otherwise runs the backward kernel.
struct HipLinearXentFn : public torch::autograd::Function<HipLinearXentFn> {
  static NtsVar forward(AutogradContext* ctx, NtsVar y, NtsVar W, NtsVar target, int64_t cs_ptr,
                        bool train, int64_t correct_ptr) {
    auto* correct = from_handle<uint32_t>(correct_ptr);
    auto* cs = from_handle<NtsStream>(cs_ptr);
    NtsVar yc = row_major(y), Wc = W.contiguous(), tc = target.contiguous();
    const int64_t n = yc.size(0), K = yc.size(1), C = Wc.size(1);
    TORCH_CHECK(Wc.size(0) == K && tc.numel() == n && tc.scalar_type() == torch::kInt64,
                "hip_linear_xent: shape mismatch");
    NtsVar loss = torch::empty({}, yc.options());
    if (train) {
      NtsVar dY = torch::empty({n, K}, yc.options());
      NtsVar dW = torch::empty({K, C}, Wc.options());
      NTS_CALL(nts_hip_linear_xent_train, cs->ctx(), yc.data_ptr<float>(), (uint64_t)yc.stride(0),
               (int)n, (int)K, Wc.data_ptr<float>(), (int)C, tc.data_ptr<int64_t>(),
               loss.data_ptr<float>(), dY.data_ptr<float>(), dW.data_ptr<float>(), correct);
      ctx->saved_data["dY"] = dY;
      ctx->saved_data["dW"] = dW;
    } else {
      NTS_CALL(nts_hip_linear_xent_fwd, cs->ctx(), yc.data_ptr<float>(), (uint64_t)yc.stride(0),
               (int)n, (int)K, Wc.data_ptr<float>(), (int)C, tc.data_ptr<int64_t>(),
               loss.data_ptr<float>(), correct);
    }
    ctx->save_for_backward({yc, Wc, tc});
    ctx->saved_data["cs"] = cs_ptr;
    return loss;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    NtsVar y = saved[0], W = saved[1], t = saved[2];
    auto* cs = from_handle<NtsStream>(ctx->saved_data["cs"]);
    NtsVar g = grads[0];
    NtsVar dY, dW;
    if (ctx->saved_data.count("dY") &&
        g.data_ptr() == unit_scalar(g.device()).data_ptr()) {  // d loss == 1: precomputed
      dY = ctx->saved_data["dY"].toTensor();
      dW = ctx->saved_data["dW"].toTensor();
    } else {
      g = g.contiguous();
      const int64_t n = y.size(0), K = y.size(1), C = W.size(1);
      dY = torch::empty({n, K}, y.options());
      dW = torch::empty({K, C}, W.options());
      NTS_CALL(nts_hip_linear_xent_bwd, cs->ctx(), y.data_ptr<float>(), (uint64_t)y.stride(0),
               (int)n, (int)K, W.data_ptr<float>(), (int)C, t.data_ptr<int64_t>(),
               g.data_ptr<float>(), dY.data_ptr<float>(), dW.data_ptr<float>());
    }
    ctx->saved_data.erase("dY");
    ctx->saved_data.erase("dW");
    return no_grads({ctx->needs_input_grad(0) ? dY : NtsVar(), dW}, 4);
  }
};
// Multi-label output layer + mean sigmoid-BCE in fused kernels (nts_hip.h).
// Under grad mode the forward runs the training kernel (loss, dY and dW for
// d loss = 1); the backward returns them, scaled when the upstream gradient
// is not the unit seed of self_backward.
struct HipLinearBceFn : public torch::autograd::Function<HipLinearBceFn> {
  static NtsVar forward(AutogradContext* ctx, NtsVar y, NtsVar W, NtsVar bits, int64_t index_ptr,
                        int64_t cs_ptr, bool train, int64_t counts_ptr) {
    auto* counts = from_handle<uint32_t>(counts_ptr);
    auto* index = from_handle<const uint32_t>(index_ptr);
    auto* cs = from_handle<NtsStream>(cs_ptr);
    NtsVar yc = row_major(y), Wc = W.contiguous();
    const int64_t n = yc.size(0), K = yc.size(1), C = Wc.size(1);
    TORCH_CHECK(Wc.size(0) == K && bits.dim() == 2 && bits.is_contiguous() &&
                    bits.scalar_type() == torch::kInt32 && bits.size(1) == (C + 31) / 32,
                "hip_linear_bce: shape mismatch");
    const auto* lb = dptr<const uint32_t>(bits);
    NtsVar loss = torch::empty({}, yc.options());
    if (train) {
      NtsVar dY = torch::empty({n, K}, yc.options());
      NtsVar dW = torch::empty({K, C}, Wc.options());
      NTS_CALL(nts_hip_linear_bce_train, cs->ctx(), yc.data_ptr<float>(), (uint64_t)yc.stride(0),
               (int)n, (int)K, Wc.data_ptr<float>(), (int)C, lb, (uint32_t)bits.size(1), index,
               loss.data_ptr<float>(), dY.data_ptr<float>(), dW.data_ptr<float>(), counts);
      ctx->saved_data["dY"] = dY;
      ctx->saved_data["dW"] = dW;
    } else {
      NTS_CALL(nts_hip_linear_bce_fwd, cs->ctx(), yc.data_ptr<float>(), (uint64_t)yc.stride(0),
               (int)n, (int)K, Wc.data_ptr<float>(), (int)C, lb, (uint32_t)bits.size(1), index,
               loss.data_ptr<float>(), counts);
    }
    return loss;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    TORCH_CHECK(ctx->saved_data.count("dY"), "hip_linear_bce: backward without a training forward");
    NtsVar g = grads[0];
    NtsVar dY = ctx->saved_data["dY"].toTensor(), dW = ctx->saved_data["dW"].toTensor();
    if (g.data_ptr() != unit_scalar(g.device()).data_ptr()) {  // d loss != the unit seed
      dY = dY * g;
      dW = dW * g;
    }
    ctx->saved_data.erase("dY");
    ctx->saved_data.erase("dW");
    return no_grads({ctx->needs_input_grad(0) ? dY : NtsVar(), dW}, 5);
  }
};
}  // namespace

namespace {
struct HipLpBceFn : public torch::autograd::Function<HipLpBceFn> {
  static NtsVar forward(AutogradContext* ctx, NtsVar h, int64_t pairs_ptr, NtsVar score,
                        int64_t cs_ptr, bool train, int64_t mrr_ptr) {
    const auto& pr = *from_handle<const LpPairs>(pairs_ptr);
    auto* cs = from_handle<NtsStream>(cs_ptr);
    auto* mrr = from_handle<float>(mrr_ptr);
    NtsVar hc = row_major(h);
    const int64_t n = hc.size(0), D = hc.size(1);
    const int64_t P = (int64_t)pr.B * (1 + (int64_t)pr.K);
    TORCH_CHECK(score.is_cuda() && score.scalar_type() == torch::kFloat32 && score.numel() >= P,
                "hip_lp_bce: score must hold one float per pair");
    NtsVar loss = torch::empty({}, hc.options());
    if (train) {
      NtsVar dH = torch::empty({n, D}, hc.options());
      NTS_CALL(nts_hip_lp_bce_train, cs->ctx(), hc.data_ptr<float>(), (uint64_t)hc.stride(0),
               (uint32_t)D, pr.pair_u, pr.pair_v, pr.B, pr.K, pr.inc_offset, pr.inc_slot, pr.v_size,
               (uint32_t)n, score.data_ptr<float>(), loss.data_ptr<float>(), dH.data_ptr<float>(),
               (uint64_t)D, mrr);
      ctx->saved_data["dH"] = dH;
    } else {
      NTS_CALL(nts_hip_lp_bce_fwd, cs->ctx(), hc.data_ptr<float>(), (uint64_t)hc.stride(0),
               (uint32_t)D, pr.pair_u, pr.pair_v, pr.B, pr.K, score.data_ptr<float>(),
               loss.data_ptr<float>(), mrr);
    }
    return loss;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    TORCH_CHECK(ctx->saved_data.count("dH"), "hip_lp_bce: backward without a training forward");
    NtsVar g = grads[0];
    NtsVar dH = ctx->saved_data["dH"].toTensor();
    if (g.data_ptr() != unit_scalar(g.device()).data_ptr()) dH = dH * g;  // d loss != the unit seed
    ctx->saved_data.erase("dH");
    return no_grads({dH}, 5);
  }
};
}  // namespace

NtsVar hip_lp_bce(const NtsVar& h, const LpPairs& pairs, NtsVar& score, NtsStream* cs, float* mrr) {
  const bool train = torch::GradMode::is_enabled() && h.requires_grad();
  return HipLpBceFn::apply(h, to_handle(&pairs), score, to_handle(cs), train, to_handle(mrr));
}

NtsVar hip_linear_act(const NtsVar& x, const NtsVar& W, double p, uint64_t seed, uint64_t offset,
                      NtsStream* cs, bool pair_split) {
  return HipLinearActFn::apply(x, W, p, (int64_t)seed, (int64_t)offset, to_handle(cs), pair_split);
}

// dropout(relu(x)) on its own (nts_hip_relu_dropout_f32, the GEMM epilogue's
// keep bits); backward dx = dy ⊙ [y > 0] / (1-p) (nts_hip_act_backward)
struct HipActFn : public torch::autograd::Function<HipActFn> {
  static NtsVar forward(AutogradContext* ctx, NtsVar x, double p, int64_t seed, int64_t offset,
                        int64_t cs_ptr) {
    auto* cs = from_handle<NtsStream>(cs_ptr);
    NtsVar xc = row_major(x);
    NtsVar y = torch::empty({xc.size(0), xc.size(1)}, xc.options());
    NTS_CALL(nts_hip_relu_dropout_f32, cs->ctx(), (uint32_t)xc.size(0), (uint32_t)xc.size(1),
             xc.data_ptr<float>(), (uint64_t)xc.stride(0), (float)p, (uint64_t)seed,
             (uint64_t)offset, y.data_ptr<float>(), (uint64_t)y.size(1));
    ctx->save_for_backward({y});
    ctx->saved_data["cs"] = cs_ptr;
    ctx->saved_data["scale"] = keep_scale(p);
    return y;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    NtsVar y = ctx->get_saved_variables()[0];
    auto* cs = from_handle<NtsStream>(ctx->saved_data["cs"]);
    NtsVar g = grads[0].contiguous();
    NtsVar dx = torch::empty_like(y);
    act_backward(*cs, g, y, (float)ctx->saved_data["scale"].toDouble(), dx);
    return no_grads({dx}, 4);
  }
};

NtsVar hip_relu_dropout(const NtsVar& x, double p, uint64_t seed, uint64_t offset, NtsStream* cs) {
  return HipActFn::apply(x, p, (int64_t)seed, (int64_t)offset, to_handle(cs));
}

// dropout(relu(LayerNorm(z))) in one pass (nts_hip_ln_act_fwd); backward dz,
// dgamma, dbeta in one pass plus the partials' reduction (nts_hip_ln_act_bwd).
// Without a backward to come (eval, inference) nothing is saved.
struct HipLnActFn : public torch::autograd::Function<HipLnActFn> {
  static NtsVar forward(AutogradContext* ctx, NtsVar z, NtsVar gamma, NtsVar beta, double eps,
                        double p, int64_t seed, int64_t offset, int64_t cs_ptr, bool train) {
    auto* cs = from_handle<NtsStream>(cs_ptr);
    NtsVar zc = row_major(z), gc = gamma.contiguous(), bc = beta.contiguous();
    const int64_t M = zc.size(0), N = zc.size(1);
    TORCH_CHECK(gc.numel() == N && bc.numel() == N, "hip_ln_act: shape mismatch");
    NtsVar y = torch::empty({M, N}, zc.options());
    NtsVar mean, rstd;
    if (train) {
      mean = torch::empty({M}, zc.options());
      rstd = torch::empty({M}, zc.options());
    }
    NTS_CALL(nts_hip_ln_act_fwd, cs->ctx(), (uint64_t)M, (uint32_t)N, zc.data_ptr<float>(),
             (uint64_t)zc.stride(0), gc.data_ptr<float>(), bc.data_ptr<float>(), (float)eps,
             (float)p, (uint64_t)seed, (uint64_t)offset, y.data_ptr<float>(), (uint64_t)N,
             train ? mean.data_ptr<float>() : nullptr, train ? rstd.data_ptr<float>() : nullptr);
    if (train) ctx->save_for_backward({zc, y, mean, rstd, gc});
    ctx->saved_data["cs"] = cs_ptr;
    ctx->saved_data["scale"] = keep_scale(p);
    return y;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    TORCH_CHECK(saved.size() == 5, "hip_ln_act: backward without a training forward");
    NtsVar z = saved[0], y = saved[1], mean = saved[2], rstd = saved[3], gamma = saved[4];
    auto* cs = from_handle<NtsStream>(ctx->saved_data["cs"]);
    NtsVar g = grads[0].contiguous();
    const int64_t M = y.size(0), N = y.size(1);
    NtsVar dz = torch::empty({M, N}, y.options());
    NtsVar dgamma = torch::empty({N}, y.options()), dbeta = torch::empty({N}, y.options());
    NTS_CALL(nts_hip_ln_act_bwd, cs->ctx(), (uint64_t)M, (uint32_t)N, g.data_ptr<float>(),
             (uint64_t)N, y.data_ptr<float>(), (uint64_t)N, z.data_ptr<float>(),
             (uint64_t)z.stride(0), mean.data_ptr<float>(), rstd.data_ptr<float>(),
             gamma.data_ptr<float>(), (float)ctx->saved_data["scale"].toDouble(),
             dz.data_ptr<float>(), (uint64_t)N, dgamma.data_ptr<float>(), dbeta.data_ptr<float>());
    return no_grads({dz, dgamma, dbeta}, 6);
  }
};

NtsVar hip_ln_act(const NtsVar& z, const NtsVar& gamma, const NtsVar& beta, double eps, double p,
                  uint64_t seed, uint64_t offset, NtsStream* cs) {
  // a backward follows only under grad mode with an input requiring grad
  const bool train = torch::GradMode::is_enabled() &&
                     (z.requires_grad() || gamma.requires_grad() || beta.requires_grad());
  return HipLnActFn::apply(z, gamma, beta, eps, p, (int64_t)seed, (int64_t)offset, to_handle(cs),
                           train);
}

// dropout(relu(BatchNorm(z))) from the batch's statistics (nts_hip_bn_act_fwd:
// statistics, running-buffer update and the apply pass); backward dz, dgamma,
// dbeta in a reduction and an apply pass (nts_hip_bn_act_bwd).
struct HipBnActFn : public torch::autograd::Function<HipBnActFn> {
  static NtsVar forward(AutogradContext* ctx, NtsVar z, NtsVar gamma, NtsVar beta,
                        NtsVar running_mean, NtsVar running_var, double eps, double momentum,
                        double p, int64_t seed, int64_t offset, int64_t cs_ptr) {
    auto* cs = from_handle<NtsStream>(cs_ptr);
    NtsVar zc = row_major(z), gc = gamma.contiguous(), bc = beta.contiguous();
    const int64_t M = zc.size(0), N = zc.size(1);
    TORCH_CHECK(gc.numel() == N && bc.numel() == N, "hip_bn_act: shape mismatch");
    NtsVar y = torch::empty({M, N}, zc.options());
    NtsVar mean = torch::empty({N}, zc.options()), rstd = torch::empty({N}, zc.options());
    NTS_CALL(nts_hip_bn_act_fwd, cs->ctx(), (uint64_t)M, (uint32_t)N, zc.data_ptr<float>(),
             (uint64_t)zc.stride(0), gc.data_ptr<float>(), bc.data_ptr<float>(), (float)eps,
             (float)momentum, (float)p, (uint64_t)seed, (uint64_t)offset, y.data_ptr<float>(),
             (uint64_t)N, mean.data_ptr<float>(), rstd.data_ptr<float>(),
             running_mean.data_ptr<float>(), running_var.data_ptr<float>());
    ctx->save_for_backward({zc, y, mean, rstd, gc});
    ctx->saved_data["cs"] = cs_ptr;
    ctx->saved_data["scale"] = keep_scale(p);
    return y;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    NtsVar z = saved[0], y = saved[1], mean = saved[2], rstd = saved[3], gamma = saved[4];
    auto* cs = from_handle<NtsStream>(ctx->saved_data["cs"]);
    NtsVar g = grads[0].contiguous();
    const int64_t M = y.size(0), N = y.size(1);
    NtsVar dz = torch::empty({M, N}, y.options());
    NtsVar dgamma = torch::empty({N}, y.options()), dbeta = torch::empty({N}, y.options());
    NTS_CALL(nts_hip_bn_act_bwd, cs->ctx(), (uint64_t)M, (uint32_t)N, g.data_ptr<float>(),
             (uint64_t)N, y.data_ptr<float>(), (uint64_t)N, z.data_ptr<float>(),
             (uint64_t)z.stride(0), mean.data_ptr<float>(), rstd.data_ptr<float>(),
             gamma.data_ptr<float>(), (float)ctx->saved_data["scale"].toDouble(),
             dz.data_ptr<float>(), (uint64_t)N, dgamma.data_ptr<float>(), dbeta.data_ptr<float>());
    return no_grads({dz, dgamma, dbeta}, 8);
  }
};

NtsVar hip_bn_act(const NtsVar& z, const NtsVar& gamma, const NtsVar& beta,
                  const NtsVar& running_mean, const NtsVar& running_var, bool train, double eps,
                  double momentum, double p, uint64_t seed, uint64_t offset, NtsStream* cs) {
  const int64_t N = z.size(1);
  TORCH_CHECK(running_mean.is_contiguous() && running_var.is_contiguous() &&
                  running_mean.numel() == N && running_var.numel() == N,
              "hip_bn_act: running statistics must be contiguous [F]");
  if (train)
    return HipBnActFn::apply(z, gamma, beta, running_mean, running_var, eps, momentum, p,
                             (int64_t)seed, (int64_t)offset, to_handle(cs));
  // eval: the running statistics, one elementwise pass, no graph
  torch::NoGradGuard ng;
  NtsVar zc = row_major(z), gc = gamma.contiguous(), bc = beta.contiguous();
  TORCH_CHECK(gc.numel() == N && bc.numel() == N, "hip_bn_act: shape mismatch");
  NtsVar y = torch::empty({zc.size(0), N}, zc.options());
  NTS_CALL(nts_hip_bn_act_eval, cs->ctx(), (uint64_t)zc.size(0), (uint32_t)N, zc.data_ptr<float>(),
           (uint64_t)zc.stride(0), gc.data_ptr<float>(), bc.data_ptr<float>(),
           running_mean.data_ptr<float>(), running_var.data_ptr<float>(), (float)eps,
           y.data_ptr<float>(), (uint64_t)N);
  return y;
}

void set_bottom_gemm_hooks(std::function<void()> after_fwd_gemm,
                           std::function<void()> before_bwd_gemm) {
  g_after_fwd_gemm = std::move(after_fwd_gemm);
  g_before_bwd_gemm = std::move(before_bwd_gemm);
}

NtsVar hip_bottom_transform(const NtsVar& table, const NtsVar& W, sampCSC* sg, double p,
                            uint64_t seed, uint64_t offset, NtsStream* cs, KernelProfiler* prof,
                            float* h_out, const PairTable* pairs) {
  return HipBottomTFFn::apply(table, W, to_handle(sg), to_handle(cs), p, (int64_t)seed,
                              (int64_t)offset, to_handle(prof), to_handle(h_out), to_handle(pairs));
}

NtsVar hip_linear(const NtsVar& x, const NtsVar& W, NtsStream* cs) {
  return HipLinearFn::apply(x, W, to_handle(cs));
}

bool hip_linear_xent_supported(int64_t K, int64_t C) {
  // mirrors the argument checks of nts_hip_linear_xent_fwd/bwd/train:
  // K % 16 == 0; C <= 64 with W, 64 Y rows and 64 dZ rows in LDS; 64 < C <= 512
  // (the wide form, W streamed from global memory) with K <= 512
  const int64_t Cp = (C + 15) / 16 * 16;
  if (K < 16 || K % 16 != 0 || C < 1 || C > 512) return false;
  if (C > 64) return K <= 512;
  return (K * Cp + 64 * (K + 4) + 64 * Cp) * 4 <= 160 * 1024;
}

bool hip_linear_bce_supported(int64_t K, int64_t C) {
  // mirrors the argument checks of nts_hip_linear_bce_fwd/train (C <= 128,
  // K % 16 == 0; W, 16 Y rows, 5 x 16 logit rows and 16 words in LDS)
  const int64_t Cp = (C + 15) / 16 * 16;
  return K >= 16 && K % 16 == 0 && C >= 1 && C <= 128 &&
         (K * Cp + 16 * (K + 4) + 5 * 16 * Cp + 16) * 4 <= 160 * 1024;
}

NtsVar hip_linear_bce(const NtsVar& y, const NtsVar& W, const NtsVar& label_bits,
                      const VertexId* index, NtsStream* cs, uint32_t* counts) {
  const bool train = torch::GradMode::is_enabled() && (y.requires_grad() || W.requires_grad());
  return HipLinearBceFn::apply(y, W, label_bits, to_handle(index), to_handle(cs), train,
                               to_handle(counts));
}

NtsVar pack_label_bits(const NtsVar& labels) {
  TORCH_CHECK(labels.dim() == 2 && labels.size(1) >= 1, "multi-label targets must be [V, C]");
  const auto dt = labels.scalar_type();
  TORCH_CHECK(dt == torch::kUInt8 || dt == torch::kBool || dt == torch::kInt64,
              "multi-label targets must be uint8, bool or int64");
  const int64_t V = labels.size(0), C = labels.size(1), wpr = (C + 31) / 32;
  NtsVar out = torch::empty({V, wpr}, labels.options().dtype(torch::kInt32));
  NtsVar weight = torch::ones({1}, labels.options().dtype(torch::kInt64))
                      .bitwise_left_shift(torch::arange(32, labels.options().dtype(torch::kInt64)));
  const int64_t chunk = 1 << 16;  // rows per pass: bounds the int64 temporaries
  for (int64_t r = 0; r < V; r += chunk) {
    const int64_t m = std::min(chunk, V - r);
    NtsVar x = labels.narrow(0, r, m).to(torch::kInt64);
    TORCH_CHECK(!x.lt(0).logical_or(x.gt(1)).any().item<bool>(),
                "multi-label targets must be 0 or 1");
    x = torch::constant_pad_nd(x, {0, wpr * 32 - C}).view({m, wpr, 32});
    NtsVar wd = (x * weight).sum(2);  // in [0, 2^32): wrap bit 31 into int32
    wd = wd - wd.bitwise_right_shift(31).bitwise_left_shift(32);
    out.narrow(0, r, m).copy_(wd);
  }
  return out;
}

NtsVar unpack_label_bits(const NtsVar& words, int64_t C) {
  NtsVar sh = torch::arange(32, words.options().dtype(torch::kInt64));
  NtsVar b = words.to(torch::kInt64).unsqueeze(2).bitwise_right_shift(sh).bitwise_and(1);
  return b.view({words.size(0), words.size(1) * 32}).narrow(1, 0, C).to(torch::kFloat32);
}

NtsVar hip_linear_xent(const NtsVar& y, const NtsVar& W, const NtsVar& target, NtsStream* cs,
                       uint32_t* correct) {
  // a backward follows only under grad mode with an input requiring grad
  const bool train = torch::GradMode::is_enabled() && (y.requires_grad() || W.requires_grad());
  return HipLinearXentFn::apply(y, W, target, to_handle(cs), train, to_handle(correct));
}

}  // namespace nts
