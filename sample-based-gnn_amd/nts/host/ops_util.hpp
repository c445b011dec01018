// Private helpers of the host layer's translation units (not part of
// nts_host.hpp): the one typed call path from libtorch tensors to the C-ABI.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "nts_host.hpp"

namespace nts {

inline void hip_rt(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// NTS_HOST_PROFILE=1: host-side durations of the sampler issue/finish calls
inline bool host_profile() {
  static const bool on = getenv("NTS_HOST_PROFILE") != nullptr;
  return on;
}

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// A C-ABI call checked under its own name: NTS_CALL(nts_hip_adam, ctx, ...).
// (Calls whose label says more than the name keep hip_check.)
#define NTS_CALL(fn, ...) ::nts::hip_check(fn(__VA_ARGS__), #fn)

// A 2-D fp32 tensor as the C-ABI takes it: pointer, leading dimension, rows,
// cols.  No copy: the tensor must already have unit column stride (row_major);
// a padded row pitch is carried as ld.
struct fmat {
  float* p;
  uint64_t ld;
  int64_t rows, cols;
  fmat(const NtsVar& t) {  // NOLINT: tensors convert where a view is taken
    // (a dimension of size 1 may carry any stride in a contiguous tensor)
    TORCH_CHECK(t.dim() == 2 && (t.stride(1) == 1 || t.size(1) == 1),
                "fmat: not a row-major matrix");
    p = t.data_ptr<float>();
    rows = t.size(0);
    cols = t.size(1);
    ld = (uint64_t)(rows > 1 ? t.stride(0) : std::max(t.stride(0), cols));
  }
  fmat top(int64_t n) const {  // the first n rows
    TORCH_CHECK(n >= 0 && n <= rows, "fmat: ", n, " rows of ", rows);
    fmat v = *this;
    v.rows = n;
    return v;
  }
};

// C = A B (trans == 0) or A^T B on nts_hip_gemm_f32, M, N, K and the leading
// dimensions taken from the views; `tag` completes the error label.
inline void gemm(NtsStream& cs, int trans, fmat A, fmat B, fmat C, const char* tag) {
  static const char fn[] = "nts_hip_gemm_f32";
  const int64_t M = C.rows, N = C.cols, K = trans ? A.rows : A.cols;
  TORCH_CHECK((trans ? A.cols : A.rows) == M && B.rows == K && B.cols == N, fn, "(", tag,
              "): shapes [", A.rows, ", ", A.cols, "]", trans ? "^T" : "", " [", B.rows, ", ",
              B.cols, "] -> [", M, ", ", N, "]");
  const int rc = nts_hip_gemm_f32(cs.ctx(), trans, (int)M, (int)N, (int)K, A.p, A.ld, B.p, B.ld,
                                  C.p, C.ld);
  if (rc != NTS_OK) hip_check(rc, (std::string(fn) + "(" + tag + ")").c_str());
}

// out = g ⊙ [y > 0] * scale over g's rows and columns (nts_hip_act_backward)
inline void act_backward(NtsStream& cs, fmat g, fmat y, float scale, fmat out) {
  NTS_CALL(nts_hip_act_backward, cs.ctx(), (uint32_t)g.rows, (uint32_t)g.cols, g.p, g.ld, y.p,
           y.ld, scale, out.p, out.ld);
}

// inverted dropout's 1 / (1 - p) in float arithmetic (0 when everything drops)
inline double keep_scale(double p) { return p < 1.0 ? (double)(1.0f / (1.0f - (float)p)) : 0.0; }

// Non-tensor objects through Function::apply and saved_data travel as integers.
inline int64_t to_handle(const void* p) { return reinterpret_cast<int64_t>(p); }
template <typename T>
inline T* from_handle(int64_t h) {
  return reinterpret_cast<T*>(h);
}
template <typename T>
inline T* from_handle(const c10::IValue& v) {
  return from_handle<T>(v.toInt());
}

// a backward's result: `grads`, then no gradient for its n trailing inputs
inline torch::autograd::variable_list no_grads(torch::autograd::variable_list grads, size_t n) {
  grads.resize(grads.size() + n);
  return grads;
}

}  // namespace nts
