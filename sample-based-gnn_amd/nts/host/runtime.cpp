// C++ host layer, runtime: the C-ABI error check, streams, the kernel profiler,
// parameters (Adam) and the RCCL communicator.  See nts_host.hpp for the
// reference classes each of these mirrors.
#include <c10/hip/HIPStream.h>

#include <cmath>

#include "ops_util.hpp"

namespace nts {

void hip_check(int rc, const char* what) {
  if (rc != NTS_OK)
    throw std::runtime_error(std::string(what) + ": nts_hip error " + std::to_string(rc) + ": " +
                             nts_hip_last_error());
}

// ---------------------------------------------------------------------------
// The structs of include/nts_hip.h are passed by pointer: a host layer built
// against another header revision must not reach the kernels.
static void check_abi() {
  TORCH_CHECK(nts_hip_abi_version() == NTS_HIP_ABI_VERSION, "libnts_hip.so ABI ",
              nts_hip_abi_version(), " != host layer ABI ", NTS_HIP_ABI_VERSION,
              ": rebuild (python -c 'import __graft_entry__ as g; g.build()')");
}

NtsStream::NtsStream(int device, void* stream, uint64_t seed, bool high_priority)
    : device_(device),
      torch_stream_(stream ? c10::hip::getStreamFromExternal((hipStream_t)stream, (c10::DeviceIndex)device)
                           : c10::hip::getStreamFromPool(high_priority, (c10::DeviceIndex)device)) {
  // a pool stream, never the legacy NULL stream: our kernels must not
  // serialise with every other blocking stream of the device
  check_abi();
  NTS_CALL(nts_hip_ctx_create, &ctx_, device, (void*)torch_stream_.stream(), seed);
}
static hipStream_t create_masked(int device, const std::vector<uint32_t>& mask) {
  hip_rt(hipSetDevice(device), "hipSetDevice");
  hipStream_t s = nullptr;
  hip_rt(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()),
         "hipExtStreamCreateWithCUMask");
  return s;
}
NtsStream::NtsStream(int device, const std::vector<uint32_t>& cu_mask, uint64_t seed)
    : device_(device),
      torch_stream_(c10::hip::getStreamFromExternal(create_masked(device, cu_mask),
                                                    (c10::DeviceIndex)device)) {
  check_abi();
  owned_ = torch_stream_.stream();
  NTS_CALL(nts_hip_ctx_create, &ctx_, device, (void*)owned_, seed);
}
NtsStream::~NtsStream() {
  nts_hip_ctx_destroy(ctx_);
  if (owned_) (void)hipStreamDestroy(owned_);
}

std::vector<uint32_t> cu_mask_spread(int device, int n, bool complement) {
  hipDeviceProp_t prop;
  hip_rt(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
  const int total = prop.multiProcessorCount;
  TORCH_CHECK(n > 0 && n < total, "CU partition size must be in (0, ", total, ")");
  const int step = total / n;
  std::vector<uint32_t> mask((total + 31) / 32, 0u);
  int taken = 0;
  for (int i = 0; i < total; ++i) {
    const bool in = (i % step == 0) && taken < n;
    if (in) ++taken;
    if (in != complement) mask[i / 32] |= 1u << (i % 32);
  }
  return mask;
}
void NtsStream::setNewStream(void* stream) {
  hip_check(nts_hip_ctx_set_stream(ctx_, stream), "setNewStream");
  torch_stream_ = c10::hip::getStreamFromExternal((hipStream_t)stream, (c10::DeviceIndex)device_);
}
void* NtsStream::stream() const { return nts_hip_ctx_get_stream(ctx_); }
void NtsStream::synchronize() const {
  hip_rt(hipStreamSynchronize((hipStream_t)stream()), "hipStreamSynchronize");
}

// ---------------------------------------------------------------------------
KernelProfiler::~KernelProfiler() {
  for (auto& e : pool_) {
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
}
const char* KernelProfiler::name(int id) {
  static const char* n[kCount] = {"bottom_aggregation", "gather_gemm", "gather_gemm_tn",
                                  "bottom_backward", "gat_forward"};
  return n[id];
}
void KernelProfiler::begin(Id id, hipStream_t st) {
  if (open_[id] >= 0) return;  // nested begin: keep the outer interval
  if (!active(id)) return;     // another class is timed this step
  if (used_ >= 4096) resolve();
  if (used_ == pool_.size()) {
    Slot sl;
    // timing-only events: no system-scope fence (an L2 writeback + invalidate
    // per record, ~5 us of gap each in the training stream's trace)
    hip_rt(hipEventCreateWithFlags(&sl.a, hipEventDisableSystemFence), "hipEventCreate");
    hip_rt(hipEventCreateWithFlags(&sl.b, hipEventDisableSystemFence), "hipEventCreate");
    pool_.push_back(sl);
  }
  Slot& sl = pool_[used_];
  sl.id = id;
  sl.units = 0;
  hip_rt(hipEventRecord(sl.a, st), "hipEventRecord");
  open_[id] = (int)used_++;
}
void KernelProfiler::end(Id id, hipStream_t st, double units) {
  const int k = open_[id];
  if (k < 0) return;
  hip_rt(hipEventRecord(pool_[k].b, st), "hipEventRecord");
  pool_[k].units = units;
  open_[id] = -1;
}
void KernelProfiler::resolve() {
  for (size_t i = 0; i < used_; ++i) {
    Slot& sl = pool_[i];
    if (open_[sl.id] == (int)i) continue;  // never closed (exception): drop it
    hip_rt(hipEventSynchronize(sl.b), "hipEventSynchronize");
    float ms = 0;
    hip_rt(hipEventElapsedTime(&ms, sl.a, sl.b), "hipEventElapsedTime");
    stat[sl.id].ms += ms;
    stat[sl.id].units += sl.units;
    stat[sl.id].calls += 1;
  }
  used_ = 0;
  for (int& o : open_) o = -1;
}
void KernelProfiler::reset() {
  resolve();
  for (auto& x : stat) x = Stat();
}

// ---------------------------------------------------------------------------
Parameter::Parameter(size_t w, size_t h, ValueType alpha_, ValueType beta1_, ValueType beta2_,
                     ValueType epsilon_, ValueType weight_decay_, int device, int64_t init_seed)
    : row((int)w), col((int)h), alpha(alpha_), beta1(beta1_), beta2(beta2_), epsilon(epsilon_),
      weight_decay(weight_decay_), beta1_t(beta1_), beta2_t(beta2_) {
  // xavier_uniform_ (core/NtsScheduler.hpp:731-733), seeded for reproducibility
  auto gen = at::detail::createCPUGenerator(init_seed);
  const double a = std::sqrt(6.0 / (double)(w + h));
  auto Wc = torch::empty({(int64_t)w, (int64_t)h}, torch::kFloat32).uniform_(-a, a, gen);
  W = Wc.to(torch::Device(torch::kCUDA, device)).set_requires_grad(true);
  M = torch::zeros_like(W).set_requires_grad(false);
  V = torch::zeros_like(W).set_requires_grad(false);
}

static void adam_step(Parameter& p, NtsStream& cs, int bias_correction) {
  TORCH_CHECK(p.W.grad().defined(), "Parameter has no gradient");
  NtsVar g = p.W.grad().contiguous();
  torch::NoGradGuard ng;
  NTS_CALL(nts_hip_adam, cs.ctx(), p.W.data_ptr<float>(), g.data_ptr<float>(),
           p.M.data_ptr<float>(), p.V.data_ptr<float>(), (uint64_t)p.W.numel(), p.alpha, p.beta1,
           p.beta2, p.epsilon, p.weight_decay, p.beta1_t, p.beta2_t, bias_correction);
}

void Parameter::adam_from(NtsStream& cs, const float* grad, bool bias_correction) {
  torch::NoGradGuard ng;
  NTS_CALL(nts_hip_adam, cs.ctx(), W.data_ptr<float>(), grad, M.data_ptr<float>(),
           V.data_ptr<float>(), (uint64_t)W.numel(), alpha, beta1, beta2, epsilon, weight_decay,
           beta1_t, beta2_t, bias_correction ? 1 : 0);
}

void Parameter::learnC2C_with_decay_Adam(NtsStream& cs) { adam_step(*this, cs, 1); }
void Parameter::learn_local_with_decay_Adam(NtsStream& cs) { adam_step(*this, cs, 0); }

void Parameter::next() {
  beta1_t *= beta1;
  beta2_t *= beta2;
  ++curr_epoch;
}

// The gradient is dropped rather than zero-filled: the next backward then
// assigns W.grad instead of accumulating into zeros (no fill + add kernels).
void Parameter::zero_grad() {
  if (W.grad().defined()) W.mutable_grad() = NtsVar();
}

// ---------------------------------------------------------------------------
Communicator::Communicator(int n, int r, const std::vector<uint8_t>& uid, int device)
    : nranks(n), rank(r) {
  TORCH_CHECK(uid.size() == 128, "RCCL unique id must be 128 bytes");
  NTS_CALL(nts_hip_comm_init, &comm_, n, r, uid.data(), device);
}
Communicator::Communicator(int n, int r, HostCollective host)
    : nranks(n), rank(r), host_(std::move(host)) {
  TORCH_CHECK(host_ && n >= 1 && r >= 0 && r < n, "host collective: ranks");
}
Communicator::~Communicator() {
  for (auto& e : tev_) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  if (comm_) nts_hip_comm_destroy(comm_);
}
void Communicator::timing_reset() {
  if (tused_) TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "hipDeviceSynchronize");
  tused_ = 0;
  host_us_ = 0;
  host_calls_ = 0;
}
std::tuple<double, uint64_t, std::string> Communicator::timing_stats() {
  if (host_) return {host_calls_ ? host_us_ / (double)host_calls_ : 0.0, host_calls_, "host-wall"};
  double us = 0;
  for (size_t i = 0; i < tused_; ++i) {
    TORCH_CHECK(hipEventSynchronize(tev_[i].second) == hipSuccess, "hipEventSynchronize");
    float ms = 0;
    TORCH_CHECK(hipEventElapsedTime(&ms, tev_[i].first, tev_[i].second) == hipSuccess,
                "hipEventElapsedTime");
    us += 1e3 * ms;
  }
  return {tused_ ? us / (double)tused_ : 0.0, (uint64_t)tused_, "hip-events"};
}
void Communicator::host_call(float* buf, uint64_t n, void* stream, int op, int root) {
  TORCH_CHECK(hipStreamSynchronize((hipStream_t)stream) == hipSuccess, "hipStreamSynchronize");
  int dev = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess, "hipGetDevice");
  host_(torch::from_blob(buf, {(int64_t)n}, f32_opts(dev)), op, root);
  TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "hipDeviceSynchronize");
}
void Communicator::allreduce_sum(float* buf, uint64_t n, void* stream) {
  if (host_) {
    const double t0 = now_s();
    host_call(buf, n, stream, 0, 0);
    if (timing_) {
      host_us_ += 1e6 * (now_s() - t0);
      ++host_calls_;
    }
    return;
  }
  if (timing_) {
    if (tused_ == tev_.size()) {
      hipEvent_t a, b;
      TORCH_CHECK(hipEventCreateWithFlags(&a, hipEventDisableSystemFence) == hipSuccess &&
                      hipEventCreateWithFlags(&b, hipEventDisableSystemFence) == hipSuccess,
                  "hipEventCreateWithFlags");
      tev_.push_back({a, b});
    }
    TORCH_CHECK(hipEventRecord(tev_[tused_].first, (hipStream_t)stream) == hipSuccess, "hipEventRecord");
  }
  NTS_CALL(nts_hip_allreduce_sum_f32, comm_, buf, n, stream);
  if (timing_) {
    TORCH_CHECK(hipEventRecord(tev_[tused_].second, (hipStream_t)stream) == hipSuccess, "hipEventRecord");
    ++tused_;
  }
}
void Communicator::broadcast(float* buf, uint64_t n, int root, void* stream) {
  if (host_) return host_call(buf, n, stream, 1, root);
  NTS_CALL(nts_hip_broadcast_f32, comm_, buf, n, root, stream);
}
std::pair<int, int> Communicator::rccl_count() const {
  if (host_) return {-1, -1};
  int n = 0, r = 0;
  NTS_CALL(nts_hip_comm_count, comm_, &n, &r);
  return {n, r};
}
std::vector<uint8_t> Communicator::unique_id() {
  std::vector<uint8_t> id(128);
  NTS_CALL(nts_hip_comm_unique_id, id.data());
  return id;
}

}  // namespace nts
