// Python bindings for the BigCLAM CDNA4 kernels (bigclam._C).
#include <torch/extension.h>

#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <optional>

#include "sparse_sweep.h"

extern "C" void launch_k1(const float*, const long long*, const int*,
                          const float*, const int*, float*, double*, int, int,
                          float, float, hipStream_t);
extern "C" void launch_k4(const float*, const long long*, const int*,
                          const float*, const int*, double*, int, int, float,
                          float, hipStream_t);
extern "C" void launch_k2(const float*, const long long*, const int*,
                          const float*, const float*, const double*,
                          const int*, const float*, float*, int, int, int,
                          float, float, float, float, float, hipStream_t);
extern "C" void launch_k3(float*, const float*, const float*, int, int,
                          float, float, hipStream_t);
extern "C" void launch_k1_bf16(const void*, const long long*, const int*,
                               const float*, const int*, float*, double*,
                               int, int, float, float, hipStream_t);
extern "C" void launch_k4_bf16(const void*, const long long*, const int*,
                               const float*, const int*, double*, int, int,
                               float, float, hipStream_t);
extern "C" void launch_k2_bf16(const void*, const long long*, const int*,
                               const float*, const float*, const double*,
                               const int*, const float*, float*, int, int,
                               int, float, float, float, float, float,
                               hipStream_t);
extern "C" void launch_k3_bf16(void*, const float*, const float*, int, int,
                               float, float, hipStream_t);
extern "C" void launch_k3_rows(void*, int, const float*, const float*, int,
                               int, float, float, const int*, int,
                               unsigned char*, hipStream_t);
extern "C" void launch_k5(const long long*, const int*, double*, int, double,
                          hipStream_t);
extern "C" void launch_kf(const float*, const long long*, const int*,
                          const float*, const int*, float*, double*,
                          const float*, float*, int, int, int, float, float,
                          float, float, float, hipStream_t);
extern "C" void launch_kf_bf16(const void*, const long long*, const int*,
                               const float*, const int*, float*, double*,
                               const float*, float*, int, int, int, float,
                               float, float, float, float, hipStream_t);
extern "C" void launch_k3_colsum_bf16(void*, const float*, const float*,
                                      float*, int, int, float, float,
                                      hipStream_t);
extern "C" void launch_kf_mfma(const float*, const long long*, const int*,
                               const float*, const int*, float*, double*,
                               const float*, float*, int, int, int, float,
                               float, float, float, float, hipStream_t);
extern "C" void launch_kf_mfma_bf16(const void*, const long long*, const int*,
                                    const float*, const int*, float*, double*,
                                    const float*, float*, int, int, int,
                                    float, float, float, float, float,
                                    hipStream_t);
extern "C" void launch_k1_chunked(const void*, int, const long long*,
                                  const int*, const float*, const int*,
                                  float*, float*, double*, int, int, float,
                                  float, hipStream_t);
extern "C" void launch_k6(void*, int, int, const long long*,
                          const long long*, const long long*, int, long long,
                          long long, int, hipStream_t);
extern "C" void launch_k7_count(const void*, int, int, int, int, float, int*,
                                hipStream_t);
extern "C" void launch_k7_fill(const void*, int, int, int, int, float,
                               const long long*, int*, hipStream_t);
extern "C" void launch_k8_cover_match(const long long*, const int*,
                                      const long long*, const int*,
                                      const int*, int, long long, int,
                                      long long, int, int, int*, int*,
                                      hipStream_t);
extern "C" int k8_max_tile();
extern "C" void launch_k10_community_scores(const long long*, const int*,
                                            const long long*, const int*,
                                            int, long long, int, long long,
                                            int, int, int*, long long*,
                                            long long*, int*, int*,
                                            hipStream_t);
extern "C" int k10_max_tile();
extern "C" void launch_k11_topn_links(
    const long long*, const int*, const float*, const long long*, const int*,
    const float*, const long long*, const int*, const int*, const int*,
    const int*, const long long*, int*, float*, int, int, int, long long,
    long long, int, int, int, int*, float*, int*, hipStream_t);
extern "C" int k11_max_n();
extern "C" int k11_min_slots();
extern "C" int k11_max_lds_slots();
extern "C" void launch_k9_pair_dot(const void*, const void*, int, const int*,
                                   const int*, float*, long long, int, int,
                                   int, hipStream_t);
extern "C" void launch_mfma_probe_bf16(const void*, const void*, float*,
                                       hipStream_t);
extern "C" void launch_mfma_probe_f32(const float*, const float*, float*,
                                      hipStream_t);

namespace {

#define CHECK_IN(t, type)                                            \
  TORCH_CHECK(t.is_cuda(), #t " must be on GPU");                    \
  TORCH_CHECK(t.is_contiguous(), #t " must be contiguous");          \
  TORCH_CHECK(t.scalar_type() == type, #t " has wrong dtype");

#define CHECK_F(t)                                                          \
  TORCH_CHECK(t.is_cuda(), #t " must be on GPU");                           \
  TORCH_CHECK(t.is_contiguous(), #t " must be contiguous");                 \
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 ||                         \
                  t.scalar_type() == torch::kBFloat16,                      \
              #t " must be fp32 or bf16");

bool is_bf16(const torch::Tensor& t) {
  return t.scalar_type() == torch::kBFloat16;
}

hipStream_t current_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

void edge_grad_llh(torch::Tensor F, torch::Tensor indptr,
                   torch::Tensor indices, torch::Tensor sumF,
                   torch::Tensor order, torch::Tensor grad, torch::Tensor llh,
                   double min_p, double max_p) {
  CHECK_F(F);
  CHECK_IN(indptr, torch::kInt64);
  CHECK_IN(indices, torch::kInt32);
  CHECK_IN(sumF, torch::kFloat32);
  CHECK_IN(order, torch::kInt32);
  CHECK_IN(grad, torch::kFloat32);
  CHECK_IN(llh, torch::kFloat64);
  const int n_local = (int)indptr.size(0) - 1;
  // grid = #nodes listed in `order` (may be a subset: halo overlap split)
  const int n_blocks = (int)order.size(0);
  const int K = (int)F.size(1);
  TORCH_CHECK(grad.size(0) == n_local && grad.size(1) == K);
  const auto ip = reinterpret_cast<const long long*>(indptr.data_ptr<int64_t>());
  if (is_bf16(F)) {
    TORCH_CHECK(K % 8 == 0, "bf16 K must be padded to a multiple of 8");
    launch_k1_bf16(F.data_ptr(), ip, indices.data_ptr<int>(),
                   sumF.data_ptr<float>(), order.data_ptr<int>(),
                   grad.data_ptr<float>(), llh.data_ptr<double>(), n_blocks,
                   K, (float)min_p, (float)max_p, current_stream());
  } else {
    TORCH_CHECK(K % 4 == 0, "K must be padded to a multiple of 4");
    launch_k1(F.data_ptr<float>(), ip, indices.data_ptr<int>(),
              sumF.data_ptr<float>(), order.data_ptr<int>(),
              grad.data_ptr<float>(), llh.data_ptr<double>(), n_blocks, K,
              (float)min_p, (float)max_p, current_stream());
  }
}

void llh_only(torch::Tensor F, torch::Tensor indptr, torch::Tensor indices,
              torch::Tensor sumF, torch::Tensor order, torch::Tensor llh,
              double min_p, double max_p) {
  CHECK_F(F);
  CHECK_IN(indptr, torch::kInt64);
  CHECK_IN(indices, torch::kInt32);
  CHECK_IN(sumF, torch::kFloat32);
  CHECK_IN(order, torch::kInt32);
  CHECK_IN(llh, torch::kFloat64);
  const int n_local = (int)indptr.size(0) - 1;
  const int K = (int)F.size(1);
  const auto ip = reinterpret_cast<const long long*>(indptr.data_ptr<int64_t>());
  if (is_bf16(F)) {
    TORCH_CHECK(K % 8 == 0, "bf16 K must be padded to a multiple of 8");
    launch_k4_bf16(F.data_ptr(), ip, indices.data_ptr<int>(),
                   sumF.data_ptr<float>(), order.data_ptr<int>(),
                   llh.data_ptr<double>(), n_local, K, (float)min_p,
                   (float)max_p, current_stream());
  } else {
    TORCH_CHECK(K % 4 == 0, "K must be padded to a multiple of 4");
    launch_k4(F.data_ptr<float>(), ip, indices.data_ptr<int>(),
              sumF.data_ptr<float>(), order.data_ptr<int>(),
              llh.data_ptr<double>(), n_local, K, (float)min_p, (float)max_p,
              current_stream());
  }
}

void linesearch(torch::Tensor F, torch::Tensor indptr, torch::Tensor indices,
                torch::Tensor sumF, torch::Tensor grad, torch::Tensor llh,
                torch::Tensor order, torch::Tensor ladder, torch::Tensor best,
                double alpha, double min_p, double max_p, double min_f,
                double max_f) {
  CHECK_F(F);
  CHECK_IN(indptr, torch::kInt64);
  CHECK_IN(indices, torch::kInt32);
  CHECK_IN(sumF, torch::kFloat32);
  CHECK_IN(grad, torch::kFloat32);
  CHECK_IN(llh, torch::kFloat64);
  CHECK_IN(order, torch::kInt32);
  CHECK_IN(ladder, torch::kFloat32);
  CHECK_IN(best, torch::kFloat32);
  // grid = #nodes listed in `order` (may be a subset: the sparse path's
  // dense hub remainder); unlisted best[] entries stay untouched
  const int n_blocks = (int)order.size(0);
  const int K = (int)F.size(1);
  const auto ip = reinterpret_cast<const long long*>(indptr.data_ptr<int64_t>());
  if (is_bf16(F)) {
    TORCH_CHECK(K % 8 == 0, "bf16 K must be padded to a multiple of 8");
    launch_k2_bf16(F.data_ptr(), ip, indices.data_ptr<int>(),
                   sumF.data_ptr<float>(), grad.data_ptr<float>(),
                   llh.data_ptr<double>(), order.data_ptr<int>(),
                   ladder.data_ptr<float>(), best.data_ptr<float>(),
                   n_blocks, K, (int)ladder.size(0), (float)alpha,
                   (float)min_p, (float)max_p, (float)min_f, (float)max_f,
                   current_stream());
  } else {
    TORCH_CHECK(K % 4 == 0, "K must be padded to a multiple of 4");
    launch_k2(F.data_ptr<float>(), ip, indices.data_ptr<int>(),
              sumF.data_ptr<float>(), grad.data_ptr<float>(),
              llh.data_ptr<double>(), order.data_ptr<int>(),
              ladder.data_ptr<float>(), best.data_ptr<float>(), n_blocks, K,
              (int)ladder.size(0), (float)alpha, (float)min_p, (float)max_p,
              (float)min_f, (float)max_f, current_stream());
  }
}

// rows given: list mode — only the listed rows are committed (grid = list
// length, an empty list launches nothing), and dirty (uint8 [>= n_local],
// optional) receives (steps[u] > 0) at every listed row.  The caller
// guarantees 0 <= rows[i] < n_local.
void apply_step(torch::Tensor F_local, torch::Tensor grad,
                torch::Tensor steps, double min_f, double max_f,
                std::optional<torch::Tensor> rows,
                std::optional<torch::Tensor> dirty) {
  CHECK_F(F_local);
  CHECK_IN(grad, torch::kFloat32);
  CHECK_IN(steps, torch::kFloat32);
  const int n_local = (int)F_local.size(0);
  const int K = (int)F_local.size(1);
  TORCH_CHECK(grad.size(0) == n_local && grad.size(1) == K);
  TORCH_CHECK(steps.size(0) == n_local);
  TORCH_CHECK(K % (is_bf16(F_local) ? 8 : 4) == 0,
              "K must be padded to a multiple of 8 (bf16) or 4 (fp32)");
  if (rows.has_value()) {
    const torch::Tensor& rl = *rows;
    CHECK_IN(rl, torch::kInt32);
    TORCH_CHECK(rl.dim() == 1 && rl.size(0) <= n_local);
    unsigned char* dp = nullptr;
    if (dirty.has_value()) {
      TORCH_CHECK(dirty->is_cuda() && dirty->is_contiguous() &&
                  dirty->scalar_type() == torch::kUInt8 &&
                  dirty->size(0) >= n_local);
      dp = dirty->data_ptr<uint8_t>();
    }
    launch_k3_rows(F_local.data_ptr(), is_bf16(F_local) ? 1 : 0,
                   grad.data_ptr<float>(), steps.data_ptr<float>(), n_local,
                   K, (float)min_f, (float)max_f, rl.data_ptr<int>(),
                   (int)rl.size(0), dp, current_stream());
    return;
  }
  TORCH_CHECK(!dirty.has_value(), "dirty is written in list mode only");
  if (is_bf16(F_local)) {
    launch_k3_bf16(F_local.data_ptr(), grad.data_ptr<float>(),
                   steps.data_ptr<float>(), n_local, K, (float)min_f,
                   (float)max_f, current_stream());
  } else {
    launch_k3(F_local.data_ptr<float>(), grad.data_ptr<float>(),
              steps.data_ptr<float>(), n_local, K, (float)min_f,
              (float)max_f, current_stream());
  }
}

// n_mfma: the first n_mfma entries of `order` (degree-descending, so the
// high-degree prefix) run the MFMA phase-B kernel; the rest the direct
// one.  The two launches cover disjoint nodes.
void fused_grad_ls(torch::Tensor F, torch::Tensor indptr,
                   torch::Tensor indices, torch::Tensor sumF,
                   torch::Tensor order, torch::Tensor grad, torch::Tensor llh,
                   torch::Tensor ladder, torch::Tensor best, double alpha,
                   double min_p, double max_p, double min_f, double max_f,
                   int64_t n_mfma) {
  CHECK_F(F);
  CHECK_IN(indptr, torch::kInt64);
  CHECK_IN(indices, torch::kInt32);
  CHECK_IN(sumF, torch::kFloat32);
  CHECK_IN(order, torch::kInt32);
  CHECK_IN(grad, torch::kFloat32);
  CHECK_IN(llh, torch::kFloat64);
  CHECK_IN(ladder, torch::kFloat32);
  CHECK_IN(best, torch::kFloat32);
  const int n_local = (int)indptr.size(0) - 1;
  const int n_blocks = (int)order.size(0);
  const int K = (int)F.size(1);
  TORCH_CHECK(grad.size(0) == n_local && grad.size(1) == K);
  const auto ip =
      reinterpret_cast<const long long*>(indptr.data_ptr<int64_t>());
  TORCH_CHECK(n_mfma >= 0 && n_mfma <= n_blocks, "bad n_mfma");
  const int n_hi = (int)n_mfma;
  const int n_lo = n_blocks - n_hi;
  const int* ord = order.data_ptr<int>();
  if (is_bf16(F)) {
    TORCH_CHECK(K % 8 == 0 && K <= 26000,
                "bf16 fused kernel: K padded to 8, K <= 26000 (the direct "
                "kernel additionally requires K <= 16384 for its share)");
    launch_kf_mfma_bf16(F.data_ptr(), ip, indices.data_ptr<int>(),
                        sumF.data_ptr<float>(), ord, grad.data_ptr<float>(),
                        llh.data_ptr<double>(), ladder.data_ptr<float>(),
                        best.data_ptr<float>(), n_hi, K, (int)ladder.size(0),
                        (float)alpha, (float)min_p, (float)max_p,
                        (float)min_f, (float)max_f, current_stream());
    launch_kf_bf16(F.data_ptr(), ip, indices.data_ptr<int>(),
                   sumF.data_ptr<float>(), ord + n_hi,
                   grad.data_ptr<float>(), llh.data_ptr<double>(),
                   ladder.data_ptr<float>(), best.data_ptr<float>(), n_lo,
                   K, (int)ladder.size(0), (float)alpha, (float)min_p,
                   (float)max_p, (float)min_f, (float)max_f,
                   current_stream());
  } else {
    TORCH_CHECK(K % 4 == 0 && K <= 8192, "fused kernel: K padded, K <= 8192");
    launch_kf_mfma(F.data_ptr<float>(), ip, indices.data_ptr<int>(),
                   sumF.data_ptr<float>(), ord, grad.data_ptr<float>(),
                   llh.data_ptr<double>(), ladder.data_ptr<float>(),
                   best.data_ptr<float>(), n_hi, K, (int)ladder.size(0),
                   (float)alpha, (float)min_p, (float)max_p, (float)min_f,
                   (float)max_f, current_stream());
    launch_kf(F.data_ptr<float>(), ip, indices.data_ptr<int>(),
              sumF.data_ptr<float>(), ord + n_hi, grad.data_ptr<float>(),
              llh.data_ptr<double>(), ladder.data_ptr<float>(),
              best.data_ptr<float>(), n_lo, K, (int)ladder.size(0),
              (float)alpha, (float)min_p, (float)max_p, (float)min_f,
              (float)max_f, current_stream());
  }
}

// K3 + column partial sums fused (bf16 storage): commits F in place and
// writes per-stripe fp32 column partials; sumF = partials.sum(0) on the
// caller side (deterministic stage-2).
void apply_step_colsum(torch::Tensor F_local, torch::Tensor grad,
                       torch::Tensor steps, torch::Tensor partials,
                       double min_f, double max_f) {
  TORCH_CHECK(F_local.scalar_type() == torch::kBFloat16 &&
                  F_local.is_contiguous(),
              "apply_step_colsum is the bf16 path");
  CHECK_IN(grad, torch::kFloat32);
  CHECK_IN(steps, torch::kFloat32);
  CHECK_IN(partials, torch::kFloat32);
  const int n_local = (int)F_local.size(0);
  const int K = (int)F_local.size(1);
  TORCH_CHECK(K % 8 == 0, "bf16 K must be padded to a multiple of 8");
  TORCH_CHECK(grad.size(0) == n_local && grad.size(1) == K);
  TORCH_CHECK(steps.size(0) == n_local);
  TORCH_CHECK(partials.size(0) == (n_local + 511) / 512 &&
              partials.size(1) == K);
  launch_k3_colsum_bf16(F_local.data_ptr(), grad.data_ptr<float>(),
                        steps.data_ptr<float>(), partials.data_ptr<float>(),
                        n_local, K, (float)min_f, (float)max_f,
                        current_stream());
}

// On-device MFMA C/D-layout probe: D = A @ B with Bc = B column-major.
void mfma_probe(torch::Tensor A, torch::Tensor Bc, torch::Tensor D) {
  TORCH_CHECK(D.scalar_type() == torch::kFloat32 && D.is_contiguous());
  TORCH_CHECK(A.is_contiguous() && Bc.is_contiguous());
  TORCH_CHECK(A.scalar_type() == Bc.scalar_type());
  if (is_bf16(A)) {
    TORCH_CHECK(A.size(0) == 16 && A.size(1) == 32);
    launch_mfma_probe_bf16(A.data_ptr(), Bc.data_ptr(),
                           D.data_ptr<float>(), current_stream());
  } else {
    TORCH_CHECK(A.size(0) == 16 && A.size(1) == 4);
    launch_mfma_probe_f32(A.data_ptr<float>(), Bc.data_ptr<float>(),
                          D.data_ptr<float>(), current_stream());
  }
}

// Chunked large-K K1 (KD dot pass into the per-edge x buffer, then KW
// chunked weighted accumulate) — no K cap; see kd_dot_t/kw_grad_t.
void edge_grad_llh_chunked(torch::Tensor F, torch::Tensor indptr,
                           torch::Tensor indices, torch::Tensor sumF,
                           torch::Tensor order, torch::Tensor grad,
                           torch::Tensor llh, torch::Tensor xbuf,
                           double min_p, double max_p) {
  CHECK_F(F);
  CHECK_IN(indptr, torch::kInt64);
  CHECK_IN(indices, torch::kInt32);
  CHECK_IN(sumF, torch::kFloat32);
  CHECK_IN(order, torch::kInt32);
  CHECK_IN(grad, torch::kFloat32);
  CHECK_IN(llh, torch::kFloat64);
  CHECK_IN(xbuf, torch::kFloat32);
  const int n_local = (int)indptr.size(0) - 1;
  const int n_blocks = (int)order.size(0);
  const int K = (int)F.size(1);
  TORCH_CHECK(grad.size(0) == n_local && grad.size(1) == K);
  TORCH_CHECK(xbuf.size(0) >= indices.size(0), "xbuf too small");
  TORCH_CHECK(K % (is_bf16(F) ? 8 : 4) == 0, "K must be padded");
  const auto ip =
      reinterpret_cast<const long long*>(indptr.data_ptr<int64_t>());
  launch_k1_chunked(F.data_ptr(), is_bf16(F) ? 1 : 0, ip,
                    indices.data_ptr<int>(), sumF.data_ptr<float>(),
                    order.data_ptr<int>(), xbuf.data_ptr<float>(),
                    grad.data_ptr<float>(), llh.data_ptr<double>(), n_blocks,
                    K, (float)min_p, (float)max_p, current_stream());
}

// Sparse-adaptive sweep (KAF/K1S/K2S/K3S — docs/sparse_sweep_design.md).
// A side stream per device with its fork / join events.  The single
// (one wave per node) part of a packed wave class holds the widest nodes
// of the class: a few thousand long waves that fill a fraction of the
// device.  Alone after the packed launch they cost their full latency;
// on the side stream they run next to it.
struct WaveSide {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
static WaveSide& wave_side() {
  static WaveSide per_dev[64];
  int dev = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64);
  WaveSide& w = per_dev[dev];
  if (!w.stream) {
    TORCH_CHECK(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking) ==
                hipSuccess);
    TORCH_CHECK(hipEventCreateWithFlags(&w.fork, hipEventDisableTiming) ==
                hipSuccess);
    TORCH_CHECK(hipEventCreateWithFlags(&w.join, hipEventDisableTiming) ==
                hipSuccess);
  }
  return w;
}

static const long long* i64p(const torch::Tensor& t) {
  return reinterpret_cast<const long long*>(t.data_ptr<int64_t>());
}

void sparse_support(torch::Tensor F, torch::Tensor soffset,
                    torch::Tensor scount, torch::Tensor sidx,
                    torch::Tensor sval, int64_t cap, bool fill,
                    torch::Tensor dirty,
                    std::optional<torch::Tensor> rows) {
  // rows given: list mode — one block per listed row (still subject to
  // the dirty mask); an empty list launches nothing.  The caller
  // guarantees 0 <= rows[i] < n_rows (the kernel drops anything above).
  CHECK_F(F);
  CHECK_IN(soffset, torch::kInt64);
  CHECK_IN(scount, torch::kInt32);
  CHECK_IN(sidx, torch::kInt32);
  CHECK_IN(sval, torch::kFloat32);
  const int n_rows = (int)F.size(0);
  const int K = (int)F.size(1);
  TORCH_CHECK(scount.size(0) == n_rows && soffset.size(0) == n_rows);
  const unsigned char* dp = nullptr;
  if (dirty.numel()) {
    TORCH_CHECK(dirty.scalar_type() == torch::kUInt8 &&
                dirty.is_contiguous() && dirty.size(0) == n_rows);
    dp = dirty.data_ptr<uint8_t>();
  }
  const int* rp = nullptr;
  int n_list = 0;
  if (rows.has_value()) {
    const torch::Tensor& rl = *rows;
    CHECK_IN(rl, torch::kInt32);
    TORCH_CHECK(rl.dim() == 1);
    n_list = (int)rl.size(0);
    if (n_list == 0) return;
    rp = rl.data_ptr<int>();
  }
  launch_kaf(F.data_ptr(), is_bf16(F) ? 1 : 0, n_rows, K, (int)cap,
             i64p(soffset), scount.data_ptr<int>(), sidx.data_ptr<int>(),
             sval.data_ptr<float>(), fill ? 1 : 0, dp, rp, n_list,
             current_stream());
}

void sparse_fused(torch::Tensor F, torch::Tensor indptr,
                  torch::Tensor indices, torch::Tensor sumF,
                  torch::Tensor order, torch::Tensor soffset,
                  torch::Tensor sidx, torch::Tensor sval,
                  torch::Tensor scount, torch::Tensor epre,
                  torch::Tensor bound, torch::Tensor goffset, torch::Tensor gidx,
                  torch::Tensor gval, torch::Tensor gcount,
                  torch::Tensor llh, torch::Tensor GG, torch::Tensor ladder,
                  torch::Tensor best, int64_t cap, double alpha,
                  double min_p, double max_p, double min_f, double max_f,
                  int64_t n_block, int64_t wcap, int64_t qcap,
                  std::optional<torch::Tensor> wsplit, int64_t n_pack,
                  bool skip, int64_t n_zero, int64_t n_rep,
                  std::optional<torch::Tensor> zscr) {
  // order[:n_block] runs the block kernel (KFS), order[n_block:] the
  // one-wave-per-node kernel (KFW, bound <= wcap); pools and gcount are
  // indexed by position in `order` for both.  With qcap > 0 and the
  // routing's wsplit, the wave class runs as two launches: the pack
  // positions wsplit[:n_pack] four nodes per wave (KFP), the rest
  // wsplit[n_pack:n_wave] one wave per node (KFW).  skip selects the
  // KFW/KFP instantiations that pass over empty edges and empty active
  // sets (bitwise the same outputs; false = the A/B reference).
  // With zscr (the routing's zero class) the packed part of wsplit holds
  // n_pack + n_zero positions and zscr lists them again as zsplit = [bound
  // > 0 | zero]: KFP runs zsplit[:n_pack] and, in a second launch, the n_rep
  // representatives; kz_fill then copies each degree's llh / best to the
  // other zero nodes zsplit[n_pack : n_pack + n_zero].  The single part is
  // wsplit[n_pack + n_zero : n_wave] as without it.
  CHECK_F(F);
  CHECK_IN(indptr, torch::kInt64);
  CHECK_IN(indices, torch::kInt32);
  CHECK_IN(sumF, torch::kFloat32);
  CHECK_IN(order, torch::kInt32);
  CHECK_IN(soffset, torch::kInt64);
  CHECK_IN(sidx, torch::kInt32);
  CHECK_IN(sval, torch::kFloat32);
  CHECK_IN(scount, torch::kInt32);
  CHECK_IN(epre, torch::kInt32);
  CHECK_IN(bound, torch::kInt32);
  CHECK_IN(goffset, torch::kInt64);
  CHECK_IN(gidx, torch::kInt32);
  CHECK_IN(gval, torch::kFloat32);
  CHECK_IN(gcount, torch::kInt32);
  CHECK_IN(llh, torch::kFloat64);
  CHECK_IN(GG, torch::kFloat32);
  CHECK_IN(ladder, torch::kFloat32);
  CHECK_IN(best, torch::kFloat32);
  const int bf16 = is_bf16(F) ? 1 : 0;
  const int n_blocks = (int)order.size(0);
  TORCH_CHECK(goffset.size(0) >= n_blocks && gcount.size(0) >= n_blocks);
  TORCH_CHECK(epre.size(0) == indices.size(0), "epre must be [nnz]");
  TORCH_CHECK(bound.size(0) + 1 == indptr.size(0), "bound must be [n_local]");
  TORCH_CHECK(n_block >= 0 && n_block <= n_blocks, "n_block out of range");
  const int n_wave = n_blocks - (int)n_block;
  TORCH_CHECK(n_wave == 0 || (wcap > 0 && wcap <= cap),
              "wave class needs 0 < wcap <= cap");
  const bool packed = qcap > 0 && wsplit.has_value();
  const int* wsp = nullptr;
  const int* zsp = nullptr;
  const int* kfp_pos = nullptr;  // KFP's position list
  int n_pz = 0;  // packed and zero nodes: the front of wsplit
  TORCH_CHECK(packed || n_zero == 0, "the zero class needs the packed split");
  hipStream_t main_s = current_stream();
  hipStream_t wave_s = main_s;  // where the single-wave launch goes
  WaveSide* side = nullptr;
  if (packed) {
    CHECK_IN((*wsplit), torch::kInt32);
    TORCH_CHECK(qcap <= wcap, "packed wave class needs qcap <= wcap <= cap");
    TORCH_CHECK(n_pack >= 0 && n_pack <= n_wave, "n_pack out of range");
    TORCH_CHECK(wsplit->dim() == 1 && wsplit->size(0) >= n_wave,
                "wsplit must hold the wave class");
    TORCH_CHECK(kfp_lds_bytes(bf16, (int)F.size(1), (int)qcap) <= 64 * 1024,
                "qcap exceeds the packed kernel's LDS budget");
    wsp = kfp_pos = wsplit->data_ptr<int>();
    TORCH_CHECK(n_zero >= 0 && n_pack + n_zero <= n_wave,
                "n_zero out of range");
    if (n_zero > 0) {
      TORCH_CHECK(zscr.has_value(), "the zero class needs zscr");
      CHECK_IN((*zscr), torch::kInt32);
      const int64_t n_local = bound.size(0);
      const int64_t zs_at =
          ZR_TILES + 6 * ((n_local + route_tile() - 1) / route_tile());
      TORCH_CHECK(zscr->dim() == 1 && zscr->size(0) >= zs_at + n_local,
                  "zscr must be the routing's buffer");
      TORCH_CHECK(n_rep > 0 && n_rep <= KFP_DEG + 1 && n_rep <= n_zero,
                  "n_rep out of range");
      zsp = zscr->data_ptr<int>();
      kfp_pos = zsp + zs_at;  // [bound > 0 | zero]
    }
    n_pz = (int)(n_pack + n_zero);
    if (n_pz > 0 && n_pz < n_wave) {
      // both parts non-empty: the single part forks to the side stream
      // (it only reads what the main stream has finished writing, and
      // writes positions no other launch of this call touches)
      side = &wave_side();
      TORCH_CHECK(hipEventRecord(side->fork, main_s) == hipSuccess);
      TORCH_CHECK(hipStreamWaitEvent(side->stream, side->fork, 0) ==
                  hipSuccess);
      wave_s = side->stream;
    }
  }
  const int w_first = packed ? n_pz : (int)n_block;
  const int w_count = packed ? n_wave - n_pz : n_wave;
  SweepArgs a;
  a.K = (int)F.size(1);
  a.indptr = i64p(indptr);
  a.indices = indices.data_ptr<int>();
  a.sumF = sumF.data_ptr<float>();
  a.order = order.data_ptr<int>();
  a.soffset = i64p(soffset);
  a.sidx = sidx.data_ptr<int>();
  a.sval = sval.data_ptr<float>();
  a.scount = scount.data_ptr<int>();
  a.epre = epre.data_ptr<int>();
  a.bound = bound.data_ptr<int>();
  a.goffset = i64p(goffset);
  a.gidx = gidx.data_ptr<int>();
  a.gval = gval.data_ptr<float>();
  a.gcount = gcount.data_ptr<int>();
  a.llh = llh.data_ptr<double>();
  a.GG = GG.data_ptr<float>();
  a.ladder = ladder.data_ptr<float>();
  a.best = best.data_ptr<float>();
  a.n_ladder = (int)ladder.size(0);
  a.alpha = (float)alpha;
  a.min_p = (float)min_p;
  a.max_p = (float)max_p;
  a.min_f = (float)min_f;
  a.max_f = (float)max_f;
  if (w_count > 0)
    launch_kfw(a, bf16, w_first, wsp, w_count, (int)wcap, skip ? 1 : 0,
               wave_s);
  if (side) TORCH_CHECK(hipEventRecord(side->join, wave_s) == hipSuccess);
  if (packed)
    launch_kfp(a, bf16, kfp_pos, (int)n_pack, (int)qcap, skip ? 1 : 0,
               main_s);
  if (zsp) {
    launch_kfp(a, bf16, zsp + ZR_REP, (int)n_rep, (int)qcap, skip ? 1 : 0,
               main_s);
    launch_kz_fill(a, kfp_pos + n_pack, (int)n_zero, zsp + ZR_NODE, main_s);
  }
  if (side)
    TORCH_CHECK(hipStreamWaitEvent(main_s, side->join, 0) == hipSuccess);
  launch_kfs(a, F.data_ptr(), bf16, (int)n_block, (int)cap, main_s);
}

void sparse_commit(torch::Tensor F, torch::Tensor order,
                   torch::Tensor goffset, torch::Tensor gidx,
                   torch::Tensor gval, torch::Tensor gcount,
                   torch::Tensor best, torch::Tensor soffset,
                   torch::Tensor sidx, torch::Tensor sval,
                   torch::Tensor scount, int64_t cap, double min_f,
                   double max_f, int64_t n_block, int64_t wcap,
                   std::optional<torch::Tensor> dirty) {
  // order[:n_block] commits one block per node (K3S), order[n_block:] one
  // wave per node (K3W; its nodes have gcount <= wcap <= cap, so their
  // rewritten lists fit the cap-strided slots).  n_block < 0: all K3S.
  // dirty (uint8, indexed by row) gets 0 at every routed row.
  CHECK_F(F);
  CHECK_IN(order, torch::kInt32);
  CHECK_IN(goffset, torch::kInt64);
  CHECK_IN(gidx, torch::kInt32);
  CHECK_IN(gval, torch::kFloat32);
  CHECK_IN(gcount, torch::kInt32);
  CHECK_IN(best, torch::kFloat32);
  CHECK_IN(soffset, torch::kInt64);
  CHECK_IN(sidx, torch::kInt32);
  CHECK_IN(sval, torch::kFloat32);
  CHECK_IN(scount, torch::kInt32);
  const int n_total = (int)order.size(0);
  TORCH_CHECK(goffset.size(0) >= n_total && gcount.size(0) >= n_total);
  if (n_block < 0) n_block = n_total;
  TORCH_CHECK(n_block <= n_total, "n_block out of range");
  TORCH_CHECK(n_block == n_total || (wcap > 0 && wcap <= cap),
              "wave class needs 0 < wcap <= cap");
  unsigned char* dp = nullptr;
  if (dirty.has_value()) {
    TORCH_CHECK(dirty->is_cuda() && dirty->is_contiguous() &&
                dirty->scalar_type() == torch::kUInt8 &&
                dirty->size(0) >= F.size(0));
    dp = dirty->data_ptr<uint8_t>();
  }
  launch_k3s(F.data_ptr(), is_bf16(F) ? 1 : 0, order.data_ptr<int>(),
             (int)n_block, n_total, i64p(goffset), gidx.data_ptr<int>(),
             gval.data_ptr<float>(), gcount.data_ptr<int>(),
             best.data_ptr<float>(), i64p(soffset), sidx.data_ptr<int>(),
             sval.data_ptr<float>(), scount.data_ptr<int>(), dp, (int)cap,
             (int)F.size(1), (float)min_f, (float)max_f, current_stream());
}

// K6: seed-init F scatter from the seeds' compact adjacency (see
// k6_seed_init_t); F_local is the rank's [n_local, kp] slice.
void seed_init(torch::Tensor F_local, torch::Tensor sindptr,
               torch::Tensor snbrs, torch::Tensor seeds, int64_t start,
               int64_t stop, bool include_seed) {
  CHECK_F(F_local);
  CHECK_IN(sindptr, torch::kInt64);
  CHECK_IN(snbrs, torch::kInt64);
  CHECK_IN(seeds, torch::kInt64);
  TORCH_CHECK(F_local.dim() == 2, "F_local must be [n_local, kp]");
  TORCH_CHECK(sindptr.dim() == 1 && snbrs.dim() == 1 && seeds.dim() == 1,
              "sindptr, snbrs and seeds must be 1-D");
  const int n_seeds = (int)seeds.size(0);
  // column c = seed c: past the row width the scatter would run into the
  // next row, and past the buffer on the last one
  TORCH_CHECK(seeds.size(0) <= F_local.size(1), "n_seeds (", seeds.size(0),
              ") exceeds the F_local width (", F_local.size(1), ")");
  TORCH_CHECK(sindptr.size(0) == n_seeds + 1);
  TORCH_CHECK(start <= stop, "start (", start, ") must be <= stop (", stop,
              ")");
  TORCH_CHECK(stop - start == F_local.size(0));
  // one host read; init runs once per fit
  const int64_t n_nbrs = sindptr[n_seeds].item<int64_t>();
  TORCH_CHECK(n_nbrs == snbrs.size(0), "sindptr[-1] (", n_nbrs,
              ") must equal the length of snbrs (", snbrs.size(0), ")");
  launch_k6(F_local.data_ptr(), is_bf16(F_local) ? 1 : 0,
            (int)F_local.size(1),
            i64p(sindptr), i64p(snbrs), i64p(seeds), n_seeds, (long long)start, (long long)stop,
            include_seed ? 1 : 0, current_stream());
}

// List-based column sums for the sparse path (see kcs_lists_t).
void sparse_colsum(torch::Tensor F_local, torch::Tensor soffset,
                   torch::Tensor sidx, torch::Tensor sval,
                   torch::Tensor scount, torch::Tensor dirty, int64_t cap,
                   torch::Tensor partials) {
  CHECK_F(F_local);
  CHECK_IN(soffset, torch::kInt64);
  CHECK_IN(sidx, torch::kInt32);
  CHECK_IN(sval, torch::kFloat32);
  CHECK_IN(scount, torch::kInt32);
  CHECK_IN(partials, torch::kFloat32);
  TORCH_CHECK(dirty.scalar_type() == torch::kUInt8 && dirty.is_contiguous());
  const int n_local = (int)F_local.size(0);
  const int K = (int)F_local.size(1);
  TORCH_CHECK(partials.size(0) == (n_local + 511) / 512 &&
              partials.size(1) == K);
  launch_kcs_lists(F_local.data_ptr(), is_bf16(F_local) ? 1 : 0, n_local, K,
                   i64p(soffset), sidx.data_ptr<int>(),
                   sval.data_ptr<float>(), scount.data_ptr<int>(),
                   dirty.data_ptr<uint8_t>(), (int)cap,
                   partials.data_ptr<float>(), current_stream());
}

// Stage 2 of the column-sum refresh: out[k] = sum_s partials[s, k] in a
// fixed order (see kcs_stage2).
void colsum_stage2(torch::Tensor partials, torch::Tensor out) {
  CHECK_IN(partials, torch::kFloat32);
  CHECK_IN(out, torch::kFloat32);
  TORCH_CHECK(partials.dim() == 2 && out.dim() == 1 &&
              out.size(0) == partials.size(1));
  TORCH_CHECK(partials.size(1) % 4 == 0, "K must be a multiple of 4");
  launch_kcs_stage2(partials.data_ptr<float>(), (int)partials.size(0),
                    (int)partials.size(1), out.data_ptr<float>(),
                    current_stream());
}

// Sparse-path routing (kr_bounds / kr_scan / kr_place): fills epre
// [nnz], bound [n_local], by_class [n_local] = [block | wave | dense] and
// GG [1]; returns the three class sizes (the sweep's routing host sync).
// cls/tcount/tbase/totals are scratch the caller keeps allocated.
// With qcap / wsplit [n_local] / pscr [4 * tiles + 1] given, the same three
// launches also split the wave class for the packed kernel (KFP):
// wsplit[:n_pack] = pack positions (n_block + rank in the wave class) of
// the nodes with bound <= qcap and degree <= 16, wsplit[n_pack:n_wave]
// those of the others, both in launch order; n_pack is returned as a
// fourth value from the same host sync.  Nothing else changes.
// With zscr [ZR_TILES + 6 * tiles + n_local] given as well, all counts come
// back in ONE device-to-host copy (they sit side by side at its start), and
// with `zero` the packed part is listed once more at the end of zscr
// (zsplit, from ZR_TILES + 6 * tiles): zsplit[:n_pack] the packable nodes
// with bound > 0, zsplit[n_pack : n_pack + n_zero] those with bound 0 (the
// zero class), both in launch order.  wsplit is what it is without zscr: the
// packed part holds n_pack + n_zero positions.  zscr[ZR_REP ..] then lists the pack position of the first zero
// node of each degree (degree-descending, -1 past the count), zscr[ZR_NODE
// + deg] its node id (-1: none).  Returns six values: the three class
// sizes, n_pack, n_zero and the number of representatives.
std::vector<int64_t> sparse_route(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor scount,
    torch::Tensor order, torch::Tensor sumF, int64_t cap, int64_t wcap,
    torch::Tensor epre, torch::Tensor bound, torch::Tensor cls,
    torch::Tensor tcount, torch::Tensor tbase, torch::Tensor totals,
    torch::Tensor GG, torch::Tensor by_class,
    std::optional<int64_t> qcap, std::optional<torch::Tensor> wsplit,
    std::optional<torch::Tensor> pscr, std::optional<torch::Tensor> zscr,
    bool zero) {
  CHECK_IN(indptr, torch::kInt64);
  CHECK_IN(indices, torch::kInt32);
  CHECK_IN(scount, torch::kInt32);
  CHECK_IN(order, torch::kInt32);
  CHECK_IN(sumF, torch::kFloat32);
  CHECK_IN(epre, torch::kInt32);
  CHECK_IN(bound, torch::kInt32);
  CHECK_IN(cls, torch::kUInt8);
  CHECK_IN(tcount, torch::kInt32);
  CHECK_IN(tbase, torch::kInt32);
  CHECK_IN(totals, torch::kInt32);
  CHECK_IN(GG, torch::kFloat32);
  CHECK_IN(by_class, torch::kInt32);
  const int64_t n_local = order.size(0);
  const int64_t n_tiles = (n_local + route_tile() - 1) / route_tile();
  TORCH_CHECK(indptr.size(0) == n_local + 1 && scount.size(0) >= n_local);
  TORCH_CHECK(epre.size(0) == indices.size(0), "epre must be [nnz]");
  TORCH_CHECK(bound.size(0) == n_local && cls.size(0) == n_local &&
              by_class.size(0) == n_local);
  TORCH_CHECK(tcount.size(0) >= 3 * n_tiles && tbase.size(0) >= 3 * n_tiles &&
              totals.size(0) >= 3 && GG.size(0) >= 1);
  TORCH_CHECK(cap >= 0 && cap < (1 << 29) && wcap >= 0 && wcap <= cap,
              "need 0 <= wcap <= cap < 2^29");
  const bool split = wsplit.has_value();
  TORCH_CHECK(split == qcap.has_value() && split == pscr.has_value(),
              "qcap, wsplit and pscr go together");
  int* wsp = nullptr;
  int* psp = nullptr;
  int q = 0;
  if (split) {
    CHECK_IN((*wsplit), torch::kInt32);
    CHECK_IN((*pscr), torch::kInt32);
    q = (int)*qcap;
    TORCH_CHECK(*qcap >= 0 && *qcap <= wcap, "need 0 <= qcap <= wcap");
    TORCH_CHECK(wsplit->dim() == 1 && wsplit->size(0) == n_local,
                "wsplit must be int32 [n_local]");
    TORCH_CHECK(pscr->dim() == 1 && pscr->size(0) >= 4 * n_tiles + 1,
                "pscr must hold 4 ints per routing tile + 1");
    wsp = wsplit->data_ptr<int>();
    psp = pscr->data_ptr<int>();
  }
  int* zsp = nullptr;
  if (zscr.has_value()) {
    TORCH_CHECK(split, "zscr goes with qcap, wsplit and pscr");
    CHECK_IN((*zscr), torch::kInt32);
    TORCH_CHECK(zscr->dim() == 1 &&
                    zscr->size(0) >= ZR_TILES + 6 * n_tiles + n_local,
                "zscr must hold ZR_TILES + 6 ints per routing tile + n_local");
    zsp = zscr->data_ptr<int>();
    TORCH_CHECK(reinterpret_cast<uintptr_t>(zsp) % 16 == 0,
                "zscr must be 16-byte aligned");
  }
  TORCH_CHECK(!zero || zsp, "the zero class needs zscr");
  hipStream_t stream = current_stream();
  launch_route(i64p(indptr), indices.data_ptr<int>(), scount.data_ptr<int>(),
               order.data_ptr<int>(), (int)n_local, (int)cap, (int)wcap,
               sumF.data_ptr<float>(), (int)sumF.size(0),
               epre.data_ptr<int>(), bound.data_ptr<int>(),
               cls.data_ptr<uint8_t>(), tcount.data_ptr<int>(),
               tbase.data_ptr<int>(), totals.data_ptr<int>(),
               GG.data_ptr<float>(), by_class.data_ptr<int>(), q, psp, wsp,
               zsp, zero ? 1 : 0, stream);
  if (zsp) {  // every count in one copy
    int z[ZR_HOST];
    TORCH_CHECK(hipMemcpyAsync(z, zsp, sizeof(z), hipMemcpyDeviceToHost,
                               stream) == hipSuccess);
    TORCH_CHECK(hipStreamSynchronize(stream) == hipSuccess);
    return {z[0], z[1], z[2], z[ZR_NPACK], z[ZR_NZERO], z[ZR_NREP]};
  }
  int h[4] = {0, 0, 0, 0};
  TORCH_CHECK(hipMemcpyAsync(h, totals.data_ptr<int>(), 3 * sizeof(int),
                             hipMemcpyDeviceToHost, stream) == hipSuccess);
  if (split)
    TORCH_CHECK(hipMemcpyAsync(h + 3, psp + 4 * n_tiles, sizeof(int),
                               hipMemcpyDeviceToHost, stream) == hipSuccess);
  TORCH_CHECK(hipStreamSynchronize(stream) == hipSuccess);
  if (split) return {h[0], h[1], h[2], h[3]};
  return {h[0], h[1], h[2]};
}

// K7 community extraction: two deterministic passes (count, then fill
// after a host/torch prefix-sum) — see k7_membership in the .hip file.
void extract_count(torch::Tensor F_local, int64_t k_true, double delta,
                   torch::Tensor counts) {
  CHECK_F(F_local);
  CHECK_IN(counts, torch::kInt32);
  TORCH_CHECK(F_local.dim() == 2, "F_local must be [n, ldF]");
  TORCH_CHECK(counts.dim() == 1, "counts must be 1-D");
  const int n = (int)F_local.size(0);
  const int ldF = (int)F_local.size(1);
  // the bf16 kernel reads rows as 32-bit words
  TORCH_CHECK(!is_bf16(F_local) || ldF % 2 == 0,
              "ldF must be even for bf16, got ", ldF);
  TORCH_CHECK(counts.size(0) == n);
  TORCH_CHECK(k_true >= 1 && k_true <= ldF, "bad k_true");
  launch_k7_count(F_local.data_ptr(), is_bf16(F_local) ? 1 : 0, n,
                  (int)k_true, ldF, (float)delta, counts.data_ptr<int>(),
                  current_stream());
}

void extract_fill(torch::Tensor F_local, int64_t k_true, double delta,
                  torch::Tensor offsets, torch::Tensor comms) {
  CHECK_F(F_local);
  CHECK_IN(offsets, torch::kInt64);
  CHECK_IN(comms, torch::kInt32);
  TORCH_CHECK(F_local.dim() == 2, "F_local must be [n, ldF]");
  TORCH_CHECK(offsets.dim() == 1, "offsets must be 1-D");
  const int n = (int)F_local.size(0);
  const int ldF = (int)F_local.size(1);
  TORCH_CHECK(!is_bf16(F_local) || ldF % 2 == 0,
              "ldF must be even for bf16, got ", ldF);
  TORCH_CHECK(offsets.size(0) == n);
  TORCH_CHECK(k_true >= 1 && k_true <= ldF, "bad k_true");
  launch_k7_fill(F_local.data_ptr(), is_bf16(F_local) ? 1 : 0, n,
                 (int)k_true, ldF, (float)delta,
                 reinterpret_cast<const long long*>(
                     offsets.data_ptr<int64_t>()),
                 comms.data_ptr<int>(), current_stream());
}

// K8: best-match community of cover Y for every community of cover X
// (exact integer selection; see k8_cover_match in cover_kernels.hip).
// X is group-major (grp_ptr/grp_nodes), Y node-major (node_ptr/node_comm,
// ascending per node) with its community sizes in size_y.
void cover_best_match(torch::Tensor grp_ptr, torch::Tensor grp_nodes,
                      torch::Tensor node_ptr, torch::Tensor node_comm,
                      torch::Tensor size_y, int64_t tile,
                      torch::Tensor best_idx, torch::Tensor best_inter) {
  CHECK_IN(grp_ptr, torch::kInt64);
  CHECK_IN(grp_nodes, torch::kInt32);
  CHECK_IN(node_ptr, torch::kInt64);
  CHECK_IN(node_comm, torch::kInt32);
  CHECK_IN(size_y, torch::kInt32);
  CHECK_IN(best_idx, torch::kInt32);
  CHECK_IN(best_inter, torch::kInt32);
  TORCH_CHECK(grp_ptr.dim() == 1 && grp_ptr.size(0) >= 1,
              "grp_ptr must be [G+1]");
  TORCH_CHECK(node_ptr.dim() == 1 && node_ptr.size(0) >= 1,
              "node_ptr must be [N+1]");
  TORCH_CHECK(tile >= 1 && tile <= k8_max_tile(), "tile must be in [1, ",
              k8_max_tile(), "], got ", tile);
  const int64_t G = grp_ptr.size(0) - 1;
  const int64_t N = node_ptr.size(0) - 1;
  const int64_t Gy = size_y.size(0);
  TORCH_CHECK(N < (int64_t(1) << 31), "N must be < 2^31");
  TORCH_CHECK(G < (int64_t(1) << 31) && Gy < (int64_t(1) << 31),
              "community counts must be < 2^31");
  TORCH_CHECK(best_idx.size(0) == G && best_inter.size(0) == G,
              "best_idx/best_inter must be [G]");
  launch_k8_cover_match(i64p(grp_ptr), grp_nodes.data_ptr<int>(),
                        i64p(node_ptr), node_comm.data_ptr<int>(),
                        size_y.data_ptr<int>(), (int)G,
                        (long long)grp_nodes.size(0), (int)N,
                        (long long)node_comm.size(0), (int)Gy, (int)tile,
                        best_idx.data_ptr<int>(), best_inter.data_ptr<int>(),
                        current_stream());
}

// K10: per-community integer edge counts of a cover on a graph (see
// k10_community_scores in score_kernels.hip).  The cover is group-major
// (grp_ptr/grp_nodes, ascending per community), the graph a symmetric CSR;
// dmed = floor(median degree) from the host.
void community_scores(torch::Tensor grp_ptr, torch::Tensor grp_nodes,
                      torch::Tensor indptr, torch::Tensor indices,
                      int64_t dmed, int64_t tile, torch::Tensor int_deg,
                      torch::Tensor vol, torch::Tensor m2,
                      torch::Tensor n_flake, torch::Tensor n_fomd) {
  CHECK_IN(grp_ptr, torch::kInt64);
  CHECK_IN(grp_nodes, torch::kInt32);
  CHECK_IN(indptr, torch::kInt64);
  CHECK_IN(indices, torch::kInt32);
  CHECK_IN(int_deg, torch::kInt32);
  CHECK_IN(vol, torch::kInt64);
  CHECK_IN(m2, torch::kInt64);
  CHECK_IN(n_flake, torch::kInt32);
  CHECK_IN(n_fomd, torch::kInt32);
  const auto dev = grp_ptr.device();
  TORCH_CHECK(grp_nodes.device() == dev && indptr.device() == dev &&
                  indices.device() == dev && int_deg.device() == dev &&
                  vol.device() == dev && m2.device() == dev &&
                  n_flake.device() == dev && n_fomd.device() == dev,
              "all tensors must be on the same device");
  TORCH_CHECK(grp_ptr.dim() == 1 && grp_ptr.size(0) >= 1,
              "grp_ptr must be [G+1]");
  TORCH_CHECK(indptr.dim() == 1 && indptr.size(0) >= 1,
              "indptr must be [N+1]");
  TORCH_CHECK(grp_nodes.dim() == 1 && indices.dim() == 1,
              "grp_nodes and indices must be 1-D");
  TORCH_CHECK(tile >= 1 && tile <= k10_max_tile(), "tile must be in [1, ",
              k10_max_tile(), "], got ", tile);
  const int64_t G = grp_ptr.size(0) - 1;
  const int64_t N = indptr.size(0) - 1;
  const int64_t M = grp_nodes.size(0);
  TORCH_CHECK(N < (int64_t(1) << 31), "N must be < 2^31");
  TORCH_CHECK(G < (int64_t(1) << 31), "community count must be < 2^31");
  TORCH_CHECK(dmed >= 0 && dmed < (int64_t(1) << 31), "dmed out of range");
  TORCH_CHECK(int_deg.dim() == 1 && int_deg.size(0) == M,
              "int_deg must be [M]");
  TORCH_CHECK(vol.dim() == 1 && vol.size(0) == G && m2.dim() == 1 &&
                  m2.size(0) == G && n_flake.dim() == 1 &&
                  n_flake.size(0) == G && n_fomd.dim() == 1 &&
                  n_fomd.size(0) == G,
              "vol/m2/n_flake/n_fomd must be [G]");
  launch_k10_community_scores(
      i64p(grp_ptr), grp_nodes.data_ptr<int>(), i64p(indptr),
      indices.data_ptr<int>(), (int)G, (long long)M, (int)N,
      (long long)indices.size(0), (int)dmed, (int)tile,
      int_deg.data_ptr<int>(),
      reinterpret_cast<long long*>(vol.data_ptr<int64_t>()),
      reinterpret_cast<long long*>(m2.data_ptr<int64_t>()),
      n_flake.data_ptr<int>(), n_fomd.data_ptr<int>(), current_stream());
}

// K11: top-n link recommendation for the queries q[sel[*]] from the sparse
// model (row- and column-major) against the graph's CSR (see k11_topn_links
// in link_kernels.hip).  One launch: lds_slots > 0 keeps every table in
// LDS, lds_slots == 0 in the slices tab_off of scratch_keys/scratch_vals.
// Everything the kernel indexes with is verified here, once per call, from
// the min/max of the index tensors.
void topn_links(torch::Tensor row_ptr, torch::Tensor row_col,
                torch::Tensor row_val, torch::Tensor col_ptr,
                torch::Tensor col_row, torch::Tensor col_val,
                torch::Tensor indptr, torch::Tensor indices, torch::Tensor q,
                torch::Tensor sel, torch::Tensor tab_slots,
                torch::Tensor tab_off, torch::Tensor scratch_keys,
                torch::Tensor scratch_vals, int64_t n, int64_t lds_slots,
                int64_t block, torch::Tensor top_id, torch::Tensor top_score,
                torch::Tensor n_cand) {
  CHECK_IN(row_ptr, torch::kInt64);
  CHECK_IN(row_col, torch::kInt32);
  CHECK_IN(row_val, torch::kFloat32);
  CHECK_IN(col_ptr, torch::kInt64);
  CHECK_IN(col_row, torch::kInt32);
  CHECK_IN(col_val, torch::kFloat32);
  CHECK_IN(indptr, torch::kInt64);
  CHECK_IN(indices, torch::kInt32);
  CHECK_IN(q, torch::kInt32);
  CHECK_IN(sel, torch::kInt32);
  CHECK_IN(tab_slots, torch::kInt32);
  CHECK_IN(tab_off, torch::kInt64);
  CHECK_IN(scratch_keys, torch::kInt32);
  CHECK_IN(scratch_vals, torch::kFloat32);
  CHECK_IN(top_id, torch::kInt32);
  CHECK_IN(top_score, torch::kFloat32);
  CHECK_IN(n_cand, torch::kInt32);
  const auto dev = row_ptr.device();
  for (const auto& t :
       {row_col, row_val, col_ptr, col_row, col_val, indptr, indices, q, sel,
        tab_slots, tab_off, scratch_keys, scratch_vals, top_id, top_score,
        n_cand})
    TORCH_CHECK(t.device() == dev, "all tensors must be on the same device");
  TORCH_CHECK(n >= 1 && n <= k11_max_n(), "n must be in [1, ", k11_max_n(),
              "], got ", n);
  TORCH_CHECK(block == 64 || block == 128 || block == 256,
              "block must be 64, 128 or 256, got ", block);
  TORCH_CHECK(lds_slots >= 0 && lds_slots <= k11_max_lds_slots(),
              "lds_slots must be in [0, ", k11_max_lds_slots(), "], got ",
              lds_slots);
  for (const auto& t : {row_ptr, row_col, row_val, col_ptr, col_row, col_val,
                        indptr, indices, q, sel, tab_slots, tab_off,
                        scratch_keys, scratch_vals, n_cand})
    TORCH_CHECK(t.dim() == 1, "index and value arrays must be 1-D");
  TORCH_CHECK(row_ptr.size(0) >= 1 && indptr.size(0) == row_ptr.size(0),
              "row_ptr and indptr must both be [N+1]");
  TORCH_CHECK(col_ptr.size(0) >= 1, "col_ptr must be [K+1]");
  const int64_t N = row_ptr.size(0) - 1;
  const int64_t K = col_ptr.size(0) - 1;
  const int64_t mnnz = row_col.size(0);
  const int64_t Q = q.size(0);
  const int64_t Qsel = sel.size(0);
  TORCH_CHECK(N < (int64_t(1) << 31) && K < (int64_t(1) << 31) &&
                  Q < (int64_t(1) << 31),
              "N, K and the query count must be < 2^31");
  TORCH_CHECK(row_val.size(0) == mnnz && col_row.size(0) == mnnz &&
                  col_val.size(0) == mnnz,
              "row_col/row_val/col_row/col_val must all be [nnz]");
  TORCH_CHECK(tab_slots.size(0) == Qsel, "tab_slots must be [len(sel)]");
  TORCH_CHECK(lds_slots > 0 || tab_off.size(0) == Qsel,
              "tab_off must be [len(sel)] for global tables");
  TORCH_CHECK(scratch_vals.size(0) == scratch_keys.size(0),
              "scratch_keys and scratch_vals must have one length");
  TORCH_CHECK(top_id.dim() == 2 && top_id.size(0) == Q && top_id.size(1) == n,
              "top_id must be [Q, n]");
  TORCH_CHECK(top_score.dim() == 2 && top_score.size(0) == Q &&
                  top_score.size(1) == n,
              "top_score must be [Q, n]");
  TORCH_CHECK(n_cand.size(0) == Q, "n_cand must be [Q]");
  if (Qsel == 0) return;
  TORCH_CHECK(q.min().item<int>() >= 0 && q.max().item<int>() < N,
              "q out of range [0, N)");
  TORCH_CHECK(sel.min().item<int>() >= 0 && sel.max().item<int>() < Q,
              "sel out of range [0, Q)");
  const int64_t smin = tab_slots.min().item<int>();
  const int64_t smax = tab_slots.max().item<int>();
  TORCH_CHECK(smin >= k11_min_slots() &&
                  tab_slots.bitwise_and(tab_slots - 1).max().item<int>() == 0,
              "tab_slots must be powers of two >= ", k11_min_slots());
  if (lds_slots > 0) {
    TORCH_CHECK(smax <= lds_slots, "a table exceeds lds_slots");
  } else {
    TORCH_CHECK(tab_off.min().item<int64_t>() >= 0 &&
                    (tab_off + tab_slots).max().item<int64_t>() <=
                        scratch_keys.size(0),
                "a table slice lies outside the scratch buffer");
  }
  launch_k11_topn_links(
      i64p(row_ptr), row_col.data_ptr<int>(), row_val.data_ptr<float>(),
      i64p(col_ptr), col_row.data_ptr<int>(), col_val.data_ptr<float>(),
      i64p(indptr), indices.data_ptr<int>(), q.data_ptr<int>(),
      sel.data_ptr<int>(), tab_slots.data_ptr<int>(), i64p(tab_off),
      scratch_keys.data_ptr<int>(), scratch_vals.data_ptr<float>(), (int)Qsel,
      (int)N, (int)K, (long long)mnnz, (long long)indices.size(0), (int)n,
      (int)lds_slots, (int)block, top_id.data_ptr<int>(),
      top_score.data_ptr<float>(), n_cand.data_ptr<int>(), current_stream());
}

// K9: x[i] = F[pu[i]] . F[pv[i]] over the row space [F_own ; F_extra]
// (index < n_own reads F_own, otherwise F_extra[index - n_own]; see
// k9_pair_dot_t in pair_kernels.hip).  The index range is verified here,
// once per call, from the min/max of the index tensors — the kernel itself
// carries no per-element check that could fail.
void pair_dot(torch::Tensor F_own, torch::Tensor F_extra, torch::Tensor pu,
              torch::Tensor pv, torch::Tensor x) {
  CHECK_IN(pu, torch::kInt32);
  CHECK_IN(pv, torch::kInt32);
  CHECK_IN(x, torch::kFloat32);
  TORCH_CHECK(F_own.is_cuda(), "F_own must be on GPU");
  TORCH_CHECK(F_extra.is_cuda(), "F_extra must be on GPU");
  TORCH_CHECK(F_own.scalar_type() == torch::kFloat32 ||
                  F_own.scalar_type() == torch::kBFloat16,
              "F_own has wrong dtype (fp32 or bf16)");
  TORCH_CHECK(F_extra.scalar_type() == F_own.scalar_type(),
              "F_extra has wrong dtype (must match F_own)");
  TORCH_CHECK(F_own.is_contiguous(), "F_own must be contiguous");
  TORCH_CHECK(F_extra.is_contiguous(), "F_extra must be contiguous");
  TORCH_CHECK(F_own.dim() == 2 && F_extra.dim() == 2,
              "F_own/F_extra must be [rows, kp]");
  const auto dev = F_own.device();
  TORCH_CHECK(F_extra.device() == dev && pu.device() == dev &&
                  pv.device() == dev && x.device() == dev,
              "all tensors must be on the same device");
  const int64_t kp = F_own.size(1);
  TORCH_CHECK(F_extra.size(1) == kp, "F_own and F_extra differ in kp (",
              kp, " vs ", F_extra.size(1), ")");
  const bool bf16 = is_bf16(F_own);
  TORCH_CHECK(kp >= 1 && kp % (bf16 ? 8 : 4) == 0,
              "kp must be padded to a multiple of ", bf16 ? 8 : 4);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(F_own.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(F_extra.data_ptr()) % 16 == 0,
              "F_own/F_extra must be 16-byte aligned");
  TORCH_CHECK(pu.dim() == 1 && pv.dim() == 1 && pu.size(0) == pv.size(0),
              "pu and pv must be 1-D of the same length");
  const int64_t P = pu.size(0);
  TORCH_CHECK(x.dim() == 1 && x.size(0) == P, "x must be [P]");
  const int64_t n_own = F_own.size(0);
  const int64_t n_extra = F_extra.size(0);
  TORCH_CHECK(n_own + n_extra < (int64_t(1) << 31),
              "row count must be < 2^31");
  if (P == 0) return;
  const int64_t lo =
      std::min(pu.min().item<int64_t>(), pv.min().item<int64_t>());
  const int64_t hi =
      std::max(pu.max().item<int64_t>(), pv.max().item<int64_t>());
  TORCH_CHECK(lo >= 0 && hi < n_own + n_extra,
              "pair index out of range: [", lo, ", ", hi, "] vs ",
              n_own + n_extra, " rows");
  launch_k9_pair_dot(F_own.data_ptr(), F_extra.data_ptr(), bf16 ? 1 : 0,
                     pu.data_ptr<int>(), pv.data_ptr<int>(),
                     x.data_ptr<float>(), (long long)P, (int)n_own,
                     (int)n_extra, (int)kp, current_stream());
}

void conductance(torch::Tensor indptr, torch::Tensor indices,
                 torch::Tensor cond, double total_degree) {
  CHECK_IN(indptr, torch::kInt64);
  CHECK_IN(indices, torch::kInt32);
  CHECK_IN(cond, torch::kFloat64);
  TORCH_CHECK(indptr.dim() == 1 && indptr.size(0) >= 1,
              "indptr must be 1-D and non-empty ([N+1])");
  TORCH_CHECK(cond.dim() == 1, "cond must be 1-D");
  const int n = (int)indptr.size(0) - 1;
  TORCH_CHECK(cond.size(0) == n);
  launch_k5(reinterpret_cast<const long long*>(indptr.data_ptr<int64_t>()),
            indices.data_ptr<int>(), cond.data_ptr<double>(), n,
            total_degree, current_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("edge_grad_llh", &edge_grad_llh,
        "K1: fused per-node gradient + local LLH (CDNA4)");
  m.def("llh_only", &llh_only, "K4: per-node local LLH (CDNA4)");
  m.def("linesearch", &linesearch,
        "K2: 16-candidate Armijo line search in one edge pass (CDNA4)");
  m.def("apply_step", &apply_step,
        "K3: in-place projected commit F += s*grad (CDNA4); rows=: only "
        "the listed rows, recording dirty[u] = steps[u] > 0",
        py::arg("F_local"), py::arg("grad"), py::arg("steps"),
        py::arg("min_f"), py::arg("max_f"), py::arg("rows") = py::none(),
        py::arg("dirty") = py::none());
  m.def("conductance", &conductance,
        "K5: ego-net conductance per node (CDNA4)");
  m.def("fused_grad_ls", &fused_grad_ls,
        "KF: fused K1 gradient+LLH and K2 line search, one pass per node "
        "(MFMA tiles for the high-degree prefix)");
  m.def("apply_step_colsum", &apply_step_colsum,
        "K3+colsum fused (bf16): commit F and emit per-stripe column sums");
  m.def("sparse_support", &sparse_support,
        "KAF: per-row support compaction of F (count or fill pass); "
        "rows=: only the listed rows",
        py::arg("F"), py::arg("soffset"), py::arg("scount"), py::arg("sidx"),
        py::arg("sval"), py::arg("cap"), py::arg("fill"), py::arg("dirty"),
        py::arg("rows") = py::none());
  m.def("sparse_fused", &sparse_fused,
        "KFS/KFW/KFP: fused compact gradient + 16-candidate Armijo for routed "
        "nodes (LDS bitmap active sets); order[:n_block] one block per "
        "node, order[n_block:] one wave per node, or four per wave for the "
        "pack positions wsplit[:n_pack] when qcap > 0; with zscr the zero "
        "class among them is filled from its representatives",
        py::arg("F"), py::arg("indptr"), py::arg("indices"), py::arg("sumF"),
        py::arg("order"), py::arg("soffset"), py::arg("sidx"),
        py::arg("sval"), py::arg("scount"), py::arg("epre"),
        py::arg("bound"), py::arg("goffset"), py::arg("gidx"),
        py::arg("gval"), py::arg("gcount"), py::arg("llh"), py::arg("GG"),
        py::arg("ladder"), py::arg("best"), py::arg("cap"), py::arg("alpha"),
        py::arg("min_p"), py::arg("max_p"), py::arg("min_f"),
        py::arg("max_f"), py::arg("n_block"), py::arg("wcap"),
        py::arg("qcap") = 0, py::arg("wsplit") = py::none(),
        py::arg("n_pack") = 0, py::arg("skip") = true,
        py::arg("n_zero") = 0, py::arg("n_rep") = 0,
        py::arg("zscr") = py::none());
  m.def("sparse_commit_group", []() { return (int64_t)k3w_group(); },
        "wave-class positions one wave of the sparse commit (K3W) serves");
  m.def("sparse_pack_lds_bytes",
        [](bool bf16, int64_t K, int64_t qcap) {
          return (int64_t)kfp_lds_bytes(bf16 ? 1 : 0, (int)K, (int)qcap);
        },
        "KFP dynamic LDS bytes at (dtype, padded K, qcap)");
  m.def("sparse_wave_lds_bytes",
        [](bool bf16, int64_t K, int64_t wcap) {
          return (int64_t)kfw_lds_bytes(bf16 ? 1 : 0, (int)K, (int)wcap);
        },
        "KFW dynamic LDS bytes at (dtype, padded K, wcap)");
  m.def("sparse_colsum", &sparse_colsum,
        "list-based column sums (sparse path; stale/over-cap rows dense)");
  m.def("colsum_stage2", &colsum_stage2,
        "fixed-order sum of the [n_stripes, K] column partials into out[K]");
  m.def("sparse_route", &sparse_route,
        "routing: node-local support prefix, bounds, classes and the stable "
        "[block | wave | dense] order; returns the three class sizes (and "
        "n_pack when the packed split is requested; with zscr: n_pack, "
        "n_zero and the number of zero-class representatives)",
        py::arg("indptr"), py::arg("indices"), py::arg("scount"),
        py::arg("order"), py::arg("sumF"), py::arg("cap"), py::arg("wcap"),
        py::arg("epre"), py::arg("bound"), py::arg("cls"), py::arg("tcount"),
        py::arg("tbase"), py::arg("totals"), py::arg("GG"),
        py::arg("by_class"), py::arg("qcap") = py::none(),
        py::arg("wsplit") = py::none(), py::arg("pscr") = py::none(),
        py::arg("zscr") = py::none(), py::arg("zero") = false);
  m.def("sparse_zero_layout",
        []() {
          return std::vector<int64_t>{ZR_REP, ZR_NODE, ZR_TILES};
        },
        "zscr offsets: representatives' pack positions, representative node "
        "by degree, start of the per-tile scratch (6 ints per tile; zsplit "
        "[n_local] follows it)");
  m.def("sparse_route_tile", []() { return (int64_t)route_tile(); },
        "launch-order positions per routing tile");
  m.def("sparse_commit", &sparse_commit,
        "K3S/K3W: sparse projected commit confined to the active set; "
        "order[:n_block] one block per node, order[n_block:] one wave per "
        "node",
        py::arg("F"), py::arg("order"), py::arg("goffset"), py::arg("gidx"),
        py::arg("gval"), py::arg("gcount"), py::arg("best"),
        py::arg("soffset"), py::arg("sidx"), py::arg("sval"),
        py::arg("scount"), py::arg("cap"), py::arg("min_f"),
        py::arg("max_f"), py::arg("n_block") = -1, py::arg("wcap") = 0,
        py::arg("dirty") = py::none());
  m.def("edge_grad_llh_chunked", &edge_grad_llh_chunked,
        "K1 large-K: KD per-edge dots + KW chunked weighted accumulate");
  m.def("seed_init", &seed_init,
        "K6: seed-init F scatter (community c = neighbors of seed c)");
  m.def("extract_count", &extract_count,
        "K7 pass 1: per-row membership counts (threshold/argmax-fallback)");
  m.def("extract_fill", &extract_fill,
        "K7 pass 2: write ascending community ids at per-row offsets");
  m.def("cover_best_match", &cover_best_match,
        "K8: exact best-match (F1/Jaccard argmax) of cover Y per community "
        "of cover X, tiled LDS intersection histogram");
  m.attr("COVER_MAX_TILE") = k8_max_tile();
  m.def("community_scores", &community_scores,
        "K10: per-community integer edge counts (int_deg, vol, m2, n_flake, "
        "n_fomd) of a cover on a CSR graph, 16-lane group per member, tiled "
        "LDS membership search");
  m.attr("SCORE_MAX_TILE") = k10_max_tile();
  m.def("topn_links", &topn_links,
        "K11: top-n link recommendation per query node from the sparse "
        "model, one block per query, open-addressing (id, score) table in "
        "LDS or global scratch, ordered fp32 accumulation");
  m.attr("LINK_MAX_N") = k11_max_n();
  m.attr("LINK_MIN_SLOTS") = k11_min_slots();
  m.attr("LINK_MAX_LDS_SLOTS") = k11_max_lds_slots();
  m.def("pair_dot", &pair_dot,
        "K9: F row dot products for arbitrary node pairs over the row space "
        "[F_own ; F_extra], one wave per pair, deterministic");
  m.def("mfma_probe", &mfma_probe,
        "MFMA C/D layout probe: one 16x16 D = A @ Bc^T tile");
}
