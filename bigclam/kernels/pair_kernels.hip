// BigCLAM CDNA4 (gfx950 / MI355X) HIP kernels — arbitrary node-pair scoring.
//
//   K9 k9_pair_dot_t<T> — x[i] = F[pu[i]] · F[pv[i]] for a list of node
//                         pairs that need not be edges (held-out edges and
//                         sampled non-edges; engine/holdout.py).
//
// The rows live in two buffers: the rank's own shard F_own [n_own, kp] and
// the off-shard rows fetched for this call, F_extra [n_extra, kp]
// (core/pairs.py).  An index idx < n_own reads F_own[idx], any other index
// reads F_extra[idx - n_own]; the kernel takes both base pointers, so the
// owned shard is never copied to form one buffer.
//
// One wave per pair, four pairs per 256-thread block.  Lane l reads the
// 16-byte vectors l, l + 64, l + 128, ... of both rows (float4, or 8 bf16 as
// one uint4), so a wave's load is 1 KiB contiguous per row per step; kp is
// padded by the caller to a whole number of vectors (core/state.py).  Each
// lane folds its elements, in ascending k, into ONE fp32 accumulator by
// fmaf, and the 64 partial sums are combined by a fixed 6-level __shfl_xor
// butterfly (offsets 32, 16, ..., 1).  Lane 0 writes x[i] with an ordinary
// vector store.
//
// The longest fp32 addition chain is therefore
//   d = (vectors per lane) * (elements per vector) + 6
//     = ceil(kp / 256) * 4 + 6  (fp32),  ceil(kp / 512) * 8 + 6  (bf16),
// and a bf16 x bf16 product is exact in fp32 (8 + 8 significand bits), which
// is what tests/test_gpu_holdout.py derives its tolerance from.
//
// No atomics and no LDS: x[i] depends on rows pu[i], pv[i] alone, through a
// fixed summation order, so it is bitwise reproducible run to run and
// independent of P and of which other pairs share the launch.
//
// Pairs arrive sorted by (u, v) (engine/holdout.py sorts them).  Consecutive
// waves then read the same row u, which they share through the XCD's L2;
// there is deliberately no staging of row u beyond that.  The kernel is
// dense over kp: it does not use the sparse sweep's support lists.
//
// The index range is checked once on the host (bindings.cpp pair_dot); the
// kernel only refuses to dereference an index outside [0, n_own + n_extra)
// and writes NaN for such a pair.

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#define K9_WAVE 64
#define K9_BLOCK 256
#define K9_NWAVE (K9_BLOCK / K9_WAVE)

// 16 bytes of a row -> fmaf chain over its elements, ascending k
__device__ __forceinline__ float k9_fma_vec(const float4 a, const float4 b,
                                            float acc) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  acc = fmaf(a.w, b.w, acc);
  return acc;
}

// one u32 = two packed bf16 (element 2j in the low half); bf16 = the high
// 16 bits of the fp32 with the same value
__device__ __forceinline__ float k9_fma_bf2(unsigned a, unsigned b,
                                            float acc) {
  acc = fmaf(__uint_as_float(a << 16), __uint_as_float(b << 16), acc);
  acc = fmaf(__uint_as_float(a & 0xffff0000u), __uint_as_float(b & 0xffff0000u),
             acc);
  return acc;
}

__device__ __forceinline__ float k9_fma_vec(const uint4 a, const uint4 b,
                                            float acc) {
  acc = k9_fma_bf2(a.x, b.x, acc);
  acc = k9_fma_bf2(a.y, b.y, acc);
  acc = k9_fma_bf2(a.z, b.z, acc);
  acc = k9_fma_bf2(a.w, b.w, acc);
  return acc;
}

// V = float4 (fp32 rows) or uint4 (bf16 rows); nvec = 16-byte vectors per row
template <typename V>
__global__ void __launch_bounds__(K9_BLOCK) k9_pair_dot_t(
    const V* __restrict__ F_own, const V* __restrict__ F_extra,
    const int* __restrict__ pu, const int* __restrict__ pv,
    float* __restrict__ x, long long P, int n_own, int n_extra, int nvec) {
  const int lane = threadIdx.x & (K9_WAVE - 1);
  const long long i =
      (long long)blockIdx.x * K9_NWAVE + (threadIdx.x / K9_WAVE);
  if (i >= P) return;  // wave-uniform
  const int u = pu[i];
  const int v = pv[i];
  const unsigned n_rows = (unsigned)n_own + (unsigned)n_extra;
  if ((unsigned)u >= n_rows || (unsigned)v >= n_rows) {  // wave-uniform
    if (lane == 0) x[i] = __builtin_nanf("");
    return;
  }
  const V* __restrict__ ru = u < n_own
                                 ? F_own + (size_t)u * nvec
                                 : F_extra + (size_t)(u - n_own) * nvec;
  const V* __restrict__ rv = v < n_own
                                 ? F_own + (size_t)v * nvec
                                 : F_extra + (size_t)(v - n_own) * nvec;
  float acc = 0.0f;
#pragma unroll 2
  for (int j = lane; j < nvec; j += K9_WAVE) acc = k9_fma_vec(ru[j], rv[j], acc);
#pragma unroll
  for (int off = K9_WAVE / 2; off > 0; off >>= 1)
    acc += __shfl_xor(acc, off, K9_WAVE);
  if (lane == 0) x[i] = acc;
}

extern "C" void launch_k9_pair_dot(const void* F_own, const void* F_extra,
                                   int is_bf16, const int* pu, const int* pv,
                                   float* x, long long P, int n_own,
                                   int n_extra, int kp, hipStream_t stream) {
  if (P == 0) return;
  const long long blocks = (P + K9_NWAVE - 1) / K9_NWAVE;
  if (blocks > 0x7fffffffLL)
    throw std::runtime_error("k9_pair_dot: too many pairs for one launch");
  if (is_bf16) {
    hipLaunchKernelGGL(k9_pair_dot_t<uint4>, dim3((unsigned)blocks),
                       dim3(K9_BLOCK), 0, stream,
                       static_cast<const uint4*>(F_own),
                       static_cast<const uint4*>(F_extra), pu, pv, x, P, n_own,
                       n_extra, kp / 8);
  } else {
    hipLaunchKernelGGL(k9_pair_dot_t<float4>, dim3((unsigned)blocks),
                       dim3(K9_BLOCK), 0, stream,
                       static_cast<const float4*>(F_own),
                       static_cast<const float4*>(F_extra), pu, pv, x, P, n_own,
                       n_extra, kp / 4);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("HIP error: ") +
                             hipGetErrorString(e) + " at " __FILE__);
}
