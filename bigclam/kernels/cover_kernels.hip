// BigCLAM CDNA4 (gfx950 / MI355X) HIP kernels — ground-truth cover matching.
//
//   K8 k8_cover_match — for every community A of cover X, the community B of
//                       cover Y that maximises F1(A,B) = 2c/(|A|+|B|),
//                       c = |A∩B| (equivalently Jaccard: F1 = 2J/(1+J) is
//                       monotone in J, so one argmax serves both scores).
//
// Inputs: X group-major (grp_ptr/grp_nodes: the members of each community),
// Y node-major (node_ptr/node_comm: the communities of each node, ascending
// per node — exactly K7's output shape) and |B| per Y-community.
//
// One 256-thread block per X-community.  The block keeps an LDS histogram
// of intersection counts over a TILE of Y ids and walks the Y side tile by
// tile (no cap on G or Gy):
//   1. clear the tile's counters;
//   2. members strided across threads; each thread walks its node's
//      Y-memberships and LDS-atomicAdds 1 on hist[y - lo] for ids inside
//      the tile (the ascending order lets the walk stop at the tile's end);
//   3. barrier;
//   4. scan the tile keeping a per-thread running best (c, |B|, idx).
// After the last tile the per-thread bests are block-reduced.
//
// Selection is EXACT: c1/(a+b1) vs c2/(a+b2) is compared by 64-bit integer
// cross-multiplication (c < 2^31, a+b < 2^32, so the products fit), ties go
// to the lowest Y index, and "no overlap" is (idx -1, c 0).  Scores are
// computed on the host in fp64 from the integer triples.
//
// Determinism: no global atomics and no K×T matrix in HBM; the only atomics
// are INTEGER LDS adds, which are order-independent, so (best_idx,
// best_inter) is bitwise reproducible and equals the CPU implementation
// (ops/cover_cpu.py) exactly.  This is unlike the sparse sweep's fp32 LDS
// atomics (see the KFS note in bigclam_kernels.hip: "the sparse path's
// documented determinism trade") — K8 is not an exception to that note, it
// simply has no floating-point accumulation at all.
//
// LDS: hist[K8_MAX_TILE] int = 64 KB static, 2 blocks/CU of the 160 KiB
// (docs/kernels.md records the compiler's resource report).  `tile` is a
// runtime value <= K8_MAX_TILE so tests can force the multi-tile path at
// tiny shapes.

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#define K8_WAVE 64
#define K8_BLOCK 256
#define K8_NWAVE (K8_BLOCK / K8_WAVE)
#define K8_MAX_TILE 16384

typedef unsigned long long k8_u64;

// true iff candidate (c2, b2, i2) beats the incumbent (c1, b1, i1) for an
// X-community of size a: larger c/(a+b) exactly, ties to the lower index.
// A "none" entry is (0, 0, -1): it loses to any c > 0 and never beats
// another "none".
__device__ __forceinline__ bool k8_better(int c2, int b2, int i2, int c1,
                                          int b1, int i1, k8_u64 a) {
  const k8_u64 l = (k8_u64)c2 * (a + (k8_u64)b1);
  const k8_u64 r = (k8_u64)c1 * (a + (k8_u64)b2);
  return l > r || (l == r && c2 > 0 && i2 < i1);
}

extern "C" __global__ void __launch_bounds__(K8_BLOCK) k8_cover_match(
    const long long* __restrict__ grp_ptr, const int* __restrict__ grp_nodes,
    const long long* __restrict__ node_ptr, const int* __restrict__ node_comm,
    const int* __restrict__ size_y, int G, long long M, int N, long long nnz_y,
    int Gy, int tile, int* __restrict__ best_idx,
    int* __restrict__ best_inter) {
  __shared__ int hist[K8_MAX_TILE];
  const int x = blockIdx.x;
  if (x >= G) return;
  const int tid = threadIdx.x;
  long long m0 = grp_ptr[x];
  long long m1 = grp_ptr[x + 1];
  // defensive clamps: a malformed CSR must not read out of bounds
  m0 = m0 < 0 ? 0 : m0;
  m1 = m1 > M ? M : m1;
  if (m1 <= m0) {  // empty X-community (block-uniform)
    if (tid == 0) {
      best_idx[x] = -1;
      best_inter[x] = 0;
    }
    return;
  }
  const k8_u64 a = (k8_u64)(m1 - m0);

  int bc = 0, bb = 0, bi = -1;
  for (int lo = 0; lo < Gy; lo += tile) {
    const int w = min(tile, Gy - lo);
    const int hi = lo + w;
    for (int i = tid; i < w; i += K8_BLOCK) hist[i] = 0;
    __syncthreads();
    for (long long m = m0 + tid; m < m1; m += K8_BLOCK) {
      const int u = grp_nodes[m];
      if ((unsigned)u >= (unsigned)N) continue;
      long long p = node_ptr[u];
      long long p1 = node_ptr[u + 1];
      p = p < 0 ? 0 : p;
      p1 = p1 > nnz_y ? nnz_y : p1;
      for (; p < p1; ++p) {
        const int y = node_comm[p];
        if (y >= hi) break;  // ascending per node
        if (y >= lo) atomicAdd(&hist[y - lo], 1);
      }
    }
    __syncthreads();
    for (int i = tid; i < w; i += K8_BLOCK) {
      const int c = hist[i];
      if (c > 0) {
        const int b = size_y[lo + i];
        if (k8_better(c, b, lo + i, bc, bb, bi, a)) {
          bc = c;
          bb = b;
          bi = lo + i;
        }
      }
    }
    __syncthreads();  // scan done before the next tile's clear
  }

  // block reduction with the same comparison: wave butterfly, then the
  // NWAVE partials through LDS (hist is free after the last barrier)
#pragma unroll
  for (int off = K8_WAVE / 2; off > 0; off >>= 1) {
    const int oc = __shfl_xor(bc, off, K8_WAVE);
    const int ob = __shfl_xor(bb, off, K8_WAVE);
    const int oi = __shfl_xor(bi, off, K8_WAVE);
    if (k8_better(oc, ob, oi, bc, bb, bi, a)) {
      bc = oc;
      bb = ob;
      bi = oi;
    }
  }
  const int lane = tid & (K8_WAVE - 1);
  const int wid = tid / K8_WAVE;
  if (lane == 0) {
    hist[3 * wid + 0] = bc;
    hist[3 * wid + 1] = bb;
    hist[3 * wid + 2] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int wv = 1; wv < K8_NWAVE; ++wv) {
      const int oc = hist[3 * wv + 0];
      const int ob = hist[3 * wv + 1];
      const int oi = hist[3 * wv + 2];
      if (k8_better(oc, ob, oi, bc, bb, bi, a)) {
        bc = oc;
        bb = ob;
        bi = oi;
      }
    }
    best_idx[x] = bi;
    best_inter[x] = bc;
  }
}

extern "C" int k8_max_tile() { return K8_MAX_TILE; }

extern "C" void launch_k8_cover_match(
    const long long* grp_ptr, const int* grp_nodes, const long long* node_ptr,
    const int* node_comm, const int* size_y, int G, long long M, int N,
    long long nnz_y, int Gy, int tile, int* best_idx, int* best_inter,
    hipStream_t stream) {
  if (G == 0) return;
  if (tile < 1 || tile > K8_MAX_TILE)
    throw std::runtime_error("k8_cover_match: tile out of range");
  hipLaunchKernelGGL(k8_cover_match, dim3(G), dim3(K8_BLOCK), 0, stream,
                     grp_ptr, grp_nodes, node_ptr, node_comm, size_y, G, M, N,
                     nnz_y, Gy, tile, best_idx, best_inter);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("HIP error: ") +
                             hipGetErrorString(e) + " at " __FILE__);
}
