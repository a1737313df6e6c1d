// BigCLAM CDNA4 (gfx950 / MI355X) HIP kernels — per-community structural
// scores of a cover on a graph.
//
//   K10 k10_community_scores — for every community S of a cover the integer
//                              edge counts that conductance, internal
//                              density, expansion, cut ratio, Flake-ODF and
//                              FOMD (Yang & Leskovec, "Defining and
//                              evaluating network communities based on
//                              ground-truth") are functions of.
//
// Inputs: the graph as a symmetric CSR (indptr int64 [N+1], indices int32
// [nnz], both directions of every edge, no self-loops) and the cover
// group-major (grp_ptr/grp_nodes: the members of each community, ASCENDING
// per community).  Outputs, all integer:
//   int_deg[m]  for member pair m = (x, u): CSR entries v of row u, v in S
//   vol[x]      sum of deg(u) over the members
//   m2[x]       sum of int_deg over the members (twice the internal edges)
//   n_flake[x]  members with 2*int_deg < deg
//   n_fomd[x]   members with int_deg > dmed (dmed = floor(median degree),
//               computed on the host)
// An empty community writes zeros; member ids outside [0, N) are skipped
// (int_deg 0, no contribution); malformed pointer ranges are clamped.
//
// One 256-thread block per community.  The block stages a TILE of at most
// `tile` of the community's sorted member ids in LDS and walks the CSR rows
// of ALL its members against it, one 16-lane group per member (16 members
// in flight per block): the group's lanes stride over the row, so the loads
// of `indices` are coalesced and a hub row is a longer loop for its group,
// never one thread's.  Per neighbour v: a range check against the tile's
// first and last id, then a lower-bound binary search in the LDS tile.  The
// group reduces its hit count with xor 8/4/2/1 and lane 0 of the group
// stores int_deg[m] in the first pass and adds to it in later ones — the
// same lane owns the same slot in every pass, so these are plain stores.
// Tiles partition S by id range, so every internal entry is counted in
// exactly one pass; a community larger than `tile` makes one pass over its
// members' edges per tile.
//
// During the last pass the owning lanes accumulate vol, m2, n_flake and
// n_fomd from the finished int_deg; the block reduces them with an integer
// wave butterfly plus a four-entry LDS round and thread 0 stores each once.
//
// Determinism: no global atomics and no floating-point arithmetic at all;
// integer sums are order-independent, so all five outputs are bitwise
// reproducible and equal the CPU implementation (ops/cover_cpu.py
// community_scores_cpu) exactly.  Scores are formed on the host in fp64.
//
// LDS: dynamic, 4*tile bytes (at least K10_RED_BYTES: the reduction round
// reuses the tile's space after the last barrier).  `tile` is a runtime
// value in [1, K10_MAX_TILE]; the wrapper sizes it to the largest
// community, so a cover of small communities runs at register-limited
// occupancy, and tests pass small tiles to force the multi-tile path.
// One very large community is one long block, as in K8.

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#define K10_WAVE 64
#define K10_BLOCK 256
#define K10_NWAVE (K10_BLOCK / K10_WAVE)
#define K10_GROUP 16
#define K10_NGROUP (K10_BLOCK / K10_GROUP)
#define K10_MAX_TILE 16384
// reduction round: NWAVE x (vol, m2) int64 + NWAVE x (n_flake, n_fomd) int
#define K10_RED_BYTES (K10_NWAVE * 2 * 8 + K10_NWAVE * 2 * 4)

extern "C" __global__ void __launch_bounds__(K10_BLOCK) k10_community_scores(
    const long long* __restrict__ grp_ptr, const int* __restrict__ grp_nodes,
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    int G, long long M, int N, long long nnz, int dmed, int tile,
    int* __restrict__ int_deg, long long* __restrict__ vol,
    long long* __restrict__ m2, int* __restrict__ n_flake,
    int* __restrict__ n_fomd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* ids = reinterpret_cast<int*>(smem);
  const int x = blockIdx.x;
  if (x >= G) return;
  const int tid = threadIdx.x;
  long long m0 = grp_ptr[x];
  long long m1 = grp_ptr[x + 1];
  // defensive clamps: a malformed CSR must not read out of bounds
  m0 = m0 < 0 ? 0 : m0;
  m1 = m1 > M ? M : m1;
  if (m1 <= m0) {  // empty community (block-uniform)
    if (tid == 0) {
      vol[x] = 0;
      m2[x] = 0;
      n_flake[x] = 0;
      n_fomd[x] = 0;
    }
    return;
  }
  const int sub = tid & (K10_GROUP - 1);
  const int grp = tid / K10_GROUP;

  long long a_vol = 0, a_m2 = 0;  // nonzero on the groups' lane 0 only
  int a_flake = 0, a_fomd = 0;
  for (long long t0 = m0; t0 < m1; t0 += tile) {
    const long long rest = m1 - t0;
    const int w = rest < (long long)tile ? (int)rest : tile;
    const bool first = t0 == m0;
    const bool last = t0 + w >= m1;
    for (int i = tid; i < w; i += K10_BLOCK) ids[i] = grp_nodes[t0 + i];
    __syncthreads();
    const int lo = ids[0];
    const int hi = ids[w - 1];
    for (long long m = m0 + grp; m < m1; m += K10_NGROUP) {
      const int u = grp_nodes[m];
      long long p = 0, p1 = 0;
      if ((unsigned)u < (unsigned)N) {
        p = indptr[u];
        p1 = indptr[u + 1];
        p = p < 0 ? 0 : p;
        p1 = p1 > nnz ? nnz : p1;
        p1 = p1 < p ? p : p1;
      }
      int cnt = 0;
      for (long long e = p + sub; e < p1; e += K10_GROUP) {
        const int v = indices[e];
        if (v < lo || v > hi) continue;
        int a = 0, b = w;  // lower bound of v in ids[0, w)
        while (a < b) {
          const int mid = (a + b) >> 1;
          if (ids[mid] < v) a = mid + 1;
          else b = mid;
        }
        cnt += (a < w && ids[a] == v) ? 1 : 0;
      }
#pragma unroll
      for (int off = K10_GROUP / 2; off > 0; off >>= 1)
        cnt += __shfl_xor(cnt, off, K10_GROUP);
      if (sub == 0) {
        const int d = first ? cnt : int_deg[m] + cnt;
        int_deg[m] = d;
        if (last) {
          const long long deg = p1 - p;
          a_vol += deg;
          a_m2 += d;
          a_flake += (2LL * d < deg) ? 1 : 0;
          a_fomd += (d > dmed) ? 1 : 0;
        }
      }
    }
    __syncthreads();  // walk done before the next tile overwrites ids
  }

  // block reduction: wave butterfly, then the NWAVE partials through LDS
  // (ids is free after the last barrier)
#pragma unroll
  for (int off = K10_WAVE / 2; off > 0; off >>= 1) {
    a_vol += __shfl_xor(a_vol, off, K10_WAVE);
    a_m2 += __shfl_xor(a_m2, off, K10_WAVE);
    a_flake += __shfl_xor(a_flake, off, K10_WAVE);
    a_fomd += __shfl_xor(a_fomd, off, K10_WAVE);
  }
  long long* red64 = reinterpret_cast<long long*>(smem);
  int* red32 = reinterpret_cast<int*>(smem + K10_NWAVE * 2 * 8);
  const int lane = tid & (K10_WAVE - 1);
  const int wid = tid / K10_WAVE;
  if (lane == 0) {
    red64[2 * wid + 0] = a_vol;
    red64[2 * wid + 1] = a_m2;
    red32[2 * wid + 0] = a_flake;
    red32[2 * wid + 1] = a_fomd;
  }
  __syncthreads();
  if (tid == 0) {
    for (int wv = 1; wv < K10_NWAVE; ++wv) {
      a_vol += red64[2 * wv + 0];
      a_m2 += red64[2 * wv + 1];
      a_flake += red32[2 * wv + 0];
      a_fomd += red32[2 * wv + 1];
    }
    vol[x] = a_vol;
    m2[x] = a_m2;
    n_flake[x] = a_flake;
    n_fomd[x] = a_fomd;
  }
}

extern "C" int k10_max_tile() { return K10_MAX_TILE; }

extern "C" void launch_k10_community_scores(
    const long long* grp_ptr, const int* grp_nodes, const long long* indptr,
    const int* indices, int G, long long M, int N, long long nnz, int dmed,
    int tile, int* int_deg, long long* vol, long long* m2, int* n_flake,
    int* n_fomd, hipStream_t stream) {
  if (G == 0) return;
  if (tile < 1 || tile > K10_MAX_TILE)
    throw std::runtime_error("k10_community_scores: tile out of range");
  size_t lds = (size_t)tile * sizeof(int);
  if (lds < K10_RED_BYTES) lds = K10_RED_BYTES;
  hipLaunchKernelGGL(k10_community_scores, dim3(G), dim3(K10_BLOCK), lds,
                     stream, grp_ptr, grp_nodes, indptr, indices, G, M, N, nnz,
                     dmed, tile, int_deg, vol, m2, n_flake, n_fomd);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("HIP error: ") +
                             hipGetErrorString(e) + " at " __FILE__);
}
