// BigCLAM CDNA4 (gfx950 / MI355X) HIP kernels — top-n link recommendation
// from the sparse form of a fitted model.
//
//   K11 k11_topn_links — for every query node u the n nodes v with the
//                        largest F_u . F_v among the nodes that are not u,
//                        not a CSR neighbour of u, and share at least one
//                        nonzero column with u: one row of F . F^T, sparse
//                        times sparse-transposed.
//
// Inputs: the model twice, row-major (row_ptr int64 [N+1], row_col int32
// ascending per row, row_val fp32) and column-major (col_ptr int64 [K+1],
// col_row int32 ascending per column, col_val fp32), and the graph as a
// symmetric CSR (indptr int64 [N+1], indices int32 ascending per row).
//
// Score, defined operationally: acc = 0.0f; for the columns c of row u in
// ASCENDING order, for every member v of c:
//   p = __fmul_rn(F_uc, F_vc);  acc_v = __fadd_rn(acc_v, p);
// two separately rounded fp32 operations, never an FMA, so the CPU
// implementation (ops/links_cpu.py, NumPy float32) performs the identical
// IEEE operations and the outputs agree bitwise.
//
// One block per query.  Scores accumulate in an open-addressing table of
// (id, score) with linear probing, keyed by candidate id.  The outer loop
// over u's columns is serial and block-uniform; the threads stride over
// the column's member list.  Members are distinct within a column, so
// every slot takes at most one update per column: the thread that holds v
// finds or claims v's slot with an integer compare-and-swap and adds with
// a plain read-modify-write.  A __syncthreads() between columns orders
// the updates of one column before the next one's, which makes the order
// of every fp32 sum the column order.  Slots are never released while
// columns are walked, so a key stays reachable from its hash position.
// WHICH slot a key lands in depends on the race; the (id, score) content
// of the table does not.
//
// Afterwards the threads stride over the slots and clear u itself, u's CSR
// neighbours (lower-bound binary search in the sorted row, as K5 and K10)
// and scores that are not > 0; the survivors are counted (n_cand).  Then n
// rounds of a block arg-max on (score descending, id ascending): per
// thread over its slots, wave butterfly, one LDS round across the waves;
// thread 0 stores the winner and clears its slot.  The rounds stop early
// when the table is empty.  Output rows are pre-filled with the pads
// (-1, 0) by the caller.
//
// The table has `slots` entries (a power of two, per query) and lives in
// dynamic LDS (template LDS_TABLE = true, 8 bytes per slot) or in the
// query's slice [off, off + slots) of a global scratch (false); the code
// is otherwise the same.  The host sizes it to at least twice the exact
// candidate bound T_u = sum of |members(c)| over u's columns, so it can
// never fill; a probe still gives up after `slots` steps, so a malformed
// size cannot spin or write elsewhere.
//
// Determinism: the only atomics are the integer CAS that claim slots; no
// floating-point atomics.  A query's result depends on its own row, its
// columns and its CSR row only — not on the other queries of the launch,
// on the table's placement or on the block size.
//
// Defensive: pointer ranges are clamped to the arrays (as K10), column ids
// outside [0, K) and member ids outside [0, N) are skipped.

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#define K11_WAVE 64
#define K11_MAX_BLOCK 256
#define K11_MAX_NWAVE (K11_MAX_BLOCK / K11_WAVE)
#define K11_MAX_N 64
#define K11_MIN_SLOTS 64
#define K11_MAX_LDS_SLOTS 8192  // 64 KB of (id, score)

// (score desc, id asc); id < 0 = nothing
__device__ __forceinline__ bool k11_better(float s, int id, float bs, int bid) {
  if (id < 0) return false;
  if (bid < 0) return true;
  return s > bs || (s == bs && id < bid);
}

template <bool LDS_TABLE>
__global__ void __launch_bounds__(K11_MAX_BLOCK) k11_topn_links(
    const long long* __restrict__ row_ptr, const int* __restrict__ row_col,
    const float* __restrict__ row_val, const long long* __restrict__ col_ptr,
    const int* __restrict__ col_row, const float* __restrict__ col_val,
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const int* __restrict__ q, const int* __restrict__ sel,
    const int* __restrict__ tab_slots, const long long* __restrict__ tab_off,
    int* g_keys, float* g_vals, int Qsel, int N, int K, long long mnnz,
    long long gnnz, int n, int* __restrict__ top_id,
    float* __restrict__ top_score, int* __restrict__ n_cand) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float red_s[K11_MAX_NWAVE];
  __shared__ int red_id[K11_MAX_NWAVE];
  __shared__ int red_slot[K11_MAX_NWAVE];

  const int b = blockIdx.x;
  if (b >= Qsel) return;
  const int tid = threadIdx.x;
  const int nthr = blockDim.x;
  const int lane = tid & (K11_WAVE - 1);
  const int wid = tid / K11_WAVE;
  const int nwave = nthr / K11_WAVE;
  const int i = sel[b];
  const int u = q[i];
  const int slots = tab_slots[b];  // power of two >= K11_MIN_SLOTS
  const unsigned mask = (unsigned)slots - 1u;
  const int shift = __clz(slots) + 1;  // 32 - log2(slots)

  int* keys;
  float* vals;
  if (LDS_TABLE) {
    keys = reinterpret_cast<int*>(smem);
    vals = reinterpret_cast<float*>(smem) + slots;
  } else {
    keys = g_keys + tab_off[b];
    vals = g_vals + tab_off[b];
  }
  for (int s = tid; s < slots; s += nthr) {
    keys[s] = -1;
    vals[s] = 0.0f;
  }
  __syncthreads();

  long long r0 = 0, r1 = 0, e0 = 0, e1 = 0;
  if ((unsigned)u < (unsigned)N) {
    r0 = row_ptr[u];
    r1 = row_ptr[u + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > mnnz ? mnnz : r1;
    e0 = indptr[u];
    e1 = indptr[u + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > gnnz ? gnnz : e1;
  }

  // accumulate: columns of u serially, ascending (block-uniform loop)
  for (long long j = r0; j < r1; ++j) {
    const int c = row_col[j];
    const float a = row_val[j];
    long long m0 = 0, m1 = 0;
    if ((unsigned)c < (unsigned)K) {
      m0 = col_ptr[c];
      m1 = col_ptr[c + 1];
      m0 = m0 < 0 ? 0 : m0;
      m1 = m1 > mnnz ? mnnz : m1;
    }
    for (long long m = m0 + tid; m < m1; m += nthr) {
      const int v = col_row[m];
      if ((unsigned)v >= (unsigned)N) continue;
      const float p = __fmul_rn(a, col_val[m]);
      unsigned s = ((unsigned)v * 0x9E3779B1u) >> shift;
      for (int step = 0; step < slots; ++step) {
        int old = keys[s];
        if (old == -1) old = atomicCAS(&keys[s], -1, v);
        if (old == -1 || old == v) {
          vals[s] = __fadd_rn(vals[s], p);
          break;
        }
        s = (s + 1u) & mask;
      }
    }
    __syncthreads();  // this column's updates before the next column's
  }

  // exclusions: u, its CSR neighbours, scores not > 0; count the rest
  int cnt = 0;
  for (int s = tid; s < slots; s += nthr) {
    const int v = keys[s];
    if (v < 0) continue;
    bool drop = v == u || !(vals[s] > 0.0f);
    if (!drop) {
      long long lo = e0, hi = e1;  // lower bound of v in indices[e0, e1)
      while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (indices[mid] < v) lo = mid + 1;
        else hi = mid;
      }
      drop = lo < e1 && indices[lo] == v;
    }
    if (drop) keys[s] = -1;
    else ++cnt;
  }
#pragma unroll
  for (int off = K11_WAVE / 2; off > 0; off >>= 1)
    cnt += __shfl_xor(cnt, off, K11_WAVE);
  if (lane == 0) red_id[wid] = cnt;
  __syncthreads();  // also: cleared keys visible to the arg-max rounds
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < nwave; ++w) total += red_id[w];
    n_cand[i] = total;
  }
  __syncthreads();  // red_id is reused below

  // n rounds of block arg-max on (score desc, id asc)
  for (int r = 0; r < n; ++r) {
    float bs = 0.0f;
    int bid = -1, bslot = -1;
    for (int s = tid; s < slots; s += nthr) {
      const int v = keys[s];
      const float sc = vals[s];
      if (k11_better(sc, v, bs, bid)) {
        bs = sc;
        bid = v;
        bslot = s;
      }
    }
#pragma unroll
    for (int off = K11_WAVE / 2; off > 0; off >>= 1) {
      const float os = __shfl_xor(bs, off, K11_WAVE);
      const int oid = __shfl_xor(bid, off, K11_WAVE);
      const int oslot = __shfl_xor(bslot, off, K11_WAVE);
      if (k11_better(os, oid, bs, bid)) {
        bs = os;
        bid = oid;
        bslot = oslot;
      }
    }
    if (lane == 0) {
      red_s[wid] = bs;
      red_id[wid] = bid;
      red_slot[wid] = bslot;
    }
    __syncthreads();
    bs = red_s[0];
    bid = red_id[0];
    bslot = red_slot[0];
    for (int w = 1; w < nwave; ++w) {
      if (k11_better(red_s[w], red_id[w], bs, bid)) {
        bs = red_s[w];
        bid = red_id[w];
        bslot = red_slot[w];
      }
    }
    if (bid < 0) break;  // table empty (block-uniform)
    if (tid == 0) {
      top_id[(long long)i * n + r] = bid;
      top_score[(long long)i * n + r] = bs;
      keys[bslot] = -1;
    }
    __syncthreads();  // winner cleared, red_* free for the next round
  }
}

extern "C" int k11_max_n() { return K11_MAX_N; }
extern "C" int k11_min_slots() { return K11_MIN_SLOTS; }
extern "C" int k11_max_lds_slots() { return K11_MAX_LDS_SLOTS; }

// One launch over the Qsel queries sel[0..Qsel): lds_slots > 0 puts every
// table in dynamic LDS sized for lds_slots entries (the largest table of
// the launch); lds_slots == 0 uses the slices tab_off of g_keys/g_vals.
extern "C" void launch_k11_topn_links(
    const long long* row_ptr, const int* row_col, const float* row_val,
    const long long* col_ptr, const int* col_row, const float* col_val,
    const long long* indptr, const int* indices, const int* q, const int* sel,
    const int* tab_slots, const long long* tab_off, int* g_keys, float* g_vals,
    int Qsel, int N, int K, long long mnnz, long long gnnz, int n,
    int lds_slots, int block, int* top_id, float* top_score, int* n_cand,
    hipStream_t stream) {
  if (Qsel == 0) return;
  if (n < 1 || n > K11_MAX_N)
    throw std::runtime_error("k11_topn_links: n out of range");
  if (block != 64 && block != 128 && block != 256)
    throw std::runtime_error("k11_topn_links: block must be 64, 128 or 256");
  if (lds_slots < 0 || lds_slots > K11_MAX_LDS_SLOTS)
    throw std::runtime_error("k11_topn_links: lds_slots out of range");
  if (lds_slots > 0) {
    const size_t lds = (size_t)lds_slots * (sizeof(int) + sizeof(float));
    hipLaunchKernelGGL(k11_topn_links<true>, dim3(Qsel), dim3(block), lds,
                       stream, row_ptr, row_col, row_val, col_ptr, col_row,
                       col_val, indptr, indices, q, sel, tab_slots, tab_off,
                       g_keys, g_vals, Qsel, N, K, mnnz, gnnz, n, top_id,
                       top_score, n_cand);
  } else {
    hipLaunchKernelGGL(k11_topn_links<false>, dim3(Qsel), dim3(block), 0,
                       stream, row_ptr, row_col, row_val, col_ptr, col_row,
                       col_val, indptr, indices, q, sel, tab_slots, tab_off,
                       g_keys, g_vals, Qsel, N, K, mnnz, gnnz, n, top_id,
                       top_score, n_cand);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("HIP error: ") +
                             hipGetErrorString(e) + " at " __FILE__);
}
