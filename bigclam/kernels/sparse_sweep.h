// Host interface of the sparse sweep: the one typed prototype of every
// sparse-path launcher and getter, the argument block the three fused
// sweep kernels share, and their LDS layouts.  Plain C++17, included by
// bindings.cpp (host) and bigclam_kernels.hip (host + device).
#pragma once

#include <hip/hip_runtime.h>

#if defined(__HIPCC__)
#define SWEEP_HD __host__ __device__ __forceinline__
#else
#define SWEEP_HD inline
#endif

#define KFW_ECAP 64   // edges of a node whose table entry KFW keeps in LDS
#define KFP_DEG 16    // most edges of a node on the packed wave path (KFP)
#define KFP_NODES 4   // nodes per wave in KFP

// Routing's zero-class buffer (int32, ZR_TILES + 6 per routing tile +
// n_local): the counts the host reads in one copy, the representatives, tile
// scratch, and zsplit: the packed positions as [bound > 0 | zero class].
#define ZR_NPACK 3    // [0..2] block / wave / dense; packed with bound > 0
#define ZR_NZERO 4    // packed with bound 0 (the zero class)
#define ZR_NREP 5     // representatives = degrees present in the zero class
#define ZR_HOST 6     // the host's one copy: the ints up to here
#define ZR_MASK 6     // bit d: a zero node of degree d exists
#define ZR_REP 8      // [KFP_DEG + 1] pack positions, degree-descending, -1
#define ZR_NODE 25    // [KFP_DEG + 1] representative node by degree, -1
#define ZR_TILES 44   // per tile (16 bytes): packable count, zero count, the
                      // zero nodes' degree mask, 0; then per tile: zero
                      // base, degrees of the earlier tiles; then zsplit
                      // [n_local]
static_assert(ZR_NODE == ZR_REP + KFP_DEG + 1 &&
                  ZR_TILES >= ZR_NODE + KFP_DEG + 1 && ZR_TILES % 4 == 0,
              "zero-class buffer layout");

// What KFS, KFW and KFP share (pools by position in `order`, lists by row)
struct SweepArgs {
  int K;
  const long long* indptr;
  const int *indices, *order;
  const float* sumF;
  const long long* soffset;  // support lists: offset, columns, values, count
  const int *sidx, *scount;
  const float* sval;
  const int *epre, *bound;   // per edge: staging prefix; per row: |S_u| bound
  const long long* goffset;  // gradient pools: offset, columns, values, count
  int *gidx, *gcount;
  float* gval;
  double* llh;
  const float *GG, *ladder;
  float* best;
  int n_ladder;
  float alpha, min_p, max_p, min_f, max_f;
};

// ------------------------------------------------------------ LDS layouts
// One layout per kernel, keyed on (bf16, K, slot cap).  The launcher takes
// `total` from it, the kernel its pointers.  Offsets are bytes from the
// start of dynamic LDS; they are exact whenever `total` fits a workgroup
// (the launchers refuse anything else), `total` is exact always.
// Arrays (S = slots, vs = 2 | 4 bytes per value):
//   bmap  u32  active-column bitmap          gacc  f32[S]  accumulator
//   sf    f32[S]  KFW/KFP: sumF at the slots; KFS: the finalized gradient
//   ebs   u32[ecap]  edge table (none in KFS)
//   nidx  u16[S]  staged columns, then slots   kS  u16[S]  sorted columns
//   nval  vs[S]   staged neighbour values      fu  vs[S]   own row values
//   pref  u16  per-bitmap-word exclusive prefix
struct SweepLds {
  int bmap, gacc, sf, ebs, nidx, kS, nval, fu, pref;  // byte offsets
  int nbm, npref, slots, vs, ecap;  // reserved elements (vs: bytes each)
  long long total;
};

// `len` bytes at the cursor; 64-bit so that `total` cannot wrap
SWEEP_HD constexpr int lds_take(long long& cur, long long len) {
  const long long at = cur;
  cur += len;
  return (int)at;
}

// The part KFW and KFP share, from `c` on: gacc | sf | ebs | (fp32: nval
// fu) | nidx | kS | pref | (bf16: nval fu).  Returns the end.
SWEEP_HD constexpr long long lds_wave_arrays(SweepLds& L, long long c) {
  const long long S = L.slots;
  L.gacc = lds_take(c, 4 * S);
  L.sf = lds_take(c, 4 * S);
  L.ebs = lds_take(c, 4LL * L.ecap);
  if (L.vs == 4) L.nval = lds_take(c, 4 * S), L.fu = lds_take(c, 4 * S);
  L.nidx = lds_take(c, 2 * S);
  L.kS = lds_take(c, 2 * S);
  L.pref = lds_take(c, 2LL * L.npref);
  if (L.vs == 2) L.nval = lds_take(c, 2 * S), L.fu = lds_take(c, 2 * S);
  return c;
}

// KFS (one block per node), cap slots:
//   bmap | gacc | sf (gS) | nidx | kS | nval | (pad to 4) fu | pref
// in nw*6 + cap*(16|20) bytes, and 16 bytes of slack.
SWEEP_HD constexpr SweepLds kfs_layout(bool bf16, int K, int cap) {
  const int nw = (K + 31) >> 5;
  SweepLds L{0, 0, 0, 0, 0, 0, 0, 0, 0, nw, nw, cap, bf16 ? 2 : 4, 0, 0};
  long long c = 0;
  L.bmap = lds_take(c, 4LL * nw);
  L.gacc = lds_take(c, 4LL * cap);
  L.sf = lds_take(c, 4LL * cap);
  L.nidx = lds_take(c, 2LL * cap);
  L.kS = lds_take(c, 2LL * cap);
  L.nval = lds_take(c, (long long)L.vs * cap);
  c = (c + 3) & ~3LL;
  L.fu = lds_take(c, (long long)L.vs * cap);
  L.pref = lds_take(c, 2LL * nw);
  L.total = 6LL * nw + (long long)cap * (bf16 ? 16 : 20) + 16;
  return L;
}

// KFW (one wave per node), wcap slots: bmap, then the wave arrays with a
// KFW_ECAP edge table and the prefix rounded to 2 entries.
SWEEP_HD constexpr SweepLds kfw_layout(bool bf16, int K, int wcap) {
  const int nw = (K + 31) >> 5;
  SweepLds L{0, 0, 0, 0, 0, 0, 0, 0, 0, nw, (nw + 1) & ~1, wcap,
             bf16 ? 2 : 4, KFW_ECAP, 0};
  L.total = lds_wave_arrays(L, 4LL * nw);
  return L;
}

// KFP (four nodes per wave), qcap slots rounded up to 4: the four bitmaps
// first (each rounded to 4 words, so together they clear as uint4), then
// per node the wave arrays with a KFP_DEG edge table, rounded to 16 bytes.
// `node` picks whose offsets the layout holds; `total` covers all four.
SWEEP_HD constexpr SweepLds kfp_layout(bool bf16, int K, int qcap,
                                       int node = 0) {
  const int nwp = (((K + 31) >> 5) + 3) & ~3;
  SweepLds L{0, 0, 0, 0, 0, 0, 0, 0, 0, nwp, nwp, (qcap + 3) & ~3,
             bf16 ? 2 : 4, KFP_DEG, 0};
  const long long region = (lds_wave_arrays(L, 0) + 15) & ~15LL;
  L.bmap = (int)(4LL * nwp * node);
  lds_wave_arrays(L, 4LL * nwp * KFP_NODES + region * node);
  L.total = KFP_NODES * (4LL * nwp + region);
  return L;
}

// Pinned at build time at K = 33, 5000, 25000, both value types, caps 4,
// 64, 256 and that K's default block cap: the total is the literal size
// formula the host clamps wcap / qcap against, every array is aligned to
// its element (KFP's uint4-cleared bitmaps to 16), none overlap or overrun.
namespace sweep_check {
struct Span {
  long long off, len;
  int align;
};
// the spans of n layouts (n = 4: KFP's nodes) against their common total
constexpr bool ok(const SweepLds* L, int n, int bmap_align, long long want) {
  Span s[9 * KFP_NODES] = {};
  for (int g = 0; g < n; ++g) {
    const SweepLds& l = L[g];
    const long long S = l.slots;
    const Span a[9] = {{l.bmap, 4LL * l.nbm, bmap_align}, {l.gacc, 4 * S, 4},
                       {l.sf, 4 * S, 4},   {l.ebs, 4LL * l.ecap, 4},
                       {l.nidx, 2 * S, 2}, {l.kS, 2 * S, 2},
                       {l.nval, l.vs * S, l.vs}, {l.fu, l.vs * S, l.vs},
                       {l.pref, 2LL * l.npref, 2}};
    for (int i = 0; i < 9; ++i) s[9 * g + i] = a[i];
    if (l.total != want) return false;
  }
  for (int i = 0; i < 9 * n; ++i) {
    if (s[i].off < 0 || s[i].off % s[i].align || s[i].off + s[i].len > want)
      return false;
    for (int j = 0; j < i; ++j)
      if (s[i].len > 0 && s[j].len > 0 && s[i].off < s[j].off + s[j].len &&
          s[j].off < s[i].off + s[i].len)
        return false;
  }
  return true;
}
constexpr bool at(bool bf, int K, int cap) {
  const long long nw = (K + 31) / 32, nwp = (nw + 3) & ~3LL;
  const long long per = bf ? 16 : 20, q4 = (cap + 3) & ~3;
  const SweepLds s = kfs_layout(bf, K, cap), w = kfw_layout(bf, K, cap);
  const SweepLds p[KFP_NODES] = {
      kfp_layout(bf, K, cap, 0), kfp_layout(bf, K, cap, 1),
      kfp_layout(bf, K, cap, 2), kfp_layout(bf, K, cap, 3)};
  return ok(&s, 1, 4, nw * 6 + cap * per + 16) &&
         ok(&w, 1, 4,
            nw * 4 + ((nw + 1) & ~1LL) * 2 + cap * per + KFW_ECAP * 4) &&
         ok(p, KFP_NODES, 16,
            KFP_NODES * (nwp * 4 +
                         ((q4 * per + KFP_DEG * 4 + nwp * 2 + 15) & ~15LL)));
}
constexpr bool at_K(int K, int cap_bf16, int cap_fp32) {
  const int caps[3] = {4, 64, 256};
  for (int cap : caps)
    if (!at(true, K, cap) || !at(false, K, cap)) return false;
  return at(true, K, cap_bf16) && at(false, K, cap_fp32);
}
static_assert(at_K(33, 8, 8) && at_K(5000, 1248, 1248) &&
                  at_K(25000, 1784, 1424),
              "sweep LDS layout: size formula, alignment or overlap");
}  // namespace sweep_check

// --------------------------------------------------- launchers and getters
// Defined in bigclam_kernels.hip; KFS / KFW / KFP: shared block + extras.
extern "C" {
// KAF: support lists of the rows of F (rows == nullptr: every row)
void launch_kaf(const void* F, int bf16, int n_rows, int K, int cap,
                const long long* soffset, int* scount, int* sidx,
                float* sval, int fill, const unsigned char* dirty,
                const int* rows, int n_list, hipStream_t stream);
// routing: bounds + classes, tile scan (+ GG), stable placement
int route_tile();
int kfp_deg();
void launch_route(const long long* indptr, const int* indices,
                  const int* scount, const int* order, int n_local, int cap,
                  int wcap, const float* sumF, int K, int* epre, int* bound,
                  unsigned char* cls, int* tcount, int* tbase, int* totals,
                  float* GG, int* by_class, int qcap, int* pscr, int* wsplit,
                  int* zscr, int zero, hipStream_t stream);
// LDS bytes of a KFW / KFP workgroup: the host clamps wcap / qcap with them
long long kfw_lds_bytes(int bf16, int K, int wcap);
long long kfp_lds_bytes(int bf16, int K, int qcap);
// KFS over order[0 .. n_blocks), one block per node
void launch_kfs(const SweepArgs& a, const void* F, int bf16, int n_blocks,
                int cap, hipStream_t stream);
// KFW over n_blocks positions: blk0 + i, or pos[blk0 + i] with pos given
void launch_kfw(const SweepArgs& a, int bf16, int blk0, const int* pos,
                int n_blocks, int wcap, int skip, hipStream_t stream);
// KFP over the pack positions pos[0 .. n_pack), four per workgroup
void launch_kfp(const SweepArgs& a, int bf16, const int* pos, int n_pack,
                int qcap, int skip, hipStream_t stream);
// kz_fill over the zero segment pos[0 .. n_zero): llh / best of the
// degree's representative (zrep_node[0 .. KFP_DEG]), gcount = 0
void launch_kz_fill(const SweepArgs& a, const int* pos, int n_zero,
                    const int* zrep_node, hipStream_t stream);
// commit of a routed order laid out [block | wave] (K3S / K3W)
int k3w_group();
void launch_k3s(void* F, int bf16, const int* order, int n_block,
                int n_total, const long long* goffset, const int* gidx,
                const float* gval, const int* gcount, const float* best,
                const long long* soffset, int* sidx, float* sval, int* scount,
                unsigned char* dirty, int cap, int K, float min_f,
                float max_f, hipStream_t stream);
// list-based column sums, and their fixed-order stage 2
void launch_kcs_lists(const void* F, int bf16, int n_local, int K,
                      const long long* soffset, const int* sidx,
                      const float* sval, const int* scount,
                      const unsigned char* dirty, int cap, float* partials,
                      hipStream_t stream);
void launch_kcs_stage2(const float* partials, int ns, int K, float* out,
                       hipStream_t stream);
}  // extern "C"
