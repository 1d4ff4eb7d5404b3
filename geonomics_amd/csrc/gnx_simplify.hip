// Which rows of the recorded pedigree the living still descend from (reference
// structs/species.py:1107-1142 _sort_and_simplify_table_collection, sim/model.py:756-768: there
// tskit's simplify, every tskit_simp_interval main steps).  A node v is ANCESTRAL at locus l if
// the lineage at l of some sample node passes through v; its ancestral mask is that set of loci,
// as W64 words in the layout of gnx_state::paths.  The masks follow from the children alone:
//
//   mask[2 prow + 1] |= mask[c] &  (paths[key(c)] ^ start(c))     (start broadcast over all bits)
//   mask[2 prow + 0] |= mask[c] & ~(paths[key(c)] ^ start(c))     for every node c with parent row prow
//
// and a parent is born in an earlier main step than its child, so one pass over the birth
// cohorts, youngest first, is exact.  The host turns the node table round (per parent row, the
// list of its child nodes) and a cohort is GATHERED: one launch per cohort, a thread owns one
// 16-byte chunk of one parent row's two masks, ORs its children's chunks in registers and writes
// both masks once with plain stores - no atomics on the masks, every mask written exactly once,
// nothing zeroed but the per-node `nonzero` bytes and the per-node locus counts.  Consecutive
// lanes hold consecutive chunks of one row, then the next row: a child's entry and its path are
// read by neighbouring lanes in whole lines.
//
//   gnx_pedigree_reach     per node the number of loci at which it is ancestral (0: the row can
//                          go if its other node has none either), and the masks of listed nodes
//   gnx_lineage_forget     drop the resident copy of the node table (the host renumbers it)
#include <algorithm>
#include <climits>
#include <vector>
#include "gnx_internal.h"

typedef unsigned long long u64;

// rows [r0, r0 + n_par) are one birth cohort; the masks hold the words [w0, w0 + 2 C) of every
// node, C chunks of 16 bytes.  child_off [n_rows + 1] / child [..]: per parent row its child nodes
__global__ void __launch_bounds__(256)
k_reach_cohort(int64_t r0, int64_t n_par, int C, int w0, int L, int W64,
               const int32_t* __restrict__ child_off, const int32_t* __restrict__ child,
               const int2* __restrict__ tab, const u64* __restrict__ paths,
               const uint8_t* __restrict__ is_sample, ulonglong2* __restrict__ mask,
               uint8_t* __restrict__ nonzero, int32_t* __restrict__ node_loci) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n_par * C) return;
  const int64_t row = r0 + gid / C;
  const int ch = (int)(gid % C);
  ulonglong2 a0{0ull, 0ull}, a1{0ull, 0ull};
  if (is_sample[row]) {                       // a sample node is ancestral at every locus
    const int64_t b = ((int64_t)w0 + 2 * ch) * 64;
    a0.x = b + 64 <= L ? ~0ull : (b < L ? (1ull << (L - b)) - 1ull : 0ull);
    a0.y = b + 128 <= L ? ~0ull : (b + 64 < L ? (1ull << (L - b - 64)) - 1ull : 0ull);
    a1 = a0;
  }
  const int32_t k1 = child_off[row + 1];
  for (int32_t k = child_off[row]; k < k1; ++k) {
    const int32_t c = child[k];
    if (!nonzero[c]) continue;
    const int32_t ks = tab[c].y;
    const ulonglong2 m = mask[(int64_t)c * C + ch];
    const ulonglong2 p =
        *reinterpret_cast<const ulonglong2*>(paths + (int64_t)(ks >> 1) * W64 + w0 + 2 * ch);
    const u64 s = (ks & 1) ? ~0ull : 0ull;
    const u64 x = p.x ^ s, y = p.y ^ s;
    a1.x |= m.x & x;
    a1.y |= m.y & y;
    a0.x |= m.x & ~x;
    a0.y |= m.y & ~y;
  }
  mask[(2 * row) * C + ch] = a0;
  mask[(2 * row + 1) * C + ch] = a1;
  const int n0 = __popcll(a0.x) + __popcll(a0.y), n1 = __popcll(a1.x) + __popcll(a1.y);
  if (n0) {
    nonzero[2 * row] = 1;
    atomicAdd(&node_loci[2 * row], n0);
  }
  if (n1) {
    nonzero[2 * row + 1] = 1;
    atomicAdd(&node_loci[2 * row + 1], n1);
  }
}

// out [n][C] chunks = the masks of the listed nodes
__global__ void __launch_bounds__(256)
k_reach_masks(int64_t n, int C, const int32_t* __restrict__ nodes,
              const ulonglong2* __restrict__ mask, ulonglong2* __restrict__ out) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n * C) return;
  out[gid] = mask[(int64_t)nodes[gid / C] * C + gid % C];
}

extern "C" int gnx_pedigree_reach(gnx_state* h, int64_t n_rows, const int32_t* node_tab,
                                  const int32_t* birth_t, int64_t n_samples,
                                  const int32_t* sample_rows, int32_t* node_loci, int64_t n_req,
                                  const int32_t* req_nodes, uint64_t* req_masks) {
  const char* who = "gnx_pedigree_reach";
  GNXCHK(lin_table(h, who, n_rows, node_tab, birth_t, 0));
  h->lin_ms = 0.0;
  h->lin_launches = 0;
  if (!node_loci) {
    gnx_set_error("%s: null output", who);
    return 1;
  }
  if (n_samples < 1 || !sample_rows) {
    gnx_set_error("%s: at least one sample row", who);
    return 1;
  }
  if (n_req < 0 || (n_req > 0 && (!req_nodes || !req_masks))) {
    gnx_set_error("%s: requested nodes and their masks go together", who);
    return 1;
  }
  // the cohorts are contiguous row ranges, youngest last; every parent is of an earlier one
  for (int64_t r = 1; r < n_rows; ++r)
    if (birth_t[r] > birth_t[r - 1]) {
      gnx_set_error("%s: birth_t must not ascend along the rows (row %lld)", who, (long long)r);
      return 1;
    }
  std::vector<int32_t> off((size_t)n_rows + 1, 0);
  int64_t n_child = 0;
  for (int64_t c = 0; c < 2 * n_rows; ++c) {
    const int32_t prow = node_tab[2 * c];
    if (prow == -1) continue;
    if (prow < 0 || prow >= (c >> 1) || birth_t[prow] <= birth_t[c >> 1]) {
      gnx_set_error("%s: node %lld: parent row %d is not of an earlier birth cohort", who,
                    (long long)c, prow);
      return 1;
    }
    off[(size_t)prow + 1] += 1;
    ++n_child;
  }
  std::vector<uint8_t> is_sample((size_t)n_rows, 0);
  for (int64_t i = 0; i < n_samples; ++i) {
    const int32_t r = sample_rows[i];
    if (r < 0 || r >= n_rows) {
      gnx_set_error("%s: sample row %d outside 0..%lld", who, r, (long long)(n_rows - 1));
      return 1;
    }
    if (is_sample[r]) {
      gnx_set_error("%s: sample row %d is listed twice", who, r);
      return 1;
    }
    is_sample[r] = 1;
  }
  for (int64_t i = 0; i < n_req; ++i)
    if (req_nodes[i] < 0 || req_nodes[i] >= 2 * n_rows) {
      gnx_set_error("%s: requested node %d outside 0..%lld", who, req_nodes[i],
                    (long long)(2 * n_rows - 1));
      return 1;
    }
  // counting sort: per parent row its child nodes, ascending
  for (int64_t r = 0; r < n_rows; ++r) off[(size_t)r + 1] += off[(size_t)r];
  std::vector<int32_t> child((size_t)std::max<int64_t>(n_child, 1));
  {
    std::vector<int32_t> at(off.begin(), off.end() - 1);
    for (int64_t c = 0; c < 2 * n_rows; ++c) {
      const int32_t prow = node_tab[2 * c];
      if (prow >= 0) child[(size_t)at[prow]++] = (int32_t)c;
    }
  }
  // the cohorts, as row ranges
  std::vector<int64_t> cohort{0};
  for (int64_t r = 1; r < n_rows; ++r)
    if (birth_t[r] != birth_t[r - 1]) cohort.push_back(r);
  cohort.push_back(n_rows);
  // words per column block: the masks of all nodes under the byte budget, whole 16-byte chunks
  const int W64 = h->W64, L = h->cfg.L;
  const int64_t budget = h->lin_budget > 0 ? h->lin_budget : LIN_BUDGET;
  int64_t Wb = budget / (2 * n_rows * 8) / 2 * 2;
  Wb = std::min<int64_t>(std::max<int64_t>(Wb, 2), W64);
  if (((n_rows + 255) / 256) * (Wb / 2) > INT_MAX) {
    gnx_set_error("%s: the table is too large for one launch; lower the byte budget", who);
    return 1;
  }
  GnxScratch s(who);
  int32_t *d_off = nullptr, *d_child = nullptr, *d_loci = nullptr, *d_req = nullptr;
  uint8_t *d_samp = nullptr, *d_nz = nullptr;
  u64 *d_mask = nullptr, *d_out = nullptr;
  GNXCHK(s.get(&d_off, (size_t)n_rows + 1));
  GNXCHK(s.get(&d_child, child.size()));
  GNXCHK(s.get(&d_loci, (size_t)2 * n_rows));
  GNXCHK(s.get(&d_samp, (size_t)n_rows));
  GNXCHK(s.get(&d_nz, (size_t)2 * n_rows));
  GNXCHK(s.get(&d_mask, (size_t)2 * n_rows * Wb));
  // requested masks leave in pieces under the budget as well
  const int64_t req_per = std::min<int64_t>(std::max<int64_t>(budget / (Wb * 8), 1), n_req);
  std::vector<u64> stage;
  if (n_req > 0) {
    GNXCHK(s.get(&d_req, (size_t)n_req));
    GNXCHK(s.get(&d_out, (size_t)req_per * Wb));
    GNXCHK(gnx_h2d(h, d_req, req_nodes, (size_t)n_req * 4));
    if (Wb < W64) stage.resize((size_t)req_per * Wb);
  }
  GNXCHK(gnx_h2d(h, d_off, off.data(), ((size_t)n_rows + 1) * 4));
  GNXCHK(gnx_h2d(h, d_child, child.data(), child.size() * 4));
  GNXCHK(gnx_h2d(h, d_samp, is_sample.data(), (size_t)n_rows));
  HIPCHK(hipMemsetAsync(d_loci, 0, (size_t)2 * n_rows * 4, h->stream));
  GnxCallTimer tm(h, &h->lin_ms, &h->lin_launches);
  for (int w0 = 0; w0 < W64; w0 += (int)Wb) {
    const int C = (int)std::min<int64_t>(Wb, W64 - w0) / 2;
    HIPCHK(hipMemsetAsync(d_nz, 0, (size_t)2 * n_rows, h->stream));
    tm.start();
    for (size_t k = cohort.size() - 1; k-- > 0;) {
      const int64_t r0 = cohort[k], n_par = cohort[k + 1] - r0;
      hipLaunchKernelGGL(k_reach_cohort, dim3((unsigned)((n_par * C + 255) / 256)), dim3(256), 0,
                         h->stream, r0, n_par, C, w0, L, W64, d_off, d_child,
                         (const int2*)h->lin_tab, (const u64*)h->paths, d_samp,
                         (ulonglong2*)d_mask, d_nz, d_loci);
    }
    HIPCHK(hipGetLastError());
    GNXCHK(tm.stop((int64_t)cohort.size() - 1));
    for (int64_t i0 = 0; i0 < n_req; i0 += req_per) {
      const int64_t n = std::min<int64_t>(req_per, n_req - i0);
      tm.start();
      hipLaunchKernelGGL(k_reach_masks, dim3((unsigned)((n * C + 255) / 256)), dim3(256), 0,
                         h->stream, n, C, d_req + i0, (const ulonglong2*)d_mask,
                         (ulonglong2*)d_out);
      HIPCHK(hipGetLastError());
      GNXCHK(tm.stop());
      if (2 * C == W64) {
        GNXCHK(gnx_d2h(h, req_masks + i0 * W64, d_out, (size_t)n * W64 * 8));
      } else {
        GNXCHK(gnx_d2h(h, stage.data(), d_out, (size_t)n * 2 * C * 8));
        for (int64_t i = 0; i < n; ++i)
          memcpy(req_masks + (i0 + i) * W64 + w0, stage.data() + i * 2 * C, (size_t)2 * C * 8);
      }
    }
  }
  GNXCHK(gnx_d2h(h, node_loci, d_loci, (size_t)2 * n_rows * 4));
  return 0;
}

extern "C" int gnx_lineage_forget(gnx_state* h) {
  (void)hipFree(h->lin_tab);
  (void)hipFree(h->lin_bt);
  h->lin_tab = h->lin_bt = nullptr;
  h->lin_rows = 0;
  h->lin_sum = 0;
  return 0;
}
