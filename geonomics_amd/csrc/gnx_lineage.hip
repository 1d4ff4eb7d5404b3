// Lineages through the recorded spatial pedigree (reference structs/genome.py:1638-1782,
// _get_lineage_dicts -> _get_lineage: tskit's tree.parent() followed recursively in Python, one
// node and one locus at a time).  The pedigree itself is recorded on the host
// (geonomics_amd/structs/pedigree.py); a lineage at a locus is a chain of look-ups
//
//   node 2 row + h  ->  {parent row, path key, start homologue}      (the node table)
//   parent homologue at locus l = start ^ bit l of path `key`        (gnx_state::paths)
//
// and both tables sit on the device here.  One thread walks one (sample node, locus) chain.
// Consecutive lanes of a wave hold consecutive requested loci of the SAME sample node:
// neighbouring loci share their lineage until a switch point separates them, so the lanes of a
// wave mostly read the same 8-byte node entry and the same path word, and a hop costs a few
// cache lines per wave, not 64.  The table is far smaller than L2 + Infinity Cache for every
// pedigree the host records, so the walk is bound by dependent-gather latency: what helps is
// waves in flight (small kernels, no LDS), not bytes.
//
//   gnx_lineage_trace    root / youngest kept / oldest kept / number kept per (locus, node),
//                        and per locus the min and max of the oldest kept node over the sample
//                        (all _check_coalescence needs: nothing n_loci x n_nodes comes back)
//   gnx_lineage_chains   the same walk writing every kept node at its CSR offset
#include <algorithm>
#include <climits>
#include <vector>
#include "gnx_internal.h"

typedef unsigned long long u64;

#define LIN_NPT 8                 // sample nodes per thread of the trace kernel
#define LIN_CHECK_ROWS 1024       // rows at the table's end that the reuse checksum covers

namespace {

struct LinWindow {
  int32_t t_curr, drop, min_ago, max_ago;
};

// walk the chain of `node` at `locus` back to its founder node; kept(node) for every node the
// reference keeps (genome.py:1747 and :1720-1729).  Ends because a parent's row is smaller
// than its child's (checked on the host before the table is uploaded).  -> the founder node
template <class F>
__device__ __forceinline__ int32_t lin_walk(const int2* __restrict__ tab,
                                            const int32_t* __restrict__ bt,
                                            const u64* __restrict__ paths, int W64, int32_t node,
                                            int32_t locus, LinWindow w, F kept) {
  const int lw = locus >> 6, lb = locus & 63;
  int32_t cur = node;
  for (;;) {
    const int32_t t = bt[cur >> 1];
    const int2 e = tab[cur];
    const int32_t ago = t + w.t_curr;
    if ((!w.drop || t < 0) && ago >= w.min_ago && ago <= w.max_ago) kept(cur);
    if (e.x < 0) return cur;
    const u64 pw = paths[(int64_t)(e.y >> 1) * W64 + lw];
    cur = 2 * e.x + ((e.y & 1) ^ (int)((pw >> lb) & 1ull));
  }
}

// lane -> (locus of the launch's list, group of sample nodes).  A wave holds TL = 2^tl_log2
// consecutive loci (64 unless the list is shorter) of 64 / TL groups; the waves that share a
// group are neighbours in the grid.
struct LinLane {
  int32_t q;       // locus index in the launch's list, < 0: none
  int64_t g;       // node group
  int sub;         // the lane's group inside its wave
};
__device__ __forceinline__ LinLane lin_lane(int n_q, int tl_log2, int n_ltiles) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(gid & 63);
  const int64_t wave = gid >> 6;
  const int TL = 1 << tl_log2;
  LinLane r;
  r.sub = lane >> tl_log2;
  const int q = (int)(wave % n_ltiles) * TL + (lane & (TL - 1));
  r.q = q < n_q ? q : -1;
  r.g = (wave / n_ltiles) * (64 >> tl_log2) + r.sub;
  return r;
}

}  // namespace

__global__ void k_lin_fill(int32_t n, int32_t* __restrict__ lo, int32_t* __restrict__ hi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    lo[i] = INT_MAX;
    hi[i] = INT_MIN;
  }
}

// outputs [n_q][n_nodes] of this launch's loci (each may be null); lo / hi [n_q]
__global__ void __launch_bounds__(256)
k_lin_trace(int64_t n_nodes, const int32_t* __restrict__ nodes, int n_q,
            const int32_t* __restrict__ loci, int tl_log2, int n_ltiles,
            const int2* __restrict__ tab, const int32_t* __restrict__ bt,
            const u64* __restrict__ paths, int W64, LinWindow w, int32_t* __restrict__ root,
            int32_t* __restrict__ first, int32_t* __restrict__ last, int32_t* __restrict__ n_kept,
            int32_t* __restrict__ lo, int32_t* __restrict__ hi) {
  const LinLane ln = lin_lane(n_q, tl_log2, n_ltiles);
  const int64_t i0 = ln.g * LIN_NPT;
  const int32_t locus = ln.q >= 0 ? loci[ln.q] : 0;
  int32_t r_root[LIN_NPT], r_first[LIN_NPT], r_last[LIN_NPT], r_n[LIN_NPT];
  int32_t mn = INT_MAX, mx = INT_MIN;
#pragma unroll
  for (int j = 0; j < LIN_NPT; ++j) {
    int32_t f = -1, l = -1, n = 0, r = -1;
    if (ln.q >= 0 && i0 + j < n_nodes) {
      r = lin_walk(tab, bt, paths, W64, nodes[i0 + j], locus, w, [&](int32_t c) {
        if (n == 0) f = c;
        l = c;
        ++n;
      });
      mn = min(mn, l);
      mx = max(mx, l);
    }
    r_root[j] = r;
    r_first[j] = f;
    r_last[j] = l;
    r_n[j] = n;
  }
  if (ln.q >= 0) {
    const int64_t o = (int64_t)ln.q * n_nodes + i0;
#pragma unroll
    for (int j = 0; j < LIN_NPT; ++j)
      if (i0 + j < n_nodes) {
        if (root) root[o + j] = r_root[j];
        if (first) first[o + j] = r_first[j];
        if (last) last[o + j] = r_last[j];
        if (n_kept) n_kept[o + j] = r_n[j];
      }
  }
  // per locus: the wave's lanes that hold it first, then one atomic per wave and locus
  if (lo) {
    for (int s = 1 << tl_log2; s < 64; s <<= 1) {
      mn = min(mn, __shfl_xor(mn, s));
      mx = max(mx, __shfl_xor(mx, s));
    }
    if (ln.q >= 0 && ln.sub == 0 && mx != INT_MIN) {
      atomicMin(&lo[ln.q], mn);
      atomicMax(&hi[ln.q], mx);
    }
  }
}

// every kept node of query (q, i) at chain[off[q * n_nodes + i] - off[0] ...]; a chain that is
// not as long as its offsets say raises *bad and never writes outside its own stretch
__global__ void __launch_bounds__(256)
k_lin_chains(int64_t n_nodes, const int32_t* __restrict__ nodes, int n_q,
             const int32_t* __restrict__ loci, int tl_log2, int n_ltiles,
             const int2* __restrict__ tab, const int32_t* __restrict__ bt,
             const u64* __restrict__ paths, int W64, LinWindow w,
             const int64_t* __restrict__ off, int32_t* __restrict__ chain,
             int32_t* __restrict__ bad) {
  const LinLane ln = lin_lane(n_q, tl_log2, n_ltiles);
  if (ln.q < 0 || ln.g >= n_nodes) return;
  const int64_t idx = (int64_t)ln.q * n_nodes + ln.g;
  const int64_t base = off[idx] - off[0], len = off[idx + 1] - off[idx];
  int64_t k = 0;
  lin_walk(tab, bt, paths, W64, nodes[ln.g], loci[ln.q], w, [&](int32_t c) {
    if (k < len) chain[base + k] = c;
    ++k;
  });
  if (k != len) atomicOr(bad, 1);
}

namespace {

uint64_t lin_checksum(int64_t n_rows, const int32_t* tab, const int32_t* bt, int n_paths) {
  const int64_t r0 = std::max<int64_t>(0, n_rows - LIN_CHECK_ROWS);
  uint64_t s = 1469598103934665603ull ^ (uint64_t)n_rows;
  auto mix = [&](uint32_t v) { s = (s ^ v) * 1099511628211ull; };
  mix((uint32_t)n_paths);
  for (int64_t r = r0; r < n_rows; ++r) {
    for (int c = 0; c < 4; ++c) mix((uint32_t)tab[4 * r + c]);
    mix((uint32_t)bt[r]);
  }
  return s;
}

}  // namespace

// the handle takes lineage requests; the node table is on the device (uploaded, or the copy of
// an earlier call when nothing was appended since) and every index in it is in range
int lin_table(gnx_state* h, const char* who, int64_t n_rows, const int32_t* tab,
              const int32_t* bt, int32_t t_curr) {
  if (h->cfg.L == 0 || !h->genomes_assigned) {
    gnx_set_error("%s: genomes not assigned", who);
    return 1;
  }
  if (h->n_ghost > 0) {
    gnx_set_error("%s: the handle holds ghost records (a tile): not supported", who);
    return 1;
  }
  if (h->n_paths == 0 || !h->paths) {
    gnx_set_error("%s: no recombination paths (gnx_set_recomb_paths)", who);
    return 1;
  }
  if (n_rows < 1 || n_rows > (1ll << 30) - 1 || !tab || !bt) {
    gnx_set_error("%s: a node table of 1..2^30 - 1 rows", who);
    return 1;
  }
  if (t_curr <= -(1 << 30) || t_curr >= (1 << 30)) {
    gnx_set_error("%s: t_curr out of range", who);
    return 1;
  }
  h->lin_uploaded = 0;
  const uint64_t sum = lin_checksum(n_rows, tab, bt, h->n_paths);
  if (h->lin_tab && h->lin_rows == n_rows && h->lin_sum == sum) return 0;
  for (int64_t r = 0; r < n_rows; ++r) {
    if (bt[r] <= -(1 << 30) || bt[r] >= (1 << 30)) {
      gnx_set_error("%s: birth time of row %lld out of range", who, (long long)r);
      return 1;
    }
    for (int hh = 0; hh < 2; ++hh) {
      const int32_t prow = tab[4 * r + 2 * hh], ks = tab[4 * r + 2 * hh + 1];
      if (prow == -1) continue;                                  // a founder node
      if (prow < 0 || prow >= r) {
        gnx_set_error("%s: node %lld: parent row %d is not an earlier row", who,
                      (long long)(2 * r + hh), prow);
        return 1;
      }
      if (ks < 0 || (ks >> 1) >= h->n_paths) {
        gnx_set_error("%s: node %lld: path key %d outside 0..%d", who, (long long)(2 * r + hh),
                      ks >> 1, h->n_paths - 1);
        return 1;
      }
    }
  }
  (void)hipFree(h->lin_tab);
  (void)hipFree(h->lin_bt);
  h->lin_tab = h->lin_bt = nullptr;
  h->lin_rows = 0;
  if (hipMalloc((void**)&h->lin_tab, (size_t)n_rows * 16) != hipSuccess ||
      hipMalloc((void**)&h->lin_bt, (size_t)n_rows * 4) != hipSuccess) {
    (void)hipFree(h->lin_tab);
    h->lin_tab = nullptr;
    gnx_set_error("%s: out of device memory for the node table (%lld rows)", who,
                  (long long)n_rows);
    return 1;
  }
  GNXCHK(gnx_h2d(h, h->lin_tab, tab, (size_t)n_rows * 16));
  GNXCHK(gnx_h2d(h, h->lin_bt, bt, (size_t)n_rows * 4));
  h->lin_rows = n_rows;
  h->lin_sum = sum;
  h->lin_uploaded = 1;
  return 0;
}

// the sample nodes and the loci, checked and uploaded
int lin_request(gnx_state* h, const char* who, int64_t n_rows, int64_t n_nodes,
                const int32_t* nodes, int32_t n_loci, const int32_t* loci, GnxScratch& s,
                int32_t** d_nodes, int32_t** d_loci) {
  if (n_nodes < 1 || n_loci < 1 || !nodes || !loci) {
    gnx_set_error("%s: at least one sample node and one locus", who);
    return 1;
  }
  for (int64_t i = 0; i < n_nodes; ++i)
    if (nodes[i] < 0 || nodes[i] >= 2 * n_rows) {
      gnx_set_error("%s: sample node %d outside 0..%lld", who, nodes[i],
                    (long long)(2 * n_rows - 1));
      return 1;
    }
  for (int q = 0; q < n_loci; ++q)
    if (loci[q] < 0 || loci[q] >= h->cfg.L) {
      gnx_set_error("%s: locus %d outside 0..%d", who, loci[q], h->cfg.L - 1);
      return 1;
    }
  GNXCHK(s.get(d_nodes, (size_t)n_nodes));
  GNXCHK(s.get(d_loci, (size_t)n_loci));
  GNXCHK(gnx_h2d(h, *d_nodes, nodes, (size_t)n_nodes * sizeof(int32_t)));
  GNXCHK(gnx_h2d(h, *d_loci, loci, (size_t)n_loci * sizeof(int32_t)));
  return 0;
}

namespace {

// the lane layout of a launch over n_q loci and n_groups node groups
struct LinGrid {
  int tl_log2, n_ltiles;
  unsigned blocks;
};
int lin_grid(const char* who, int n_q, int64_t n_groups, LinGrid* g) {
  g->tl_log2 = 0;
  while ((1 << g->tl_log2) < std::min(n_q, 64)) ++g->tl_log2;
  const int TL = 1 << g->tl_log2;
  g->n_ltiles = (n_q + TL - 1) / TL;
  const int per_wave = 64 / TL;
  const int64_t waves = (n_groups + per_wave - 1) / per_wave * g->n_ltiles;
  const int64_t blocks = (waves + 3) / 4;
  if (blocks > INT_MAX) {
    gnx_set_error("%s: the request is too large for one launch; lower the byte budget", who);
    return 1;
  }
  g->blocks = (unsigned)blocks;
  return 0;
}

}  // namespace

extern "C" int gnx_lineage_budget(gnx_state* h, int64_t bytes) {
  if (bytes < 0) {
    gnx_set_error("gnx_lineage_budget: bytes >= 0 (0: the default)");
    return 1;
  }
  h->lin_budget = bytes;
  return 0;
}

extern "C" int gnx_lineage_info(gnx_state* h, double* kernel_ms, int64_t* launches,
                                int64_t* uploaded) {
  if (kernel_ms) *kernel_ms = h->lin_ms;
  if (launches) *launches = h->lin_launches;
  if (uploaded) *uploaded = h->lin_uploaded;
  return 0;
}

extern "C" int gnx_lineage_trace(gnx_state* h, int64_t n_rows, const int32_t* node_tab,
                                 const int32_t* birth_t, int64_t n_nodes, const int32_t* nodes,
                                 int32_t n_loci, const int32_t* loci, int32_t t_curr,
                                 int32_t drop_before_sim, int32_t min_ago, int32_t max_ago,
                                 int32_t* root, int32_t* first, int32_t* last, int32_t* n_kept,
                                 int32_t* locus_lo, int32_t* locus_hi) {
  const char* who = "gnx_lineage_trace";
  if ((locus_lo == nullptr) != (locus_hi == nullptr)) {
    gnx_set_error("%s: locus_lo and locus_hi go together", who);
    return 1;
  }
  GNXCHK(lin_table(h, who, n_rows, node_tab, birth_t, t_curr));
  GnxScratch s(who);
  int32_t *d_nodes = nullptr, *d_loci = nullptr;
  GNXCHK(lin_request(h, who, n_rows, n_nodes, nodes, n_loci, loci, s, &d_nodes, &d_loci));
  int32_t* host[4] = {root, first, last, n_kept};
  int n_out = 0;
  for (int32_t* p : host) n_out += p != nullptr;
  // loci per launch: its outputs stay under the byte budget
  const int64_t budget = h->lin_budget > 0 ? h->lin_budget : LIN_BUDGET;
  int64_t per = n_loci;
  if (n_out > 0) per = std::max<int64_t>(1, budget / (n_out * 4 * n_nodes));
  per = std::min<int64_t>(per, n_loci);
  int32_t* dev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < 4; ++k)
    if (host[k]) GNXCHK(s.get(&dev[k], (size_t)per * n_nodes));
  int32_t *d_lo = nullptr, *d_hi = nullptr;
  if (locus_lo) {
    GNXCHK(s.get(&d_lo, (size_t)n_loci));
    GNXCHK(s.get(&d_hi, (size_t)n_loci));
    hipLaunchKernelGGL(k_lin_fill, dim3(gnx_grid(n_loci, 256)), dim3(256), 0, h->stream, n_loci,
                       d_lo, d_hi);
  }
  const LinWindow w{t_curr, drop_before_sim != 0, min_ago, max_ago};
  const int64_t n_groups = (n_nodes + LIN_NPT - 1) / LIN_NPT;
  h->lin_ms = 0.0;
  h->lin_launches = 0;
  GnxCallTimer tm(h, &h->lin_ms, &h->lin_launches);
  for (int64_t q0 = 0; q0 < n_loci; q0 += per) {
    const int n_q = (int)std::min<int64_t>(per, n_loci - q0);
    LinGrid g;
    GNXCHK(lin_grid(who, n_q, n_groups, &g));
    tm.start();
    hipLaunchKernelGGL(k_lin_trace, dim3(g.blocks), dim3(256), 0, h->stream, n_nodes, d_nodes,
                       n_q, d_loci + q0, g.tl_log2, g.n_ltiles, (const int2*)h->lin_tab,
                       h->lin_bt, (const u64*)h->paths, h->W64, w, dev[0], dev[1], dev[2], dev[3],
                       d_lo ? d_lo + q0 : nullptr, d_hi ? d_hi + q0 : nullptr);
    HIPCHK(hipGetLastError());
    GNXCHK(tm.stop());
    for (int k = 0; k < 4; ++k)
      if (host[k])
        GNXCHK(gnx_d2h(h, host[k] + q0 * n_nodes, dev[k], (size_t)n_q * n_nodes * 4));
  }
  if (locus_lo) {
    GNXCHK(gnx_d2h(h, locus_lo, d_lo, (size_t)n_loci * 4));
    GNXCHK(gnx_d2h(h, locus_hi, d_hi, (size_t)n_loci * 4));
  }
  return 0;
}

extern "C" int gnx_lineage_chains(gnx_state* h, int64_t n_rows, const int32_t* node_tab,
                                  const int32_t* birth_t, int64_t n_nodes, const int32_t* nodes,
                                  int32_t n_loci, const int32_t* loci, int32_t t_curr,
                                  int32_t drop_before_sim, int32_t min_ago, int32_t max_ago,
                                  const int64_t* offsets, int32_t* chain_nodes) {
  const char* who = "gnx_lineage_chains";
  GNXCHK(lin_table(h, who, n_rows, node_tab, birth_t, t_curr));
  GnxScratch s(who);
  int32_t *d_nodes = nullptr, *d_loci = nullptr;
  GNXCHK(lin_request(h, who, n_rows, n_nodes, nodes, n_loci, loci, s, &d_nodes, &d_loci));
  const int64_t nq = (int64_t)n_loci * n_nodes;
  if (!offsets || offsets[0] != 0) {
    gnx_set_error("%s: offsets start at 0", who);
    return 1;
  }
  for (int64_t i = 0; i < nq; ++i)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > n_rows) {
      gnx_set_error("%s: offsets must ascend by at most n_rows per chain", who);
      return 1;
    }
  if (offsets[nq] > 0 && !chain_nodes) {
    gnx_set_error("%s: null output", who);
    return 1;
  }
  const LinWindow w{t_curr, drop_before_sim != 0, min_ago, max_ago};
  const int64_t budget = h->lin_budget > 0 ? h->lin_budget : LIN_BUDGET;
  int32_t* d_bad = nullptr;
  GNXCHK(s.get(&d_bad, 1));
  HIPCHK(hipMemsetAsync(d_bad, 0, 4, h->stream));
  h->lin_ms = 0.0;
  h->lin_launches = 0;
  GnxCallTimer tm(h, &h->lin_ms, &h->lin_launches);
  for (int64_t q0 = 0; q0 < n_loci;) {
    // loci of this launch: chain entries (4 bytes) and offsets (8 bytes) under the budget
    int64_t q1 = q0 + 1;
    while (q1 < n_loci && (offsets[(q1 + 1) * n_nodes] - offsets[q0 * n_nodes]) * 4 +
                                  ((q1 + 1 - q0) * n_nodes + 1) * 8 <= budget)
      ++q1;
    const int n_q = (int)(q1 - q0);
    const int64_t n_ent = offsets[q1 * n_nodes] - offsets[q0 * n_nodes];
    GnxScratch cs(who);
    int64_t* d_off = nullptr;
    int32_t* d_chain = nullptr;
    GNXCHK(cs.get(&d_off, (size_t)n_q * n_nodes + 1));
    GNXCHK(cs.get(&d_chain, (size_t)n_ent));
    GNXCHK(gnx_h2d(h, d_off, offsets + q0 * n_nodes, ((size_t)n_q * n_nodes + 1) * 8));
    LinGrid g;
    GNXCHK(lin_grid(who, n_q, n_nodes, &g));
    tm.start();
    hipLaunchKernelGGL(k_lin_chains, dim3(g.blocks), dim3(256), 0, h->stream, n_nodes, d_nodes,
                       n_q, d_loci + q0, g.tl_log2, g.n_ltiles, (const int2*)h->lin_tab,
                       h->lin_bt, (const u64*)h->paths, h->W64, w, d_off, d_chain, d_bad);
    HIPCHK(hipGetLastError());
    GNXCHK(tm.stop());
    GNXCHK(gnx_d2h(h, chain_nodes + offsets[q0 * n_nodes], d_chain, (size_t)n_ent * 4));
    q0 = q1;
  }
  int32_t bad = 0;
  GNXCHK(gnx_d2h(h, &bad, d_bad, 4));
  if (bad) {
    gnx_set_error("%s: the offsets are not the scan of this request's n_kept", who);
    return 1;
  }
  return 0;
}
