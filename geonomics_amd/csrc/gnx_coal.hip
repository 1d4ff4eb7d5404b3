// Pairwise coalescence through the recorded pedigree (the reference has no such analysis; what
// tskit's divergence(mode='branch'), pair_coalescence_counts and ibd_segments answer): for every
// (pair of sample nodes a != b, listed locus l) the most recent common ancestor in the local
// tree, as include/gnx_hip.h defines it, through the tables of gnx_lineage.hip
//
//   node 2 row + h  ->  {parent row, path key, start homologue}      (the node table)
//   parent homologue at locus l = start ^ bit l of path `key`        (gnx_state::paths)
//
// The heart is a merge walk: hold hi > lo (the two lineages' current nodes); replace hi by its
// parent node at l until hi == lo (the MRCA) or hi is a founder node (none).  Node ids descend
// along a chain, so the first node the two chains share is their largest common node; nothing
// is stored, and the walk is at most len(chain a) + len(chain b) dependent look-ups.  The lanes
// of a wave hold 64 consecutive listed loci of the SAME pair (k_lin_trace's argument: neighbouring
// loci share both lineages until a switch point separates them, so a hop costs a few cache
// lines per wave and the lanes rarely diverge).  The walk is bound by dependent-gather latency:
// small kernels, no LDS in the walk, many waves in flight.
//
//   gnx_coal_times      sum / count of T per pair and per locus, the largest T per locus, a
//                       histogram of T, and on request the MRCA of every (locus, pair)
//   gnx_coal_segments   the stretches of listed loci over which a pair keeps one MRCA (IBD
//                       segments): count, length, longest per pair, histogram, cover
//
// Every output is an integer function of the MRCAs: integer atomics only, exact in any order.
#include <algorithm>
#include <climits>
#include <vector>
#include "gnx_internal.h"

typedef unsigned long long u64;

#define COAL_MAX_NODES 4096
#define COAL_NB 64                // bins at most (both histograms)

namespace {

struct CoalAge {
  int32_t t_curr;
  int32_t max_ago;                // INT_MAX: no limit
  int32_t stop_early;             // birth_t does not ascend along the rows and there is a limit
};

// the MRCA of sample nodes a != b at `locus` where the pair coalesces, else -1 (no common node,
// or the MRCA is older than max_ago).  With stop_early a smaller node id is never younger, so
// once hi is too old the MRCA (<= lo < hi) is too old as well
__device__ __forceinline__ int32_t coal_walk(const int2* __restrict__ tab,
                                             const int32_t* __restrict__ bt,
                                             const u64* __restrict__ paths, int W64, int32_t a,
                                             int32_t b, int32_t locus, CoalAge w) {
  const int lw = locus >> 6, lb = locus & 63;
  int32_t hi = max(a, b), lo = min(a, b);
  while (hi != lo) {
    if (w.stop_early && bt[hi >> 1] + w.t_curr > w.max_ago) return -1;
    const int2 e = tab[hi];
    if (e.x < 0) return -1;
    const u64 pw = paths[(int64_t)(e.y >> 1) * W64 + lw];
    const int32_t p = 2 * e.x + ((e.y & 1) ^ (int)((pw >> lb) & 1ull));
    hi = max(p, lo);
    lo = min(p, lo);
  }
  if (bt[hi >> 1] + w.t_curr > w.max_ago) return -1;
  return hi;
}

// pair p of the row-major upper triangle of n nodes -> (i, j), i < j; p < n (n - 1) / 2
__device__ __forceinline__ int64_t coal_row_start(int64_t i, int64_t n) {
  return i * (2 * n - i - 1) / 2;
}
__device__ __forceinline__ void coal_pair(int64_t p, int n, int* i, int* j) {
  int a = 0, b = n - 2;                                // the largest row whose start is <= p
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (coal_row_start(mid, n) <= p) a = mid;
    else b = mid - 1;
  }
  *i = a;
  *j = a + 1 + (int)(p - coal_row_start(a, n));
}

__device__ __forceinline__ long long coal_wave_sum(long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ long long coal_wave_max(long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}

// the bin of v among edges E[0..nb] (strictly ascending), or -1
template <class T>
__device__ __forceinline__ int coal_bin(const T* E, int nb, T v) {
  if (v < E[0] || !(v < E[nb])) return -1;
  int lo = 0, hi = nb;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (v >= E[mid]) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace

// A wave keeps one tile of 64 listed loci (of this launch's n_q) and loops over a chunk of
// `per_wave` pairs: the per-locus sums stay in registers and leave with one atomic per lane at
// the end; a pair's sum over the tile is reduced in the wave and leaves with one atomic.
// pair_sum / pair_cnt [n][n] (upper triangle), locus_* [n_q], thist [nb], mrca [n_q][n_pairs]:
// each may be null (locus_sum, locus_cnt and locus_max together).  locus_max starts at INT_MIN
__global__ void __launch_bounds__(256)
k_coal_times(int n, const int32_t* __restrict__ nodes, int64_t n_pairs, int per_wave, int n_q,
             const int32_t* __restrict__ loci, int n_ltiles, const int2* __restrict__ tab,
             const int32_t* __restrict__ bt, const u64* __restrict__ paths, int W64, CoalAge w,
             int nb, const int32_t* __restrict__ tedges, u64* __restrict__ pair_sum,
             int32_t* __restrict__ pair_cnt, u64* __restrict__ locus_sum,
             u64* __restrict__ locus_cnt, int32_t* __restrict__ locus_max,
             u64* __restrict__ thist, int32_t* __restrict__ mrca) {
  __shared__ int32_t E[COAL_NB + 1];
  __shared__ u64 Hs[COAL_NB];
  const int tid = threadIdx.x, lane = tid & 63;
  if (nb > 0 && tid <= nb) E[tid] = tedges[tid];
  if (tid < COAL_NB) Hs[tid] = 0ull;
  __syncthreads();
  const int64_t wave = (int64_t)blockIdx.x * 4 + (tid >> 6);
  const int64_t chunk = wave / n_ltiles;
  const int q = (int)(wave % n_ltiles) * 64 + lane;
  const int64_t p0 = chunk * per_wave;
  if (p0 < n_pairs) {                                   // wave-uniform
    const int64_t p1 = min(n_pairs, p0 + per_wave);
    const bool live = q < n_q;
    const int32_t locus = live ? loci[q] : 0;
    int i, j;
    coal_pair(p0, n, &i, &j);
    long long l_sum = 0, l_cnt = 0;
    int32_t l_max = INT_MIN;
    for (int64_t p = p0; p < p1; ++p) {
      int32_t m = -1, T = 0;
      if (live) {
        m = coal_walk(tab, bt, paths, W64, nodes[i], nodes[j], locus, w);
        if (m >= 0) T = bt[m >> 1] + w.t_curr;
      }
      const bool hit = m >= 0;
      if (mrca && live) mrca[(int64_t)q * n_pairs + p] = m;
      if (hit) {
        l_sum += T;
        l_cnt += 1;
        l_max = max(l_max, T);
        if (nb > 0) {
          const int k = coal_bin(E, nb, T);
          if (k >= 0) atomicAdd(&Hs[k], 1ull);
        }
      }
      if (pair_sum) {
        const long long s = coal_wave_sum(hit ? (long long)T : 0ll);
        const int c = __popcll(__ballot(hit));
        if (lane == 0 && c) {
          atomicAdd(&pair_sum[(int64_t)i * n + j], (u64)s);
          atomicAdd(&pair_cnt[(int64_t)i * n + j], c);
        }
      }
      if (++j == n) {
        ++i;
        j = i + 1;
      }
    }
    if (locus_sum && l_cnt) {
      atomicAdd(&locus_sum[q], (u64)l_sum);
      atomicAdd(&locus_cnt[q], (u64)l_cnt);
      atomicMax(&locus_max[q], l_max);
    }
  }
  __syncthreads();
  if (tid < nb && Hs[tid]) atomicAdd(&thist[tid], Hs[tid]);
}

__global__ void k_coal_fill(int32_t n, int32_t v, int32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}

// the lower triangle of [n][n] matrices from the upper (each may be null)
__global__ void k_coal_mirror(int64_t n, int32_t* __restrict__ c32, u64* __restrict__ a64,
                              u64* __restrict__ b64) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * n; t += stride) {
    const int64_t i = t / n, j = t - i * n;
    if (i > j) {
      const int64_t u = j * n + i;
      if (c32) c32[t] = c32[u];
      if (a64) a64[t] = a64[u];
      if (b64) b64[t] = b64[u];
    }
  }
}

// A wave carries one pair through the tiles of the locus list in order.  Lane `lane` of tile t
// holds list position q = 64 t + lane and its MRCA m (-1: the pair does not coalesce there, or
// q is past the list).  A segment continues into q iff m >= 0, m equals the MRCA at q - 1 and
// brk[q] is not set; the MRCA at q - 1 is the neighbouring lane's, for lane 0 the last lane of
// the tile before (wave-uniform, like the start of the segment that is open there).  A segment
// is counted by the lane after its last position, which sees that it does not continue; one
// tile past the list's end closes what is still open.  cnt / len / longest [n][n]: both
// triangles are written here; hist [nb][2] and cdiff [n_loci + 1] add up over the launch
__global__ void __launch_bounds__(256)
k_coal_segments(int n, const int32_t* __restrict__ nodes, int64_t n_pairs, int n_loci,
                const int32_t* __restrict__ loci, const long long* __restrict__ pos,
                const uint8_t* __restrict__ brk, const int2* __restrict__ tab,
                const int32_t* __restrict__ bt, const u64* __restrict__ paths, int W64,
                CoalAge w, int min_loci, long long min_len, int nb,
                const long long* __restrict__ edges, int32_t* __restrict__ cnt,
                long long* __restrict__ len, long long* __restrict__ longest,
                u64* __restrict__ hist, int* __restrict__ cdiff) {
  __shared__ long long E[COAL_NB + 1];
  __shared__ u64 Hs[COAL_NB * 2];
  const int tid = threadIdx.x, lane = tid & 63;
  if (nb > 0 && tid <= nb) E[tid] = edges[tid];
  if (tid < 2 * COAL_NB) Hs[tid] = 0ull;
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * 4 + (tid >> 6);
  if (p < n_pairs) {                                    // wave-uniform
    int i, j;
    coal_pair(p, n, &i, &j);
    const int32_t a = nodes[i], b = nodes[j];
    long long a_cnt = 0, a_len = 0, a_longest = 0;
    int32_t carry_m = -1;
    int carry_s = 0;
    const int n_tiles = n_loci / 64 + 1;                // position n_loci at least: it closes
    for (int t = 0; t < n_tiles; ++t) {
      const int base = t * 64, q = base + lane;
      int32_t m = -1;
      if (q < n_loci) m = coal_walk(tab, bt, paths, W64, a, b, loci[q], w);
      int32_t prev = __shfl_up(m, 1, 64);
      if (lane == 0) prev = carry_m;
      const bool cut = brk && q > 0 && q < n_loci && brk[q];
      const bool cont = m >= 0 && prev == m && !cut;
      const u64 S = __ballot(m >= 0 && !cont);          // the positions where a segment starts
      if (prev >= 0 && !cont) {                         // the segment that ends at q - 1
        const u64 below = S & ((1ull << lane) - 1ull);
        const int s = below ? base + 63 - __clzll((long long)below) : carry_s;
        const int e = q - 1;
        const int c = e - s + 1;
        const long long ln = pos[e] - pos[s];
        if (c >= min_loci && ln >= min_len) {
          a_cnt += 1;
          a_len += ln;
          a_longest = max(a_longest, ln);
          if (nb > 0) {
            const int k = coal_bin(E, nb, ln);
            if (k >= 0) {
              atomicAdd(&Hs[2 * k], 1ull);
              atomicAdd(&Hs[2 * k + 1], (u64)ln);
            }
          }
          if (cdiff) {
            atomicAdd(&cdiff[s], 1);
            atomicAdd(&cdiff[e + 1], -1);
          }
        }
      }
      carry_m = __shfl(m, 63, 64);
      if (S) carry_s = base + 63 - __clzll((long long)S);
    }
    const long long c = coal_wave_sum(a_cnt), l = coal_wave_sum(a_len);
    const long long g = coal_wave_max(a_longest);
    if (lane == 0) {
      const int64_t u = (int64_t)i * n + j, v = (int64_t)j * n + i;
      if (cnt) cnt[u] = cnt[v] = (int32_t)c;
      if (len) len[u] = len[v] = l;
      if (longest) longest[u] = longest[v] = g;
    }
  }
  __syncthreads();
  if (tid < 2 * nb && Hs[tid]) atomicAdd(&hist[tid], Hs[tid]);
}

// cover[q] = cdiff[0] + .. + cdiff[q], q < n (one workgroup: a chunk of positions per thread)
__global__ void __launch_bounds__(1024)
k_coal_cover(int n, const int* __restrict__ cdiff, long long* __restrict__ cover) {
  __shared__ long long part[1024];
  const int tid = threadIdx.x;
  const int chunk = (n + 1023) / 1024;
  const int64_t a = (int64_t)tid * chunk, b = min((int64_t)n, a + chunk);
  long long s = 0;
  for (int64_t l = a; l < b; ++l) s += cdiff[l];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int k = 0; k < 1024; ++k) {
      const long long v = part[k];
      part[k] = run;
      run += v;
    }
  }
  __syncthreads();
  s = part[tid];
  for (int64_t l = a; l < b; ++l) {
    s += cdiff[l];
    cover[l] = s;
  }
}

namespace {

// what both entry points refuse beside lin_table's and lin_request's refusals; -> the age window
int coal_check(const char* who, int64_t n_rows, const int32_t* birth_t, int64_t n_nodes,
               const int32_t* nodes, int32_t n_loci, int32_t t_curr, int32_t max_ago,
               int64_t* work, CoalAge* w) {
  if (n_nodes < 2 || n_nodes > COAL_MAX_NODES || !nodes) {
    gnx_set_error("%s: 2..%d sample nodes per call (got %lld)", who, COAL_MAX_NODES,
                  (long long)n_nodes);
    return 1;
  }
  std::vector<int32_t> sorted(nodes, nodes + n_nodes);
  std::sort(sorted.begin(), sorted.end());
  for (int64_t i = 1; i < n_nodes; ++i)
    if (sorted[(size_t)i] == sorted[(size_t)i - 1]) {
      gnx_set_error("%s: sample node %d is listed twice", who, sorted[(size_t)i]);
      return 1;
    }
  if (n_loci < 1) {
    gnx_set_error("%s: at least one sample node and one locus", who);
    return 1;
  }
  if (!work) {
    gnx_set_error("%s: null work", who);
    return 1;
  }
  w->t_curr = t_curr;
  w->max_ago = max_ago < 0 ? INT_MAX : max_ago;
  w->stop_early = max_ago >= 0;
  for (int64_t r = 1; r < n_rows && w->stop_early; ++r)
    if (birth_t[r] > birth_t[r - 1]) w->stop_early = 0;
  return 0;
}

int coal_work(const char* who, int64_t n_nodes, int32_t n_loci, int64_t max_work,
              int64_t* work) {
  const int64_t n_pairs = n_nodes * (n_nodes - 1) / 2;
  *work = n_pairs * n_loci;
  if (max_work > 0 && *work > max_work) {
    gnx_set_error("%s: %lld pairs of sample nodes x %d loci = %lld look-up chains of work exceed "
                  "max_work = %lld", who, (long long)n_pairs, n_loci, (long long)*work,
                  (long long)max_work);
    return 1;
  }
  return 0;
}

}  // namespace

extern "C" int gnx_coal_times(gnx_state* h, int64_t n_rows, const int32_t* node_tab,
                              const int32_t* birth_t, int64_t n_nodes, const int32_t* nodes,
                              int32_t n_loci, const int32_t* loci, int32_t t_curr,
                              int32_t max_ago, int32_t n_tedges, const int32_t* tedges,
                              int64_t max_work, int64_t* work, int64_t* pair_sum,
                              int32_t* pair_cnt, int64_t* locus_sum, int64_t* locus_cnt,
                              int32_t* locus_max, int64_t* thist, int32_t* mrca) {
  const char* who = "gnx_coal_times";
  GNXCHK(lin_table(h, who, n_rows, node_tab, birth_t, t_curr));
  h->lin_ms = 0.0;
  h->lin_launches = 0;
  CoalAge w;
  GNXCHK(coal_check(who, n_rows, birth_t, n_nodes, nodes, n_loci, t_curr, max_ago, work, &w));
  if (thist || n_tedges != 0 || tedges) {
    if (n_tedges < 2 || n_tedges > COAL_NB + 1 || !tedges || !thist) {
      gnx_set_error("%s: 2..%d time edges with thist, or neither (got %d)", who, COAL_NB + 1,
                    n_tedges);
      return 1;
    }
    for (int k = 1; k < n_tedges; ++k)
      if (!(tedges[k] > tedges[k - 1])) {
        gnx_set_error("%s: time edges must be strictly ascending (tedges[%d] = %d)", who, k,
                      tedges[k]);
        return 1;
      }
  }
  GnxScratch s(who);
  int32_t *d_nodes = nullptr, *d_loci = nullptr;
  GNXCHK(lin_request(h, who, n_rows, n_nodes, nodes, n_loci, loci, s, &d_nodes, &d_loci));
  GNXCHK(coal_work(who, n_nodes, n_loci, max_work, work));
  if (max_work <= 0) return 0;
  const int n = (int)n_nodes;
  const int64_t n_pairs = n_nodes * (n_nodes - 1) / 2;
  const bool want_pair = pair_sum || pair_cnt;
  const bool want_locus = locus_sum || locus_cnt || locus_max;
  const int nb = thist ? n_tedges - 1 : 0;
  u64 *d_psum = nullptr, *d_lsum = nullptr, *d_lcnt = nullptr, *d_hist = nullptr;
  int32_t *d_pcnt = nullptr, *d_lmax = nullptr, *d_edges = nullptr, *d_mrca = nullptr;
  if (want_pair) {
    GNXCHK(s.get(&d_psum, (size_t)n * n));
    GNXCHK(s.get(&d_pcnt, (size_t)n * n));
    HIPCHK(hipMemsetAsync(d_psum, 0, (size_t)n * n * sizeof(u64), h->stream));
    HIPCHK(hipMemsetAsync(d_pcnt, 0, (size_t)n * n * sizeof(int32_t), h->stream));
  }
  if (want_locus) {
    GNXCHK(s.get(&d_lsum, (size_t)n_loci));
    GNXCHK(s.get(&d_lcnt, (size_t)n_loci));
    GNXCHK(s.get(&d_lmax, (size_t)n_loci));
    HIPCHK(hipMemsetAsync(d_lsum, 0, (size_t)n_loci * sizeof(u64), h->stream));
    HIPCHK(hipMemsetAsync(d_lcnt, 0, (size_t)n_loci * sizeof(u64), h->stream));
    hipLaunchKernelGGL(k_coal_fill, dim3(gnx_grid(n_loci, 256)), dim3(256), 0, h->stream, n_loci,
                       INT_MIN, d_lmax);
  }
  if (nb) {
    GNXCHK(s.get(&d_edges, (size_t)n_tedges));
    GNXCHK(s.get(&d_hist, (size_t)nb));
    GNXCHK(gnx_h2d(h, d_edges, tedges, (size_t)n_tedges * sizeof(int32_t)));
    HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)nb * sizeof(u64), h->stream));
  }
  // loci per launch: the MRCAs, the only output n_loci x n_pairs, stay under the byte budget
  const int64_t budget = h->lin_budget > 0 ? h->lin_budget : LIN_BUDGET;
  int64_t per = n_loci;
  if (mrca) {
    per = std::min<int64_t>(n_loci, std::max<int64_t>(1, budget / (4 * n_pairs)));
    GNXCHK(s.get(&d_mrca, (size_t)per * n_pairs));
  }
  GnxCallTimer tm(h, &h->lin_ms, &h->lin_launches);
  for (int64_t q0 = 0; q0 < n_loci; q0 += per) {
    const int n_q = (int)std::min<int64_t>(per, n_loci - q0);
    const int n_ltiles = (n_q + 63) / 64;
    // pairs per wave: enough waves to fill the device, few enough per-locus atomics
    const int per_wave = (int)std::min<int64_t>(
        256, std::max<int64_t>(8, (n_pairs * n_ltiles + 65535) / 65536));
    const int64_t waves = (n_pairs + per_wave - 1) / per_wave * n_ltiles;
    const int64_t blocks = (waves + 3) / 4;
    if (blocks > INT_MAX) {
      gnx_set_error("%s: the request is too large for one launch", who);
      return 1;
    }
    tm.start();
    hipLaunchKernelGGL(k_coal_times, dim3((unsigned)blocks), dim3(256), 0, h->stream, n, d_nodes,
                       n_pairs, per_wave, n_q, d_loci + q0, n_ltiles, (const int2*)h->lin_tab,
                       h->lin_bt, (const u64*)h->paths, h->W64, w, nb, d_edges, d_psum, d_pcnt,
                       d_lsum ? d_lsum + q0 : nullptr, d_lcnt ? d_lcnt + q0 : nullptr,
                       d_lmax ? d_lmax + q0 : nullptr, d_hist, d_mrca);
    HIPCHK(hipGetLastError());
    GNXCHK(tm.stop());
    if (mrca) GNXCHK(gnx_d2h(h, mrca + q0 * n_pairs, d_mrca, (size_t)n_q * n_pairs * 4));
  }
  if (want_pair) {
    tm.start();
    hipLaunchKernelGGL(k_coal_mirror, dim3(gnx_grid((int64_t)n * n, 256, 256 * 64)), dim3(256), 0,
                       h->stream, (int64_t)n, d_pcnt, d_psum, (u64*)nullptr);
    HIPCHK(hipGetLastError());
    GNXCHK(tm.stop());
    if (pair_sum) GNXCHK(gnx_d2h(h, pair_sum, d_psum, (size_t)n * n * sizeof(int64_t)));
    if (pair_cnt) GNXCHK(gnx_d2h(h, pair_cnt, d_pcnt, (size_t)n * n * sizeof(int32_t)));
  }
  if (want_locus) {
    std::vector<int64_t> lc((size_t)n_loci);
    GNXCHK(gnx_d2h(h, lc.data(), d_lcnt, (size_t)n_loci * sizeof(int64_t)));
    if (locus_sum) GNXCHK(gnx_d2h(h, locus_sum, d_lsum, (size_t)n_loci * sizeof(int64_t)));
    if (locus_cnt) std::copy(lc.begin(), lc.end(), locus_cnt);
    if (locus_max) {
      GNXCHK(gnx_d2h(h, locus_max, d_lmax, (size_t)n_loci * sizeof(int32_t)));
      for (int q = 0; q < n_loci; ++q)
        if (lc[(size_t)q] == 0) locus_max[q] = -1;
    }
  }
  if (thist) GNXCHK(gnx_d2h(h, thist, d_hist, (size_t)nb * sizeof(int64_t)));
  return 0;
}

extern "C" int gnx_coal_segments(gnx_state* h, int64_t n_rows, const int32_t* node_tab,
                                 const int32_t* birth_t, int64_t n_nodes, const int32_t* nodes,
                                 int32_t n_loci, const int32_t* loci, const int64_t* pos,
                                 const uint8_t* brk, int32_t t_curr, int32_t max_ago,
                                 int32_t min_loci, int64_t min_len, int32_t n_edges,
                                 const int64_t* edges, int64_t max_work, int64_t* work,
                                 int32_t* cnt, int64_t* len, int64_t* longest, int64_t* hist,
                                 int64_t* cover) {
  const char* who = "gnx_coal_segments";
  GNXCHK(lin_table(h, who, n_rows, node_tab, birth_t, t_curr));
  h->lin_ms = 0.0;
  h->lin_launches = 0;
  CoalAge w;
  GNXCHK(coal_check(who, n_rows, birth_t, n_nodes, nodes, n_loci, t_curr, max_ago, work, &w));
  if (!loci || !pos) {
    gnx_set_error("%s: null loci or pos", who);
    return 1;
  }
  for (int q = 1; q < n_loci; ++q) {
    if (loci[q] <= loci[q - 1]) {
      gnx_set_error("%s: loci must be strictly ascending (loci[%d] = %d)", who, q, loci[q]);
      return 1;
    }
    if (pos[q] < pos[q - 1]) {
      gnx_set_error("%s: pos must be non-decreasing (pos[%d] = %lld)", who, q,
                    (long long)pos[q]);
      return 1;
    }
  }
  // (lengths are differences of two coordinates: they must stay inside int64)
  if (pos[0] < -(1ll << 62) || pos[n_loci - 1] > (1ll << 62)) {
    gnx_set_error("%s: pos must lie within +-2^62", who);
    return 1;
  }
  if (min_len < 0) {
    gnx_set_error("%s: min_len >= 0 (got %lld)", who, (long long)min_len);
    return 1;
  }
  if (hist || n_edges != 0 || edges) {
    if (n_edges < 2 || n_edges > COAL_NB + 1 || !edges || !hist) {
      gnx_set_error("%s: 2..%d edges with hist, or neither (got %d)", who, COAL_NB + 1, n_edges);
      return 1;
    }
    for (int k = 1; k < n_edges; ++k)
      if (!(edges[k] > edges[k - 1])) {
        gnx_set_error("%s: edges must be strictly ascending (edges[%d] = %lld)", who, k,
                      (long long)edges[k]);
        return 1;
      }
  }
  GnxScratch s(who);
  int32_t *d_nodes = nullptr, *d_loci = nullptr;
  GNXCHK(lin_request(h, who, n_rows, n_nodes, nodes, n_loci, loci, s, &d_nodes, &d_loci));
  GNXCHK(coal_work(who, n_nodes, n_loci, max_work, work));
  if (max_work <= 0) return 0;
  const int n = (int)n_nodes;
  const int64_t n_pairs = n_nodes * (n_nodes - 1) / 2;
  const int nb = hist ? n_edges - 1 : 0;
  long long *d_pos = nullptr, *d_edges = nullptr, *d_len = nullptr, *d_longest = nullptr;
  long long* d_cover = nullptr;
  uint8_t* d_brk = nullptr;
  int32_t* d_cnt = nullptr;
  u64* d_hist = nullptr;
  int* d_cdiff = nullptr;
  GNXCHK(s.get(&d_pos, (size_t)n_loci));
  GNXCHK(gnx_h2d(h, d_pos, pos, (size_t)n_loci * sizeof(int64_t)));
  if (brk) {
    GNXCHK(s.get(&d_brk, (size_t)n_loci));
    GNXCHK(gnx_h2d(h, d_brk, brk, (size_t)n_loci));
  }
  if (nb) {
    GNXCHK(s.get(&d_edges, (size_t)n_edges));
    GNXCHK(s.get(&d_hist, (size_t)nb * 2));
    GNXCHK(gnx_h2d(h, d_edges, edges, (size_t)n_edges * sizeof(int64_t)));
    HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)nb * 2 * sizeof(u64), h->stream));
  }
  // (the kernel writes both triangles; the diagonal stays zero)
  if (cnt) {
    GNXCHK(s.get(&d_cnt, (size_t)n * n));
    HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)n * n * sizeof(int32_t), h->stream));
  }
  if (len) {
    GNXCHK(s.get(&d_len, (size_t)n * n));
    HIPCHK(hipMemsetAsync(d_len, 0, (size_t)n * n * sizeof(long long), h->stream));
  }
  if (longest) {
    GNXCHK(s.get(&d_longest, (size_t)n * n));
    HIPCHK(hipMemsetAsync(d_longest, 0, (size_t)n * n * sizeof(long long), h->stream));
  }
  if (cover) {
    GNXCHK(s.get(&d_cdiff, (size_t)n_loci + 1));
    GNXCHK(s.get(&d_cover, (size_t)n_loci));
    HIPCHK(hipMemsetAsync(d_cdiff, 0, ((size_t)n_loci + 1) * sizeof(int), h->stream));
  }
  GnxCallTimer tm(h, &h->lin_ms, &h->lin_launches);
  tm.start();
  hipLaunchKernelGGL(k_coal_segments, dim3((unsigned)((n_pairs + 3) / 4)), dim3(256), 0,
                     h->stream, n, d_nodes, n_pairs, n_loci, d_loci, d_pos, d_brk,
                     (const int2*)h->lin_tab, h->lin_bt, (const u64*)h->paths, h->W64, w,
                     std::max(1, min_loci), (long long)min_len, nb, d_edges, d_cnt, d_len,
                     d_longest, d_hist, d_cdiff);
  if (cover)
    hipLaunchKernelGGL(k_coal_cover, dim3(1), dim3(1024), 0, h->stream, n_loci, d_cdiff, d_cover);
  HIPCHK(hipGetLastError());
  GNXCHK(tm.stop(cover ? 2 : 1));
  if (cnt) GNXCHK(gnx_d2h(h, cnt, d_cnt, (size_t)n * n * sizeof(int32_t)));
  if (len) GNXCHK(gnx_d2h(h, len, d_len, (size_t)n * n * sizeof(int64_t)));
  if (longest) GNXCHK(gnx_d2h(h, longest, d_longest, (size_t)n * n * sizeof(int64_t)));
  if (hist) GNXCHK(gnx_d2h(h, hist, d_hist, (size_t)nb * 2 * sizeof(int64_t)));
  if (cover) GNXCHK(gnx_d2h(h, cover, d_cover, (size_t)n_loci * sizeof(int64_t)));
  return 0;
}
