// Least-cost distances over the landscape's cells (geonomics_amd/sim/cost.py; the reference has
// no such analysis).  Nodes: the H x W cells, each joined to its 8 neighbours; the edge between
// cells u, v costs
//
//   w = (0.5 * (R[u] + R[v])) * len        len = res_x, res_y or sqrt(res_x^2 + res_y^2)
//
// in fp64, in that order, without contraction; R = inf closes a cell.  d[v] = min over the
// neighbours u of d[u] + w below d[source] = 0.  The rounded addition is monotone, so that fixed
// point is unique and the order of relaxation does not show in the result.
//
//   gnx_cost_surfaces   the accumulated-cost raster of every source
//   gnx_cost_matrix     the pairwise distances of a list of cells (only the matrix leaves the
//                       device)
//   gnx_cost_budget / gnx_cost_info
//
// A block-based fast iterative method.  The raster is cut into tiles of CT x CT cells.  One
// workgroup relaxes one (tile, source) pair to its local fixed point: the tile's distances and a
// one-cell halo live in LDS (fp64), a thread owns a CP x CP patch and keeps the resistances of
// the patch and of the ring around it in registers (loaded once per visit, through the same LDS
// array), and recomputes w from them: the same expression on every path.  A sweep reads the ring
// from LDS, relaxes the patch in place (so a value crosses a patch in one sweep) and writes the
// patch back; the workgroup leaves when no thread changed a value, or after CSWEEPS sweeps with
// the tile flagged active again.  Halo cells past the raster hold R = inf and d = inf and stay so.
//
// A round is one launch over the active pairs of the batch of sources.  A tile whose border row,
// column or corner cell changed marks the neighbour beyond it active for the next round (plain
// stores of 1 into the other of two flag arrays); k_cost_list turns the flags into the next
// round's list and counts it, and the host reads that one word back and stops at 0, or with an
// error after H W + 2 rounds.  Distances only decrease and a tile is written by one workgroup per
// round; a neighbour that reads a halo value while it is being lowered reads the old or the new
// one (an aligned 8-byte store), and is flagged for the next round either way.  No atomics on
// distances, no waits between workgroups.
#include <cmath>
#include <limits>
#include "gnx_geno.h"

#define CT 64                       // tile side
#define CP 4                        // patch side: a thread owns CP x CP cells
#define CTH ((CT / CP) * (CT / CP)) // threads per workgroup
#define CLD (CT + 2)                // tile + halo
#define CSWEEPS (2 * CT * CT)       // sweeps of one visit: twice the longest simple path in a tile
#define COST_BUDGET (2ll << 30)     // bytes of distance rasters per batch unless gnx_cost_budget says so
#define COST_MAX_CELLS 32768        // cells of one gnx_cost_matrix
#define COST_MAX_GRID 0x7fffffff     // thread = element kernels cover their range in one pass

static_assert(CTH == 256 && CT % CP == 0, "16 x 16 patches of 4 x 4 cells");

__global__ void k_cost_fill(int64_t n, double* __restrict__ d) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    d[i] = INFINITY;
}

// d[s][src[s]] = 0; active: the tile of src[s] and every tile whose halo holds that cell (the
// source's own value never changes, so no visit would flag them)
__global__ void k_cost_seed(int nb, const int32_t* __restrict__ src, int W, int ntx, int n_tiles,
                            int64_t HW, double* __restrict__ d, int32_t* __restrict__ flag) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nb) return;
  const int c = src[s];
  const int y = c / W, x = c - y * W;
  d[(int64_t)s * HW + c] = 0.0;
  const int H = (int)(HW / W);
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = y + dy, xx = x + dx;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W)
        flag[(int64_t)s * n_tiles + (yy / CT) * ntx + xx / CT] = 1;
    }
}

// the flagged (source, tile) pairs, in any order, and their number
__global__ void k_cost_list(int m, const int32_t* __restrict__ flag, int32_t* __restrict__ list,
                            int32_t* __restrict__ count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m && flag[i]) list[atomicAdd(count, 1)] = i;
}

__global__ void __launch_bounds__(CTH)
k_cost_solve(int H, int W, int ntx, int nty, const double* __restrict__ R, double lx, double ly,
             double ld, const int32_t* __restrict__ list, double* dist,
             int32_t* __restrict__ nxt) {
  __shared__ double Ds[CLD][CLD + 1];
  const int n_tiles = ntx * nty;
  const int pair = list[blockIdx.x];
  const int s = pair / n_tiles, t = pair - s * n_tiles;
  const int tyi = t / ntx, txi = t - tyi * ntx;
  const int y0 = tyi * CT - 1, x0 = txi * CT - 1;          // the halo's first row and column
  double* d = dist + (int64_t)s * H * W;
  const int tid = threadIdx.x, px = (tid & 15) * CP, py = (tid >> 4) * CP;
  double Rr[CP + 2][CP + 2], dr[CP + 2][CP + 2];
  for (int q = tid; q < CLD * CLD; q += CTH) {
    const int r = q / CLD, c = q - r * CLD;
    const int y = y0 + r, x = x0 + c;
    Ds[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? R[(int64_t)y * W + x] : INFINITY;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CP + 2; ++i)
#pragma unroll
    for (int j = 0; j < CP + 2; ++j) Rr[i][j] = Ds[py + i][px + j];
  __syncthreads();
  for (int q = tid; q < CLD * CLD; q += CTH) {
    const int r = q / CLD, c = q - r * CLD;
    const int y = y0 + r, x = x0 + c;
    Ds[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? d[(int64_t)y * W + x] : INFINITY;
  }
  __syncthreads();
#pragma unroll
  for (int i = 1; i <= CP; ++i)
#pragma unroll
    for (int j = 1; j <= CP; ++j) dr[i][j] = Ds[py + i][px + j];
  // which of the patch's border cells changed: rows 1 and CP (bits 0, 1), columns 1 and CP
  // (2, 3), the corners (1, 1), (1, CP), (CP, 1), (CP, CP) (4..7)
  unsigned mask = 0;
  bool ever = false, capped = false;
  for (int sweep = 1;; ++sweep) {
#pragma unroll
    for (int j = 0; j < CP + 2; ++j) {
      dr[0][j] = Ds[py][px + j];
      dr[CP + 1][j] = Ds[py + CP + 1][px + j];
    }
#pragma unroll
    for (int i = 1; i <= CP; ++i) {
      dr[i][0] = Ds[py + i][px];
      dr[i][CP + 1] = Ds[py + i][px + CP + 1];
    }
    bool chg = false;
#pragma unroll
    for (int i = 1; i <= CP; ++i)
#pragma unroll
      for (int j = 1; j <= CP; ++j) {
        double best = dr[i][j];
#pragma unroll
        for (int di = -1; di <= 1; ++di)
#pragma unroll
          for (int dj = -1; dj <= 1; ++dj) {
            if (di == 0 && dj == 0) continue;
            const double len = di == 0 ? lx : (dj == 0 ? ly : ld);
            const double w = (0.5 * (Rr[i][j] + Rr[i + di][j + dj])) * len;
            const double cand = dr[i + di][j + dj] + w;
            best = cand < best ? cand : best;
          }
        if (best < dr[i][j]) {
          dr[i][j] = best;
          chg = true;
          mask |= (i == 1 ? 1u : 0u) | (i == CP ? 2u : 0u) | (j == 1 ? 4u : 0u) |
                  (j == CP ? 8u : 0u) | (i == 1 && j == 1 ? 16u : 0u) |
                  (i == 1 && j == CP ? 32u : 0u) | (i == CP && j == 1 ? 64u : 0u) |
                  (i == CP && j == CP ? 128u : 0u);
        }
      }
    ever |= chg;
    __syncthreads();                                 // every ring of this sweep has been read
    if (chg) {
#pragma unroll
      for (int i = 1; i <= CP; ++i)
#pragma unroll
        for (int j = 1; j <= CP; ++j) Ds[py + i][px + j] = dr[i][j];
    }
    if (!__syncthreads_or(chg ? 1 : 0)) break;
    if (sweep >= CSWEEPS) {
      capped = true;
      break;
    }
  }
  if (ever) {
#pragma unroll
    for (int i = 1; i <= CP; ++i)
#pragma unroll
      for (int j = 1; j <= CP; ++j) {
        const int y = y0 + py + i, x = x0 + px + j;
        if (y < H && x < W) d[(int64_t)y * W + x] = dr[i][j];
      }
  }
  // the neighbours beyond a border that changed (a tile with a neighbour below or to the right
  // is a whole one: its last row and column are the patches' rows and columns CP)
  int32_t* f = nxt + (int64_t)s * n_tiles;
  const bool top = py == 0, bot = py == CT - CP, lef = px == 0, rig = px == CT - CP;
  const bool hasN = tyi > 0, hasS = tyi + 1 < nty, hasW = txi > 0, hasE = txi + 1 < ntx;
  if (top && hasN && (mask & 1u)) f[t - ntx] = 1;
  if (bot && hasS && (mask & 2u)) f[t + ntx] = 1;
  if (lef && hasW && (mask & 4u)) f[t - 1] = 1;
  if (rig && hasE && (mask & 8u)) f[t + 1] = 1;
  if (top && lef && hasN && hasW && (mask & 16u)) f[t - ntx - 1] = 1;
  if (top && rig && hasN && hasE && (mask & 32u)) f[t - ntx + 1] = 1;
  if (bot && lef && hasS && hasW && (mask & 64u)) f[t + ntx - 1] = 1;
  if (bot && rig && hasS && hasE && (mask & 128u)) f[t + ntx + 1] = 1;
  if (capped && tid == 0) f[t] = 1;
}

// Dm[s0 + s][t] = the distance of source s of the batch at cell cells[t]
__global__ void k_cost_gather(int nb, int s0, int n_cells, const int32_t* __restrict__ cells,
                              int64_t HW, const double* __restrict__ d, double* __restrict__ Dm) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)nb * n_cells) return;
  const int s = (int)(q / n_cells), t = (int)(q - (int64_t)s * n_cells);
  Dm[(int64_t)(s0 + s) * n_cells + t] = d[(int64_t)s * HW + cells[t]];
}

// Dm[a][b] = Dm[b][a] for a > b: the entry computed from the source with the lower index
__global__ void k_cost_mirror(int n, double* Dm) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)n * n) return;
  const int a = (int)(q / n), b = (int)(q - (int64_t)a * n);
  if (a > b) Dm[q] = Dm[(int64_t)b * n + a];
}

namespace {

// what every entry point checks first
int cost_no_ghosts(gnx_state* h, const char* who) {
  if (h->n_ghost > 0) {
    gnx_set_error("%s: the handle holds ghost records (a tile): not supported", who);
    return 1;
  }
  return 0;
}

struct CostRun {
  gnx_state* h;
  int H, W, ntx, nty, n_tiles;
  int64_t HW;
  double lx, ly, ld;
  int nb_max;                        // sources per batch
  double* d_R = nullptr;
  double* d_dist = nullptr;          // [nb_max][H][W]
  int32_t *d_flag[2] = {nullptr, nullptr}, *d_list = nullptr, *d_count = nullptr,
          *d_src = nullptr;
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  ~CostRun() {
    if (ev_a) (void)hipEventDestroy(ev_a);
    if (ev_b) (void)hipEventDestroy(ev_b);
  }
};

// the checks every entry point makes, the raster on the device and the batch's scratch
int cost_begin(gnx_state* h, const char* who, const double* R, double res_x, double res_y,
               int64_t n_src, GnxScratch& sc, CostRun& c) {
  if (!R) {
    gnx_set_error("%s: null R", who);
    return 1;
  }
  if (!(res_x > 0.0) || !(res_y > 0.0) || !std::isfinite(res_x) || !std::isfinite(res_y)) {
    gnx_set_error("%s: res_x and res_y must be positive and finite (got %g, %g)", who, res_x,
                  res_y);
    return 1;
  }
  c.h = h;
  c.H = h->cfg.H;
  c.W = h->cfg.W;
  c.HW = (int64_t)c.H * c.W;
  if (c.HW < 1 || c.HW > (1ll << 30)) {
    gnx_set_error("%s: 1..2^30 cells (the landscape has %lld)", who, (long long)c.HW);
    return 1;
  }
  for (int64_t i = 0; i < c.HW; ++i)
    if (!(R[i] > 0.0)) {                               // nan too
      gnx_set_error("%s: R[%lld] = %g: every entry must be > 0, or inf where impassable", who,
                    (long long)i, R[i]);
      return 1;
    }
  c.ntx = (c.W + CT - 1) / CT;
  c.nty = (c.H + CT - 1) / CT;
  c.n_tiles = c.ntx * c.nty;
  c.lx = res_x;
  c.ly = res_y;
  c.ld = std::sqrt(res_x * res_x + res_y * res_y);
  const int64_t budget = h->cost_budget > 0 ? h->cost_budget : COST_BUDGET;
  const int64_t per = c.HW * (int64_t)sizeof(double);
  if (budget < per) {
    gnx_set_error("%s: the budget of %lld bytes is below one source's raster (%lld bytes)", who,
                  (long long)budget, (long long)per);
    return 1;
  }
  int64_t nb = std::min<int64_t>(n_src, budget / per);
  nb = std::min<int64_t>(nb, ((1ll << 31) - 1) / c.n_tiles);      // pairs are int32
  c.nb_max = (int)std::max<int64_t>(nb, 1);
  const size_t pairs = (size_t)c.nb_max * c.n_tiles;
  GNXCHK(sc.get(&c.d_R, (size_t)c.HW));
  GNXCHK(sc.get(&c.d_dist, (size_t)c.nb_max * c.HW));
  GNXCHK(sc.get(&c.d_flag[0], pairs));
  GNXCHK(sc.get(&c.d_flag[1], pairs));
  GNXCHK(sc.get(&c.d_list, pairs));
  GNXCHK(sc.get(&c.d_count, 1));
  GNXCHK(sc.get(&c.d_src, (size_t)c.nb_max));
  GNXCHK(gnx_h2d(h, c.d_R, R, (size_t)c.HW * sizeof(double)));
  HIPCHK(hipEventCreate(&c.ev_a));
  HIPCHK(hipEventCreate(&c.ev_b));
  h->cost_ms = 0.0;
  h->cost_launches = h->cost_rounds = h->cost_batches = 0;
  return 0;
}

// the distance rasters of the nb sources src (host, checked) into c.d_dist
int cost_solve(CostRun& c, const char* who, int nb, const int32_t* src) {
  gnx_state* h = c.h;
  hipStream_t st = h->stream;
  const int m = nb * c.n_tiles;
  GNXCHK(gnx_h2d(h, c.d_src, src, (size_t)nb * sizeof(int32_t)));
  HIPCHK(hipEventRecord(c.ev_a, st));
  hipLaunchKernelGGL(k_cost_fill, dim3(gnx_grid((int64_t)nb * c.HW, 256, 1 << 16)), dim3(256), 0,
                     st, (int64_t)nb * c.HW, c.d_dist);
  HIPCHK(hipMemsetAsync(c.d_flag[0], 0, (size_t)m * sizeof(int32_t), st));
  HIPCHK(hipMemsetAsync(c.d_count, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(k_cost_seed, dim3(gnx_grid(nb, 256)), dim3(256), 0, st, nb, c.d_src, c.W,
                     c.ntx, c.n_tiles, c.HW, c.d_dist, c.d_flag[0]);
  hipLaunchKernelGGL(k_cost_list, dim3(gnx_grid(m, 256, COST_MAX_GRID)), dim3(256), 0, st, m, c.d_flag[0],
                     c.d_list, c.d_count);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c.ev_b, st));
  int32_t count = 0;
  GNXCHK(gnx_d2h(h, &count, c.d_count, sizeof(int32_t)));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, c.ev_a, c.ev_b) == hipSuccess) h->cost_ms += ms;
  h->cost_launches += 3;
  h->cost_batches += 1;
  int cur = 0;
  for (int64_t round = 0; count > 0; ++round) {
    if (round >= c.HW + 2) {
      gnx_set_error("%s: did not converge in %lld rounds", who, (long long)round);
      return 1;
    }
    if (count > m) {
      gnx_set_error("%s: %d active pairs of %d", who, count, m);
      return 1;
    }
    int32_t* nxt = c.d_flag[cur ^ 1];
    HIPCHK(hipEventRecord(c.ev_a, st));
    HIPCHK(hipMemsetAsync(nxt, 0, (size_t)m * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_cost_solve, dim3(count), dim3(CTH), 0, st, c.H, c.W, c.ntx, c.nty, c.d_R,
                       c.lx, c.ly, c.ld, c.d_list, c.d_dist, nxt);
    HIPCHK(hipMemsetAsync(c.d_count, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_cost_list, dim3(gnx_grid(m, 256, COST_MAX_GRID)), dim3(256), 0, st, m, nxt, c.d_list,
                       c.d_count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c.ev_b, st));
    GNXCHK(gnx_d2h(h, &count, c.d_count, sizeof(int32_t)));
    if (hipEventElapsedTime(&ms, c.ev_a, c.ev_b) == hipSuccess) h->cost_ms += ms;
    h->cost_launches += 2;
    h->cost_rounds += 1;
    cur ^= 1;
  }
  return 0;
}

int cost_check_cells(const char* who, const char* what, int64_t n, const int32_t* cells,
                     int64_t HW, bool distinct) {
  if (n > 0 && !cells) {
    gnx_set_error("%s: null %s", who, what);
    return 1;
  }
  std::vector<bool> seen(distinct ? (size_t)HW : 0, false);
  for (int64_t i = 0; i < n; ++i) {
    if (cells[i] < 0 || cells[i] >= HW) {
      gnx_set_error("%s: %s[%lld] = %d is not a cell in 0..%lld", who, what, (long long)i,
                    cells[i], (long long)HW - 1);
      return 1;
    }
    if (distinct) {
      if (seen[(size_t)cells[i]]) {
        gnx_set_error("%s: cell %d is listed twice", who, cells[i]);
        return 1;
      }
      seen[(size_t)cells[i]] = true;
    }
  }
  return 0;
}

}  // namespace

extern "C" int gnx_cost_budget(gnx_state* h, int64_t bytes) {
  GNXCHK(cost_no_ghosts(h, "gnx_cost_budget"));
  if (bytes < 0) {
    gnx_set_error("gnx_cost_budget: bytes >= 0 (0: the default)");
    return 1;
  }
  const int64_t per = (int64_t)h->cfg.H * h->cfg.W * (int64_t)sizeof(double);
  if (bytes > 0 && bytes < per) {
    gnx_set_error("gnx_cost_budget: %lld bytes are below one source's raster (%lld bytes)",
                  (long long)bytes, (long long)per);
    return 1;
  }
  h->cost_budget = bytes;
  return 0;
}

extern "C" int gnx_cost_info(gnx_state* h, double* kernel_ms, int64_t* launches, int64_t* rounds,
                             int64_t* batches) {
  GNXCHK(cost_no_ghosts(h, "gnx_cost_info"));
  if (kernel_ms) *kernel_ms = h->cost_ms;
  if (launches) *launches = h->cost_launches;
  if (rounds) *rounds = h->cost_rounds;
  if (batches) *batches = h->cost_batches;
  return 0;
}

extern "C" int gnx_cost_surfaces(gnx_state* h, const double* R, double res_x, double res_y,
                                 int32_t n_src, const int32_t* src, double* out) {
  const char* who = "gnx_cost_surfaces";
  GNXCHK(cost_no_ghosts(h, who));
  if (n_src < 1 || !out) {
    gnx_set_error("%s: at least one source, and a non-null out (n_src = %d)", who, n_src);
    return 1;
  }
  GNXCHK(cost_check_cells(who, "src", n_src, src, (int64_t)h->cfg.H * h->cfg.W, false));
  GnxScratch sc(who);
  CostRun c;
  GNXCHK(cost_begin(h, who, R, res_x, res_y, n_src, sc, c));
  for (int s0 = 0; s0 < n_src; s0 += c.nb_max) {
    const int nb = std::min(c.nb_max, n_src - s0);
    GNXCHK(cost_solve(c, who, nb, src + s0));
    GNXCHK(gnx_d2h(h, out + (int64_t)s0 * c.HW, c.d_dist, (size_t)nb * c.HW * sizeof(double)));
  }
  return 0;
}

extern "C" int gnx_cost_matrix(gnx_state* h, const double* R, double res_x, double res_y,
                               int32_t n_cells, const int32_t* cells, double* D) {
  const char* who = "gnx_cost_matrix";
  GNXCHK(cost_no_ghosts(h, who));
  if (n_cells < 1 || n_cells > COST_MAX_CELLS || !D) {
    gnx_set_error("%s: 1..%d cells, and a non-null D (n_cells = %d)", who, COST_MAX_CELLS,
                  n_cells);
    return 1;
  }
  GNXCHK(cost_check_cells(who, "cells", n_cells, cells, (int64_t)h->cfg.H * h->cfg.W, true));
  GnxScratch sc(who);
  CostRun c;
  GNXCHK(cost_begin(h, who, R, res_x, res_y, n_cells, sc, c));
  int32_t* d_cells = nullptr;
  double* d_D = nullptr;
  GNXCHK(sc.get(&d_cells, (size_t)n_cells));
  GNXCHK(sc.get(&d_D, (size_t)n_cells * n_cells));
  GNXCHK(gnx_h2d(h, d_cells, cells, (size_t)n_cells * sizeof(int32_t)));
  for (int s0 = 0; s0 < n_cells; s0 += c.nb_max) {
    const int nb = std::min(c.nb_max, n_cells - s0);
    GNXCHK(cost_solve(c, who, nb, cells + s0));
    hipLaunchKernelGGL(k_cost_gather, dim3(gnx_grid((int64_t)nb * n_cells, 256, COST_MAX_GRID)), dim3(256), 0,
                       h->stream, nb, s0, (int)n_cells, d_cells, c.HW, c.d_dist, d_D);
    HIPCHK(hipGetLastError());
    h->cost_launches += 1;
  }
  hipLaunchKernelGGL(k_cost_mirror, dim3(gnx_grid((int64_t)n_cells * n_cells, 256, COST_MAX_GRID)), dim3(256), 0,
                     h->stream, (int)n_cells, d_D);
  HIPCHK(hipGetLastError());
  h->cost_launches += 1;
  return gnx_d2h(h, D, d_D, (size_t)n_cells * n_cells * sizeof(double));
}
