// What the calls that visit the pairs of nearby individuals share (gnx_sgs.hip: sums per distance
// class; gnx_kin.hip: the list of close-kin pairs): the grid of cells whose side is at least the
// reach, the sample sorted by cell, and the host's list of 64 x 64 tiles over the pairs of rows of
// the same or adjacent cells.  The kernels are gnx_sgs.hip's; the functions below launch them
// exactly as gnx_sgs_sums always has.
#pragma once
#include <cmath>
#include <limits>
#include "gnx_geno.h"

#define SGS_MAX_CELLS (1 << 22)

// a 64 x 64 tile of pairs: rows a0 .. a0 + na - 1 against rows b0 .. b0 + nb - 1 of the sorted
// sample (na, nb <= 64); a0 == b0 only for a diagonal tile of a cell with itself
struct SgsTask {
  int32_t a0, na, b0, nb;
};

// gnx_sgs.hip
// key[i] = the cell of sample index i, val[i] = i
__global__ void k_sgs_cells(int64_t n, const int64_t* __restrict__ slots,
                            const float* __restrict__ x, const float* __restrict__ y, double side,
                            int ncx, int ncy, uint32_t* __restrict__ key,
                            int32_t* __restrict__ val);
// start[c] = the first sorted position whose cell is >= c (c = 0 .. n_cells)
__global__ void k_sgs_cell_start(int64_t n, int n_cells, const uint32_t* __restrict__ key,
                                 int32_t* __restrict__ start);
// sorted position j holds sample index o = order[j]: its own coordinates, and the genome row of
// sample index perm[o]
__global__ void k_sgs_arrange(int64_t n, const int32_t* __restrict__ order,
                              const int64_t* __restrict__ slots, const int32_t* __restrict__ perm,
                              const int32_t* __restrict__ rows, const float* __restrict__ x,
                              const float* __restrict__ y, int32_t* __restrict__ rows_sorted,
                              float* __restrict__ xs, float* __restrict__ ys);

namespace {

struct SgsGrid {
  double side;
  int64_t ncx, ncy;
  int n_cells, bits;           // bits: of the cell number, for the sort
};

// the grid: a side a little above the reach (so that rounding in r or in the cell number cannot
// part two individuals closer than it by more than one cell), larger where the landscape would
// have more than SGS_MAX_CELLS cells; reach <= 0 or infinite: one cell
SgsGrid sgs_grid(const gnx_state* h, double reach) {
  SgsGrid g;
  if (!(reach > 0.0) || std::isinf(reach)) {
    g.side = std::numeric_limits<double>::infinity();
    g.ncx = g.ncy = 1;
  } else {
    const double Wd = std::max(1, h->cfg.W), Hd = std::max(1, h->cfg.H);
    g.side = reach * (1.0 + 1e-6);
    for (;;) {
      const double fx = std::ceil(Wd / g.side), fy = std::ceil(Hd / g.side);
      if (fx * fy <= (double)SGS_MAX_CELLS) {
        g.ncx = std::max<int64_t>(1, (int64_t)fx);
        g.ncy = std::max<int64_t>(1, (int64_t)fy);
        break;
      }
      g.side = std::max(g.side * 1.25, std::sqrt(Wd * Hd / (double)SGS_MAX_CELLS));
    }
  }
  g.n_cells = (int)(g.ncx * g.ncy);
  g.bits = 1;
  while ((1ll << g.bits) < g.n_cells) ++g.bits;
  return g;
}

// the sample sorted by cell (gnx_prim_sort on the cell number, stable): *d_order [n] on the
// device = the sample index at each sorted position, start [n_cells + 1] on the host = the cells'
// row ranges
int sgs_sort_cells(gnx_state* h, GnxScratch& s, const SgsGrid& g, int64_t n,
                   const int64_t* d_slots, int32_t** d_order, std::vector<int32_t>& start) {
  const GnxSoA a = h->soa[h->cur];
  uint32_t *d_key = nullptr, *d_key2 = nullptr;
  int32_t *d_val = nullptr, *d_start = nullptr;
  char* d_tmp = nullptr;
  size_t tmp_bytes = 0;
  GNXCHK(gnx_prim_sort_bytes((size_t)n, g.bits, &tmp_bytes));
  GNXCHK(s.get(&d_key, (size_t)n));
  GNXCHK(s.get(&d_key2, (size_t)n));
  GNXCHK(s.get(&d_val, (size_t)n));
  GNXCHK(s.get(d_order, (size_t)n));
  GNXCHK(s.get(&d_start, (size_t)g.n_cells + 1));
  GNXCHK(s.get(&d_tmp, tmp_bytes));
  hipLaunchKernelGGL(k_sgs_cells, dim3(gnx_grid(n, 256)), dim3(256), 0, h->stream, n, d_slots,
                     a.x, a.y, g.side, (int)g.ncx, (int)g.ncy, d_key, d_val);
  GNXCHK(gnx_prim_sort(d_tmp, tmp_bytes, d_key, d_key2, d_val, *d_order, (size_t)n, g.bits,
                       h->stream));
  hipLaunchKernelGGL(k_sgs_cell_start, dim3(gnx_grid(g.n_cells + 1, 256)), dim3(256), 0,
                     h->stream, n, g.n_cells, d_key2, d_start);
  HIPCHK(hipGetLastError());
  start.resize((size_t)g.n_cells + 1);
  GNXCHK(gnx_d2h(h, start.data(), d_start, start.size() * sizeof(int32_t)));
  return 0;
}

// a cell is paired with itself and with its four forward neighbours
static const int SGS_FWD[4][2] = {{1, 0}, {-1, 1}, {0, 1}, {1, 1}};

inline int64_t sgs_cell_count(const SgsGrid& g, const std::vector<int32_t>& start, int64_t cxi,
                              int64_t cyi) {
  if (cxi < 0 || cxi >= g.ncx || cyi >= g.ncy) return 0;
  const int64_t c = cyi * g.ncx + cxi;
  return start[c + 1] - start[c];
}

// the candidate pairs and the tiles that cover them
void sgs_count_pairs(const SgsGrid& g, const std::vector<int32_t>& start, int64_t* cand,
                     int64_t* n_tasks) {
  *cand = *n_tasks = 0;
  for (int64_t cyi = 0; cyi < g.ncy; ++cyi)
    for (int64_t cxi = 0; cxi < g.ncx; ++cxi) {
      const int64_t m = sgs_cell_count(g, start, cxi, cyi);
      if (!m) continue;
      const int64_t ta = (m + 63) / 64;
      *cand += m * (m - 1) / 2;
      *n_tasks += ta * (ta + 1) / 2;
      for (const auto& f : SGS_FWD) {
        const int64_t m2 = sgs_cell_count(g, start, cxi + f[0], cyi + f[1]);
        *cand += m * m2;
        *n_tasks += ta * ((m2 + 63) / 64);
      }
    }
}

// the tiles, cell by cell: (cell, cell) with its diagonal and upper tiles, then (cell, forward
// neighbour) in the order of SGS_FWD
void sgs_list_tasks(const SgsGrid& g, const std::vector<int32_t>& start, int64_t n_tasks,
                    std::vector<SgsTask>& tasks) {
  tasks.clear();
  tasks.reserve((size_t)n_tasks);
  for (int64_t cyi = 0; cyi < g.ncy; ++cyi)
    for (int64_t cxi = 0; cxi < g.ncx; ++cxi) {
      const int64_t m = sgs_cell_count(g, start, cxi, cyi);
      if (!m) continue;
      const int32_t a0 = start[cyi * g.ncx + cxi];
      for (int64_t i = 0; i < m; i += 64)
        for (int64_t j = i; j < m; j += 64)
          tasks.push_back(SgsTask{(int32_t)(a0 + i), (int32_t)std::min<int64_t>(64, m - i),
                                  (int32_t)(a0 + j), (int32_t)std::min<int64_t>(64, m - j)});
      for (const auto& f : SGS_FWD) {
        const int64_t m2 = sgs_cell_count(g, start, cxi + f[0], cyi + f[1]);
        if (!m2) continue;
        const int32_t b0 = start[(cyi + f[1]) * g.ncx + cxi + f[0]];
        for (int64_t i = 0; i < m; i += 64)
          for (int64_t j = 0; j < m2; j += 64)
            tasks.push_back(SgsTask{(int32_t)(a0 + i), (int32_t)std::min<int64_t>(64, m - i),
                                    (int32_t)(b0 + j), (int32_t)std::min<int64_t>(64, m2 - j)});
      }
    }
}

}  // namespace
