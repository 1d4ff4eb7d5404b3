// Introductions (reference structs/species.py:1631-2077, Species._add_individuals with a
// Species as the source): individuals of one handle appended to another one on the same
// device, genomes included, without the host and without unpacking a genome.
//
// A genome is 2 * NB table entries that name physical blocks (gnx_half.h), and after a few
// steps most entries of a population name a block that other individuals name too.  The
// transplant keeps that: every DISTINCT source block the newcomers refer to is copied once
// into a fresh block of the recipient, and every newcomer's entry is linked to the copy.
//
//   k_tp_dedup    thread = logical block of a newcomer: its source block goes into an
//                 open-addressing table (atomicCAS on the 32-bit block number), the reference
//                 is counted, the first claimant appends the block to the job list
//   (host)        D = jobs = distinct source blocks is read back; slots, rows and D free
//                 blocks are checked before anything of the recipient changes
//   k_tp_columns  thread = newcomer: logical row, x, y, id, age and sex
//   k_tp_assign   thread = job: a free block of the recipient (wave-aggregated pop)
//   k_tp_copy     lane = 16-byte chunk of the job list laid end to end
//   k_tp_link     thread = logical block: the recipient's table entry, GNX_OWN iff nobody
//                 else among the newcomers refers to the block
//   k_tp_fitness  thread = newcomer: the fitness k_death_probs would store
//
// Scratch per call (M = 2 * NB * n logical blocks, T = the power of two in [2 M, 4 M)):
// 12 T bytes of table (key, reference count, recipient block), 4 M of table positions,
// 12 M of jobs, 16 n of slots and coordinates: 40 to 64 bytes per logical block, whatever
// the source's capacity.
#include <algorithm>
#include "gnx_internal.h"

namespace {

struct TpTable {
  int32_t* key;     // [T] source block, -1 = empty
  int32_t* ref;     // [T] newcomers' table entries that name it
  int32_t* blk;     // [T] its copy in the recipient
  int bits;         // T = 1 << bits
};

struct TpJobs {
  int32_t* src;     // [M] source block
  int32_t* pos;     // [M] its position in the table
  int32_t* dst;     // [M] recipient block
  int32_t* n;       // [1]
};

}  // namespace

// Fibonacci hashing: block numbers come in runs (row * 2 NB + q), the product spreads them
__device__ __forceinline__ uint32_t tp_hash(int32_t key, int bits) {
  return ((uint32_t)key * 0x9E3779B1u) >> (32 - bits);
}

__global__ void __launch_bounds__(256)
k_tp_dedup(int64_t M, int per, const int64_t* __restrict__ slots,
           const int32_t* __restrict__ src_grow, const int32_t* __restrict__ src_hmap, TpTable T,
           int32_t* __restrict__ ent, TpJobs J) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = t < M;                 // (no early return: the append is a wave's business)
  bool first = false;
  int32_t key = 0;
  uint32_t p = 0;
  if (live) {
    const int64_t k = t / per;
    const int q = (int)(t - k * per);
    key = GNX_BLK(src_hmap[(int64_t)src_grow[slots[k]] * per + q]);
    const uint32_t mask = (1u << T.bits) - 1u;
    p = tp_hash(key, T.bits);
    for (;;) {
      const int32_t seen = atomicCAS(&T.key[p], -1, key);
      if (seen == -1) {
        first = true;
        break;
      }
      if (seen == key) break;
      p = (p + 1u) & mask;
    }
    atomicAdd(&T.ref[p], 1);
    ent[t] = (int32_t)p;
  }
  const int32_t j = gnx_wave_append(J.n, first);
  if (first) {
    J.src[j] = key;
    J.pos[j] = (int32_t)p;
  }
}

__global__ void __launch_bounds__(256)
k_tp_columns(int64_t N, int64_t n, int64_t cap, GnxSoA d, GnxSoA s,
             const int64_t* __restrict__ slots, const float* __restrict__ x,
             const float* __restrict__ y, int64_t first_id, const int32_t* __restrict__ free_rows,
             int64_t n_free, int has_rows, int n_traits) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int64_t from = slots[k], slot = N + k;
  const int32_t age = s.age[from];
  const uint8_t sex = s.sex[from];
  const int32_t row = has_rows ? free_rows[n_free - 1 - k] : -1;    // (as k_unpack pops them)
  d.x[slot] = x[k];
  d.y[slot] = y[k];
  d.age[slot] = age;
  d.sex[slot] = sex;
  d.id[slot] = first_id + k;
  d.ghost[slot] = 0;
  d.grow[slot] = row;
  d.fit[slot] = 1.0f;
  if (!has_rows)
    for (int t = 0; t < n_traits; ++t) d.z[(int64_t)t * cap + slot] = 0.f;
}

__global__ void __launch_bounds__(256)
k_tp_assign(GnxHalves H, TpTable T, TpJobs J) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool want = j < *J.n;              // (every lane takes part in the pop's ballot)
  const int32_t b = gnx_half_pop(H, want);
  if (want) {
    J.dst[j] = b;
    T.blk[J.pos[j]] = b;
  }
}

// The jobs' blocks laid end to end, C chunks of 16 bytes each: lane = chunk, so a wave moves
// 64 / C jobs per access whatever the block size (C = 40 at L = 10^5, 16 at L = 10^4) and no
// lane idles; four independent loads are in flight per lane before the first store.
__global__ void __launch_bounds__(256)
k_tp_copy(int64_t D, int C, const uint4* __restrict__ Gs, uint4* __restrict__ Gd,
          const int32_t* __restrict__ jsrc, const int32_t* __restrict__ jdst) {
  const int64_t total = D * C;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g0 < total; g0 += 4 * stride) {
    uint4 v[4];
    int64_t o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // (a chunk past the end reads the last one again and stores nothing: no branch
      // around the loads, the four stay in registers and in flight together)
      const int64_t g = min(g0 + u * stride, total - 1);
      const int64_t j = g / C;
      const int c = (int)(g - j * C);
      v[u] = Gs[(int64_t)jsrc[j] * C + c];
      o[u] = (int64_t)jdst[j] * C + c;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (g0 + u * stride < total) Gd[o[u]] = v[u];
  }
}

__global__ void __launch_bounds__(256)
k_tp_link(int64_t M, int per, int64_t N, const int32_t* __restrict__ grow,
          const int32_t* __restrict__ ent, TpTable T, int32_t* __restrict__ hmap) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M) return;
  const int64_t k = t / per;
  const int q = (int)(t - k * per);
  const int32_t p = ent[t];
  // a block that several newcomers refer to is nobody's own: a mutation copies it first
  const uint32_t own = T.ref[p] == 1 ? GNX_OWN : 0u;
  hmap[(int64_t)grow[N + k] * per + q] = (int32_t)((uint32_t)T.blk[p] | own);
}

// What k_death_probs stores in `fit` (ops/selection.py:51-125): w = max(prod_t (1 - phi_t
// |e^(not univ_adv) - z_t|^gamma_t), 0.001) x prod_del (1 - s_l (g_l0 + g_l1)), the deleterious
// loci read from the selected-locus table behind the trait loci.
__global__ void __launch_bounds__(256)
k_tp_fitness(int64_t first, int64_t n, int64_t cap, int W, GnxSoA s, GnxTraitTab T, int n_delet,
             int n_tl, int TW, const double* __restrict__ delet_s) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int64_t i = first + k;
  const int cx = (int)s.x[i], cy = (int)s.y[i];
  double w = 1.0;
  if (T.n_traits > 0) {
    for (int t = 0; t < T.n_traits; ++t) {
      double e = (double)s.e[(int64_t)T.layer[t] * cap + i];
      if (T.univ_adv[t]) e = 1.0;                      // e ** 0
      const double z = (double)s.z[(int64_t)t * cap + i];
      const double phi = T.phi_rast[t] ? (double)T.phi_rast[t][(int64_t)cy * W + cx] : T.phi[t];
      const double dz = fabs(e - z);
      w *= 1.0 - phi * (T.gamma[t] == 1.0 ? dz : pow(dz, T.gamma[t]));
    }
    w = fmax(w, 0.001);
  }
  if (n_delet > 0) {
    const uint64_t* t0 = s.tb + (i * 2 + 0) * TW;
    const uint64_t* t1 = t0 + TW;
    for (int q = 0; q < n_delet; ++q) {
      const int e = n_tl + q;
      const int cnt = (int)((t0[e >> 6] >> (e & 63)) & 1ull) + (int)((t1[e >> 6] >> (e & 63)) & 1ull);
      w *= 1.0 - (double)cnt * delet_s[q];
    }
  }
  s.fit[i] = (float)w;
}

namespace {

int tp_refuse(const char* why) {
  gnx_set_error("gnx_transplant: %s", why);
  return 1;
}

// nothing of a step is half done on the handle: its counts are the host's
int tp_settled(gnx_state* h, const char* which) {
  if (h->dd_active) GNXCHK(gnx_dd_leave(h));
  if (h->mort_wait || h->pairs_wait || h->tile2_mode) {
    gnx_set_error("gnx_transplant: the %s is inside a split or tiled step", which);
    return 1;
  }
  return 0;
}

}  // namespace

extern "C" int gnx_transplant(gnx_state* dst, gnx_state* src, int64_t n, const int64_t* src_slots,
                              const float* x, const float* y, int64_t first_id, int64_t* out) {
  if (!dst || !src || !out || n < 0 || (n > 0 && (!src_slots || !x || !y)))
    return tp_refuse("null handle, output or list");
  if (dst == src) return tp_refuse("source and recipient are the same handle");
  if (dst->cfg.device != src->cfg.device)
    return tp_refuse("source and recipient live on different devices");
  if (dst->n_ghost > 0 || src->n_ghost > 0)
    return tp_refuse("a handle holds ghost records (a tile): not supported");
  if (dst->cfg.L != src->cfg.L || dst->W64 != src->W64)
    return tp_refuse("source and recipient have genomes of different lengths");
  const bool rows = dst->cfg.L > 0;
  if (rows && !(dst->genomes_assigned && src->genomes_assigned))
    return tp_refuse("genomes are not assigned on both handles");
  const GnxHalves Hd = gnx_halves(dst), Hs = gnx_halves(src);
  if (rows && (Hd.NB != Hs.NB || Hd.BW != Hs.BW))
    return tp_refuse("source and recipient store their genomes in blocks of different sizes");
  GNXCHK(tp_settled(src, "source"));
  GNXCHK(tp_settled(dst, "recipient"));
  if (first_id <= dst->max_id) {
    gnx_set_error("gnx_transplant: first_id %lld is not above the recipient's largest id %lld",
                  (long long)first_id, (long long)dst->max_id);
    return 1;
  }
  const gnx_config& c = dst->cfg;
  for (int64_t k = 0; k < n; ++k)
    if (!(x[k] >= 0 && x[k] < c.W && y[k] >= 0 && y[k] < c.H)) {
      gnx_set_error("gnx_transplant: newcomer %lld at (%g, %g) is off the recipient's landscape",
                    (long long)k, (double)x[k], (double)y[k]);
      return 1;
    }
  {
    std::vector<uint8_t> taken((size_t)src->N, 0);
    for (int64_t k = 0; k < n; ++k) {
      if (src_slots[k] < 0 || src_slots[k] >= src->N) return tp_refuse("slot out of range");
      if (taken[(size_t)src_slots[k]]) return tp_refuse("a slot is listed twice");
      taken[(size_t)src_slots[k]] = 1;
    }
  }
  const int64_t N = dst->N;
  out[0] = N;
  out[1] = out[2] = 0;
  out[3] = 0;
  if (n == 0) return 0;
  const int per = 2 * Hd.NB;
  const int64_t M = rows ? (int64_t)per * n : 0;
  int bits = 6;
  while (((int64_t)1 << bits) < 2 * M) ++bits;
  if (bits > 30) return tp_refuse("too many genome blocks for one call");

  // both populations as their next reader needs them: the pending crossover written, the
  // living in slots [0, N) (gnx_geno.hip: geno_ready)
  GNXCHK(gnx_xo_join(src));
  GNXCHK(gnx_l_make_dense(src));
  GNXCHK(gnx_xo_join(dst));
  GNXCHK(gnx_l_make_dense(dst));
  HIPCHK(hipStreamSynchronize(src->stream));       // from here on: the recipient's stream only
  hipStream_t st = dst->stream;

  if (N + n > c.cap_inds || (rows && n > dst->n_free)) {
    gnx_set_error("capacity exceeded transplanting %lld individuals (N=%lld cap=%lld free rows %lld)",
                  (long long)n, (long long)N, (long long)c.cap_inds, (long long)dst->n_free);
    return 2;
  }

  GnxScratch sc("gnx_transplant");
  int64_t* d_slots = nullptr;
  float *d_x = nullptr, *d_y = nullptr;
  GNXCHK(sc.get(&d_slots, (size_t)n));
  GNXCHK(sc.get(&d_x, (size_t)n));
  GNXCHK(sc.get(&d_y, (size_t)n));
  TpTable T{};
  TpJobs J{};
  int32_t* ent = nullptr;
  T.bits = bits;
  if (rows) {
    const size_t tsz = (size_t)1 << bits;
    GNXCHK(sc.get(&T.key, tsz));
    GNXCHK(sc.get(&T.ref, tsz));
    GNXCHK(sc.get(&T.blk, tsz));
    GNXCHK(sc.get(&ent, (size_t)M));
    GNXCHK(sc.get(&J.src, (size_t)M));
    GNXCHK(sc.get(&J.pos, (size_t)M));
    GNXCHK(sc.get(&J.dst, (size_t)M));
    GNXCHK(sc.get(&J.n, 1));
  }
  GNXCHK(gnx_h2d(dst, d_slots, src_slots, (size_t)n * sizeof(int64_t)));
  GNXCHK(gnx_h2d(dst, d_x, x, (size_t)n * sizeof(float)));
  GNXCHK(gnx_h2d(dst, d_y, y, (size_t)n * sizeof(float)));

  const GnxSoA ss = src->soa[src->cur];
  int64_t D = 0;
  const int64_t gc_before = dst->gc_runs;
  if (rows) {
    const size_t tsz = (size_t)1 << bits;
    HIPCHK(hipMemsetAsync(T.key, 0xff, tsz * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(T.ref, 0, tsz * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(J.n, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_tp_dedup, dim3(gnx_grid(M, 256, 1 << 30)), dim3(256), 0, st, M, per,
                       (const int64_t*)d_slots, (const int32_t*)ss.grow,
                       (const int32_t*)src->hmap, T, ent, J);
    HIPCHK(hipGetLastError());
    int32_t d32 = 0;
    GNXCHK(gnx_d2h(dst, &d32, J.n, sizeof(d32)));      // (the one read-back: not a step path)
    D = d32;
    // D free blocks, after a collection if the host cannot be sure; nothing of the recipient
    // has changed when this returns 2
    GNXCHK(gnx_half_reserve(dst, D));
  }

  // slots appended behind a sorted population: the step's counted bins and fresh sort keys
  // do not cover them
  gnx_bins_adults_drop(dst);
  dst->fb_adults = false;
  GNXCHK(gnx_os_hist_discard(dst));
  dst->keys_fresh = false;

  const GnxSoA ds = dst->soa[dst->cur];
  hipLaunchKernelGGL(k_tp_columns, dim3(gnx_grid(n, 256)), dim3(256), 0, st, N, n, c.cap_inds, ds,
                     ss, (const int64_t*)d_slots, (const float*)d_x,
                     (const float*)d_y, first_id, (const int32_t*)dst->free_rows, dst->n_free,
                     rows ? 1 : 0, c.n_traits);
  if (rows) {
    hipLaunchKernelGGL(k_tp_assign, dim3(gnx_grid(D, 256, 1 << 30)), dim3(256), 0, st, Hd, T, J);
    const int C = Hd.BW >> 1;
    hipLaunchKernelGGL(k_tp_copy, dim3(gnx_grid((D * C + 3) / 4, 256, 256 * 16)), dim3(256), 0, st,
                       D, C, (const uint4*)src->G, (uint4*)dst->G, (const int32_t*)J.src,
                       (const int32_t*)J.dst);
    hipLaunchKernelGGL(k_tp_link, dim3(gnx_grid(M, 256, 1 << 30)), dim3(256), 0, st, M, per, N,
                       (const int32_t*)ds.grow, (const int32_t*)ent, T, dst->hmap);
    dst->n_free -= n;
  }
  HIPCHK(hipGetLastError());
  GNXCHK(gnx_l_gather_e(dst, N, n));
  if (rows) {
    GNXCHK(gnx_l_tb_from_rows(dst, N, n, nullptr, nullptr, false));
    GNXCHK(gnx_l_phenotype(dst, N, n));
  }
  hipLaunchKernelGGL(k_tp_fitness, dim3(gnx_grid(n, 256)), dim3(256), 0, st, N, n, c.cap_inds, c.W,
                     ds, gnx_trait_tab(dst), rows ? dst->n_delet : 0, dst->n_tl, dst->TW,
                     (const double*)dst->delet_s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  dst->N = N + n;
  dst->max_id = first_id + n - 1;
  // newcomers carry ids of their own: the id-ordered index is rebuilt by the next cell sort
  // (gnx_tile.hip: import_common), and the device-driven step takes its counts from the
  // host when it is entered next - no captured graph holds N, so cfg_epoch stays
  dst->ord_valid = false;
  out[1] = D;
  out[2] = M;
  out[3] = dst->gc_runs - gc_before;
  return 0;
}
