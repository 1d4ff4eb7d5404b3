// Genotype-environment association on the device (reference sim/model.py:2717-2780,
// Model.run_gea -> structs/species.py:2218-2355, _make_gea_df / _run_cca: a pandas table of
// all N x L mean genotypes plus env, lat, long on the host, then sklearn's CCA).  The fit
// needs only cross-products over the individuals (geonomics_amd/sim/gea.py), and those are
// taken here straight from the bit-packed genome table, without ever downloading N x L:
//
//   gnx_geno_locus_gram    C = D_S^T D_S and s = D_S^T 1 of the listed loci, exact int64
//   gnx_geno_locus_cross   D_S^T Z, Z^T Z, Z^T 1 in fp64, Z = [e[lyr], x, y] of the device
//
// Gram: the listed loci are transposed once into individual-major bit planes
// XT[locus][hom][word of 64 individuals] - every genome line that holds a listed locus is read
// once, through the block table, into LDS, and 64 x 64 bit tiles are turned in registers with
// wave ballots - after which d_l d_m summed over the individuals is four AND + popcounts per
// word: the tile product of gnx_geno_gram (k_geno_gram) with loci as rows.
// Cross: lane = locus, as gnx_geno_rmatmul; d z is exact in fp64, the partial sums of the
// stretches of individuals are added in a fixed order, so nothing depends on scheduling.
#include "gnx_geno.h"

#define GEA_LW 16            // words of a genome line (128 bytes, 1024 loci)
#define GEA_TI 128           // individuals per LDS stage of the cross kernel
#define GEA_ZB 256           // blocks (and partial sums) of the predictors' own products

// ---------------------------------------------------------------- transpose
// Block = 64 individuals (output word blockIdx.x) x one genome line that holds a listed locus
// (lines[blockIdx.y]).  wmask[w]: the listed loci of word w; qbase[w]: the list position of
// the first of them (the list is ascending, so a word's loci are consecutive in it).  The
// row stride of Ws is odd in u64: lanes = individuals read one column without bank conflicts.
// Individuals past n contribute 0 bits.
__global__ void __launch_bounds__(256)
k_gea_transpose(int64_t n, int W64, int Wm, const int32_t* __restrict__ rows,
                const int32_t* __restrict__ lines, const u64* __restrict__ wmask,
                const int32_t* __restrict__ qbase, const u64* __restrict__ G, GnxHalves H,
                u64* __restrict__ XT) {
  __shared__ u64 Ws[64][2 * GEA_LW + 1];
  const int tid = threadIdx.x, lane = tid & 63, v = tid >> 6;
  const int wg = lines[blockIdx.y] * GEA_LW;
  const int64_t i0 = (int64_t)blockIdx.x * 64;
  for (int q = tid; q < 64 * 2 * GEA_LW; q += 256) {      // a line's 16 words: 16 lanes
    const int j = q >> 5, hh = (q >> 4) & 1, w = q & 15;
    u64 x = 0;
    if (i0 + j < n && wg + w < W64) x = G[gnx_word_at(H, (int64_t)rows[i0 + j] * 2 + hh, wg + w)];
    Ws[j][hh * GEA_LW + w] = x;
  }
  __syncthreads();
#pragma unroll 1
  for (int u = 0; u < 4; ++u) {
    const int w = 4 * v + u;
    const u64 m = wmask[wg + w];                          // wave-uniform
    if (m == 0ull) continue;
    const int q = qbase[wg + w] + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const u64 x = Ws[lane][hh * GEA_LW + w];            // lane = individual
      u64 t = 0;                                          // lane = locus
#pragma unroll
      for (int l = 0; l < 64; ++l) {
        const u64 b = __ballot((int)((x >> l) & 1ull));
        if (lane == l) t = b;
      }
      if ((m >> lane) & 1ull) XT[((int64_t)q * 2 + hh) * Wm + blockIdx.x] = t;
    }
  }
}

// s[q] = the dosages of locus q summed: popcounts of its two planes (2 Wm consecutive words);
// one wave per locus
__global__ void __launch_bounds__(256)
k_gea_colsum(int n_loci, int Wm, const u64* __restrict__ XT, int64_t* __restrict__ s) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_loci) return;                                // wave-uniform
  const u64* p = XT + (int64_t)q * 2 * Wm;
  int c = 0;
  for (int w = lane; w < 2 * Wm; w += 64) c += __popcll(p[w]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
  if (lane == 0) s[q] = c;
}

// ---------------------------------------------------------------- D^T Z
// Block = one genome line that holds a listed locus x one stretch of individuals
// (blockIdx.y); wave v owns words 4v..4v+3 and lane = locus within the word, so every locus
// of the line has one owner.  Tiles of GEA_TI individuals are staged in LDS: their 16 words
// per homologue and their predictors (e of layer lyr, x, y, widened to fp64); every lane reads
// the same entries (broadcasts).  P[stretch][line][1024 loci][3].
__global__ void __launch_bounds__(256)
k_gea_cross(int64_t n, int64_t per_chunk, int W64, int64_t cap, int lyr,
            const int32_t* __restrict__ rows, const int64_t* __restrict__ slots,
            const int32_t* __restrict__ lines, const u64* __restrict__ G, GnxHalves H,
            const float* __restrict__ e, const float* __restrict__ x,
            const float* __restrict__ y, double* __restrict__ P) {
  __shared__ u64 Ws[GEA_TI][2][GEA_LW];
  __shared__ double Zs[GEA_TI][3];
  const int tid = threadIdx.x, lane = tid & 63, v = tid >> 6;
  const int wg = lines[blockIdx.x] * GEA_LW;
  const int64_t i_begin = (int64_t)blockIdx.y * per_chunk;
  const int64_t i_end = min(n, i_begin + per_chunk);
  double acc[4][3];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[u][c] = 0.0;
  for (int64_t t0 = i_begin; t0 < i_end; t0 += GEA_TI) {
    const int tn = (int)min((int64_t)GEA_TI, i_end - t0);
    __syncthreads();
    for (int q = tid; q < GEA_TI * 2 * GEA_LW; q += 256) {
      const int j = q >> 5, hh = (q >> 4) & 1, w = q & 15;
      u64 g = 0;
      if (j < tn && wg + w < W64) g = G[gnx_word_at(H, (int64_t)rows[t0 + j] * 2 + hh, wg + w)];
      Ws[j][hh][w] = g;
    }
    for (int q = tid; q < GEA_TI * 3; q += 256) {
      const int j = q / 3, c = q - j * 3;
      double z = 0.0;
      if (j < tn) {
        const int64_t sl = slots ? slots[t0 + j] : t0 + j;
        z = (double)(c == 0 ? e[(int64_t)lyr * cap + sl] : c == 1 ? x[sl] : y[sl]);
      }
      Zs[j][c] = z;
    }
    __syncthreads();
    for (int j = 0; j < tn; ++j) {
      const double z0 = Zs[j][0], z1 = Zs[j][1], z2 = Zs[j][2];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const u64 a = Ws[j][0][4 * v + u], b = Ws[j][1][4 * v + u];
        const double d = (double)((int)((a >> lane) & 1ull) + (int)((b >> lane) & 1ull));
        acc[u][0] += d * z0;
        acc[u][1] += d * z1;
        acc[u][2] += d * z2;
      }
    }
  }
  double* out = P + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (GEA_LW * 64 * 3);
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int c = 0; c < 3; ++c) out[((4 * v + u) * 64 + lane) * 3 + c] = acc[u][c];
}

// DtZ[q][c] = the stretches' partial sums of locus loci[q], added in stretch order
__global__ void k_gea_cross_sum(int n_loci, int chunks, int n_lines,
                                const int32_t* __restrict__ loci,
                                const int32_t* __restrict__ line_pos,
                                const double* __restrict__ P, double* __restrict__ DtZ) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_loci * 3) return;
  const int q = t / 3, c = t - q * 3;
  const int l = loci[q];
  const int64_t at = ((int64_t)line_pos[l >> 10] * (GEA_LW * 64) + (l & 1023)) * 3 + c;
  double s = 0.0;
  for (int k = 0; k < chunks; ++k) s += P[(int64_t)k * n_lines * (GEA_LW * 64 * 3) + at];
  DtZ[t] = s;
}

// The predictors' own products: thread t of GEA_ZB x 256 adds individuals t, t + 65536, ...
// in that order, the block adds its threads by a fixed tree; part[block][9] = z0 z0, z0 z1,
// z0 z2, z1 z1, z1 z2, z2 z2, z0, z1, z2.  The host adds the GEA_ZB rows in order.
__global__ void __launch_bounds__(256)
k_gea_zsums(int64_t n, int64_t cap, int lyr, const int64_t* __restrict__ slots,
            const float* __restrict__ e, const float* __restrict__ x,
            const float* __restrict__ y, double* __restrict__ part) {
  __shared__ double red[256][9];
  const int tid = threadIdx.x;
  double a[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) a[c] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)GEA_ZB * 256) {
    const int64_t sl = slots ? slots[i] : i;
    const double z0 = (double)e[(int64_t)lyr * cap + sl], z1 = (double)x[sl],
                 z2 = (double)y[sl];
    a[0] += z0 * z0;
    a[1] += z0 * z1;
    a[2] += z0 * z2;
    a[3] += z1 * z1;
    a[4] += z1 * z2;
    a[5] += z2 * z2;
    a[6] += z0;
    a[7] += z1;
    a[8] += z2;
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) red[tid][c] = a[c];
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d)
#pragma unroll
      for (int c = 0; c < 9; ++c) red[tid][c] += red[tid + d][c];
    __syncthreads();
  }
  if (tid < 9) part[blockIdx.x * 9 + tid] = red[0][tid];
}

namespace {

// the listed loci on the device and the genome lines they touch
struct LocusList {
  int32_t* d_loci = nullptr;
  int32_t* d_lines = nullptr;     // lines that hold a listed locus, ascending
  int32_t* d_line_pos = nullptr;  // [all lines] position in d_lines, or -1
  u64* d_wmask = nullptr;         // [all lines * 16] the listed loci of each word
  int32_t* d_qbase = nullptr;     // [all lines * 16] list position of a word's first locus
  int n_lines = 0;
};

int locus_list(gnx_state* h, const char* who, int32_t n_loci, const int32_t* loci, GnxScratch& s,
               LocusList& ll) {
  if (n_loci < 1 || n_loci > 8192 || !loci) {
    gnx_set_error("%s: 1..8192 loci per call (the matrix is n_loci x n_loci)", who);
    return 1;
  }
  for (int q = 0; q < n_loci; ++q)
    if (loci[q] < 0 || loci[q] >= h->cfg.L || (q > 0 && loci[q] <= loci[q - 1])) {
      gnx_set_error("%s: loci must be ascending, distinct and in 0..L-1", who);
      return 1;
    }
  const int all_lines = (h->W64 + GEA_LW - 1) / GEA_LW;
  std::vector<u64> wmask((size_t)all_lines * GEA_LW, 0ull);
  std::vector<int32_t> qbase((size_t)all_lines * GEA_LW, 0), line_pos(all_lines, -1), lines;
  for (int q = 0; q < n_loci; ++q) {
    const int w = loci[q] >> 6;
    if (wmask[w] == 0ull) qbase[w] = q;
    wmask[w] |= 1ull << (loci[q] & 63);
    if (line_pos[w / GEA_LW] < 0) {
      line_pos[w / GEA_LW] = (int32_t)lines.size();
      lines.push_back(w / GEA_LW);
    }
  }
  ll.n_lines = (int)lines.size();
  GNXCHK(s.get(&ll.d_loci, (size_t)n_loci));
  GNXCHK(s.get(&ll.d_lines, lines.size()));
  GNXCHK(s.get(&ll.d_line_pos, line_pos.size()));
  GNXCHK(s.get(&ll.d_wmask, wmask.size()));
  GNXCHK(s.get(&ll.d_qbase, qbase.size()));
  GNXCHK(gnx_h2d(h, ll.d_loci, loci, (size_t)n_loci * sizeof(int32_t)));
  GNXCHK(gnx_h2d(h, ll.d_lines, lines.data(), lines.size() * sizeof(int32_t)));
  GNXCHK(gnx_h2d(h, ll.d_line_pos, line_pos.data(), line_pos.size() * sizeof(int32_t)));
  GNXCHK(gnx_h2d(h, ll.d_wmask, wmask.data(), wmask.size() * sizeof(u64)));
  GNXCHK(gnx_h2d(h, ll.d_qbase, qbase.data(), qbase.size() * sizeof(int32_t)));
  return 0;
}

}  // namespace

extern "C" int gnx_geno_locus_gram(gnx_state* h, int32_t n_loci, const int32_t* loci, int64_t n,
                                   const int64_t* slots, int64_t* C, int64_t* s_out) {
  const char* who = "gnx_geno_locus_gram";
  GNXCHK(geno_ready(h, who));
  if (n < 1 || n > (1ll << 29)) {       // 4 n fits the tile kernel's int32 accumulators
    gnx_set_error("%s: 1..2^29 individuals per call", who);
    return 1;
  }
  GnxScratch s(who);
  LocusList ll;
  GNXCHK(locus_list(h, who, n_loci, loci, s, ll));
  if (!C || !s_out) {
    gnx_set_error("%s: null output", who);
    return 1;
  }
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  const int64_t n_tiles = (n + 63) / 64;                                   // words of 64 individuals
  const int Wm = (int)((n_tiles + GRAM_GK - 1) / GRAM_GK * GRAM_GK);
  const int64_t nl_pad = (n_loci + 63) / 64 * 64;
  u64* XT = nullptr;
  int64_t *d_C = nullptr, *d_s = nullptr;
  GNXCHK(s.get(&XT, (size_t)nl_pad * 2 * Wm));
  GNXCHK(s.get(&d_C, (size_t)n_loci * n_loci));
  GNXCHK(s.get(&d_s, (size_t)n_loci));
  // the padding (loci past n_loci, words past the last individual) must read as 0
  HIPCHK(hipMemsetAsync(XT, 0, (size_t)nl_pad * 2 * Wm * sizeof(u64), h->stream));
  hipLaunchKernelGGL(k_gea_transpose, dim3((unsigned)n_tiles, ll.n_lines), dim3(256), 0,
                     h->stream, n, h->W64, Wm, d_rows, ll.d_lines, ll.d_wmask, ll.d_qbase,
                     (const u64*)h->G, gnx_halves(h), XT);
  hipLaunchKernelGGL(k_gea_colsum, dim3((n_loci + 3) / 4), dim3(256), 0, h->stream, n_loci, Wm,
                     XT, d_s);
  const int T = (int)(nl_pad / 64);
  hipLaunchKernelGGL(k_geno_gram, dim3(T, T), dim3(256), 0, h->stream, (int64_t)n_loci, Wm, XT,
                     d_C);
  HIPCHK(hipGetLastError());
  GNXCHK(gnx_d2h(h, s_out, d_s, (size_t)n_loci * sizeof(int64_t)));
  return gnx_d2h(h, C, d_C, (size_t)n_loci * n_loci * sizeof(int64_t));
}

extern "C" int gnx_geno_locus_cross(gnx_state* h, int32_t n_loci, const int32_t* loci,
                                    int32_t lyr, int64_t n, const int64_t* slots, double* DtZ,
                                    double* ZtZ, double* Zt1) {
  const char* who = "gnx_geno_locus_cross";
  GNXCHK(geno_ready(h, who));
  if (n < 1 || lyr < 0 || lyr >= h->cfg.n_layers) {
    gnx_set_error("%s: n >= 1 and a layer in 0..%d", who, h->cfg.n_layers - 1);
    return 1;
  }
  GnxScratch s(who);
  LocusList ll;
  GNXCHK(locus_list(h, who, n_loci, loci, s, ll));
  if (!DtZ || !ZtZ || !Zt1) {
    gnx_set_error("%s: null output", who);
    return 1;
  }
  int32_t* d_rows = nullptr;
  int64_t* d_slots = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows, &d_slots));
  const GnxSoA a = h->soa[h->cur];
  const int64_t cap = h->cfg.cap_inds;
  // enough blocks to fill the device (~2048), each stretch at least one tile of individuals
  const int64_t tiles = (n + GEA_TI - 1) / GEA_TI;
  const int chunks = (int)std::min<int64_t>(std::min<int64_t>(tiles, 32),
                                            std::max(1, 2048 / ll.n_lines));
  const int64_t per_chunk = (tiles + chunks - 1) / chunks * GEA_TI;
  double *P = nullptr, *d_DtZ = nullptr, *d_part = nullptr;
  GNXCHK(s.get(&P, (size_t)chunks * ll.n_lines * GEA_LW * 64 * 3));
  GNXCHK(s.get(&d_DtZ, (size_t)n_loci * 3));
  GNXCHK(s.get(&d_part, (size_t)GEA_ZB * 9));
  hipLaunchKernelGGL(k_gea_cross, dim3(ll.n_lines, chunks), dim3(256), 0, h->stream, n, per_chunk,
                     h->W64, cap, lyr, d_rows, d_slots, ll.d_lines, (const u64*)h->G,
                     gnx_halves(h), a.e, a.x, a.y, P);
  hipLaunchKernelGGL(k_gea_cross_sum, dim3(gnx_grid((int64_t)n_loci * 3, 256)), dim3(256), 0,
                     h->stream, n_loci, chunks, ll.n_lines, ll.d_loci, ll.d_line_pos, P, d_DtZ);
  hipLaunchKernelGGL(k_gea_zsums, dim3(GEA_ZB), dim3(256), 0, h->stream, n, cap, lyr, d_slots,
                     a.e, a.x, a.y, d_part);
  HIPCHK(hipGetLastError());
  std::vector<double> part((size_t)GEA_ZB * 9);
  GNXCHK(gnx_d2h(h, part.data(), d_part, part.size() * sizeof(double)));
  double z[9] = {};
  for (int b = 0; b < GEA_ZB; ++b)
    for (int c = 0; c < 9; ++c) z[c] += part[(size_t)b * 9 + c];
  const double zz[3][3] = {{z[0], z[1], z[2]}, {z[1], z[3], z[4]}, {z[2], z[4], z[5]}};
  for (int r = 0; r < 3; ++r) {
    Zt1[r] = z[6 + r];
    for (int c = 0; c < 3; ++c) ZtZ[r * 3 + c] = zz[r][c];
  }
  return gnx_d2h(h, DtZ, d_DtZ, (size_t)n_loci * 3 * sizeof(double));
}
