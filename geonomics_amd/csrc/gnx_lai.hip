// Local ancestry along the genome: the linkage model of Falush, Stephens & Pritchard (2003) with
// the ancestral allele frequencies held fixed and one admixture time, painted along every phased
// haplotype of the sample by the forward-backward recurrences of a hidden Markov model over the
// bit-packed genomes.  The reference has no such analysis (nor any haplotype analysis): this is
// an extension beside gnx_admix_sweep, whose frequencies it takes.  The model, the order of every
// operation and every output are stated in include/gnx_hip.h; geonomics_amd/sim/lai.py restates
// them in numpy (brute_paint) and holds what surrounds the call.
//
//   gnx_lai_paint   host buffers in, host buffers out
//
// The chain over the loci is sequential, so a thread is a haplotype and a wave 64 of them; the
// haplotypes are worked off in batches (a multiple of 64) whose posteriors fit the byte budget.
//
// k_lai_fwd<K, STORE>: one wave per workgroup.  Per stage of 64 used loci the lanes put f, g =
// 1 - f, sw, stay and the locus number in LDS, then every lane reads the same entry (a
// broadcast); the lane's own genome word comes through the block table whenever the stage moves
// to another word (once per 64 loci when all are used).  alpha and q stay in registers; the
// normalised alpha goes to S [L_u][K][batch], haplotype-fastest, so that a wave's store is one
// 512-byte line; ln c is summed per haplotype.  STORE = false (want_post == 0) writes nothing
// but the log-likelihood.
// k_lai_bwd<K, CALLS>: the same stages in descending order; reads alpha from S and writes gamma
// over it, sums gamma per haplotype (descending l), takes the hard call and counts the switches;
// the calls go to CT [L_u][batch] bytes, haplotype-fastest.
// k_lai_locus: thread = one (locus, k) row of S; a wave stages a 64 x 32 tile of S through LDS
// (coalesced along the haplotypes) and every lane adds its row's 32 values in ascending t to the
// running sum of the haplotype's group, kept in LDS [groups][64] and carried from batch to batch
// in the output buffer: the order of every sum is ascending t whatever the budget.
// k_lai_calls_t: CT [L_u][batch] -> calls [batch][L_u] through a 64 x 64 LDS tile.
// No floating-point atomics anywhere; a call repeated is bit-equal in every output.
#include <cmath>
#include "gnx_geno.h"

#define LAI_KMAX 8
#define LAI_GMAX 64
#define LAI_TC 32                  // haplotypes per LDS stage of k_lai_locus
#define LAI_BUDGET (4ll << 30)     // bytes of posteriors (and calls) per batch unless the caller says so

// see the head of the file.  The batch is haplotypes t0 .. t0 + cnt - 1 of the sample; S has
// pitch nb (a multiple of 64) haplotypes
template <int K, bool STORE>
__global__ void __launch_bounds__(64)
k_lai_fwd(int64_t t0, int64_t cnt, int64_t nb, int L_u, const int32_t* __restrict__ loci,
          const int32_t* __restrict__ rows, const u64* __restrict__ G, GnxHalves H,
          const double* __restrict__ F, const double* __restrict__ sw,
          const double* __restrict__ stay, const double* __restrict__ Q,
          double* __restrict__ S, double* __restrict__ loglik) {
  __shared__ double Fs[64][K], Gs[64][K], SWs[64], STs[64];
  __shared__ int32_t Ls[64];
  const int lane = threadIdx.x;
  const int64_t tl = (int64_t)blockIdx.x * 64 + lane;         // within the batch
  const bool live = tl < cnt;
  const int64_t t = t0 + (live ? tl : 0);
  const int64_t lh = (int64_t)rows[t >> 1] * 2 + (t & 1);
  double q[K], a[K];
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = q[k] = Q[(t >> 1) * K + k];
  double ll = 0.0;
  int cur_w = -1;
  u64 word = 0;
  for (int j0 = 0; j0 < L_u; j0 += 64) {
    const int jn = min(64, L_u - j0);
    __syncthreads();                                          // the last stage is read
    if (lane < jn) {
      const int j = j0 + lane;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double f = F[(int64_t)j * K + k];
        Fs[lane][k] = f;
        Gs[lane][k] = 1.0 - f;
      }
      SWs[lane] = sw[j];
      STs[lane] = stay[j];
      Ls[lane] = loci ? loci[j] : j;
    }
    __syncthreads();
    for (int jj = 0; jj < jn; ++jj) {
      const int l = Ls[jj];
      if ((l >> 6) != cur_w) {                                // wave-uniform
        cur_w = l >> 6;
        word = G[gnx_word_at(H, lh, cur_w)];
      }
      const bool one = (word >> (l & 63)) & 1ull;
      const double s_l = SWs[jj], st_l = STs[jj];
      double b[K];
      double c = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        b[k] = (st_l * a[k] + s_l * q[k]) * (one ? Fs[jj][k] : Gs[jj][k]);
        c = k ? c + b[k] : b[k];
      }
#pragma unroll
      for (int k = 0; k < K; ++k) a[k] = b[k] / c;
      ll += log(c);
      if (STORE && live) {
        double* out = S + (int64_t)(j0 + jj) * K * nb + tl;
#pragma unroll
        for (int k = 0; k < K; ++k) out[(int64_t)k * nb] = a[k];
      }
    }
  }
  if (live) loglik[t] = ll;
}

// see the head of the file.  anc_hap [2n][K], switches [2n]; CT [L_u][nb] (CALLS only)
template <int K, bool CALLS>
__global__ void __launch_bounds__(64)
k_lai_bwd(int64_t t0, int64_t cnt, int64_t nb, int L_u, const int32_t* __restrict__ loci,
          const int32_t* __restrict__ rows, const u64* __restrict__ G, GnxHalves H,
          const double* __restrict__ F, const double* __restrict__ sw,
          const double* __restrict__ stay, const double* __restrict__ Q,
          double* __restrict__ S, double* __restrict__ anc_hap, int32_t* __restrict__ switches,
          uint8_t* __restrict__ CT) {
  __shared__ double Fs[64][K], Gs[64][K], SWs[64], STs[64];
  __shared__ int32_t Ls[64];
  const int lane = threadIdx.x;
  const int64_t tl = (int64_t)blockIdx.x * 64 + lane;
  const bool live = tl < cnt;
  const int64_t t = t0 + (live ? tl : 0);
  const int64_t tc = live ? tl : 0;                           // (a dead lane reads column 0)
  const int64_t lh = (int64_t)rows[t >> 1] * 2 + (t & 1);
  double q[K], be[K], acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    q[k] = Q[(t >> 1) * K + k];
    be[k] = 1.0;
    acc[k] = 0.0;
  }
  int cur_w = -1, prev_call = -1, n_sw = 0;
  u64 word = 0;
  double al[K];                                               // alpha of the locus at hand
#pragma unroll
  for (int k = 0; k < K; ++k) al[k] = S[((int64_t)(L_u - 1) * K + k) * nb + tc];
  const int last0 = (L_u - 1) / 64 * 64;
  for (int j0 = last0; j0 >= 0; j0 -= 64) {
    const int jn = min(64, L_u - j0);
    __syncthreads();
    if (lane < jn) {
      const int j = j0 + lane;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double f = F[(int64_t)j * K + k];
        Fs[lane][k] = f;
        Gs[lane][k] = 1.0 - f;
      }
      SWs[lane] = sw[j];
      STs[lane] = stay[j];
      Ls[lane] = loci ? loci[j] : j;
    }
    __syncthreads();
    for (int jj = jn - 1; jj >= 0; --jj) {
      const int j = j0 + jj;
      const int l = Ls[jj];
      if ((l >> 6) != cur_w) {                                // wave-uniform
        cur_w = l >> 6;
        word = G[gnx_word_at(H, lh, cur_w)];
      }
      const bool one = (word >> (l & 63)) & 1ull;
      double* col = S + (int64_t)j * K * nb + tc;
      double p[K];
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        p[k] = al[k] * be[k];
        s = k ? s + p[k] : p[k];
      }
      if (j > 0) {                                            // the next locus' alpha, a step ahead
#pragma unroll
        for (int k = 0; k < K; ++k) al[k] = col[((int64_t)k - K) * nb];
      }
      double best = 0.0;
      int call = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double g = p[k] / s;
        if (live) col[(int64_t)k * nb] = g;
        acc[k] += g;
        if (k == 0 || g > best) {
          best = g;
          call = k;
        }
      }
      if (prev_call >= 0 && call != prev_call) ++n_sw;
      prev_call = call;
      if (CALLS && live) CT[(int64_t)j * nb + tl] = (uint8_t)call;
      if (j > 0) {
        const double s_l = SWs[jj], st_l = STs[jj];
        double w[K];
        double u = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          w[k] = be[k] * (one ? Fs[jj][k] : Gs[jj][k]);
          const double qw = q[k] * w[k];
          u = k ? u + qw : qw;
        }
        double sn = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          w[k] = st_l * w[k] + s_l * u;
          sn = k ? sn + w[k] : w[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) be[k] = w[k] / sn;
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int k = 0; k < K; ++k) anc_hap[t * K + k] = acc[k];
  switches[t] = n_sw;
}

// see the head of the file.  n_rows = L_u * K rows of S (pitch nb); out [n_g][n_rows] holds the
// sums of the batches before this one (first: they are taken as 0); by [n] or null (one group).
// Dynamic LDS: tile [64][LAI_TC + 1] and sums [n_g][64] doubles, then LAI_TC labels (under 50 KB
// at 64 groups)
__global__ void __launch_bounds__(64)
k_lai_locus(int64_t t0, int64_t cnt, int64_t nb, int64_t n_rows, int n_g, int first,
            const int32_t* __restrict__ by, const double* __restrict__ S,
            double* __restrict__ out) {
  extern __shared__ double lai_lds[];
  double* tile = lai_lds;                                     // [64][LAI_TC + 1]
  double* sums = lai_lds + 64 * (LAI_TC + 1);                 // [n_g][64]
  int32_t* lab = (int32_t*)(sums + (size_t)n_g * 64);         // [LAI_TC]
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int rn = (int)min((int64_t)64, n_rows - r0);
  const bool have = lane < rn;
  for (int g = 0; g < n_g; ++g)
    sums[g * 64 + lane] = (first || !have) ? 0.0 : out[(int64_t)g * n_rows + r0 + lane];
  const int cc = lane & (LAI_TC - 1), rsub = lane / LAI_TC;   // two rows of the tile per load
  for (int64_t c0 = 0; c0 < cnt; c0 += LAI_TC) {
    const int cn = (int)min((int64_t)LAI_TC, cnt - c0);
    __syncthreads();
    for (int r = 0; r < rn; r += 64 / LAI_TC) {
      const int rr = r + rsub;
      if (rr < rn) tile[rr * (LAI_TC + 1) + cc] = cc < cn ? S[(r0 + rr) * nb + c0 + cc] : 0.0;
    }
    if (lane < cn) lab[lane] = by ? by[(t0 + c0 + lane) >> 1] : 0;
    __syncthreads();
    if (!have) continue;                                      // (the bounds above are uniform)
    for (int c = 0; c < cn; ++c) {
      const int g = lab[c];                                   // a broadcast
      if (g >= 0) sums[g * 64 + lane] += tile[lane * (LAI_TC + 1) + c];
    }
  }
  if (!have) return;
  for (int g = 0; g < n_g; ++g) out[(int64_t)g * n_rows + r0 + lane] = sums[g * 64 + lane];
}

// C [cnt][L_u] = the transpose of CT [L_u][nb] (bytes)
__global__ void __launch_bounds__(256)
k_lai_calls_t(int64_t cnt, int64_t nb, int L_u, const uint8_t* __restrict__ CT,
              uint8_t* __restrict__ C) {
  __shared__ uint8_t tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)blockIdx.y * 64;
  const int j0 = blockIdx.x * 64;
  for (int r = ty; r < 64; r += 4) {
    const int j = j0 + r;
    tile[r][tx] = (j < L_u && c0 + tx < cnt) ? CT[(int64_t)j * nb + c0 + tx] : 0;
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int64_t c = c0 + r;
    if (c < cnt && j0 + tx < L_u) C[c * L_u + j0 + tx] = tile[tx][r];
  }
}

namespace {

struct LaiArgs {
  gnx_state* h;
  int64_t t0, cnt, nb;
  int L_u;
  const int32_t *loci, *rows;
  const double *F, *sw, *stay, *Q;
  double *S, *loglik, *anc_hap;
  int32_t* switches;
  uint8_t* CT;
  bool post, calls;
};

// the passes over one batch with K as the template instance
template <int K>
void lai_launch(const LaiArgs& a) {
  gnx_state* h = a.h;
  const GnxHalves H = gnx_halves(h);
  const dim3 grid((unsigned)((a.cnt + 63) / 64)), block(64);
  const u64* G = (const u64*)h->G;
  if (!a.post) {
    hipLaunchKernelGGL((k_lai_fwd<K, false>), grid, block, 0, h->stream, a.t0, a.cnt, a.nb, a.L_u,
                       a.loci, a.rows, G, H, a.F, a.sw, a.stay, a.Q, a.S, a.loglik);
    return;
  }
  hipLaunchKernelGGL((k_lai_fwd<K, true>), grid, block, 0, h->stream, a.t0, a.cnt, a.nb, a.L_u,
                     a.loci, a.rows, G, H, a.F, a.sw, a.stay, a.Q, a.S, a.loglik);
  if (a.calls)
    hipLaunchKernelGGL((k_lai_bwd<K, true>), grid, block, 0, h->stream, a.t0, a.cnt, a.nb, a.L_u,
                       a.loci, a.rows, G, H, a.F, a.sw, a.stay, a.Q, a.S, a.anc_hap, a.switches,
                       a.CT);
  else
    hipLaunchKernelGGL((k_lai_bwd<K, false>), grid, block, 0, h->stream, a.t0, a.cnt, a.nb, a.L_u,
                       a.loci, a.rows, G, H, a.F, a.sw, a.stay, a.Q, a.S, a.anc_hap, a.switches,
                       a.CT);
}

void lai_dispatch(int K, const LaiArgs& a) {
  switch (K) {
#define LAI_CASE(k) case k: lai_launch<k>(a); break;
    LAI_CASE(1) LAI_CASE(2) LAI_CASE(3) LAI_CASE(4) LAI_CASE(5) LAI_CASE(6) LAI_CASE(7)
    LAI_CASE(8)
#undef LAI_CASE
  }
}

}  // namespace

extern "C" int gnx_lai_paint(gnx_state* h, int64_t n, const int64_t* slots, int32_t K,
                             int32_t L_u, const int32_t* loci, const double* F, const double* sw,
                             const double* stay, const double* Q, const int32_t* by,
                             int32_t n_groups, int64_t budget, int32_t want_post,
                             int32_t want_calls, double* loglik, double* anc_hap,
                             double* anc_locus, int32_t* switches, uint8_t* calls,
                             int64_t* batches, double* kernel_ms) {
  const char* who = "gnx_lai_paint";
  if (batches) *batches = 0;
  if (kernel_ms) *kernel_ms = 0.0;
  GNXCHK(geno_ready(h, who));
  const int L = h->cfg.L;
  if (K < 1 || K > LAI_KMAX) {
    gnx_set_error("%s: 1 <= K <= %d (got %d)", who, LAI_KMAX, K);
    return 1;
  }
  if (n < 1 || n > (1ll << 30)) {
    gnx_set_error("%s: 1..2^30 individuals (n = %lld)", who, (long long)n);
    return 1;
  }
  if (L_u < 1 || L_u > L) {
    gnx_set_error("%s: 1 <= L_u <= L = %d (got %d)", who, L, L_u);
    return 1;
  }
  if (!loci && L_u != L) {
    gnx_set_error("%s: L_u = %d but the genome has %d loci (loci == null)", who, L_u, L);
    return 1;
  }
  for (int j = 0; loci && j < L_u; ++j)
    if (loci[j] < 0 || loci[j] >= L || (j > 0 && loci[j] <= loci[j - 1])) {
      gnx_set_error("%s: loci ascending in 0..%d (entry %d: %d)", who, L - 1, j, loci[j]);
      return 1;
    }
  if (n_groups < 0 || n_groups > LAI_GMAX) {
    gnx_set_error("%s: 0 <= n_groups <= %d (got %d)", who, LAI_GMAX, n_groups);
    return 1;
  }
  const int n_g = std::max(n_groups, 1);
  for (int64_t i = 0; by && i < n; ++i)
    if (by[i] < -1 || by[i] >= n_g) {
      gnx_set_error("%s: labels in -1..%d (individual %lld: %d)", who, n_g - 1, (long long)i,
                    by[i]);
      return 1;
    }
  const bool post = want_post != 0, wc = post && want_calls != 0;
  if (!F || !sw || !stay || !Q || !loglik ||
      (post && (!anc_hap || !anc_locus || !switches)) || (want_calls && (!post || !calls))) {
    gnx_set_error("%s: null F, sw, stay, Q or output (anc_hap, anc_locus and switches go with "
                  "want_post, calls with want_post and want_calls)", who);
    return 1;
  }
  if (budget < 0) {
    gnx_set_error("%s: budget >= 0 (0: the default)", who);
    return 1;
  }
  // ---- the batches over the haplotypes: the posteriors (and calls) of one batch under the budget
  const int64_t T = 2 * n, T_pad = (T + 63) / 64 * 64;
  const int64_t per = (int64_t)L_u * K * 8 + (wc ? 2 * (int64_t)L_u : 0);   // bytes per haplotype
  int64_t nb = T_pad;
  if (post) {
    const int64_t cap = budget > 0 ? budget : LAI_BUDGET;
    nb = std::min(T_pad, cap / per / 64 * 64);
    if (nb < 64) {
      gnx_set_error("%s: a budget of %lld bytes cannot hold 64 haplotypes (%lld bytes each)", who,
                    (long long)cap, (long long)per);
      return 1;
    }
  }
  const int64_t n_batches = (T + nb - 1) / nb;
  const int64_t n_rows = (int64_t)L_u * K;

  GnxScratch s(who);
  int32_t *d_rows = nullptr, *d_loci = nullptr, *d_by = nullptr, *d_sw_n = nullptr;
  double *d_F = nullptr, *d_sw = nullptr, *d_stay = nullptr, *d_Q = nullptr, *d_ll = nullptr,
         *d_S = nullptr, *d_ah = nullptr, *d_al = nullptr;
  uint8_t *d_CT = nullptr, *d_C = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  GNXCHK(s.get(&d_F, (size_t)n_rows));
  GNXCHK(s.get(&d_sw, (size_t)L_u));
  GNXCHK(s.get(&d_stay, (size_t)L_u));
  GNXCHK(s.get(&d_Q, (size_t)n * K));
  GNXCHK(s.get(&d_ll, (size_t)T));
  GNXCHK(gnx_h2d(h, d_F, F, (size_t)n_rows * sizeof(double)));
  GNXCHK(gnx_h2d(h, d_sw, sw, (size_t)L_u * sizeof(double)));
  GNXCHK(gnx_h2d(h, d_stay, stay, (size_t)L_u * sizeof(double)));
  GNXCHK(gnx_h2d(h, d_Q, Q, (size_t)n * K * sizeof(double)));
  if (loci) {
    GNXCHK(s.get(&d_loci, (size_t)L_u));
    GNXCHK(gnx_h2d(h, d_loci, loci, (size_t)L_u * sizeof(int32_t)));
  }
  if (post) {
    GNXCHK(s.get(&d_S, (size_t)n_rows * nb));
    GNXCHK(s.get(&d_ah, (size_t)T * K));
    GNXCHK(s.get(&d_al, (size_t)n_g * n_rows));
    GNXCHK(s.get(&d_sw_n, (size_t)T));
    if (by) {
      GNXCHK(s.get(&d_by, (size_t)n));
      GNXCHK(gnx_h2d(h, d_by, by, (size_t)n * sizeof(int32_t)));
    }
  }
  if (wc) {
    GNXCHK(s.get(&d_CT, (size_t)L_u * nb));
    GNXCHK(s.get(&d_C, (size_t)L_u * nb));
  }
  double ms = 0.0;
  int64_t n_launch = 0;
  GnxCallTimer tm(h, &ms, &n_launch);
  LaiArgs a;
  a.h = h;
  a.nb = nb;
  a.L_u = L_u;
  a.loci = d_loci;
  a.rows = d_rows;
  a.F = d_F;
  a.sw = d_sw;
  a.stay = d_stay;
  a.Q = d_Q;
  a.S = d_S;
  a.loglik = d_ll;
  a.anc_hap = d_ah;
  a.switches = d_sw_n;
  a.CT = d_CT;
  a.post = post;
  a.calls = wc;
  const size_t lds = ((size_t)64 * (LAI_TC + 1) + (size_t)n_g * 64) * sizeof(double) +
                     LAI_TC * sizeof(int32_t);
  for (int64_t b = 0; b < n_batches; ++b) {
    a.t0 = b * nb;
    a.cnt = std::min(nb, T - a.t0);
    int64_t launches = 1;
    tm.start();
    lai_dispatch(K, a);
    if (post) {
      hipLaunchKernelGGL(k_lai_locus, dim3((unsigned)((n_rows + 63) / 64)), dim3(64), lds,
                         h->stream, a.t0, a.cnt, nb, n_rows, n_g, (int)(b == 0), d_by, d_S, d_al);
      launches += 2;
    }
    if (wc) {
      hipLaunchKernelGGL(k_lai_calls_t, dim3((unsigned)((L_u + 63) / 64),
                                             (unsigned)((a.cnt + 63) / 64)),
                         dim3(256), 0, h->stream, a.cnt, nb, L_u, d_CT, d_C);
      ++launches;
    }
    HIPCHK(hipGetLastError());
    GNXCHK(tm.stop(launches));
    if (wc) GNXCHK(gnx_d2h(h, calls + a.t0 * L_u, d_C, (size_t)a.cnt * L_u));
  }
  if (batches) *batches = n_batches;
  if (kernel_ms) *kernel_ms = ms;
  GNXCHK(gnx_d2h(h, loglik, d_ll, (size_t)T * sizeof(double)));
  if (!post) return 0;
  GNXCHK(gnx_d2h(h, anc_hap, d_ah, (size_t)T * K * sizeof(double)));
  GNXCHK(gnx_d2h(h, anc_locus, d_al, (size_t)n_g * n_rows * sizeof(double)));
  return gnx_d2h(h, switches, d_sw_n, (size_t)T * sizeof(int32_t));
}
