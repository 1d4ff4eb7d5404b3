// Identity tracts of the phased genomes on the device: runs of homozygosity per individual
// (homologue 0 against homologue 1) and tracts shared between the haplotypes of two individuals,
// as include/gnx_hip.h defines them.  Everything returned is an integer function of the
// qualifying tracts, so integer atomics are used freely: every output is exact whatever the order.
//
//   gnx_tracts_self    per [n][4], hist [n_edges - 1][2], cover [L]       1..2^25 individuals
//   gnx_tracts_pairs   cnt, len, longest [n][n], hist, cover, work        1..4096 individuals
//
// The scanner.  Z = ~(a xor b) masked to the loci (padding bits are 0: never in a tract), B = the
// break word.  The state carried from word to word is the start of the tract that is open at the
// word's last bit, or -1.  tract_step consumes one word: it closes the carried tract at the
// word's first bit when that bit differs or is a break, and hands every tract that ends inside
// the word to `emit`; it returns the new state.  An all-equal word without a break is O(1); with
// min_loci >= 63 (`fast`, uniform per launch) and no break inside the word a word with
// differences is O(1) too - a run that neither touches bit 0 nor bit 63 has at most 62 loci and
// cannot qualify, so ctz closes the carried tract and clz opens the next; otherwise the runs of
// the word are walked one ctz at a time.  A virtual all-different word after the last locus
// closes what is still open, so nothing is special at the end of the genome.
//
// Self scan, k_tract_self: a wave per individual, lanes over 64 consecutive words (512 B per
// homologue and iteration, coalesced), read through the block table.  Where both homologues'
// logical block is the same physical block the block is identical: Z is all ones and nothing is
// loaded.  A lane knows its word's state after it (tract_tail) unless the word is all equal and
// break-free, in which case it hands on what it gets: an inclusive segmented wave scan of
// (state, transparent) gives every lane the state before its word, lane 63's state is carried
// to the wave's next 64 words, and every lane then runs tract_step on its own word.
//
// Pair scan, k_tract_pairs: the operand is k_geno_gather's X (every word, full mask), tiled 64 x 64
// as k_geno_gram, upper triangle of tiles, GRAM_GK words of the tile's rows staged in LDS per
// step (GenoStage and geno_stage_load of gnx_geno.h).  Thread (tx, ty) owns the individual
// pairs (ty + 16 r, tx + 16 c) and keeps their 4 x 16 scanner states in registers across the
// stages: per stage it takes its pairs one after the other (the words of the stage in order) and
// rotates the register file of states by one pair, so the scanner exists once in the code and no
// state is indexed dynamically (no scratch).  A pair's sums go to its [i][j] entry, which only
// this thread touches; k_tract_mirror fills the lower triangle.
//
// hist is collected in LDS per workgroup and flushed with one atomic per bin; cover is an int32
// difference array (+1 at s, -1 at e + 1) summed by k_tract_cover.
#include "gnx_geno.h"

#define TR_NB 64                  // bins at most
#define TR_MAX_SELF (1ll << 25)
#define TR_MAX_PAIRS 4096

namespace {

struct TractCtx {
  const long long* pos;           // [L]
  long long min_len;
  int min_loci;                   // >= 1
  int n_bins;                     // 0: no histogram
  const long long* E;             // LDS: edges [n_bins + 1]
  unsigned long long* Hs;         // LDS: [n_bins][2]
  int* cdiff;                     // [L + 1] or null
};

struct TractAcc {
  long long cnt, loci, len, longest;
};

// a tract s..e has ended: count it if it qualifies
__device__ __forceinline__ void tract_emit(const TractCtx& C, int s, int e, bool binned,
                                           TractAcc& A) {
  const int c = e - s + 1;
  if (c < C.min_loci) return;
  const long long len = C.pos[e] - C.pos[s];
  if (len < C.min_len) return;
  A.cnt += 1;
  A.loci += c;
  A.len += len;
  A.longest = max(A.longest, len);
  if (!binned) return;
  if (C.n_bins > 0 && len >= C.E[0] && len < C.E[C.n_bins]) {
    int lo = 0, hi = C.n_bins;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (len >= C.E[mid]) lo = mid;
      else hi = mid;
    }
    atomicAdd(&C.Hs[2 * lo], 1ull);
    atomicAdd(&C.Hs[2 * lo + 1], (unsigned long long)len);
  }
  if (C.cdiff) {
    atomicAdd(&C.cdiff[s], 1);
    atomicAdd(&C.cdiff[e + 1], -1);
  }
}

// the state after a word that is entered without an open tract: the start of the run that
// reaches bit 63 (cut at the last break inside it), or -1
__device__ __forceinline__ int tract_tail(u64 Z, u64 B, int base) {
  if (!(Z >> 63)) return -1;
  const u64 nz = ~Z;
  const int lo = nz ? 64 - __clzll((long long)nz) : 0;       // first bit of the run
  const u64 bb = lo >= 63 ? 0ull : (B & (~0ull << (lo + 1)));
  if (bb) return base + 63 - __clzll((long long)bb);
  return base + lo;
}

// one word of the scan (see the head of the file); emit(s, e) takes the tracts that end
template <class Emit>
__device__ __forceinline__ int tract_step(int start, u64 Z, u64 B, int base, bool fast,
                                          Emit&& emit) {
  if (start >= 0 && (!(Z & 1ull) || (B & 1ull))) {
    emit(start, base - 1);
    start = -1;
  }
  const u64 Bm = B & ~1ull;
  if (Z == ~0ull && Bm == 0ull) return start >= 0 ? start : base;
  if (Z == 0ull) return -1;
  if (fast && Bm == 0ull) {
    const u64 nz = ~Z;                                        // != 0
    if (Z & 1ull) emit(start >= 0 ? start : base, base + __ffsll((long long)nz) - 2);
    const int u = __clzll((long long)nz);
    return u ? base + 64 - u : -1;
  }
  u64 rem = Z;
  while (rem) {
    const int s = __ffsll((long long)rem) - 1;
    const u64 inv = ~(Z >> s);
    int len = inv ? __ffsll((long long)inv) - 1 : 64;
    const u64 m = (len >= 64 ? ~0ull : ((1ull << len) - 1ull)) << s;
    const u64 bb = Bm & m & ~(1ull << s);
    if (bb) len = __ffsll((long long)bb) - 1 - s;
    const int e = s + len - 1;
    const int as = (s == 0 && start >= 0) ? start : base + s;
    if (e == 63) return as;
    emit(as, base + e);
    start = -1;
    rem &= ~((2ull << e) - 1ull);
  }
  return -1;
}

// the loci of word w as a mask (words past the last locus: 0)
__device__ __forceinline__ u64 tract_valid(int w, int L) {
  const long long left = (long long)L - (long long)w * 64;
  return left >= 64 ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
}

__device__ __forceinline__ long long tr_wave_sum(long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ long long tr_wave_max(long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}

}  // namespace

// per[i][4] of rows[i]'s own pair; hist (global, [n_bins][2]) and cdiff add up over the launch.
// Wv = the words that hold a locus; words[0] += the genome words loaded
__global__ void __launch_bounds__(256)
k_tract_self(int64_t n, const int32_t* __restrict__ rows, const u64* __restrict__ G, GnxHalves H,
             int L, int Wv, const long long* __restrict__ pos, const u64* __restrict__ brk,
             int min_loci, long long min_len, int fast, int n_bins,
             const long long* __restrict__ edges, long long* __restrict__ per,
             unsigned long long* __restrict__ hist, int* __restrict__ cdiff,
             unsigned long long* __restrict__ words) {
  __shared__ long long E[TR_NB + 1];
  __shared__ unsigned long long Hs[TR_NB * 2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid <= n_bins && n_bins > 0) E[tid] = edges[tid];
  if (tid < 2 * TR_NB) Hs[tid] = 0ull;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (i < n) {                                          // wave-uniform
    const TractCtx C{pos, min_len, min_loci, n_bins, E, Hs, cdiff};
    TractAcc A{0, 0, 0, 0};
    auto emit = [&](int s, int e) { tract_emit(C, s, e, true, A); };
    const int64_t lh = (int64_t)rows[i] * 2;
    const int iters = Wv / 64 + 1;                      // words 0 .. Wv at least: the last closes
    int carry = -1;
    long long nread = 0;
    for (int it = 0; it < iters; ++it) {
      const int w = it * 64 + lane, base = w * 64;
      u64 Z = 0ull, B = 0ull;
      if (w < Wv) {
        const int b = w / H.BW;
        u64 D = 0ull;
        if (GNX_BLK(H.hmap[lh * H.NB + b]) != GNX_BLK(H.hmap[(lh + 1) * H.NB + b])) {
          D = G[gnx_word_at(H, lh, w)] ^ G[gnx_word_at(H, lh + 1, w)];
          nread += 2;
        }
        Z = ~D & tract_valid(w, L);
        if (brk) B = brk[w];
      }
      // the state after every lane's word: a segmented scan, transparent words hand on
      bool t = Z == ~0ull && B == 0ull;
      int v = t ? base : tract_tail(Z, B, base);
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int lv = __shfl_up(v, d, 64);
        const int lt = __shfl_up((int)t, d, 64);
        if (lane >= d) {
          if (t && lv >= 0) v = lv;
          t = t && lt;
        }
      }
      const int out = (t && carry >= 0) ? carry : v;
      const int prev = __shfl_up(out, 1, 64);
      (void)tract_step(lane == 0 ? carry : prev, Z, B, base, fast != 0, emit);
      carry = __shfl(out, 63, 64);
    }
    const long long cnt = tr_wave_sum(A.cnt), loci = tr_wave_sum(A.loci);
    const long long len = tr_wave_sum(A.len), longest = tr_wave_max(A.longest);
    nread = tr_wave_sum(nread);
    if (lane == 0) {
      per[i * 4 + 0] = cnt;
      per[i * 4 + 1] = loci;
      per[i * 4 + 2] = len;
      per[i * 4 + 3] = longest;
      if (nread) atomicAdd(words, (unsigned long long)nread);
    }
  }
  __syncthreads();
  if (tid < 2 * n_bins && Hs[tid]) atomicAdd(&hist[tid], Hs[tid]);
}

// X [n rounded up to 64][2][Wm] (k_geno_gather; Wm a multiple of GRAM_GK that leaves at least
// one word past the last locus).  cnt, len, longest [n][n], zeroed: the upper triangle and the
// diagonal are written
__global__ void __launch_bounds__(256)
k_tract_pairs(int64_t n, int Wm, int L, int W64, const u64* __restrict__ X,
              const long long* __restrict__ pos, const u64* __restrict__ brk, int min_loci,
              long long min_len, int fast, int n_bins, const long long* __restrict__ edges,
              int32_t* __restrict__ cnt, long long* __restrict__ len,
              long long* __restrict__ longest, unsigned long long* __restrict__ hist,
              int* __restrict__ cdiff) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;                                // block-uniform
  __shared__ GenoStage S;
  __shared__ u64 Bk[GRAM_GK];
  __shared__ long long E[TR_NB + 1];
  __shared__ unsigned long long Hs[TR_NB * 2];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  if (tid <= n_bins && n_bins > 0) E[tid] = edges[tid];
  if (tid < 2 * TR_NB) Hs[tid] = 0ull;
  const int64_t i0 = (int64_t)ti * 64, j0 = (int64_t)tj * 64;
  const TractCtx C{pos, min_len, min_loci, n_bins, E, Hs, cdiff};
  int st[64];
#pragma unroll
  for (int q = 0; q < 64; ++q) st[q] = -1;
  for (int k0 = 0; k0 < Wm; k0 += GRAM_GK) {
    __syncthreads();                                  // the last stage's words have been read
    geno_stage_load(S, X, Wm, i0, j0, k0);
    if (tid < GRAM_GK) Bk[tid] = (brk && k0 + tid < W64) ? brk[k0 + tid] : 0ull;
    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < 16; ++p) {
      const int r = p >> 2, c = p & 3;
      const int ri = ty + 16 * r, cj = tx + 16 * c;
      const int64_t i = i0 + ri, j = j0 + cj;
      // in a diagonal tile the pair (i, j) also shows up as (j, i): the upper one is taken
      if (i < n && j < n && (ti < tj || i <= j)) {
        const bool own = i == j;                      // (a_0, a_1) only
        TractAcc A{0, 0, 0, 0};
        auto emit = [&](int s, int e) { tract_emit(C, s, e, !own, A); };
        int s0 = st[0], s1 = st[1], s2 = st[2], s3 = st[3];
#pragma unroll 1
        for (int kk = 0; kk < GRAM_GK; ++kk) {
          const int w = k0 + kk, base = w * 64;
          const u64 vm = tract_valid(w, L), B = Bk[kk];
          const u64 a0 = S.A[kk][0][ri], a1 = S.A[kk][1][ri];
          const u64 b0 = S.B[kk][0][cj], b1 = S.B[kk][1][cj];
          s1 = tract_step(s1, ~(a0 ^ b1) & vm, B, base, fast != 0, emit);
          if (!own) {
            s0 = tract_step(s0, ~(a0 ^ b0) & vm, B, base, fast != 0, emit);
            s2 = tract_step(s2, ~(a1 ^ b0) & vm, B, base, fast != 0, emit);
            s3 = tract_step(s3, ~(a1 ^ b1) & vm, B, base, fast != 0, emit);
          }
        }
        st[0] = s0, st[1] = s1, st[2] = s2, st[3] = s3;
        if (A.cnt) {
          const int64_t o = i * n + j;
          cnt[o] += (int32_t)A.cnt;
          len[o] += A.len;
          longest[o] = max(longest[o], A.longest);
        }
      }
      // the next pair's states to the front
      const int t0 = st[0], t1 = st[1], t2 = st[2], t3 = st[3];
#pragma unroll
      for (int q = 0; q < 60; ++q) st[q] = st[q + 4];
      st[60] = t0, st[61] = t1, st[62] = t2, st[63] = t3;
    }
  }
  __syncthreads();
  if (tid < 2 * n_bins && Hs[tid]) atomicAdd(&hist[tid], Hs[tid]);
}

// the lower triangle from the upper
__global__ void k_tract_mirror(int64_t n, int32_t* __restrict__ cnt, long long* __restrict__ len,
                               long long* __restrict__ longest) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * n; t += stride) {
    const int64_t i = t / n, j = t - i * n;
    if (i > j) {
      const int64_t u = j * n + i;
      cnt[t] = cnt[u];
      len[t] = len[u];
      longest[t] = longest[u];
    }
  }
}

// cover[l] = cdiff[0] + .. + cdiff[l], l < L (one workgroup: a chunk of loci per thread)
__global__ void __launch_bounds__(1024)
k_tract_cover(int L, const int* __restrict__ cdiff, long long* __restrict__ cover) {
  __shared__ long long part[1024];
  const int tid = threadIdx.x;
  const int chunk = (L + 1023) / 1024;
  const int64_t a = (int64_t)tid * chunk, b = min((int64_t)L, a + chunk);
  long long s = 0;
  for (int64_t l = a; l < b; ++l) s += cdiff[l];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int q = 0; q < 1024; ++q) {
      const long long v = part[q];
      part[q] = run;
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

// what both entry points refuse before anything is launched
int tracts_check(gnx_state* h, const char* who, int64_t n, int64_t n_max, const int64_t* slots,
                 const int64_t* pos, int64_t min_len, int32_t n_edges, const int64_t* edges,
                 const int64_t* hist) {
  h->tr_ms = 0.0;
  h->tr_launches = 0;
  h->tr_bytes = 0;
  GNXCHK(geno_ready(h, who));
  if (n < 1 || n > n_max) {
    gnx_set_error("%s: 1..%lld individuals per call (got %lld)", who, (long long)n_max,
                  (long long)n);
    return 1;
  }
  if (!slots && n != h->N) {
    gnx_set_error("%s: n = %lld but %lld individuals are alive (slots == null)", who,
                  (long long)n, (long long)h->N);
    return 1;
  }
  if (slots) {
    std::vector<bool> seen((size_t)h->N, false);
    for (int64_t i = 0; i < n; ++i) {
      if (slots[i] < 0 || slots[i] >= h->N) {
        gnx_set_error("%s: slot out of range", who);
        return 1;
      }
      if (seen[(size_t)slots[i]]) {
        gnx_set_error("%s: slot %lld is listed twice", who, (long long)slots[i]);
        return 1;
      }
      seen[(size_t)slots[i]] = true;
    }
  }
  if (!pos) {
    gnx_set_error("%s: null pos", who);
    return 1;
  }
  for (int l = 1; l < h->cfg.L; ++l)
    if (pos[l] < pos[l - 1]) {
      gnx_set_error("%s: pos must be non-decreasing (pos[%d] = %lld)", who, l, (long long)pos[l]);
      return 1;
    }
  // (lengths are differences of two coordinates: they must stay inside int64)
  if (pos[0] < -(1ll << 62) || pos[h->cfg.L - 1] > (1ll << 62)) {
    gnx_set_error("%s: pos must lie within +-2^62", who);
    return 1;
  }
  if (min_len < 0) {
    gnx_set_error("%s: min_len >= 0 (got %lld)", who, (long long)min_len);
    return 1;
  }
  if (hist || n_edges != 0 || edges) {
    if (n_edges < 2 || n_edges > TR_NB + 1 || !edges || !hist) {
      gnx_set_error("%s: 2..%d edges with hist, or neither (got %d)", who, TR_NB + 1, n_edges);
      return 1;
    }
    for (int k = 1; k < n_edges; ++k)
      if (!(edges[k] > edges[k - 1])) {
        gnx_set_error("%s: edges must be strictly ascending (edges[%d] = %lld)", who, k,
                      (long long)edges[k]);
        return 1;
      }
  }
  return 0;
}

// pos, brk (bit 0 and the bits past L cleared), edges, hist and the cover differences on the
// device
struct TractDev {
  long long* pos = nullptr;
  u64* brk = nullptr;
  long long* edges = nullptr;
  unsigned long long* hist = nullptr;
  int* cdiff = nullptr;
  long long* cover = nullptr;
  int n_bins = 0;
};

int tracts_stage(gnx_state* h, GnxScratch& s, const int64_t* pos, const uint64_t* brk,
                 int32_t n_edges, const int64_t* edges, bool want_cover, TractDev& d) {
  const int L = h->cfg.L, W64 = h->W64;
  GNXCHK(s.get(&d.pos, (size_t)L));
  GNXCHK(gnx_h2d(h, d.pos, pos, (size_t)L * sizeof(int64_t)));
  if (brk) {
    std::vector<u64> b(brk, brk + W64);
    b[0] &= ~1ull;
    for (int w = 0; w < W64; ++w) {
      const int64_t left = (int64_t)L - (int64_t)w * 64;
      if (left <= 0) b[(size_t)w] = 0;
      else if (left < 64) b[(size_t)w] &= (1ull << left) - 1ull;
    }
    bool any = false;
    for (u64 v : b) any = any || v != 0;
    if (any) {
      GNXCHK(s.get(&d.brk, (size_t)W64));
      GNXCHK(gnx_h2d(h, d.brk, b.data(), (size_t)W64 * sizeof(u64)));
    }
  }
  d.n_bins = n_edges > 0 ? n_edges - 1 : 0;
  GNXCHK(s.get(&d.edges, (size_t)TR_NB + 1));
  GNXCHK(s.get(&d.hist, (size_t)TR_NB * 2));
  if (d.n_bins) GNXCHK(gnx_h2d(h, d.edges, edges, (size_t)n_edges * sizeof(int64_t)));
  HIPCHK(hipMemsetAsync(d.hist, 0, TR_NB * 2 * sizeof(unsigned long long), h->stream));
  if (want_cover) {
    GNXCHK(s.get(&d.cdiff, (size_t)L + 1));
    GNXCHK(s.get(&d.cover, (size_t)L));
    HIPCHK(hipMemsetAsync(d.cdiff, 0, ((size_t)L + 1) * sizeof(int), h->stream));
  }
  return 0;
}

// hist and cover to the host
int tracts_finish(gnx_state* h, const TractDev& d, int64_t* hist, int64_t* cover) {
  if (hist) GNXCHK(gnx_d2h(h, hist, d.hist, (size_t)d.n_bins * 2 * sizeof(int64_t)));
  if (cover) GNXCHK(gnx_d2h(h, cover, d.cover, (size_t)h->cfg.L * sizeof(int64_t)));
  return 0;
}

}  // namespace

extern "C" int gnx_tracts_info(gnx_state* h, double* kernel_ms, int64_t* launches,
                               int64_t* bytes_read) {
  if (kernel_ms) *kernel_ms = h->tr_ms;
  if (launches) *launches = h->tr_launches;
  if (bytes_read) *bytes_read = h->tr_bytes;
  return 0;
}

extern "C" int gnx_tracts_self(gnx_state* h, int64_t n, const int64_t* slots, const int64_t* pos,
                               const uint64_t* brk, int32_t min_loci, int64_t min_len,
                               int32_t n_edges, const int64_t* edges, int64_t* per,
                               int64_t* hist, int64_t* cover) {
  const char* who = "gnx_tracts_self";
  GNXCHK(tracts_check(h, who, n, TR_MAX_SELF, slots, pos, min_len, n_edges, edges, hist));
  if (!per) {
    gnx_set_error("%s: null output", who);
    return 1;
  }
  const int L = h->cfg.L, Wv = (L + 63) / 64;
  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  TractDev d;
  GNXCHK(tracts_stage(h, s, pos, brk, n_edges, edges, cover != nullptr, d));
  long long* d_per = nullptr;
  unsigned long long* d_words = nullptr;
  GNXCHK(s.get(&d_per, (size_t)n * 4));
  GNXCHK(s.get(&d_words, 1));
  HIPCHK(hipMemsetAsync(d_words, 0, sizeof(unsigned long long), h->stream));
  const int ml = std::max(1, min_loci);
  GnxCallTimer tm(h, &h->tr_ms, &h->tr_launches);
  tm.start();
  hipLaunchKernelGGL(k_tract_self, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, h->stream, n,
                     d_rows, (const u64*)h->G, gnx_halves(h), L, Wv, d.pos, d.brk, ml,
                     (long long)min_len, (int)(ml >= 63), d.n_bins, d.edges, d_per, d.hist,
                     d.cdiff, d_words);
  if (cover)
    hipLaunchKernelGGL(k_tract_cover, dim3(1), dim3(1024), 0, h->stream, L, d.cdiff, d.cover);
  HIPCHK(hipGetLastError());
  GNXCHK(tm.stop(cover ? 2 : 1));
  unsigned long long words = 0;
  GNXCHK(gnx_d2h(h, &words, d_words, sizeof(words)));
  h->tr_bytes = (int64_t)words * 8;
  GNXCHK(gnx_d2h(h, per, d_per, (size_t)n * 4 * sizeof(int64_t)));
  return tracts_finish(h, d, hist, cover);
}

extern "C" int gnx_tracts_pairs(gnx_state* h, int64_t n, const int64_t* slots, const int64_t* pos,
                                const uint64_t* brk, int32_t min_loci, int64_t min_len,
                                int32_t n_edges, const int64_t* edges, int64_t max_work,
                                int64_t* work, int32_t* cnt, int64_t* len, int64_t* longest,
                                int64_t* hist, int64_t* cover) {
  const char* who = "gnx_tracts_pairs";
  GNXCHK(tracts_check(h, who, n, TR_MAX_PAIRS, slots, pos, min_len, n_edges, edges, hist));
  if (!work) {
    gnx_set_error("%s: null work", who);
    return 1;
  }
  const int L = h->cfg.L, Wv = (L + 63) / 64;
  *work = (2 * n * (n - 1) + n) * (int64_t)Wv;
  if (max_work <= 0) return 0;
  if (*work > max_work) {
    gnx_set_error("%s: %lld haplotype pairs x %d words = %lld word steps of work exceed "
                  "max_work = %lld", who, (long long)(2 * n * (n - 1) + n), Wv, (long long)*work,
                  (long long)max_work);
    return 1;
  }
  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  TractDev d;
  GNXCHK(tracts_stage(h, s, pos, brk, n_edges, edges, cover != nullptr, d));
  int32_t* d_cnt = nullptr;
  long long *d_len = nullptr, *d_longest = nullptr;
  GNXCHK(s.get(&d_cnt, (size_t)n * n));
  GNXCHK(s.get(&d_len, (size_t)n * n));
  GNXCHK(s.get(&d_longest, (size_t)n * n));
  HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)n * n * sizeof(int32_t), h->stream));
  HIPCHK(hipMemsetAsync(d_len, 0, (size_t)n * n * sizeof(long long), h->stream));
  HIPCHK(hipMemsetAsync(d_longest, 0, (size_t)n * n * sizeof(long long), h->stream));
  const int ml = std::max(1, min_loci);
  // the operand: every word that holds a locus, and at least one zero word after them
  std::vector<int32_t> widx;
  std::vector<u64> wmask;
  geno_words(h, nullptr, widx, wmask);
  const int64_t n_pad = (n + 63) / 64 * 64;
  const int T = (int)(n_pad / 64);
  GenoOperand op;
  GNXCHK(geno_operand(h, s, n_pad, widx, wmask, 1, &op));
  GnxCallTimer tm(h, &h->tr_ms, &h->tr_launches);
  tm.start();
  geno_gather(h, d_rows, n, op);
  hipLaunchKernelGGL(k_tract_pairs, dim3(T, T), dim3(256), 0, h->stream, n, op.Wm, L, h->W64,
                     op.X, d.pos, d.brk, ml, (long long)min_len, (int)(ml >= 63), d.n_bins,
                     d.edges, d_cnt, d_len, d_longest, d.hist, d.cdiff);
  hipLaunchKernelGGL(k_tract_mirror, dim3(gnx_grid(n * n, 256, 256 * 64)), dim3(256), 0,
                     h->stream, n, d_cnt, d_len, d_longest);
  if (cover)
    hipLaunchKernelGGL(k_tract_cover, dim3(1), dim3(1024), 0, h->stream, L, d.cdiff, d.cover);
  HIPCHK(hipGetLastError());
  GNXCHK(tm.stop(cover ? 4 : 3));
  h->tr_bytes = n * 2 * (int64_t)Wv * 8;
  if (cnt) GNXCHK(gnx_d2h(h, cnt, d_cnt, (size_t)n * n * sizeof(int32_t)));
  if (len) GNXCHK(gnx_d2h(h, len, d_len, (size_t)n * n * sizeof(int64_t)));
  if (longest) GNXCHK(gnx_d2h(h, longest, d_longest, (size_t)n * n * sizeof(int64_t)));
  return tracts_finish(h, d, hist, cover);
}
