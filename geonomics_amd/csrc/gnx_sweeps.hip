// Haplotype sweep scans on the device: extended haplotype homozygosity around a core locus, from
// which EHH, iHS, nSL and XP-EHH follow on the host (geonomics_amd/sim/sweeps.py).  The contract
// (sample, kept loci, classes, scan, status, integration) is in include/gnx_hip.h.
//
//   gnx_sweeps_scan   c1 [n_loci], area, steps, status [n_loci][2][2], curve [2][2][n_loci], work
//
// Bit rows: the kernels of gnx_ld_bins (gnx_ld_bit_rows, gnx_ld.hip) turn the sample into
// T[j][q], 64 chromosomes per word, and count c1.  c1 is read back; the host lists the kept loci
// (request index, pos, "a break lies before me") and uploads that list: no row is moved.
//
// k_sweep_scan: one wave = one task (core, direction, class).  The wave keeps the chromosomes of
// its class as an ordered list of uint16 in its own slice of dynamic LDS, ping and pong; bit 15
// of an entry says "a group starts here", a group being the chromosomes identical so far.  A
// step loads the bit row of the next kept locus (lane q holds word q, one coalesced load) and
// stable-partitions the list by the allele there, 0s then 1s, 64 positions at a time: the
// destinations are prefix popcounts of the two allele ballots plus two running offsets.  An
// element starts a group in the new list when it is the first of its allele or when the number
// of group starts up to its old position (its old group) differs from that of the previous
// element of its allele - inside a chunk that is "a flag in (previous lane, own lane]" on the
// flag ballot, across chunks a scalar per allele carries the old group.  Then
// P = sum over positions of (position - start of its group), the start from clz on the flag
// ballot of the new list, carried across chunks in a scalar.  Everything but the list itself is
// wave-uniform; no atomics, no workgroup barrier (a workgroup is one wave), a wavefront fence
// between the ping and the pong.  The LDS of a launch is sized by the largest class of the
// call, so a small sample keeps many waves per CU.
#include "gnx_geno.h"

#define SW_MAX_N 2048               // individuals at most: 4096 chromosomes, 12 bits of an entry
#define SW_FLAG 0x8000u             // "a group starts here"
#define SW_LAUNCH_WORK (1ll << 34)  // words x steps (the unit of *work) one launch may hold

__device__ __forceinline__ int sw_wave_sum(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return __builtin_amdgcn_readfirstlane(v);
}

// the wave's LDS writes are visible to its own later reads, and neither moves across
__device__ __forceinline__ void sw_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// see the head of the file.  Task t of the launch: core cores_k[(task0 + t) >> 2] (an index into
// the kept list), direction ((task0 + t) >> 1) & 1 (0: left), class (task0 + t) & 1.  kept [K],
// kpos [K], kbrk [K] (kbrk[k]: a break lies between kept k - 1 and k); T, pitch, nq: the bit
// rows; cmask: null or [2][64], the members of the two classes; m_max: entries per list.
// area, steps, status [n_loci][2][2] hold 0, 0, 5 on entry; curve null or [2][2][n_loci] of -1
__global__ void __launch_bounds__(64)
k_sweep_scan(int64_t task0, const int32_t* __restrict__ cores_k, int K,
             const int32_t* __restrict__ kept, const long long* __restrict__ kpos,
             const uint8_t* __restrict__ kbrk, const u64* __restrict__ T, int64_t pitch, int nq,
             int n_chrom, const u64* __restrict__ cmask, int m_max, long long cut_num,
             long long cut_den, long long max_gap, long long max_extent, int n_loci,
             long long* __restrict__ area, int* __restrict__ steps, uint8_t* __restrict__ status,
             long long* __restrict__ curve) {
  extern __shared__ uint16_t sw_list[];               // [2][m_max]
  const int lane = threadIdx.x;
  const int64_t task = task0 + blockIdx.x;
  const int dir = (int)(task >> 1) & 1, c = (int)task & 1;
  const int kc = cores_k[task >> 2];
  const int jc = kept[kc];
  const int64_t out = ((int64_t)jc * 2 + dir) * 2 + c;
  const u64 lt = (1ull << lane) - 1ull, le = lt | (1ull << lane);

  // the members of the class, word `lane` of them
  u64 cm = 0;
  if (cmask) {
    cm = cmask[c * 64 + lane];
  } else if (lane < nq) {
    const u64 w = T[(int64_t)jc * pitch + lane];
    u64 valid = ~0ull;
    if (lane == nq - 1 && (n_chrom & 63)) valid = (1ull << (n_chrom & 63)) - 1ull;
    cm = (c ? w : ~w) & valid;
  }
  const int m = sw_wave_sum(__popcll(cm));
  if (m < 2) {
    if (lane == 0) status[out] = 4;
    return;
  }
  uint16_t* cur = sw_list;
  uint16_t* nxt = sw_list + m_max;
  {
    int off = 0;
    for (int q = 0; q < nq; ++q) {
      const u64 wq = __shfl(cm, q, 64);
      if ((wq >> lane) & 1ull) {
        const int d = off + __popcll(wq & lt);
        cur[d] = (uint16_t)((unsigned)(q * 64 + lane) | (d == 0 ? SW_FLAG : 0u));
      }
      off += __popcll(wq);
    }
  }
  sw_lds_fence();

  const long long Tc = (long long)m * (m - 1) / 2;
  long long* cv = curve ? curve + (int64_t)(dir * 2 + c) * n_loci : nullptr;
  if (cv && lane == 0) cv[0] = Tc;
  const long long pos_c = kpos[kc];
  long long A = 0;
  int P = (int)Tc, s = 0, st = 1, k = kc;
  for (;;) {
    const int kn = dir ? k + 1 : k - 1;
    if (kn < 0 || kn >= K || kbrk[dir ? kn : k]) {
      st = 1;
      break;
    }
    const long long pk = kpos[k], pn = kpos[kn];
    const long long gap = pn > pk ? pn - pk : pk - pn;
    if (max_gap > 0 && gap > max_gap) {
      st = 2;
      break;
    }
    if (max_extent > 0 && (pn > pos_c ? pn - pos_c : pos_c - pn) > max_extent) {
      st = 3;
      break;
    }
    int Pn = 0;
    if (P > 0) {                                      // (no pair left: nothing can split)
      const u64 word = lane < nq ? T[(int64_t)kept[kn] * pitch + lane] : 0ull;
      int off0 = 0, off1 = sw_wave_sum(__popcll(cm & ~word));
      int carry_f = 0, prev_g0 = 0, prev_g1 = 0;      // old groups count from 1: 0 = none yet
      for (int base = 0; base < m; base += 64) {
        const int p = base + lane;
        const bool valid = p < m;
        const unsigned e = valid ? cur[p] : 0u;
        const unsigned x = e & 0x7fffu;
        const u64 w = __shfl(word, (int)(x >> 6), 64);
        const bool a = valid && ((w >> (x & 63u)) & 1ull);
        const u64 B1 = __ballot(a), B0 = __ballot(valid && !a);
        const u64 BF = __ballot(valid && (e & SW_FLAG));
        const u64 before = (a ? B1 : B0) & lt;
        bool nf;
        if (before) {
          const int pl = 63 - __clzll((long long)before);
          nf = (BF & le & ~((2ull << pl) - 1ull)) != 0ull;
        } else {
          nf = (carry_f + __popcll(BF & le)) != (a ? prev_g1 : prev_g0);
        }
        const int dest = a ? off1 + __popcll(B1 & lt) : off0 + __popcll(B0 & lt);
        if (valid) nxt[dest] = (uint16_t)(x | (nf ? SW_FLAG : 0u));
        if (B0) prev_g0 = carry_f + __popcll(BF & ((2ull << (63 - __clzll((long long)B0))) - 1ull));
        if (B1) prev_g1 = carry_f + __popcll(BF & ((2ull << (63 - __clzll((long long)B1))) - 1ull));
        off0 += __popcll(B0);
        off1 += __popcll(B1);
        carry_f += __popcll(BF);
      }
      sw_lds_fence();
      int acc = 0, start_c = 0;
      for (int base = 0; base < m; base += 64) {
        const int p = base + lane;
        const bool valid = p < m;
        const u64 BF = __ballot(valid && (nxt[valid ? p : 0] & SW_FLAG));
        const u64 mine = BF & le;
        const int start = mine ? base + 63 - __clzll((long long)mine) : start_c;
        if (valid) acc += p - start;
        if (BF) start_c = base + 63 - __clzll((long long)BF);
      }
      Pn = sw_wave_sum(acc);
      sw_lds_fence();
      uint16_t* t = cur;
      cur = nxt;
      nxt = t;
    }
    if (cv && lane == 0) cv[s + 1] = Pn;
    if ((long long)Pn * cut_den < cut_num * Tc) {
      st = 0;
      break;
    }
    A += (long long)(P + Pn) * gap;
    P = Pn;
    ++s;
    k = kn;
  }
  if (lane == 0) {
    area[out] = A;
    steps[out] = s;
    status[out] = (uint8_t)st;
  }
}

extern "C" int gnx_sweeps_info(gnx_state* h, double* kernel_ms, int64_t* launches,
                               int64_t* steps_total) {
  if (kernel_ms) *kernel_ms = h->sw_ms;
  if (launches) *launches = h->sw_launches;
  if (steps_total) *steps_total = h->sw_steps;
  return 0;
}

extern "C" int gnx_sweeps_scan(gnx_state* h, int64_t n, const int64_t* slots, int32_t n_loci,
                               const int32_t* loci, const int64_t* pos, const uint8_t* brk,
                               const uint8_t* cls, int32_t n_cores, const int32_t* cores,
                               int32_t min_minor, int32_t cut_num, int32_t cut_den,
                               int64_t max_gap, int64_t max_extent, int64_t max_work,
                               int64_t* work, int64_t* c1, int64_t* area, int32_t* steps,
                               uint8_t* status, int64_t* curve) {
  const char* who = "gnx_sweeps_scan";
  h->sw_ms = 0.0;
  h->sw_launches = 0;
  h->sw_steps = 0;
  GNXCHK(geno_ready(h, who));
  if (n < 1 || n > SW_MAX_N) {
    gnx_set_error("%s: 1..%d individuals (%d chromosomes) per call (got %lld)", who, SW_MAX_N,
                  2 * SW_MAX_N, (long long)n);
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
  const int L = h->cfg.L, W64 = h->W64;
  if (n_loci < 1 || !loci || !pos) {
    gnx_set_error("%s: at least one locus, with its position (n_loci = %d)", who, n_loci);
    return 1;
  }
  if (!work || !c1 || (max_work > 0 && (!area || !steps || !status))) {
    gnx_set_error("%s: null work or output", who);
    return 1;
  }
  if (cut_num < 0 || cut_den <= 0 || cut_num > cut_den) {
    gnx_set_error("%s: the cutoff cut_num / cut_den lies in 0..1 with cut_den > 0 (got %d / %d)",
                  who, cut_num, cut_den);
    return 1;
  }
  std::vector<int32_t> jof((size_t)W64 * 64, -1);
  for (int j = 0; j < n_loci; ++j) {
    if (loci[j] < 0 || loci[j] >= L) {
      gnx_set_error("%s: locus out of range (loci[%d] = %d)", who, j, loci[j]);
      return 1;
    }
    if (jof[(size_t)loci[j]] >= 0) {
      gnx_set_error("%s: locus %d is listed twice", who, loci[j]);
      return 1;
    }
    jof[(size_t)loci[j]] = j;
    if (j > 0 && pos[j] < pos[j - 1]) {
      gnx_set_error("%s: pos must be non-decreasing (pos[%d] = %lld)", who, j,
                    (long long)pos[j]);
      return 1;
    }
  }
  const int64_t n_chrom = 2 * n;
  {
    // |pos[last] - pos[0]| in 65 bits, times N (N - 1) < 2^24
    const unsigned __int128 span = (unsigned __int128)((__int128)pos[n_loci - 1] - pos[0]);
    if (span * (unsigned __int128)(n_chrom * (n_chrom - 1)) >= ((unsigned __int128)1 << 62)) {
      gnx_set_error("%s: N (N - 1) (pos[last] - pos[0]) >= 2^62: an area could leave int64 "
                    "(N = %lld chromosomes; use a coarser unit)", who, (long long)n_chrom);
      return 1;
    }
  }
  if (curve && (!cores || n_cores != 1)) {
    gnx_set_error("%s: curve is the decay of one core: n_cores == 1", who);
    return 1;
  }
  if (cores) {
    if (n_cores < 1) {
      gnx_set_error("%s: at least one core (n_cores = %d), or cores == null", who, n_cores);
      return 1;
    }
    std::vector<bool> seen((size_t)n_loci, false);
    for (int i = 0; i < n_cores; ++i) {
      if (cores[i] < 0 || cores[i] >= n_loci) {
        gnx_set_error("%s: core out of range (cores[%d] = %d)", who, i, cores[i]);
        return 1;
      }
      if (seen[(size_t)cores[i]]) {
        gnx_set_error("%s: core %d is listed twice", who, cores[i]);
        return 1;
      }
      seen[(size_t)cores[i]] = true;
    }
  }
  const int nq = (int)((n_chrom + 63) / 64);
  std::vector<u64> cmask;
  int m_cls = 0;
  if (cls) {
    cmask.assign(128, 0ull);
    int mc[2] = {0, 0};
    for (int64_t x = 0; x < n_chrom; ++x) {
      if (cls[x] == 255) continue;
      if (cls[x] > 1) {
        gnx_set_error("%s: cls holds 0, 1 or 255 (cls[%lld] = %d)", who, (long long)x, cls[x]);
        return 1;
      }
      cmask[(size_t)cls[x] * 64 + (size_t)(x >> 6)] |= 1ull << (x & 63);
      ++mc[cls[x]];
    }
    m_cls = std::max(mc[0], mc[1]);
  }

  // ---- the bit rows and c1
  GnxScratch s(who);
  GnxCallTimer tm(h, &h->sw_ms, &h->sw_launches);
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  u64* T = nullptr;
  long long* d_c1 = nullptr;
  int64_t pitch = 0;
  GNXCHK(gnx_ld_bit_rows(h, s, tm, d_rows, n_chrom, n_loci, loci, jof, &T, &pitch, &d_c1));
  std::vector<long long> c1h((size_t)n_loci);
  GNXCHK(gnx_d2h(h, c1h.data(), d_c1, c1h.size() * sizeof(long long)));

  // ---- the kept loci and the cores among them
  const long long mm = std::max<long long>(2, min_minor);
  std::vector<int32_t> kept, kof((size_t)n_loci, -1);
  std::vector<long long> kpos;
  std::vector<uint8_t> kbrk;
  bool pending = false;
  for (int j = 0; j < n_loci; ++j) {
    if (j > 0 && brk && brk[j]) pending = true;
    if (std::min<long long>(c1h[(size_t)j], n_chrom - c1h[(size_t)j]) < mm) continue;
    kof[(size_t)j] = (int32_t)kept.size();
    kept.push_back(j);
    kpos.push_back((long long)pos[j]);
    kbrk.push_back(pending && kept.size() > 1 ? 1 : 0);
    pending = false;
  }
  const int K = (int)kept.size();
  std::vector<int32_t> cores_k;
  int m_max = m_cls;
  if (cores) {
    for (int i = 0; i < n_cores; ++i)
      if (kof[(size_t)cores[i]] >= 0) cores_k.push_back(kof[(size_t)cores[i]]);
  } else {
    for (int k = 0; k < K; ++k) cores_k.push_back(k);
  }
  if (!cls)
    for (int32_t k : cores_k) {
      const long long c = c1h[(size_t)kept[(size_t)k]];
      m_max = std::max<int>(m_max, (int)std::max<long long>(c, n_chrom - c));
    }
  const int64_t per_core = 4ll * nq * std::max(0, K - 1);
  *work = (int64_t)cores_k.size() * per_core;         // < 2^31 2^2 2^6 2^31
  for (int j = 0; j < n_loci; ++j) c1[j] = c1h[(size_t)j];
  if (max_work <= 0) return 0;
  if (*work > max_work) {
    gnx_set_error("%s: %lld cores x 4 scans x %d chromosome words x %d steps = %lld word steps "
                  "of work exceed max_work = %lld", who, (long long)cores_k.size(), nq,
                  std::max(0, K - 1), (long long)*work, (long long)max_work);
    return 1;
  }

  // ---- the scans
  const size_t n_out = (size_t)n_loci * 4;
  long long *d_area = nullptr, *d_curve = nullptr, *d_kpos = nullptr;
  int *d_steps = nullptr;
  uint8_t *d_status = nullptr, *d_kbrk = nullptr;
  int32_t *d_kept = nullptr, *d_cores = nullptr;
  u64* d_cmask = nullptr;
  GNXCHK(s.get(&d_area, n_out));
  GNXCHK(s.get(&d_steps, n_out));
  GNXCHK(s.get(&d_status, n_out));
  HIPCHK(hipMemsetAsync(d_area, 0, n_out * sizeof(long long), h->stream));
  HIPCHK(hipMemsetAsync(d_steps, 0, n_out * sizeof(int), h->stream));
  HIPCHK(hipMemsetAsync(d_status, 5, n_out, h->stream));
  if (curve) {
    GNXCHK(s.get(&d_curve, n_out));
    HIPCHK(hipMemsetAsync(d_curve, 0xff, n_out * sizeof(long long), h->stream));
  }
  if (!cores_k.empty()) {
    GNXCHK(s.get(&d_kept, (size_t)K));
    GNXCHK(s.get(&d_kpos, (size_t)K));
    GNXCHK(s.get(&d_kbrk, (size_t)K));
    GNXCHK(s.get(&d_cores, cores_k.size()));
    GNXCHK(gnx_h2d(h, d_kept, kept.data(), (size_t)K * sizeof(int32_t)));
    GNXCHK(gnx_h2d(h, d_kpos, kpos.data(), (size_t)K * sizeof(long long)));
    GNXCHK(gnx_h2d(h, d_kbrk, kbrk.data(), (size_t)K));
    GNXCHK(gnx_h2d(h, d_cores, cores_k.data(), cores_k.size() * sizeof(int32_t)));
    if (cls) {
      GNXCHK(s.get(&d_cmask, (size_t)128));
      GNXCHK(gnx_h2d(h, d_cmask, cmask.data(), 128 * sizeof(u64)));
    }
    // the cores of one launch: as many as SW_LAUNCH_WORK word steps allow, and a grid below 2^30
    const int64_t batch = std::max<int64_t>(
        1, std::min<int64_t>(SW_LAUNCH_WORK / std::max<int64_t>(1, per_core), 1 << 28));
    m_max = std::max(2, m_max);
    const size_t lds = (size_t)2 * m_max * sizeof(uint16_t);
    int64_t launches = 0;
    tm.start();
    for (int64_t c0 = 0; c0 < (int64_t)cores_k.size(); c0 += batch, ++launches) {
      const int64_t nc = std::min<int64_t>(batch, (int64_t)cores_k.size() - c0);
      hipLaunchKernelGGL(k_sweep_scan, dim3((unsigned)(nc * 4)), dim3(64), lds, h->stream,
                         (int64_t)(c0 * 4), d_cores, K, d_kept, d_kpos, d_kbrk, T, pitch, nq,
                         (int)n_chrom, d_cmask, m_max, (long long)cut_num, (long long)cut_den,
                         (long long)max_gap, (long long)max_extent, (int)n_loci, d_area, d_steps,
                         d_status, d_curve);
    }
    HIPCHK(hipGetLastError());
    GNXCHK(tm.stop(launches));
  }
  GNXCHK(gnx_d2h(h, area, d_area, n_out * sizeof(long long)));
  GNXCHK(gnx_d2h(h, steps, d_steps, n_out * sizeof(int)));
  GNXCHK(gnx_d2h(h, status, d_status, n_out));
  if (curve) GNXCHK(gnx_d2h(h, curve, d_curve, n_out * sizeof(long long)));
  int64_t total = 0;
  for (size_t q = 0; q < n_out; ++q) total += steps[q];
  h->sw_steps = total;
  return 0;
}
