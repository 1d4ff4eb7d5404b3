// C-ABI of libgnxhip.so (include/gnx_hip.h): state management, uploads,
// downloads and the host-side orchestration of one time step.
#include <cmath>
#include <cstdarg>
#include <algorithm>
#include <atomic>
#include <chrono>
#include "gnx_internal.h"
#include "gnx_rng.h"
#include "gnx_compact.h"

// ---------------------------------------------------------------- errors
static thread_local char g_err[1024] = "";

void gnx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* gnx_last_error(void) { return g_err; }

extern "C" int gnx_words_per_hom(int32_t L) {
  int w = (L + 63) / 64;
  return ((w + 15) / 16) * 16;
}

extern "C" int gnx_blocks_per_hom(const gnx_state* h) { return h && h->cfg.L > 0 ? h->NB : 0; }

// ---------------------------------------------------------------- timers
// HIP events on the handle's stream around each kernel family.  Events are
// recorded without any host synchronisation inside the step (so the timed
// region is not perturbed) and resolved when gnx_kernel_time() is called.
static hipEvent_t timer_event(gnx_state* h) {
  if (!h->ev_free.empty()) {
    hipEvent_t e = h->ev_free.back();
    h->ev_free.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  // (timing only: no system-scope fence when it is recorded - the header's own advice, and
  // 2 us less per record on the stream that is being timed)
  (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  return e;
}

// GNX_HOST_TIMES=1: where the host's time goes (printed by gnx_destroy): in gnx_step as a
// whole, and of that waiting for device counts
double g_host_step_s = 0.0, g_host_wait_s = 0.0;
long long g_host_steps = 0;
bool gnx_host_times() {
  static const bool on = gnx_env_int("GNX_HOST_TIMES", 0) != 0;
  return on;
}
// GNX_HOST_TIMES=2: the host's clock where a wait for the device returns (the moment the GPU has
// got that far) - the mean time between consecutive marks, printed by gnx_destroy: which stretch
// of the step is slow without a profiler in the way
static std::vector<std::pair<int, long long>> g_marks;
void gnx_host_mark(int id) {
  static const bool on = gnx_env_int("GNX_HOST_TIMES", 0) == 2;
  if (!on) return;
  g_marks.emplace_back(id, (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(
                               std::chrono::steady_clock::now().time_since_epoch()).count());
}
static void host_marks_report() {
  if (g_marks.size() < 64) return;
  double sum[256] = {0};
  long long n[256] = {0};
  for (size_t k = g_marks.size() / 2; k < g_marks.size(); ++k) {
    const int key = (g_marks[k - 1].first & 15) * 16 + (g_marks[k].first & 15);
    sum[key] += 1e-3 * (double)(g_marks[k].second - g_marks[k - 1].second);
    n[key] += 1;
  }
  for (int key = 0; key < 256; ++key)
    if (n[key])
      fprintf(stderr, "[gnx host marks] %d -> %d: %.1f us (%lld times)\n", key / 16, key % 16,
              sum[key] / n[key], n[key]);
  g_marks.clear();
}

struct GnxHostWait {
  std::chrono::steady_clock::time_point t0;
  GnxHostWait() { if (gnx_host_times()) t0 = std::chrono::steady_clock::now(); }
  ~GnxHostWait() {
    if (gnx_host_times())
      g_host_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
};

// Events that only order streams of this device against each other need no system-scope fence
// when they are recorded (cache write-back and invalidation for the host's and other
// devices' sake): hipEventDisableSystemFence.  Measured with ten extra records / waits on
// the step's main stream: a record costs that stream 5.5 us with the fence and 3.5 without, a
// wait ~6; the step's own ten went from 0.621 to 0.606 ms (hipEventReleaseToDevice: nothing).
// Events the HOST synchronises on (ev_counts) keep the fence.
unsigned gnx_order_event_flags() { return hipEventDisableTiming | hipEventDisableSystemFence; }

int gnx_wait_published(gnx_state* h, int slot, int64_t seq) {
  GnxHostWait hw;
  volatile int64_t* word = h->h_pin + slot + 3;
  const auto t0 = std::chrono::steady_clock::now();
  for (int spin = 0; *word != seq; ++spin) {
    if ((spin & 1023) == 1023 &&
        std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {
      // something is slow or has gone wrong: let the runtime wait and report
      HIPCHK(hipStreamSynchronize(h->stream));
      if (*word != seq) {
        gnx_set_error("read-back of device counters never arrived");
        return 1;
      }
      break;
    }
    __builtin_ia32_pause();
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  gnx_host_mark(slot == 4 ? 1 : 3);
  return 0;
}

void gnx_time_begin(gnx_state* h, int kernel) {
  if (!h->profiling) return;
  if (h->profile_only >= 0 && kernel != h->profile_only) {
    h->ev_open = nullptr;
    return;
  }
  h->ev_open = timer_event(h);
  (void)hipEventRecord(h->ev_open, h->stream);
}

void gnx_time_end(gnx_state* h, int kernel, double bytes) {
  if (!h->profiling || !h->ev_open) return;
  if (h->profile_only >= 0 && kernel != h->profile_only &&
      !(h->profile_only == GNX_K_CROSSOVER && kernel == GNX_K_CROSSOVER_TAIL)) {   // one family only
    h->ev_free.push_back(h->ev_open);
    h->ev_open = nullptr;
    return;
  }
  hipEvent_t e1 = timer_event(h);
  (void)hipEventRecord(e1, h->stream);
  h->ev_pending[kernel].push_back({h->ev_open, e1});
  h->ev_open = nullptr;
  h->timers[kernel].launches += 1;
  h->timers[kernel].bytes += bytes;
}

static void timers_resolve(gnx_state* h, int kernel) {
  (void)gnx_xo_launch_pending(h);
  (void)hipStreamSynchronize(h->stream);
  if (h->stream2) (void)hipStreamSynchronize(h->stream2);
  for (auto& pr : h->ev_pending[kernel]) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) h->timers[kernel].ms += ms;
    h->ev_free.push_back(pr.first);
    h->ev_free.push_back(pr.second);
  }
  h->ev_pending[kernel].clear();
}

static int stage_reserve(gnx_state* h, size_t bytes) {
  if (bytes <= h->h_stage_bytes) return 0;
  if (h->h_stage) (void)hipHostFree(h->h_stage);
  h->h_stage = nullptr;
  h->h_stage_bytes = 0;
  size_t want = std::max<size_t>(bytes + bytes / 4, 1 << 20);
  HIPCHK(hipHostMalloc(&h->h_stage, want));
  h->h_stage_bytes = want;
  return 0;
}

int gnx_h2d(gnx_state* h, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return 0;
  const size_t chunk = 64u << 20;
  GNXCHK(stage_reserve(h, std::min(bytes, chunk)));
  for (size_t o = 0; o < bytes; o += chunk) {
    size_t n = std::min(chunk, bytes - o);
    memcpy(h->h_stage, (const char*)src + o, n);
    HIPCHK(hipMemcpyAsync((char*)dst + o, h->h_stage, n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int gnx_d2h(gnx_state* h, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return 0;
  const size_t chunk = 64u << 20;
  GNXCHK(stage_reserve(h, std::min(bytes, chunk)));
  for (size_t o = 0; o < bytes; o += chunk) {
    size_t n = std::min(chunk, bytes - o);
    HIPCHK(hipMemcpyAsync(h->h_stage, (const char*)src + o, n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy((char*)dst + o, h->h_stage, n);
  }
  return 0;
}

__global__ void k_publish(const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d,
                          int64_t* host) {
  if (a) host[0] = *a;
  if (b) host[1] = *b;
  if (c) host[2] = *c;
  if (d) host[3] = *d;
}

int gnx_publish(gnx_state* h, int slot, const int32_t* a, const int32_t* b, const int32_t* c,
                const int32_t* d) {
  hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, h->stream, a, b, c, d, h->h_pin_dev + slot);
  HIPCHK(hipGetLastError());
  return 0;
}

GnxTraitTab gnx_trait_tab(const gnx_state* h) {
  GnxTraitTab T;
  memset(&T, 0, sizeof(T));
  T.n_traits = h->cfg.n_traits;
  for (int t = 0; t < h->cfg.n_traits; ++t) {
    const GnxTrait& r = h->traits[t];
    T.n_loci[t] = r.n_loci;
    T.loci[t] = r.loci;
    T.alpha[t] = r.alpha;
    T.layer[t] = r.layer;
    T.phi[t] = r.phi;
    T.phi_rast[t] = r.phi_rast;
    T.gamma[t] = r.gamma;
    T.univ_adv[t] = r.univ_adv;
  }
  return T;
}

// ---------------------------------------------------------------- alloc helpers
template <typename T>
static int dalloc(T** p, size_t n) {
  *p = nullptr;
  if (n == 0) n = 1;
  HIPCHK(hipMalloc((void**)p, n * sizeof(T)));
  return 0;
}

static int alloc_soa(GnxSoA* s, int64_t cap, int n_layers, int n_traits) {
  GNXCHK(dalloc(&s->x, cap));
  GNXCHK(dalloc(&s->y, cap));
  GNXCHK(dalloc(&s->age, cap));
  GNXCHK(dalloc(&s->sex, cap));
  GNXCHK(dalloc(&s->id, cap));
  GNXCHK(dalloc(&s->e, cap * std::max(n_layers, 1)));
  GNXCHK(dalloc(&s->z, cap * std::max(n_traits, 1)));
  GNXCHK(dalloc(&s->fit, cap));
  GNXCHK(dalloc(&s->grow, cap));
  GNXCHK(dalloc(&s->ghost, cap));
  HIPCHK(hipMemset(s->ghost, 0, cap));
  s->tb = nullptr;           // sized by gnx_l_rebuild_sel once the selected loci are known
  return 0;
}

static void free_soa(GnxSoA* s) {
  (void)hipFree(s->x);
  (void)hipFree(s->y);
  (void)hipFree(s->age);
  (void)hipFree(s->sex);
  (void)hipFree(s->id);
  (void)hipFree(s->e);
  (void)hipFree(s->z);
  (void)hipFree(s->fit);
  (void)hipFree(s->grow);
  (void)hipFree(s->ghost);
  (void)hipFree(s->tb);
}

// ---------------------------------------------------------------- lifecycle
extern "C" int gnx_create(const gnx_config* cfg, gnx_state** out) {
  *out = nullptr;
  if (cfg->W <= 0 || cfg->H <= 0 || cfg->n_layers <= 0 || cfg->n_layers > GNX_MAX_LAYERS ||
      cfg->n_traits < 0 || cfg->n_traits > GNX_MAX_TRAITS || cfg->cap_inds <= 0 || cfg->L < 0 ||
      cfg->cap_inds > 0x7fffff00ll || cfg->cap_rows > 0x7fffff00ll) {
    gnx_set_error("gnx_create: invalid configuration");
    return 1;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    gnx_set_error("gnx_create: no HIP device available (this library has no CPU fallback)");
    return 1;
  }
  HIPCHK(hipSetDevice(cfg->device));
  gnx_state* h = new gnx_state();
  h->cfg = *cfg;
  if (cfg->L == 0) h->cfg.cap_rows = 0;
  h->W64 = cfg->L > 0 ? gnx_words_per_hom(cfg->L) : 0;
  const int64_t cap = cfg->cap_inds;
  // `stream` carries the step's many small latency-bound kernels, `stream2` the deferred
  // crossover (one long bandwidth-bound kernel per step, under the NEXT step's small
  // kernels): the small kernels get the higher dispatch priority so that they are not
  // queued behind the crossover's workgroups (keeping the crossover off a few CUs of every XCD
  // with a CU mask was measured and removed: profiles/r02_xo_overlap_*.txt)
  {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    HIPCHK(hipStreamCreateWithPriority(&h->stream, hipStreamDefault, hi));
    HIPCHK(hipStreamCreateWithPriority(&h->stream2, hipStreamDefault, lo));
  }
  h->own_stream = true;
  for (int k = 0; k < 2; ++k) GNXCHK(alloc_soa(&h->soa[k], cap, cfg->n_layers, cfg->n_traits));
  GNXCHK(dalloc(&h->rast, (size_t)cfg->n_layers * cfg->W * cfg->H));
  if (cfg->L > 0) {
    // blocks per homologue: the largest divisor of the 128-byte lines per homologue that is
    // not above 16 and leaves blocks of at least 2 lines (L = 10^5: 98 lines, 14 blocks of
    // 896 bytes - round 3's layout, superseded below; L = 10^4: 10 lines, 5 blocks of 256 bytes; GNX_HALF_BLOCKS asks for another one), as long as the block numbers fit 31
    // bits.  Measured at the metric workload (tools/ab.sh): 7 blocks 0.745 ms/step, 14 blocks
    // 0.670 - a switch point costs a block half the size, the tables twice the entries.
    // GNX_BLOCK_LINES=k: blocks of exactly k lines (k = 8: 1 024 bytes, every lane of the
    // crossover's waves carries a chunk) - the last block reaches past the homologue, the table
    // is laid out for NB * k lines per homologue (13 x 8 = 104 instead of 98 at L = 10^5)
    {
      const int lines = h->W64 / 16;
      const bool asked = getenv("GNX_HALF_BLOCKS") != nullptr;
      int want = gnx_env_int("GNX_HALF_BLOCKS", 16);                // (more only when asked for)
      want = std::max(1, std::min(want, GNX_MAX_NB));
      while (want > 1 && (lines % want || (!asked && lines / want < 2) ||
                          (double)h->cfg.cap_rows * 4 * 2.0 * want >= 2.0e9))
        --want;
      h->NB = want;
      h->BW = h->W64 / want;
      // Long homologues (>= 40 lines; round 4): blocks of 5 lines (640 bytes), or as many lines
      // as keep the block count within GNX_MAX_NB - the last block reaches past the homologue
      // (L = 10^5: 20 blocks, the table laid out for 100 lines instead of 98).  Measured at the
      // metric workload (profiles/r04_ab_runs.txt): 14 blocks of 7 lines 0.588 ms/step, 17 of 6
      // 0.587, 20 of 5 0.565, 25 of 4 0.563 - a switch point costs 1.9 KB of traffic instead of
      // 2.7, the crossover launch 0.147 ms instead of 0.178 for 0.49 GB instead of 0.70; with 25
      // blocks it shrinks further (0.132 ms) but the job builder's tables grow as much.
      // GNX_BLOCK_LINES=k: blocks of exactly k lines; 0: the divisor rule above whatever the length
      int bl = gnx_env_int("GNX_BLOCK_LINES", -1);
      if (bl < 0) bl = (!asked && lines >= 40) ? std::max(5, (lines + GNX_MAX_NB - 1) / GNX_MAX_NB) : 0;
      if (bl > 0 && (double)h->cfg.cap_rows * 4 * 2.0 * ((lines + bl - 1) / bl) >= 2.0e9) bl = 0;
      if (bl > 0 && (lines + bl - 1) / bl <= GNX_MAX_NB && (lines + bl - 1) / bl >= 1) {
        h->NB = (lines + bl - 1) / bl;
        h->BW = 16 * bl;
      }
      h->NB_alloc = h->NB;
      h->BW_alloc = h->BW;
    }
    // spread the table over up to four times its size when the device has the room
    // (GNX_ROW_SPREAD overrides: 1 = compact).  2x is not enough to be safe: the rate then
    // depends on where the driver happens to place the allocation (4.9 or 5.95 TB/s from one
    // process to the next, profiles/r02_xo_lab_footprint.txt); 3x and 4x are steady.
    {
      const size_t need = (size_t)h->cfg.cap_rows * 2 * std::max(h->W64, h->NB * h->BW) * 8;
      size_t free_b = 0, total_b = 0;
      (void)hipMemGetInfo(&free_b, &total_b);
      int want = gnx_env_int("GNX_ROW_SPREAD", 4);
      want = std::max(1, std::min(want, 8));
      while (want > 1 && ((double)need * want > 0.75 * (double)free_b ||
                          (double)h->cfg.cap_rows * want > 1.0e9))
        --want;
      // several handles may be created at once on one GPU (tiles as threads or processes
      // in rehearsals): what looked free a moment ago may be gone - fall back to less
      for (; want >= 1; --want) {
        h->G = nullptr;
        const hipError_t e = hipMalloc((void**)&h->G, need * (size_t)want);
        if (e == hipSuccess) break;
        (void)hipGetLastError();
        if (want == 1) {
          gnx_set_error("hipMalloc of the genome table (%zu bytes) failed: %s", need,
                        hipGetErrorString(e));
          return 1;
        }
      }
      h->row_spread = want;
    }
    GNXCHK(dalloc(&h->free_rows, (size_t)h->cfg.cap_rows));
    const size_t halves = (size_t)h->cfg.cap_rows * h->row_spread * 2 * h->NB;
    GNXCHK(dalloc(&h->hmap, halves));
    GNXCHK(dalloc(&h->half_mark, halves));
    GNXCHK(dalloc(&h->half_free, (size_t)h->cfg.cap_rows * 2 * h->NB));
    GNXCHK(dalloc(&h->half_top, 1));
    HIPCHK(hipMalloc(&h->xo_plan, (size_t)cap * 40));
    GNXCHK(dalloc(&h->gc_cnt, (size_t)h->cfg.cap_rows * 2 * h->NB / GNX_CB + 2));
    GNXCHK(dalloc(&h->gc_off, (size_t)h->cfg.cap_rows * 2 * h->NB / GNX_CB + 2));
    HIPCHK(hipMemset(h->half_mark, 0, halves));
    HIPCHK(hipMalloc((void**)&h->xo_jobs_acc, 2 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(h->xo_jobs_acc, 0, 2 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(h->hmap, 0xff, halves * sizeof(int32_t)));
    HIPCHK(hipMemset(h->half_top, 0, sizeof(int32_t)));
    h->alias_xo = gnx_env_int("GNX_XO_ALIAS", 1) != 0;
  }
  for (int k = 0; k < 2; ++k) {
    GNXCHK(dalloc(&h->key[k], cap));
    GNXCHK(dalloc(&h->perm[k], cap));
  }
  GNXCHK(dalloc(&h->mate, cap));
  for (int k = 0; k < 2; ++k) {
    GNXCHK(dalloc(&h->ord[k], cap));
    GNXCHK(dalloc(&h->keyk[k], cap));
    GNXCHK(dalloc(&h->valk[k], cap));
  }
  GNXCHK(dalloc(&h->newslot, cap));
  GNXCHK(dalloc(&h->fill_cnt, 4));
  HIPCHK(hipEventCreateWithFlags(&h->ev_fill, gnx_order_event_flags()));
  HIPCHK(hipEventCreateWithFlags(&h->ev_alive, gnx_order_event_flags()));
  HIPCHK(hipEventCreateWithFlags(&h->ev_moved, gnx_order_event_flags()));
  HIPCHK(hipEventCreateWithFlags(&h->ev_perm_rest, gnx_order_event_flags()));
  {
    // (zero between sorts: k_permute wipes what a sort dirtied; + 16: the wipe is in uint4s)
    // (three digit places of the 32-bit cell sort over the id-ordered index, or the seven a
    // 64-bit (cell, id) key can have: gnx_os_sort64_clean on tiles)
    const size_t nb = std::max(gnx_os_scratch_bytes((size_t)cap, 24),
                               gnx_os_words_used64((size_t)cap, 64) * sizeof(unsigned int)) + 16;
    HIPCHK(hipMalloc(&h->os_scratch, nb));
    HIPCHK(hipMemset(h->os_scratch, 0, nb));
  }
  GNXCHK(dalloc(&h->os_ktmp, cap));
  GNXCHK(dalloc(&h->os_vtmp, cap));
  GNXCHK(dalloc(&h->cell32, cap));
  GNXCHK(dalloc(&h->ord_cnt, cap / GNX_CB + 2));
  GNXCHK(dalloc(&h->ord_off, cap / GNX_CB + 2));
  HIPCHK(hipEventCreateWithFlags(&h->ev_ord, gnx_order_event_flags()));
  HIPCHK(hipStreamCreate(&h->stream3));
  HIPCHK(hipEventCreateWithFlags(&h->ev_compact, gnx_order_event_flags()));
  h->ord_mode = gnx_env_int("GNX_ORD_SORT", 1) != 0;
  GNXCHK(dalloc(&h->tag, cap));
  HIPCHK(hipMalloc(&h->cand, (size_t)cap * 16));
  GNXCHK(dalloc(&h->flag, cap + 1));
  GNXCHK(dalloc(&h->flag2, cap + 1));
  GNXCHK(dalloc(&h->scan, cap + 1));
  GNXCHK(dalloc(&h->pairs, cap * 2));
  GNXCHK(dalloc(&h->nbirths, cap + 1));
  GNXCHK(dalloc(&h->boff, cap + 1));
  GNXCHK(dalloc(&h->off_pair, cap));
  GNXCHK(dalloc(&h->off_parent, cap * 2));
  GNXCHK(dalloc(&h->off_keys, cap * 2));
  GNXCHK(dalloc(&h->off_start, cap * 2));
  GNXCHK(dalloc(&h->keep_in, cap));
  GNXCHK(dalloc(&h->inj_a, cap * GNX_DISP_ATTEMPTS));
  GNXCHK(dalloc(&h->inj_b, cap * GNX_DISP_ATTEMPTS));
  GNXCHK(dalloc(&h->mid_x, cap));
  GNXCHK(dalloc(&h->mid_y, cap));
  GNXCHK(dalloc(&h->p_death, cap));
  GNXCHK(dalloc(&h->d_cell, cap));
  GNXCHK(dalloc(&h->dead_in, cap));
  GNXCHK(dalloc(&h->nmax_bits, 1));
  GNXCHK(dalloc(&h->red, 8));
  GNXCHK(gnx_prim_sort_bytes((size_t)cap, 32, &h->sort_tmp_bytes));
  HIPCHK(hipMalloc(&h->sort_tmp, std::max<size_t>(h->sort_tmp_bytes, 16)));
  GNXCHK(gnx_prim_scan_bytes((size_t)cap + 1, &h->scan_tmp_bytes));
  HIPCHK(hipMalloc(&h->scan_tmp, std::max<size_t>(h->scan_tmp_bytes, 16)));
  GNXCHK(gnx_prim_sort64_bytes((size_t)cap, &h->sort64_tmp_bytes));
  HIPCHK(hipMalloc(&h->sort64_tmp, std::max<size_t>(h->sort64_tmp_bytes, 16)));
  GNXCHK(dalloc(&h->key64[0], cap));
  GNXCHK(dalloc(&h->key64[1], cap));
  GNXCHK(dalloc(&h->pairs2, cap * 2));
  GNXCHK(dalloc(&h->pair_goff, cap));
  GNXCHK(dalloc(&h->req_pid, cap));
  GNXCHK(dalloc(&h->req_k, cap));
  GNXCHK(dalloc(&h->req_key, cap));
  GNXCHK(dalloc(&h->req_start, cap));
  GNXCHK(dalloc(&h->req_px, cap));
  GNXCHK(dalloc(&h->req_py, cap));
  GNXCHK(dalloc(&h->req_count, 1));
  h->blk_stride = (int)((cap + 1023) / 1024) + 2;
  GNXCHK(dalloc(&h->blk_cnt, (size_t)3 * h->blk_stride));
  GNXCHK(dalloc(&h->blk_off, (size_t)3 * h->blk_stride));
  GNXCHK(dalloc(&h->cnt_dev, 8));
  GNXCHK(dalloc(&h->tickets, 8));
  GNXCHK(dalloc(&h->nmax2, 2));
  HIPCHK(hipMemset(h->nmax2, 0, 2 * sizeof(unsigned long long)));
  HIPCHK(hipEventCreateWithFlags(&h->ev_pairs, gnx_order_event_flags()));
  HIPCHK(hipEventCreateWithFlags(&h->ev_latP, gnx_order_event_flags()));
  HIPCHK(hipEventCreateWithFlags(&h->ev_perm, gnx_order_event_flags()));
  HIPCHK(hipEventCreateWithFlags(&h->ev_binsN, gnx_order_event_flags()));
  HIPCHK(hipMemset(h->tickets, 0, 8 * sizeof(unsigned int)));
  // fine-grained: the host polls words that kernels write (gnx_wait_published)
  HIPCHK(hipHostMalloc((void**)&h->h_pin, 32 * sizeof(int64_t),
                       hipHostMallocCoherent | hipHostMallocMapped));
  memset(h->h_pin, 0, 32 * sizeof(int64_t));
  HIPCHK(hipHostGetDevicePointer((void**)&h->h_pin_dev, h->h_pin, 0));
  if (cfg->L > 0) {
    for (int k = 0; k < 2; ++k) {
      HIPCHK(hipMalloc(&h->jobs[k], (size_t)cap * 2 * h->NB * 16));     // a job per cut block
      HIPCHK(hipMalloc(&h->jobs_bp[k], (size_t)cap * 2 * h->NB * 8));
      GNXCHK(dalloc(&h->n_jobs_dev[k], 1));
      HIPCHK(hipEventCreateWithFlags(&h->ev_xo_done[k], gnx_order_event_flags()));
      HIPCHK(hipEventCreateWithFlags(&h->ev_xo_wide[k], gnx_order_event_flags()));
    }
    HIPCHK(hipEventCreateWithFlags(&h->ev_jobs, gnx_order_event_flags()));
  }
  HIPCHK(hipEventCreateWithFlags(&h->ev_counts, hipEventDisableTiming));
  // When the deferred crossover of step t goes on its stream (csrc/gnx_kernels_genome.hip:
  // gnx_xo_launch_pending): as soon as its jobs are built (it runs beside the next step's
  // movement), or (xo_launch_late) behind the next step's pair list.  Since gnx_walk leaves no
  // compaction between its steps (round 6) the head of a step is the movement alone, and a
  // crossover that runs beside the births, the densities, the death draws and the next job
  // builder instead - latency-bound chains that leave the memory system idle - costs the step
  // least: 0.502 against 0.518 ms at the metric workload (profiles/r06_ab_runs.txt).  Large
  // populations only: the device-driven step of the small ones (gnx_dd.hip) schedules its own.
  // (behind the cell sort, the births or the densities: measured and removed, profiles/r06_ab_runs.txt)
  h->xo_launch_late = h->xo_launch_late_default = cap > gnx_dd_max_cap();
  h->compact_fill = gnx_env_int("GNX_COMPACT_FILL", 1) != 0;
  h->permute_split = gnx_env_int("GNX_PERMUTE_SPLIT", 1) != 0;
  *out = h;
  return 0;
}

extern "C" void gnx_destroy(gnx_state* h) {
  if (!h) return;
  host_marks_report();
  if (gnx_host_times() && g_host_steps > 0)
    fprintf(stderr, "[gnx host times] %lld steps: %.1f us/step in gnx_step, %.1f us of it waiting for counts\n",
            g_host_steps, 1e6 * g_host_step_s / g_host_steps, 1e6 * g_host_wait_s / g_host_steps);
  (void)gnx_xo_launch_pending(h);
  (void)hipStreamSynchronize(h->stream);
  gnx_dd_destroy(h);
  (void)gnx_comm_free(h);
  {
    void* vt[] = {h->vt_cls, h->vt_scls, h->vt_blk_nz, h->vt_rank, h->vt_pblk, h->vt_blk_cnt, h->vt_blk_off, h->vt_count, h->vt_base};
    for (void* q : vt)
      if (q) (void)hipFree(q);
  }
  if (h->stream2) (void)hipStreamSynchronize(h->stream2);
  if (h->stream3) (void)hipStreamSynchronize(h->stream3);    // reads ord / newslot
  for (int k = 0; k < 2; ++k) {
    (void)hipFree(h->jobs[k]);
    (void)hipFree(h->jobs_bp[k]);
    (void)hipFree(h->n_jobs_dev[k]);
    if (h->ev_xo_done[k]) (void)hipEventDestroy(h->ev_xo_done[k]);
    if (h->ev_xo_wide[k]) (void)hipEventDestroy(h->ev_xo_wide[k]);
  }
  if (h->ev_jobs) (void)hipEventDestroy(h->ev_jobs);
  if (h->ev_counts) (void)hipEventDestroy(h->ev_counts);
  for (int k = 0; k < 2; ++k) {
    free_soa(&h->soa[k]);
    (void)hipFree(h->key[k]);
    (void)hipFree(h->perm[k]);
    (void)hipFree(h->counts_rast[k]);
  }
  void* ptrs[] = {h->os_scratch, h->os_ktmp, h->os_vtmp, h->fill_cnt, h->ord[0], h->ord[1], h->keyk[0], h->keyk[1], h->valk[0], h->valk[1], h->newslot, h->cell32, h->ord_cnt, h->ord_off, h->route_geo_dev, h->xo_plan, h->gc_cnt, h->gc_off, h->half_mark, h->hmap, h->half_free, h->half_top, h->xo_jobs_acc, h->rast, h->G, h->free_rows, h->paths, h->bp_off, h->bp_loci, h->dom,
                  h->delet_loci, h->delet_s, h->cell_start, h->tag, h->cand, h->sort64_tmp, h->key64[0], h->key64[1], h->pairs2,
                  h->pair_goff, h->st_rec, h->st_z, h->st_geno, h->st_slots, h->req_pid, h->req_k, h->req_key, h->req_start, h->req_px, h->req_py,
                  h->req_count, h->sort_tmp, h->scan_tmp, h->mate,
                  h->flag, h->flag2, h->scan, h->pairs, h->nbirths, h->boff, h->off_pair,
                  h->off_parent, h->off_keys, h->off_start, h->keep_in, h->inj_a, h->inj_b,
                  h->mid_x, h->mid_y, h->p_death, h->d_cell, h->dead_in, h->nmax_bits, h->red,
                  h->sel_loci, h->path_sel, h->lat.areas, h->lat.cprime, h->spl_N.c, h->spl_P.c, h->bin_partials, h->nodes,
                  h->K_over, h->blk_cnt, h->blk_off, h->cnt_dev, h->tickets, h->nmax2, h->fb[0], h->gp_rec, h->gp_z, h->gp_slots, h->rq_sorted, h->rq_k, h->gam_out, h->gam_slot, h->chk,
                  h->lin_tab, h->lin_bt};
  for (void* p : ptrs) (void)hipFree(p);
  for (int t = 0; t < GNX_MAX_TRAITS; ++t) {
    (void)hipFree(h->traits[t].loci);
    (void)hipFree(h->traits[t].alpha);
    (void)hipFree(h->traits[t].phi_rast);
  }
  (void)hipHostFree(h->h_pin);
  if (h->h_route_pin) (void)hipHostFree(h->h_route_pin);
  (void)hipFree(h->gh_rec);
  (void)hipFree(h->route_cnt);
  if (h->h_stage) (void)hipHostFree(h->h_stage);
  for (int k = 0; k < GNX_K_COUNT; ++k) timers_resolve(h, k);
  for (hipEvent_t e : h->ev_free) (void)hipEventDestroy(e);
  if (h->own_stream) (void)hipStreamDestroy(h->stream);
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  h->stream2 = nullptr;
  if (h->stream3) {
    (void)hipStreamSynchronize(h->stream3);
    (void)hipStreamDestroy(h->stream3);
  }
  if (h->ev_ord) (void)hipEventDestroy(h->ev_ord);
  if (h->ev_compact) (void)hipEventDestroy(h->ev_compact);
  if (h->ev_fill) (void)hipEventDestroy(h->ev_fill);
  if (h->ev_alive) (void)hipEventDestroy(h->ev_alive);
  if (h->ev_moved) (void)hipEventDestroy(h->ev_moved);
  if (h->ev_perm_rest) (void)hipEventDestroy(h->ev_perm_rest);
  if (h->ev_pairs) (void)hipEventDestroy(h->ev_pairs);
  if (h->ev_latP) (void)hipEventDestroy(h->ev_latP);
  if (h->ev_perm) (void)hipEventDestroy(h->ev_perm);
  if (h->ev_binsN) (void)hipEventDestroy(h->ev_binsN);
  delete h;
}

extern "C" int gnx_set_stream(gnx_state* h, void* hip_stream) {
  GNXCHK(gnx_xo_join(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->stream2) HIPCHK(hipStreamSynchronize(h->stream2));
  if (h->own_stream) (void)hipStreamDestroy(h->stream);
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  h->stream2 = nullptr;          // no side stream next to a foreign stream: nothing is deferred
  h->stream = (hipStream_t)hip_stream;
  h->own_stream = false;
  return 0;
}

extern "C" int gnx_synchronize(gnx_state* h) {
  GNXCHK(gnx_xo_launch_pending(h));
  if (h->stream3) HIPCHK(hipStreamSynchronize(h->stream3));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->stream2) HIPCHK(hipStreamSynchronize(h->stream2));
  return 0;
}

// ---------------------------------------------------------------- setup
extern "C" int gnx_upload_rasters(gnx_state* h, const float* rasts) {
  size_t n = (size_t)h->cfg.n_layers * h->cfg.W * h->cfg.H;
  HIPCHK(hipMemcpyAsync(h->rast, rasts, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->e_stale = true;
  return 0;
}

extern "C" int gnx_upload_layer(gnx_state* h, int32_t layer, const float* rast) {
  if (layer < 0 || layer >= h->cfg.n_layers) {
    gnx_set_error("gnx_upload_layer: bad layer %d", layer);
    return 1;
  }
  size_t n = (size_t)h->cfg.W * h->cfg.H;
  HIPCHK(hipMemcpyAsync(h->rast + layer * n, rast, n * sizeof(float), hipMemcpyHostToDevice,
                        h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->e_stale = true;
  return 0;
}

// explicit carrying-capacity raster (Species.K after a demographic change event,
// ops/change.py:633-651); NULL returns to rast[K_layer] * K_factor
extern "C" int gnx_set_k_raster(gnx_state* h, const double* K) {
  h->cfg_epoch += 1;
  size_t n = (size_t)h->cfg.W * h->cfg.H;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!K) {
    (void)hipFree(h->K_over);
    h->K_over = nullptr;
    return 0;
  }
  if (!h->K_over) HIPCHK(hipMalloc((void**)&h->K_over, n * sizeof(double)));
  GNXCHK(gnx_h2d(h, h->K_over, K, n * sizeof(double)));
  return 0;
}

// density lattice geometry (utils/spatial.py:101-130,270-319): nodes at j*hww,
// j = 0..J-1, J-1 = largest even j with j*hww < dim + ww
static int lattice_nodes(int dim, double ww) {
  double hww = ww / 2.0;
  double last_edge = 0, last_inner = 0;
  // np.arange(0, d+ww, ww) and np.arange(hww, d+hww, ww)
  int ne = (int)ceil((dim + ww) / ww);
  last_edge = (ne - 1) * ww;
  int ni = (int)ceil(((dim + hww) - hww) / ww);
  last_inner = hww + (ni - 1) * ww;
  double last = std::max(last_edge, last_inner);
  return (int)llround(last / hww) + 1;
}

static int setup_lattice(gnx_state* h) {
  const gnx_config& c = h->cfg;
  double ww = h->sp.window_width;
  if (!(ww > 0)) ww = std::nearbyint(0.1 * std::max(c.W, c.H));   // python round (half-even)
  if (!(ww > 0)) ww = 1;
  GnxLattice& L = h->lat;
  (void)hipFree(L.areas);
  (void)hipFree(L.cprime);
  (void)hipFree(h->spl_N.c);
  (void)hipFree(h->spl_P.c);
  (void)hipFree(h->bin_partials);   // bins_P lives in the same allocation
  (void)hipFree(h->nodes);
  L.hww = ww / 2.0;
  L.Jx = lattice_nodes(c.W, ww);
  L.Jy = lattice_nodes(c.H, ww);
  L.nbx = L.Jx;
  L.nby = L.Jy;
  const int64_t nn = (int64_t)L.Jx * L.Jy;
  std::vector<double> areas(nn);
  for (int i = 0; i < L.Jy; ++i)
    for (int j = 0; j < L.Jx; ++j) {
      double cx = j * L.hww, cy = i * L.hww;
      double ax = std::min(cx + L.hww, (double)c.W) - std::max(cx - L.hww, 0.0);
      double ay = std::min(cy + L.hww, (double)c.H) - std::max(cy - L.hww, 0.0);
      double a = std::max(ax, 0.0) * std::max(ay, 0.0);
      if (a == 0) a = 0.0001;
      areas[(int64_t)i * L.Jx + j] = a;
    }
  int Jm = std::max(L.Jx, L.Jy);
  std::vector<double> cp(Jm + 1, 0.0);
  if (Jm > 1) cp[1] = 0.25;
  for (int k = 2; k < Jm; ++k) cp[k] = 1.0 / (4.0 - cp[k - 1]);
  GNXCHK(dalloc(&L.areas, nn));
  GNXCHK(dalloc(&L.cprime, Jm + 1));
  GNXCHK(dalloc(&h->spl_N.c, 4 * nn));
  GNXCHK(dalloc(&h->spl_P.c, 4 * nn));
  GNXCHK(dalloc(&h->nodes, nn));
  size_t nb = (size_t)L.nbx * L.nby;
  // one allocation, so that a tiled run all-reduces both fields in one call
  GNXCHK(dalloc(&h->bin_partials, 2 * nb + 4));     // (+ the tile2 counter words)
  h->bins_P = h->bin_partials + nb;
  (void)hipFree(h->fb[0]);
  GNXCHK(dalloc(&h->fb[0], 3 * nb));
  h->fb[1] = h->fb[0] + nb;
  h->fb[2] = h->fb[0] + 2 * nb;
  HIPCHK(hipMemset(h->fb[0], 0, 3 * nb * sizeof(int32_t)));
  h->fb_zero[0] = h->fb_zero[1] = h->fb_zero[2] = true;
  h->fb_adults = false;
  h->nmax_ready = false;
  HIPCHK(hipMemcpy(L.areas, areas.data(), nn * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(L.cprime, cp.data(), (Jm + 1) * sizeof(double), hipMemcpyHostToDevice));
  h->spl_N.valid = h->spl_P.valid = false;
  h->bins_zeroed[0] = h->bins_zeroed[1] = false;
  h->nmax_zeroed = false;
  return 0;
}

static int setup_hash_grid(gnx_state* h) {
  const gnx_config& c = h->cfg;
  double r = h->sp.mating_radius;
  double cs = r > 0 ? r * (1.0 + 1e-9) : 8.0;
  // nearest-mate choice walks outwards ring by ring over FINE cells (an eighth of the
  // radius): in a clumped population the 3 x 3 block of radius-sized cells holds thousands
  // of candidates, the nearest one sits a fraction of a cell away
  if (r > 0 && h->sp.mate_mode == GNX_MATE_NEAREST) cs /= 8.0;
  // uniform / inverse-distance choice, GNX_CELL_DIV=2 (opt-in, read per call): cells of HALF a
  // radius and the 5 x 5 block around the focal one's (6.25 r^2 of candidates instead of 9 r^2,
  // VERDICT r5 #5).  The canonical candidate order is that of this grid, in the oracle too
  // (oracle/gnx_oracle.py: hash_grid).  Measured at the steady states (profiles/r06_ab_runs.txt):
  // C2 / C3 unchanged, the metric workload 4 % slower (two more key bits, four times the cell
  // bounds, against a rejection rate that falls from 65 to 50 %) - so the default stays 1.
  else if (r > 0) {
    const int cell_div = std::max(1, std::min(2, gnx_env_int("GNX_CELL_DIV", 1)));
    cs /= (double)cell_div;
  }
  // bound the number of cells (<= 2048 per axis)
  cs = std::max(cs, std::max(c.W, c.H) / 2048.0);
  h->cell_ref = r > 0 ? std::max(1, (int)ceil(r * (1.0 + 1e-9) / cs - 1e-12)) : 1;
  h->cs = cs;
  h->inv_cs = 1.0 / cs;
  h->ncx = std::max(1, (int)ceil(c.W / cs));
  h->ncy = std::max(1, (int)ceil(c.H / cs));
  int64_t ncells = (int64_t)h->ncx * h->ncy;
  int bits = 1;
  while ((1ll << bits) < ncells) bits++;
  h->key_bits = bits;
  (void)hipFree(h->cell_start);
  GNXCHK(dalloc(&h->cell_start, ncells + 1));
  return 0;
}

extern "C" int gnx_set_species_params(gnx_state* h, const gnx_species_params* p) {
  h->cfg_epoch += 1;
  if (p->K_layer < 0 || p->K_layer >= h->cfg.n_layers ||
      (p->move_surf && (p->move_surf_layer < 0 || p->move_surf_layer >= h->cfg.n_layers)) ||
      (p->disp_surf && (p->disp_surf_layer < 0 || p->disp_surf_layer >= h->cfg.n_layers))) {
    gnx_set_error("gnx_set_species_params: layer index out of range");
    return 1;
  }
  if (p->n_births_fixed && (p->n_births_lambda < 0 || p->n_births_lambda != floor(p->n_births_lambda))) {
    gnx_set_error("gnx_set_species_params: n_births_fixed needs an integer lambda");
    return 1;
  }
  // k_births multiplies at most the 64 uniforms of its stream, so the mass of k >= 64 would
  // collapse onto 64: 2.4e-10 at lambda = 26, 1.0e-9 at 27, 4.4e-3 at 45
  if (!p->n_births_fixed && !(p->n_births_lambda <= GNX_BIRTHS_LAMBDA_MAX)) {
    gnx_set_error("gnx_set_species_params: n_births_lambda %g is above %d, the limit of the "
                  "Poisson births (64 uniforms per pair)", p->n_births_lambda,
                  GNX_BIRTHS_LAMBDA_MAX);
    return 1;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  h->sp = *p;
  h->have_sp = true;
  GNXCHK(setup_lattice(h));
  GNXCHK(setup_hash_grid(h));
  if (!h->counts_rast[0]) {
    GNXCHK(dalloc(&h->counts_rast[0], (size_t)h->cfg.W * h->cfg.H));
    GNXCHK(dalloc(&h->counts_rast[1], (size_t)h->cfg.W * h->cfg.H));
  }
  return 0;
}

static int need_params(gnx_state* h) {
  if (!h->have_sp) {
    gnx_set_error("species parameters not set (gnx_set_species_params)");
    return 1;
  }
  return 0;
}

extern "C" int gnx_upload_population(gnx_state* h, int64_t N, const float* x, const float* y,
                                     const int32_t* age, const uint8_t* sex, const int64_t* id) {
  h->cfg_epoch += 1;
  if (N > h->cfg.cap_inds) {
    gnx_set_error("gnx_upload_population: N %lld > cap_inds %lld", (long long)N,
                  (long long)h->cfg.cap_inds);
    return 1;
  }
  for (int64_t i = 0; i < N; ++i) {
    if (!(x[i] >= 0 && x[i] < h->cfg.W && y[i] >= 0 && y[i] < h->cfg.H)) {
      gnx_set_error("gnx_upload_population: individual %lld at (%g, %g) is off the landscape",
                    (long long)i, (double)x[i], (double)y[i]);
      return 1;
    }
  }
  GNXCHK(gnx_xo_join(h));
  GnxSoA s = h->soa[h->cur];
  hipStream_t st = h->stream;
  HIPCHK(hipMemcpyAsync(s.x, x, N * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(s.y, y, N * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(s.age, age, N * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(s.sex, sex, N * sizeof(uint8_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(s.id, id, N * sizeof(int64_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(s.grow, 0xff, N * sizeof(int32_t), st));
  HIPCHK(hipMemsetAsync(s.fit, 0, N * sizeof(float), st));
  HIPCHK(hipMemsetAsync(s.ghost, 0, N, st));
  h->n_ghost = 0;
  HIPCHK(hipStreamSynchronize(st));
  h->N = N;
  int64_t mx = -1;
  bool asc = true;
  for (int64_t i = 0; i < N; ++i) {
    asc = asc && id[i] > mx;
    mx = std::max(mx, id[i]);
  }
  h->max_id = mx;
  // ids ascending in slot order: the id-ordered index is the identity (ord_n = 0 explicit
  // entries); otherwise the next cell sort rebuilds it
  h->ord_valid = asc;
  h->ord_n = 0;
  h->genomes_assigned = false;
  // environment values (Species._set_e at creation, structs/species.py:3318)
  GNXCHK(gnx_l_gather_e(h, 0, N));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int gnx_init_population(gnx_state* h, int64_t N) {
  h->cfg_epoch += 1;
  if (N > h->cfg.cap_inds) {
    gnx_set_error("gnx_init_population: N > cap_inds");
    return 1;
  }
  GNXCHK(gnx_xo_join(h));
  h->genomes_assigned = false;
  GNXCHK(gnx_l_init_population(h, N));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---------------------------------------------------------------- genomic architecture
extern "C" int gnx_set_recomb_paths(gnx_state* h, int32_t n, const uint64_t* paths) {
  h->cfg_epoch += 1;
  if (h->cfg.L == 0 || n <= 0) {
    gnx_set_error("gnx_set_recomb_paths: species has no genome or n <= 0");
    return 1;
  }
  const int W64 = h->W64, L = h->cfg.L;
  // a crossover job packs path * 2 + start homologue into the low 24 bits of GnxXoJob.ks
  if (n >= (1 << 23)) {
    gnx_set_error("gnx_set_recomb_paths: at most %d cached paths (got %d)", (1 << 23) - 1, n);
    return 1;
  }
  GNXCHK(gnx_xo_join(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  (void)hipFree(h->paths);
  (void)hipFree(h->bp_off);
  (void)hipFree(h->bp_loci);
  h->paths = nullptr;
  h->bp_off = h->bp_loci = nullptr;
  // breakpoint CSR: loci where the path switches homologue
  std::vector<int32_t> off(n + 1, 0), loci;
  int max_bp = 0;
  for (int k = 0; k < n; ++k) {
    const uint64_t* p = paths + (size_t)k * W64;
    uint64_t carry = 0;      // path bit of locus -1 := 0
    int cnt = 0;
    for (int w = 0; w * 64 < L; ++w) {
      uint64_t v = p[w];
      if (L - w * 64 < 64) v &= (1ull << (L - w * 64)) - 1ull;
      uint64_t t = v ^ ((v << 1) | carry);          // bit l set <=> path switches at l
      if (L - w * 64 < 64) t &= (1ull << (L - w * 64)) - 1ull;
      carry = v >> 63;
      while (t) {
        int bpos = __builtin_ctzll(t);
        loci.push_back(w * 64 + bpos);
        cnt++;
        t &= t - 1;
      }
    }
    off[k + 1] = (int32_t)loci.size();
    max_bp = std::max(max_bp, cnt);
  }
  h->sparse_paths = max_bp <= GNX_SPARSE_MAX_BP;
  // dense masks switch in every block: nothing can be shared, and whole homologues stream
  // better than 1.8-KB pieces (6.9 against 6.6 TB/s) - one block per homologue then, as long
  // as no genome has been laid out yet
  if (!h->genomes_assigned) {
    h->NB = h->sparse_paths ? h->NB_alloc : 1;
    h->BW = h->sparse_paths ? h->BW_alloc : h->W64;
  }
  h->n_paths = n;
  // padding bits beyond L must be zero so children keep zero padding
  std::vector<uint64_t> clean(paths, paths + (size_t)n * W64);
  for (int k = 0; k < n; ++k)
    for (int l = L; l < W64 * 64; ++l) clean[(size_t)k * W64 + (l >> 6)] &= ~(1ull << (l & 63));
  GNXCHK(dalloc(&h->paths, (size_t)n * W64));
  GNXCHK(dalloc(&h->bp_off, n + 1));
  GNXCHK(dalloc(&h->bp_loci, loci.size()));
  HIPCHK(hipMemcpy(h->paths, clean.data(), (size_t)n * W64 * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->bp_off, off.data(), (n + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  if (!loci.empty())
    HIPCHK(hipMemcpy(h->bp_loci, loci.data(), loci.size() * sizeof(int32_t),
                     hipMemcpyHostToDevice));
  GNXCHK(gnx_l_path_sel(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int gnx_set_trait(gnx_state* h, int32_t t, int32_t n_loci, const int32_t* loci,
                             const double* alpha, int32_t layer, double phi,
                             const float* phi_rast, double gamma, int32_t univ_adv) {
  h->cfg_epoch += 1;
  if (t < 0 || t >= h->cfg.n_traits || n_loci <= 0 || layer < 0 || layer >= h->cfg.n_layers) {
    gnx_set_error("gnx_set_trait: bad trait index, locus count or layer");
    return 1;
  }
  for (int j = 0; j < n_loci; ++j)
    if (loci[j] < 0 || loci[j] >= h->cfg.L) {
      gnx_set_error("gnx_set_trait: locus %d out of range", loci[j]);
      return 1;
    }
  HIPCHK(hipStreamSynchronize(h->stream));
  GnxTrait& r = h->traits[t];
  (void)hipFree(r.loci);
  (void)hipFree(r.alpha);
  (void)hipFree(r.phi_rast);
  r.phi_rast = nullptr;
  GNXCHK(dalloc(&r.loci, n_loci));
  GNXCHK(dalloc(&r.alpha, n_loci));
  HIPCHK(hipMemcpy(r.loci, loci, n_loci * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(r.alpha, alpha, n_loci * sizeof(double), hipMemcpyHostToDevice));
  if (phi_rast) {
    size_t n = (size_t)h->cfg.W * h->cfg.H;
    GNXCHK(dalloc(&r.phi_rast, n));
    HIPCHK(hipMemcpy(r.phi_rast, phi_rast, n * sizeof(float), hipMemcpyHostToDevice));
  }
  r.n_loci = n_loci;
  r.layer = layer;
  r.phi = phi;
  r.gamma = gamma;
  r.univ_adv = univ_adv;
  h->h_trait_loci[t].assign(loci, loci + n_loci);
  return gnx_l_rebuild_sel(h);
}

// The selected loci (all trait loci trait-major, then the deleterious loci), the homologue
// every cached path is on at them (path_sel) and every individual's alleles there
// (GnxSoA.tb): rebuilt whenever a trait or the deleterious loci change (also after
// non-neutral mutations, structs/genome.py:753-788).
int gnx_l_rebuild_sel(gnx_state* h) {
  h->cfg_epoch += 1;
  std::vector<int32_t> all;
  for (int q = 0; q < h->cfg.n_traits; ++q)
    all.insert(all.end(), h->h_trait_loci[q].begin(), h->h_trait_loci[q].end());
  h->n_tl = (int)all.size();
  all.insert(all.end(), h->h_delet_loci.begin(), h->h_delet_loci.end());
  GNXCHK(gnx_xo_join(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  (void)hipFree(h->sel_loci);
  h->sel_loci = nullptr;
  h->n_sel = (int)all.size();
  const int TW = (h->n_sel + 63) / 64;
  if (TW != h->TW) {
    for (int k = 0; k < 2; ++k) {
      (void)hipFree(h->soa[k].tb);
      h->soa[k].tb = nullptr;
      if (TW > 0) {
        GNXCHK(dalloc(&h->soa[k].tb, (size_t)h->cfg.cap_inds * 2 * TW));
        HIPCHK(hipMemset(h->soa[k].tb, 0, (size_t)h->cfg.cap_inds * 2 * TW * 8));
      }
    }
    h->TW = TW;
  }
  if (h->n_sel > 0) {
    GNXCHK(dalloc(&h->sel_loci, all.size()));
    HIPCHK(hipMemcpy(h->sel_loci, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  GNXCHK(gnx_l_path_sel(h));
  if (h->genomes_assigned) GNXCHK(gnx_l_tb_from_rows(h, 0, h->N, nullptr, nullptr));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int gnx_set_dominance(gnx_state* h, const uint8_t* dom) {
  h->cfg_epoch += 1;
  HIPCHK(hipStreamSynchronize(h->stream));
  (void)hipFree(h->dom);
  h->dom = nullptr;
  if (!dom) return 0;
  bool any = false;
  for (int l = 0; l < h->cfg.L; ++l) any = any || dom[l];
  if (!any) return 0;       // GenomicArchitecture._use_dom (structs/genome.py:555)
  GNXCHK(dalloc(&h->dom, h->cfg.L));
  HIPCHK(hipMemcpy(h->dom, dom, h->cfg.L, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int gnx_set_deleterious(gnx_state* h, int32_t n, const int32_t* loci,
                                   const double* s) {
  h->cfg_epoch += 1;
  HIPCHK(hipStreamSynchronize(h->stream));
  (void)hipFree(h->delet_loci);
  (void)hipFree(h->delet_s);
  h->delet_loci = nullptr;
  h->delet_s = nullptr;
  h->n_delet = 0;
  h->h_delet_loci.clear();
  if (n <= 0) return gnx_l_rebuild_sel(h);
  for (int j = 0; j < n; ++j)
    if (loci[j] < 0 || loci[j] >= h->cfg.L) {
      gnx_set_error("gnx_set_deleterious: locus out of range");
      return 1;
    }
  GNXCHK(dalloc(&h->delet_loci, n));
  GNXCHK(dalloc(&h->delet_s, n));
  HIPCHK(hipMemcpy(h->delet_loci, loci, n * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->delet_s, s, n * sizeof(double), hipMemcpyHostToDevice));
  h->n_delet = n;
  h->h_delet_loci.assign(loci, loci + n);
  return gnx_l_rebuild_sel(h);
}

static int need_genome(gnx_state* h) {
  if (h->cfg.L == 0) {
    gnx_set_error("species has no genome (L == 0)");
    return 1;
  }
  return 0;
}

extern "C" int gnx_upload_genomes(gnx_state* h, const uint64_t* geno) {
  h->cfg_epoch += 1;
  GNXCHK(need_genome(h));
  GNXCHK(gnx_l_assign_genomes(h, nullptr));     // rows 0..N-1 in slot order
  const size_t rowb = (size_t)2 * h->W64 * 8;
  // zero the padding bits beyond L
  std::vector<uint64_t> tmp(geno, geno + (size_t)h->N * 2 * h->W64);
  for (int64_t r = 0; r < h->N * 2; ++r)
    for (int l = h->cfg.L; l < h->W64 * 64; ++l)
      tmp[(size_t)r * h->W64 + (l >> 6)] &= ~(1ull << (l & 63));
  uint64_t* d_tmp = nullptr;
  GNXCHK(dalloc(&d_tmp, (size_t)h->N * 2 * h->W64));
  int rc = gnx_h2d(h, d_tmp, tmp.data(), (size_t)h->N * rowb);
  if (!rc) rc = gnx_l_scatter_genomes(h, h->N, d_tmp, 0);
  (void)hipStreamSynchronize(h->stream);
  (void)hipFree(d_tmp);
  GNXCHK(rc);
  GNXCHK(gnx_l_tb_from_rows(h, 0, h->N, nullptr, nullptr));
  if (h->cfg.n_traits > 0) GNXCHK(gnx_l_phenotype(h, 0, h->N));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int gnx_assign_genomes(gnx_state* h, const int32_t* n_per_site) {
  h->cfg_epoch += 1;
  GNXCHK(need_genome(h));
  int32_t* d = nullptr;
  GNXCHK(dalloc(&d, h->cfg.L));
  HIPCHK(hipMemcpy(d, n_per_site, h->cfg.L * sizeof(int32_t), hipMemcpyHostToDevice));
  int r = gnx_l_assign_genomes(h, d);
  if (!r) r = gnx_l_tb_from_rows(h, 0, h->N, nullptr, nullptr);
  if (!r && h->cfg.n_traits > 0) r = gnx_l_phenotype(h, 0, h->N);
  (void)hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  return r;
}

extern "C" int gnx_set_z(gnx_state* h) {
  GNXCHK(need_genome(h));
  if (!h->genomes_assigned) {
    gnx_set_error("gnx_set_z: genomes not assigned");
    return 1;
  }
  GNXCHK(gnx_l_tb_from_rows(h, 0, h->N, nullptr, nullptr));
  GNXCHK(gnx_l_phenotype(h, 0, h->N));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int gnx_set_z_range(gnx_state* h, int64_t first, int64_t n) {
  GNXCHK(need_genome(h));
  if (!h->genomes_assigned || first < 0 || n < 0 || first + n > h->N) {
    gnx_set_error("gnx_set_z_range: genomes not assigned or range out of bounds");
    return 1;
  }
  GNXCHK(gnx_l_tb_from_rows(h, first, n, nullptr, nullptr));
  GNXCHK(gnx_l_phenotype(h, first, n));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---------------------------------------------------------------- step
extern "C" int gnx_age(gnx_state* h) { return gnx_l_age(h); }

extern "C" int gnx_move(gnx_state* h) {
  GNXCHK(need_params(h));
  return gnx_l_move(h, false, nullptr, nullptr, nullptr, nullptr, true);
}

static int check_recomb_ready(gnx_state* h, bool burn) {
  if (!burn && h->cfg.L > 0 && h->genomes_assigned && h->n_paths == 0) {
    gnx_set_error("recombination paths not set (gnx_set_recomb_paths)");
    return 1;
  }
  for (int t = 0; t < h->cfg.n_traits; ++t)
    if (h->traits[t].n_loci == 0) {
      gnx_set_error("trait %d not set (gnx_set_trait)", t);
      return 1;
    }
  return 0;
}

extern "C" int gnx_pop_dynamics_mate(gnx_state* h, int32_t burn) {
  GNXCHK(need_params(h));
  GNXCHK(check_recomb_ready(h, burn != 0));
  int64_t P = 0, B = 0;
  h->tile2_mode = false;
  // 1. mating pairs (cell-sorted population)
  //    (the columns the mate search and the pair list do not read are permuted on the side
  //    stream meanwhile, and waited for before the births)
  GNXCHK(gnx_l_sort_by_cell(h, true));
  // 2. n_pairs density of the pair midpoints (ops/demography.py:60-91), launched inside
  //    find_pairs while the pair count travels to the host
  int rc_pairs = gnx_l_find_pairs(h, nullptr, &P, true);
  GNXCHK(gnx_wait_permute_rest(h));
  GNXCHK(rc_pairs);
  if (P > 0 && !h->spl_P.valid)
    GNXCHK(gnx_l_density(h, P, h->mid_x, h->mid_y, &h->spl_P, nullptr));
  // 3. births: dispersal, crossover, phenotype (tile-major offspring ids, gnx_set_id_order: the
  //    pairs' offsets from this device's own counts - gnx_l_mate)
  GNXCHK(gnx_l_mate(h, burn != 0, false, 0, &B));
  h->last_births = B;
  return 0;
}

extern "C" int gnx_pop_dynamics_die(gnx_state* h, int32_t burn, int32_t with_selection) {
  GNXCHK(need_params(h));
  int64_t D = 0;
  // 4. N density of everyone incl. offspring (structs/species.py:845-882)
  GNXCHK(gnx_l_density_N(h));
  // 5-6. d at each individual's cell, fitness, death probability
  GNXCHK(gnx_l_death_probs(h, with_selection != 0 && !burn));
  // 7. mortality
  GNXCHK(gnx_l_mortality(h, nullptr, &D));
  h->last_deaths = D;
  return 0;
}

extern "C" int gnx_pop_dynamics(gnx_state* h, int32_t burn, int32_t with_selection) {
  GNXCHK(gnx_pop_dynamics_mate(h, burn));
  return gnx_pop_dynamics_die(h, burn, with_selection);
}

// One step in three parts, so that several handles can be stepped side by side from one
// host thread (gnx_step_many): _begin enqueues age, movement, cell sort, mate search and the
// pair list; _mid reads the pair count and enqueues births, densities, death probabilities,
// death draws, compaction and the crossover; _end reads the survivor counts.  Each handle
// has its own three streams: what one handle enqueues runs beside the others' kernels.
struct GnxStepTimer {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  bool count;
  explicit GnxStepTimer(bool c) : count(c) {}
  ~GnxStepTimer() {
    if (gnx_host_times()) {
      g_host_step_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (count) ++g_host_steps;
    }
  }
};

extern "C" int gnx_step_begin(gnx_state* h, int32_t burn) {
  GNXCHK(need_params(h));
  GNXCHK(check_recomb_ready(h, burn != 0));
  GnxStepTimer timer(true);
  if (h->mort_wait || h->pairs_wait) {
    gnx_set_error("gnx_step_begin: the previous step of this handle was not finished (gnx_step_end)");
    return 1;
  }
  h->tot[0] += 1;
  h->tot[1] += h->N - h->n_ghost;
  h->last_xo_births = 0;
  h->step_burn = burn != 0;
  h->tile2_mode = false;        // (a handle that stepped through the tile protocol before)
  if (h->moved_ahead) {
    // the last step's mortality launched this movement beside its job builder (gnx_l_move_ahead)
    GNXCHK(gnx_move_ahead_join(h));
  } else if (h->sp.move) {
    h->move_writes_keys = h->sp.mating_radius >= 0;     // the cell sort follows at once
    int rc = gnx_l_move(h, true, nullptr, nullptr, nullptr, nullptr, true);
    h->move_writes_keys = false;
    GNXCHK(rc);
  } else {
    GNXCHK(gnx_l_age(h));
  }
  // mating pairs (cell-sorted population; the columns the mate search and the pair list do
  // not read are permuted on the side stream meanwhile, and waited for before the births);
  // the n_pairs density of the pair midpoints (ops/demography.py:60-91) is launched with the
  // pair list, while the pair count travels to the host
  GNXCHK(gnx_l_sort_by_cell(h, true));
  int rc_pairs = gnx_l_find_pairs_enqueue(h, nullptr, true);
  GNXCHK(gnx_wait_permute_rest(h));
  return rc_pairs;
}

extern "C" int gnx_step_mid(gnx_state* h, int32_t burn, int32_t with_selection) {
  GnxStepTimer timer(false);
  int64_t P = 0, B = 0;
  const bool counted = h->pairs_wait;
  GNXCHK(gnx_l_find_pairs_count(h, &P));
  // The last step's crossover held back for this pair list (xo_launch_late) goes on its stream
  // BEHIND the births' enqueue: the births head the step's chain (births -> density -> death
  // probabilities -> death draws), nobody but the next crossover reads this one's rows, and handing
  // it over costs the host a wait, one or two launches and one or two records - the time the
  // births used to become runnable later than a crossover that fills the chip.  It still waits
  // for the pair list alone (ev_pairs, recorded behind k_pair_compact), not for the births.
  // (Offspring that nobody gave their crossover - xo_deferred, a step cut short - make gnx_l_mate
  // launch the held-back one itself, and Poisson births make the host wait for their sum - the
  // crossover would stand idle meanwhile: the old order for both.)
  const bool held = counted && h->xo_launch_late && h->xo_ready_buf >= 0;
  const bool births_first =
      held && h->pairs_ev && !h->xo_deferred && !h->tiled && h->sp.n_births_fixed;
  if (held && !births_first) GNXCHK(gnx_xo_launch_pending(h, GNX_PC_XO_P2));
  if (P > 0 && !h->spl_P.valid)
    GNXCHK(gnx_l_density(h, P, h->mid_x, h->mid_y, &h->spl_P, nullptr));
  // births: dispersal, alleles at the selected loci, phenotype (tile-major offspring ids,
  // gnx_set_id_order: the pairs' offsets from this device's own counts - gnx_l_mate)
  int rc = gnx_l_mate(h, burn != 0, false, 0, &B);
  // (whatever became of the births - none, or too many for the handle: once, here)
  if (births_first) {
    const int rc_xo = gnx_xo_launch_pending(h, GNX_PC_XO_P2, h->ev_pairs);
    if (!rc) rc = rc_xo;
  }
  GNXCHK(rc);
  h->last_births = B;
  // N density of everyone incl. offspring (structs/species.py:845-882); d at each
  // individual's cell, fitness, death probability; mortality
  GNXCHK(gnx_l_density_N(h));
  GNXCHK(gnx_l_death_probs(h, with_selection != 0 && !burn));
  return gnx_l_mortality_enqueue(h, nullptr);
}

extern "C" int gnx_step_end(gnx_state* h, int32_t burn) {
  GnxStepTimer timer(false);
  int64_t D = 0;
  GNXCHK(gnx_l_mortality_finish(h, &D));
  h->last_deaths = D;
  h->step += 1;
  h->tot[2] += h->last_births;
  h->tot[3] += h->last_deaths;
  if (!burn) h->tot[4] += h->last_xo_births;
  return 0;
}

extern "C" int gnx_step(gnx_state* h, int32_t burn, int32_t with_selection) {
  GNXCHK(gnx_step_begin(h, burn));
  GNXCHK(gnx_step_mid(h, burn, with_selection));
  return gnx_step_end(h, burn);
}

// n independent handles (the iterations of one model, sim/model.py:866-953 - the reference
// runs them one after another and notes at :924-925 that they could be farmed out), one step
// each: all first thirds, then all second thirds, then all last thirds.
extern "C" int gnx_step_many(gnx_state** hs, int32_t n, int32_t burn, int32_t with_selection) {
  for (int k = 0; k < n; ++k) GNXCHK(gnx_step_begin(hs[k], burn));
  for (int k = 0; k < n; ++k) GNXCHK(gnx_step_mid(hs[k], burn, with_selection));
  for (int k = 0; k < n; ++k) GNXCHK(gnx_step_end(hs[k], burn));
  return 0;
}

// 0: offspring ids in the canonical (hash cell, focal id) order of the pairs over the whole
// landscape (default); 1: virtual tile by virtual tile (gnx_kernels_pop.hip) - what
// gnx_tile_step uses, and what a one-device run must use to reproduce a tiled run id by id
extern "C" int gnx_set_id_order(gnx_state* h, int32_t mode) {
  if (mode != 0 && mode != 1) {
    gnx_set_error("gnx_set_id_order: 0 (hash cell, focal id) or 1 (virtual-tile-major)");
    return 1;
  }
  if (mode == 1 && (h->cfg.W % 8 || h->cfg.H % 8)) {
    gnx_set_error("tile-major offspring ids need landscape dimensions divisible by 8");
    return 1;
  }
  if (mode == 1) GNXCHK(gnx_vt_buffers(h));
  h->id_order = mode;
  h->cfg_epoch += 1;
  return 0;
}

extern "C" int gnx_totals(gnx_state* h, int64_t* out) {
  for (int k = 0; k < 6; ++k) out[k] = h->tot[k];
  return 0;
}

extern "C" int gnx_reset_totals(gnx_state* h) {
  for (int k = 0; k < 6; ++k) h->tot[k] = 0;
  return 0;
}

extern "C" int gnx_path_counts(gnx_state* h, int64_t* out, int32_t n) {
  for (int k = 0; k < n; ++k) out[k] = k < GNX_PC_COUNT ? h->pc[k] : 0;
  return GNX_PC_COUNT;
}

extern "C" int gnx_reset_path_counts(gnx_state* h) {
  for (int k = 0; k < GNX_PC_COUNT; ++k) h->pc[k] = 0;
  return 0;
}

// ---- pedigree of the last births (tree-sequence recording on the host; reference
// structs/species.py:692-736 adds these rows to its tskit tables one offspring at a time)
__global__ void k_gather_births(int64_t B, int64_t first, GnxSoA s, const int32_t* off_parent,
                                int64_t* child_id, int64_t* parent_id, float* xy) {
  int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  child_id[k] = s.id[first + k];
  parent_id[2 * k] = s.id[off_parent[2 * k]];
  parent_id[2 * k + 1] = s.id[off_parent[2 * k + 1]];
  xy[2 * k] = s.x[first + k];
  xy[2 * k + 1] = s.y[first + k];
}

extern "C" int gnx_last_births(gnx_state* h, int64_t* child_id, int64_t* parent_id, int32_t* keys,
                               uint8_t* starts, float* xy) {
  const int64_t B = h->last_births;
  if (B <= 0) return 0;
  if (B > h->N) {
    gnx_set_error("gnx_last_births: call it between gnx_pop_dynamics_mate and _die");
    return 1;
  }
  int64_t *d_c = nullptr, *d_p = nullptr;
  float* d_xy = nullptr;
  GNXCHK(dalloc(&d_c, B));
  GNXCHK(dalloc(&d_p, 2 * B));
  GNXCHK(dalloc(&d_xy, 2 * B));
  hipLaunchKernelGGL(k_gather_births, dim3(gnx_grid(B, 256)), dim3(256), 0, h->stream, B,
                     h->N - B, h->soa[h->cur], h->off_parent, d_c, d_p, d_xy);
  int rc = gnx_d2h(h, child_id, d_c, B * 8);
  if (!rc) rc = gnx_d2h(h, parent_id, d_p, 2 * B * 8);
  if (!rc) rc = gnx_d2h(h, xy, d_xy, 2 * B * 4);
  if (!rc && keys) rc = gnx_d2h(h, keys, h->off_keys, 2 * B * 4);
  if (!rc && starts) rc = gnx_d2h(h, starts, h->off_start, 2 * B);
  (void)hipFree(d_c);
  (void)hipFree(d_p);
  (void)hipFree(d_xy);
  HIPCHK(hipGetLastError());
  return rc;
}

extern "C" int gnx_counts(gnx_state* h, int64_t* N, int64_t* births, int64_t* deaths) {
  if (N) *N = h->N - h->n_ghost;
  if (births) *births = h->last_births;
  if (deaths) *deaths = h->last_deaths;
  return 0;
}

extern "C" int gnx_set_defer_crossover(gnx_state* h, int32_t on) {
  h->cfg_epoch += 1;
  GNXCHK(gnx_xo_join(h));
  h->defer_xo = on != 0;
  return 0;
}

extern "C" int64_t gnx_last_crossover_births(gnx_state* h) { return h->last_xo_births; }

// the job list of the last crossover (kernel lab: tools/xo_lab.hip replays it)
extern "C" int gnx_last_crossover_jobs(gnx_state* h, void* dst, int64_t max_jobs, int64_t* n_jobs) {
  GNXCHK(gnx_xo_join(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  const int buf = h->jobs_cur ^ 1;
  int32_t n = 0;
  HIPCHK(hipMemcpy(&n, h->n_jobs_dev[buf], sizeof(n), hipMemcpyDeviceToHost));
  *n_jobs = n;
  if (dst && n > 0)
    HIPCHK(hipMemcpy(dst, h->jobs[buf], (size_t)std::min<int64_t>(n, max_jobs) * 16,
                     hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int gnx_set_crossover_overlap(gnx_state* h, int32_t mode) {
  h->cfg_epoch += 1;
  GNXCHK(gnx_xo_join(h));
  h->xo_sort_waits = mode != 1;
  h->xo_wait_at = mode == 2 ? 2 : 1;      // 2: nothing else runs beside the crossover
  // (the other modes launch the crossover as soon as its jobs are built)
  h->xo_launch_late = mode == 0 && h->xo_launch_late_default;
  return 0;
}

// wide_per_1024 of every deferred crossover's jobs run at full width before the next cell
// sort, the rest narrow beside the sort and what follows it (0 or 1024: one launch)
extern "C" int gnx_set_crossover_split(gnx_state* h, int32_t wide_per_1024) {
  h->cfg_epoch += 1;
  GNXCHK(gnx_xo_join(h));
  h->xo_split = std::min(1024, std::max(0, (int)wide_per_1024));
  return 0;
}

// occupied slots, ghosts of a tiled step included (gnx_counts reports the tile's own)
extern "C" int64_t gnx_n_slots(gnx_state* h) { return h->N; }
extern "C" int64_t gnx_step_index(gnx_state* h) { return h->step; }
extern "C" int gnx_set_step_index(gnx_state* h, int64_t step) {
  h->step = step;
  return 0;
}

extern "C" int gnx_mutate(gnx_state* h, int32_t n, const int64_t* slot, const int32_t* locus,
                          const uint8_t* hom) {
  GNXCHK(need_genome(h));
  if (n <= 0) return 0;
  for (int i = 0; i < n; ++i)
    if (slot[i] < 0 || slot[i] >= h->N || locus[i] < 0 || locus[i] >= h->cfg.L || hom[i] > 1) {
      gnx_set_error("gnx_mutate: entry %d out of range", i);
      return 1;
    }
  int64_t* ds;
  int32_t* dl;
  uint8_t* dh;
  GNXCHK(dalloc(&ds, n));
  GNXCHK(dalloc(&dl, n));
  GNXCHK(dalloc(&dh, n));
  HIPCHK(hipMemcpy(ds, slot, n * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dl, locus, n * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dh, hom, n, hipMemcpyHostToDevice));
  int r = gnx_l_mutate(h, n, ds, dl, dh);
  // the compact allele table follows only where a selected locus was hit
  bool hit = false;
  if (h->n_sel > 0) {
    std::vector<int32_t> sel;
    for (int q = 0; q < h->cfg.n_traits; ++q)
      sel.insert(sel.end(), h->h_trait_loci[q].begin(), h->h_trait_loci[q].end());
    sel.insert(sel.end(), h->h_delet_loci.begin(), h->h_delet_loci.end());
    std::sort(sel.begin(), sel.end());
    for (int i = 0; i < n && !hit; ++i) hit = std::binary_search(sel.begin(), sel.end(), locus[i]);
  }
  if (!r && hit) r = gnx_l_tb_from_rows(h, 0, n, nullptr, ds);
  (void)hipStreamSynchronize(h->stream);
  (void)hipFree(ds);
  (void)hipFree(dl);
  (void)hipFree(dh);
  return r;
}

// ---------------------------------------------------------------- read-back
extern "C" int gnx_download(gnx_state* h, int32_t field, void* dst, int64_t dst_bytes) {
  GnxSoA s = h->soa[h->cur];
  const int64_t N = h->N, cap = h->cfg.cap_inds;
  const void* src = nullptr;
  int64_t elt = 0, planes = 1;
  switch (field) {
    case GNX_F_X: src = s.x; elt = 4; break;
    case GNX_F_Y: src = s.y; elt = 4; break;
    case GNX_F_AGE: src = s.age; elt = 4; break;
    case GNX_F_SEX: src = s.sex; elt = 1; break;
    case GNX_F_ID: src = s.id; elt = 8; break;
    case GNX_F_E: src = s.e; elt = 4; planes = h->cfg.n_layers; break;
    case GNX_F_Z: src = s.z; elt = 4; planes = h->cfg.n_traits; break;
    case GNX_F_FIT: src = s.fit; elt = 4; break;
    case GNX_F_GROW: src = s.grow; elt = 4; break;
    case GNX_F_GENO: {
      GNXCHK(need_genome(h));
      int64_t need = N * 2 * h->W64 * 8;
      if (dst_bytes < need) {
        gnx_set_error("gnx_download: buffer too small (%lld < %lld)", (long long)dst_bytes,
                      (long long)need);
        return 1;
      }
      if (N == 0) return 0;
      uint64_t* tmp;
      GNXCHK(dalloc(&tmp, (size_t)N * 2 * h->W64));
      int r = gnx_l_gather_genomes(h, N, nullptr, tmp);
      if (!r) {
        hipError_t e = hipMemcpyAsync(dst, tmp, need, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
          gnx_set_error("gnx_download: %s", hipGetErrorString(e));
          r = 1;
        }
      }
      (void)hipFree(tmp);
      return r;
    }
    default:
      gnx_set_error("gnx_download: unknown field %d", field);
      return 1;
  }
  if (dst_bytes < N * elt * planes) {
    gnx_set_error("gnx_download: buffer too small");
    return 1;
  }
  for (int64_t p = 0; p < planes; ++p)
    GNXCHK(gnx_d2h(h, (char*)dst + p * N * elt, (const char*)src + p * cap * elt, N * elt));
  return 0;
}

// new coordinates for every individual, in slot order (the reference lets a script
// assign Individual.x / .y and then calls Species._set_coords_and_cells,
// structs/species.py:937-939; tests/validation/wf does so every step); the environment
// values follow as in _set_e (:913-922)
extern "C" int gnx_set_positions(gnx_state* h, const float* x, const float* y) {
  h->fb_adults = false;
  GNXCHK(need_params(h));
  const int64_t N = h->N;
  if (N == 0) return 0;
  const float xmax = (float)(h->cfg.W - 0.001), ymax = (float)(h->cfg.H - 0.001);
  for (int64_t i = 0; i < N; ++i)
    if (!(x[i] >= 0 && x[i] <= xmax && y[i] >= 0 && y[i] <= ymax)) {
      gnx_set_error("gnx_set_positions: individual %lld at (%g, %g) is off the landscape "
                    "[0, dim - 0.001]", (long long)i, x[i], y[i]);
      return 1;
    }
  GnxSoA s = h->soa[h->cur];
  GNXCHK(gnx_h2d(h, s.x, x, N * sizeof(float)));
  GNXCHK(gnx_h2d(h, s.y, y, N * sizeof(float)));
  GNXCHK(gnx_l_gather_e(h, 0, N));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int gnx_download_genomes(gnx_state* h, int64_t n, const int64_t* slots,
                                    uint64_t* dst) {
  GNXCHK(need_genome(h));
  if (n <= 0) return 0;
  for (int64_t i = 0; i < n; ++i)
    if (slots[i] < 0 || slots[i] >= h->N) {
      gnx_set_error("gnx_download_genomes: slot out of range");
      return 1;
    }
  int64_t* ds;
  uint64_t* tmp;
  GNXCHK(dalloc(&ds, n));
  GNXCHK(dalloc(&tmp, (size_t)n * 2 * h->W64));
  HIPCHK(hipMemcpy(ds, slots, n * sizeof(int64_t), hipMemcpyHostToDevice));
  int r = gnx_l_gather_genomes(h, n, ds, tmp);
  if (!r) {
    hipError_t e = hipMemcpyAsync(dst, tmp, (size_t)n * 2 * h->W64 * 8, hipMemcpyDeviceToHost,
                                  h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
      gnx_set_error("gnx_download_genomes: %s", hipGetErrorString(e));
      r = 1;
    }
  }
  (void)hipFree(ds);
  (void)hipFree(tmp);
  return r;
}

extern "C" int gnx_download_raster(gnx_state* h, int32_t which, double* dst) {
  GNXCHK(need_params(h));
  size_t cells = (size_t)h->cfg.W * h->cfg.H;
  if (which == GNX_R_COUNTS) {
    std::vector<int32_t> tmp(cells);
    if (!h->counts_init) {
      gnx_set_error("count raster not initialised (gnx_spatial_diff_stats)");
      return 1;
    }
    HIPCHK(hipMemcpy(tmp.data(), h->counts_rast[h->counts_cur], cells * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < cells; ++i) dst[i] = tmp[i];
    return 0;
  }
  double* d;
  GNXCHK(dalloc(&d, cells));
  int r = gnx_l_raster(h, which, d);
  if (!r) {
    hipError_t e = hipMemcpyAsync(dst, d, cells * 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
      gnx_set_error("gnx_download_raster: %s", hipGetErrorString(e));
      r = 1;
    }
  }
  (void)hipFree(d);
  return r;
}

extern "C" int gnx_spatial_diff_stats(gnx_state* h, double* mean, double* sd) {
  GNXCHK(need_params(h));
  return gnx_l_spatial_diff(h, mean, sd);
}

extern "C" int gnx_spatial_diff_sums(gnx_state* h, double* sum, double* sum_sq) {
  GNXCHK(need_params(h));
  double r[2] = {0, 0};
  GNXCHK(gnx_l_spatial_diff(h, nullptr, nullptr, r));
  *sum = r[0];
  *sum_sq = r[1];
  return 0;
}

// ---------------------------------------------------------------- operator-level entry points
extern "C" int gnx_op_move(gnx_state* h, const float* theta, const float* dist) {
  GNXCHK(need_params(h));
  int64_t N = h->N;
  HIPCHK(hipMemcpyAsync(h->inj_a, theta, N * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->inj_b, dist, N * 4, hipMemcpyHostToDevice, h->stream));
  GNXCHK(gnx_l_move(h, false, h->inj_a, h->inj_b, nullptr, nullptr, true));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int gnx_op_move_draws(gnx_state* h, float* theta, float* dist) {
  GNXCHK(need_params(h));
  int64_t N = h->N;
  GNXCHK(gnx_l_move(h, false, nullptr, nullptr, h->inj_a, h->inj_b, false));
  HIPCHK(hipMemcpyAsync(theta, h->inj_a, N * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(dist, h->inj_b, N * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int gnx_op_find_pairs(gnx_state* h, const uint8_t* keep, int32_t* mate,
                                 int32_t* pairs, int64_t* n_pairs) {
  GNXCHK(need_params(h));
  int64_t N = h->N;
  // NB: sorts the population by hash cell first; slot order changes
  GNXCHK(gnx_l_sort_by_cell(h));
  const uint8_t* dk = nullptr;
  if (keep) {
    // keep[] is given in the caller's slot order == order before the sort;
    // permute it with the sort permutation
    std::vector<int32_t> perm(N);
    HIPCHK(hipMemcpyAsync(perm.data(), h->perm[1], N * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<uint8_t> k2(N);
    for (int64_t i = 0; i < N; ++i) k2[i] = keep[perm[i]];
    HIPCHK(hipMemcpy(h->keep_in, k2.data(), N, hipMemcpyHostToDevice));
    dk = h->keep_in;
  }
  int64_t P = 0;
  GNXCHK(gnx_l_find_pairs(h, dk, &P));
  if (mate) HIPCHK(hipMemcpy(mate, h->mate, N * 4, hipMemcpyDeviceToHost));
  if (pairs && P > 0) HIPCHK(hipMemcpy(pairs, h->pairs, P * 8, hipMemcpyDeviceToHost));
  *n_pairs = P;
  return 0;
}

extern "C" int gnx_op_crossover(gnx_state* h, int64_t B, const int32_t* parent_slots,
                                const int32_t* keys, const uint8_t* start_homs) {
  GNXCHK(need_genome(h));
  if (!h->genomes_assigned || h->n_paths == 0) {
    gnx_set_error("gnx_op_crossover: genomes / recombination paths not set");
    return 1;
  }
  if (B <= 0) return 0;
  if (h->N + B > h->cfg.cap_inds) {
    gnx_set_error("gnx_op_crossover: capacity exceeded");
    return 2;
  }
  for (int64_t k = 0; k < 2 * B; ++k)
    if (parent_slots[k] < 0 || parent_slots[k] >= h->N || keys[k] < 0 || keys[k] >= h->n_paths ||
        start_homs[k] > 1) {
      gnx_set_error("gnx_op_crossover: entry %lld out of range", (long long)k);
      return 1;
    }
  HIPCHK(hipMemcpyAsync(h->off_parent, parent_slots, 2 * B * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->off_keys, keys, 2 * B * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->off_start, start_homs, 2 * B, hipMemcpyHostToDevice, h->stream));
  int64_t births = 0;
  GNXCHK(gnx_l_mate(h, false, true, B, &births));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int gnx_op_dispersal(gnx_state* h, int64_t B, int32_t A, const float* mid_x,
                                const float* mid_y, const float* theta, const float* dist,
                                float* out_x, float* out_y, int32_t* attempt_used) {
  GNXCHK(need_params(h));
  if (B > h->cfg.cap_inds || A > GNX_DISP_ATTEMPTS * 4 || A < 1) {
    gnx_set_error("gnx_op_dispersal: B or A out of range");
    return 1;
  }
  float *dmx, *dmy, *dth, *dds, *dox, *doy;
  int32_t* du;
  GNXCHK(dalloc(&dmx, B));
  GNXCHK(dalloc(&dmy, B));
  GNXCHK(dalloc(&dth, (size_t)A * B));
  GNXCHK(dalloc(&dds, (size_t)A * B));
  GNXCHK(dalloc(&dox, B));
  GNXCHK(dalloc(&doy, B));
  GNXCHK(dalloc(&du, B));
  HIPCHK(hipMemcpy(dmx, mid_x, B * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dmy, mid_y, B * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dth, theta, (size_t)A * B * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dds, dist, (size_t)A * B * 4, hipMemcpyHostToDevice));
  int r = gnx_l_dispersal_inject(h, B, A, dmx, dmy, dth, dds, dox, doy, du);
  (void)hipStreamSynchronize(h->stream);
  if (!r) {
    (void)hipMemcpy(out_x, dox, B * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(out_y, doy, B * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(attempt_used, du, B * 4, hipMemcpyDeviceToHost);
  }
  for (void* p : {(void*)dmx, (void*)dmy, (void*)dth, (void*)dds, (void*)dox, (void*)doy, (void*)du})
    (void)hipFree(p);
  return r;
}

extern "C" int gnx_density_lattice_dims(gnx_state* h, int32_t* Jx, int32_t* Jy) {
  GNXCHK(need_params(h));
  *Jx = h->lat.Jx;
  *Jy = h->lat.Jy;
  return 0;
}

extern "C" int gnx_density_nmax(gnx_state* h, double* nmax) {
  GNXCHK(need_params(h));
  const unsigned long long* w = h->nmax_cur ? h->nmax_cur : h->nmax_bits;
  if (!w) {
    gnx_set_error("gnx_density_nmax: no density has been computed yet");
    return 1;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  unsigned long long bits = 0;
  HIPCHK(hipMemcpy(&bits, w, sizeof(bits), hipMemcpyDeviceToHost));
  memcpy(nmax, &bits, sizeof(bits));
  return 0;
}

extern "C" int gnx_op_density(gnx_state* h, int64_t n, const float* x, const float* y,
                              double* node_vals, double* raster) {
  GNXCHK(need_params(h));
  float *dx, *dy;
  GNXCHK(dalloc(&dx, n));
  GNXCHK(dalloc(&dy, n));
  HIPCHK(hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dy, y, n * 4, hipMemcpyHostToDevice));
  int r = gnx_l_density(h, n, dx, dy, &h->spl_N, nullptr);
  (void)hipStreamSynchronize(h->stream);
  (void)hipFree(dx);
  (void)hipFree(dy);
  if (r) return r;
  if (node_vals)
    HIPCHK(hipMemcpy(node_vals, h->spl_N.c, (size_t)h->lat.Jx * h->lat.Jy * 8,
                     hipMemcpyDeviceToHost));
  if (raster) return gnx_download_raster(h, GNX_R_N, raster);
  return 0;
}

extern "C" int gnx_op_death_probs(gnx_state* h, int32_t with_selection, const double* nodes_N,
                                  const double* nodes_pairs, double* p_death,
                                  double* d_at_cell) {
  GNXCHK(need_params(h));
  size_t nn = (size_t)h->lat.Jx * h->lat.Jy;
  HIPCHK(hipMemcpy(h->nodes, nodes_N, nn * 8, hipMemcpyHostToDevice));
  GNXCHK(gnx_l_density(h, 0, nullptr, nullptr, &h->spl_N, h->nodes));
  if (nodes_pairs) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->nodes, nodes_pairs, nn * 8, hipMemcpyHostToDevice));
    GNXCHK(gnx_l_density(h, 0, nullptr, nullptr, &h->spl_P, h->nodes));
  } else {
    h->spl_P.valid = false;
  }
  GNXCHK(gnx_l_death_probs(h, with_selection != 0));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (p_death) HIPCHK(hipMemcpy(p_death, h->p_death, h->N * 8, hipMemcpyDeviceToHost));
  if (d_at_cell) HIPCHK(hipMemcpy(d_at_cell, h->d_cell, h->N * 8, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int gnx_op_mortality(gnx_state* h, const uint8_t* dead) {
  HIPCHK(hipMemcpy(h->dead_in, dead, h->N, hipMemcpyHostToDevice));
  int64_t D = 0;
  GNXCHK(gnx_l_mortality(h, h->dead_in, &D));
  h->last_deaths = D;
  return 0;
}

// ---------------------------------------------------------------- measurement
extern "C" int gnx_profiling(gnx_state* h, int32_t on) {
  for (int k = 0; k < GNX_K_COUNT; ++k) {
    timers_resolve(h, k);
    h->timers[k] = GnxKernelTimer();
  }
  if (h->xo_jobs_acc) HIPCHK(hipMemset(h->xo_jobs_acc, 0, 2 * sizeof(unsigned long long)));
  h->profiling = on != 0;
  // on == 2: only the dominant kernel (crossover) is timed, so that very few
  // events are in flight (used by bench.py inside the timed region)
  h->profile_only = (on == 2) ? GNX_K_CROSSOVER : -1;
  return 0;
}

extern "C" int gnx_kernel_time(gnx_state* h, int32_t kernel, double* ms, int64_t* launches,
                               double* algorithmic_bytes) {
  if (kernel < 0 || kernel >= GNX_K_COUNT) {
    gnx_set_error("gnx_kernel_time: bad kernel id");
    return 1;
  }
  timers_resolve(h, kernel);
  if ((kernel == GNX_K_CROSSOVER || kernel == GNX_K_CROSSOVER_TAIL) && h->xo_jobs_acc) {
    // the crossover kernels count the gametes they copy (those without a switch point are
    // not copied and the host never learns how many there were)
    const int slot = kernel == GNX_K_CROSSOVER_TAIL ? 1 : 0;
    unsigned long long n = 0;
    HIPCHK(hipMemcpy(&n, h->xo_jobs_acc + slot, sizeof(n), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(h->xo_jobs_acc + slot, 0, sizeof(n)));
    // a job = a block copied: one block read, one written - and, with sparse paths, the 128-byte
    // line around the switch point from the OTHER homologue as well (a job exists because its
    // block holds a switch point; the lane that blends needs both parents' chunk there)
    h->timers[kernel].bytes =
        (double)n * (0.5 * gnx_xo_bytes_per_birth(h) / h->NB + (h->sparse_paths ? 128.0 : 0.0));
  }
  if (ms) *ms = h->timers[kernel].ms;
  if (launches) *launches = h->timers[kernel].launches;
  if (algorithmic_bytes) *algorithmic_bytes = h->timers[kernel].bytes;
  h->timers[kernel] = GnxKernelTimer();
  return 0;
}
