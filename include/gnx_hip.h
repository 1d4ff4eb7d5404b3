/*
 * gnx_hip.h - C-ABI of libgnxhip.so: the MI355X (gfx950) implementation of
 * Geonomics' per-generation simulation loop.
 *
 * The reference (erthward/geonomics 1.4.9) is pure Python and has no FFI; the
 * boundary it offers is the Python object API.  Each entry point below names
 * the reference method whose work it replaces (paths relative to
 * geonomics/ in the reference).  The Python host layer in geonomics_amd/
 * binds these with ctypes (geonomics_amd/_native.py); INTEGRATION.md shows the
 * stub a reference maintainer would add.
 *
 * Conventions
 *   - every call returns 0 on success, non-zero on failure;
 *     gnx_last_error() then returns a message.
 *   - the library owns all device memory behind the opaque handle; host
 *     buffers passed in are copied; downloads write to caller-allocated buffers.
 *   - one host thread per handle; calls are ordered on the handle's HIP stream
 *     and synchronous at download / count calls.
 *   - rasters are float32 [H][W] (row = y, col = x), the reference's
 *     Layer.rast[y, x] order (structs/landscape.py Layer; dim = (x, y)).
 *   - genotypes are bit-packed: per individual 2 homologues x W64 u64 words,
 *     bit l of homologue h == Individual.g[l, h] (structs/individual.py:103).
 *     W64 = gnx_words_per_hom(L).
 *   - extinction is not an error: N == 0 after a step (structs/species.py:841).
 */
#ifndef GNX_HIP_H
#define GNX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gnx_state gnx_state;

/* ---- enums -------------------------------------------------------------- */
enum { GNX_DIST_LOGNORMAL = 0, GNX_DIST_WALD = 1, GNX_DIST_LEVY = 2 };
enum { GNX_MATE_UNIFORM = 0, GNX_MATE_NEAREST = 1, GNX_MATE_INVERSE = 2 };
enum { GNX_SURF_NONE = 0, GNX_SURF_MIXTURE = 1, GNX_SURF_UNIMODAL = 2 };

/* fields for gnx_download() */
enum {
  GNX_F_X = 0, GNX_F_Y = 1, GNX_F_AGE = 2, GNX_F_SEX = 3, GNX_F_ID = 4,
  GNX_F_E = 5,      /* float [n_layers][N]   */
  GNX_F_Z = 6,      /* float [n_traits][N]   */
  GNX_F_FIT = 7, GNX_F_GROW = 8,
  GNX_F_GENO = 9    /* uint64 [N][2][W64], in slot order */
};
/* rasters for gnx_download_raster(): double [H][W] */
enum { GNX_R_N = 0, GNX_R_NPAIRS = 1, GNX_R_K = 2, GNX_R_D = 3, GNX_R_COUNTS = 4 };

/* kernels for gnx_kernel_time() */
enum {
  GNX_K_MOVE = 0, GNX_K_SORT = 1, GNX_K_PERMUTE = 2, GNX_K_FIND_MATES = 3,
  GNX_K_PAIRS = 4, GNX_K_OFFSPRING = 5, GNX_K_CROSSOVER = 6,
  GNX_K_PHENOTYPE = 7, GNX_K_DENSITY = 8, GNX_K_DEATH = 9, GNX_K_COMPACT = 10,
  GNX_K_CROSSOVER_TAIL = 11,   /* the narrow share of a split crossover launch */
  GNX_K_COUNT = 12
};

/* ---- configuration ------------------------------------------------------ */
typedef struct {
  int32_t W, H;            /* landscape dim (x, y): Landscape.dim            */
  int32_t n_layers;
  int32_t L;               /* loci; 0 = species without gen_arch             */
  int32_t n_traits;
  int64_t cap_inds;        /* individual-slot capacity                       */
  int64_t cap_rows;        /* genome-row capacity (0 if L == 0)              */
  uint64_t seed;           /* params.model.seed.num (sim/model.py:98-99)     */
  int32_t device;          /* HIP device ordinal                             */
  int32_t reserved;
} gnx_config;

/* The Poisson births draw a pair's count from 64 uniforms (Knuth's product): above this mean
 * the mass of counts >= 64 (2.4e-10 at 26, 1.0e-9 at 27) would collapse onto 64, and
 * gnx_set_species_params refuses it.                                                        */
#define GNX_BIRTHS_LAMBDA_MAX 26

/* Species life-history parameters: the 'mating', 'mortality' and 'movement'
 * sections of the parameters file (sim/params.py SPP_PARAMS), hoisted to
 * Species attributes at structs/species.py:409-425.                          */
typedef struct {
  /* mating */
  double  b;                       /* P(pair mates)                          */
  double  R;                       /* intrinsic growth rate                  */
  double  n_births_lambda;         /* n_births_fixed: the (integer) number of births;
                                    * else Poisson mean, <= GNX_BIRTHS_LAMBDA_MAX       */
  int32_t n_births_fixed;
  int32_t sexed;                   /* mating.sex                             */
  double  p_male;                  /* sex_ratio/(sex_ratio+1) (species.py:416) */
  double  mating_radius;           /* < 0 => None (panmixia)                 */
  int32_t mate_mode;               /* GNX_MATE_*                             */
  int32_t repro_age[2];            /* [female, male]; both equal if unsexed  */
  /* mortality */
  int32_t max_age;                 /* < 0 => None                            */
  double  d_min, d_max;
  double  window_width;            /* density_grid_window_width; <=0 => None */
  /* movement */
  int32_t move;
  double  dir_mu, dir_kappa;
  int32_t move_distr;              /* GNX_DIST_*                             */
  double  move_p1, move_p2;
  int32_t disp_distr;
  double  disp_p1, disp_p2;
  int32_t move_surf;               /* GNX_SURF_*                             */
  int32_t move_surf_layer;
  double  move_surf_kappa;
  int32_t disp_surf;
  int32_t disp_surf_layer;
  double  disp_surf_kappa;
  double  res_ratio[2];            /* Landscape._res_ratio                   */
  /* carrying capacity: K = rast[K_layer] * K_factor (species.py:546)        */
  int32_t K_layer;
  int32_t pad0;
  double  K_factor;
} gnx_species_params;

/* ---- lifecycle ---------------------------------------------------------- */
int  gnx_create(const gnx_config* cfg, gnx_state** out);
void gnx_destroy(gnx_state* h);
const char* gnx_last_error(void);
int  gnx_words_per_hom(int32_t L);
/* blocks a homologue is stored in (a block = W64*8 / n bytes is the unit the crossover copies
 * or shares with the parent, csrc/gnx_half.h); 0 without genomes                              */
int  gnx_blocks_per_hom(const gnx_state* h);
/* use an externally created hipStream_t (e.g. torch's current stream)       */
int  gnx_set_stream(gnx_state* h, void* hip_stream);
int  gnx_synchronize(gnx_state* h);

/* ---- landscape / species setup ----------------------------------------- */
/* Landscape layers: lyr.rast for every Layer (structs/landscape.py:34-120).
 * An upload leaves the individuals' e as the last mating sampled it; the next
 * step samples everybody from the new raster (its movement, or - where the
 * species does not move - one gather behind its age kernel).                */
int gnx_upload_rasters(gnx_state* h, const float* rasts /*[n_layers][H][W]*/);
int gnx_upload_layer(gnx_state* h, int32_t layer, const float* rast);
/* Species.K given explicitly, double [H][W] (demographic change events scale it:
 * ops/change.py:633-651); NULL returns to rast[K_layer] * K_factor            */
int gnx_set_k_raster(gnx_state* h, const double* K);
int gnx_set_species_params(gnx_state* h, const gnx_species_params* p);

/* Population: _make_species / _make_individual (structs/species.py:3300-3320,
 * structs/individual.py:188-228).  ids must be ascending.                   */
int gnx_upload_population(gnx_state* h, int64_t N, const float* x,
                          const float* y, const int32_t* age,
                          const uint8_t* sex, const int64_t* id);
/* N individuals at uniform random positions, ids 0..N-1, age 0              */
int gnx_init_population(gnx_state* h, int64_t N);

/* ---- genomic architecture ----------------------------------------------- */
/* Recombinations._subsetters (structs/genome.py:188-230) as path bits:
 * paths[k][w] bit l = homologue the k-th cached path is on at locus l.      */
int gnx_set_recomb_paths(gnx_state* h, int32_t n, const uint64_t* paths);
/* Trait (structs/genome.py:284-438): loci ascending, alpha per locus.
 * phi_rast == NULL => scalar phi.                                           */
int gnx_set_trait(gnx_state* h, int32_t t, int32_t n_loci, const int32_t* loci,
                  const double* alpha, int32_t layer, double phi,
                  const float* phi_rast, double gamma, int32_t univ_adv);
/* GenomicArchitecture.dom (structs/genome.py:552-555); NULL => codominant   */
int gnx_set_dominance(gnx_state* h, const uint8_t* dom /*[L]*/);
/* delet_loci / delet_loci_s (structs/genome.py:589-591)                     */
int gnx_set_deleterious(gnx_state* h, int32_t n, const int32_t* loci,
                        const double* s);
/* Individuals' genomes, in current slot order (inject / restore)            */
int gnx_upload_genomes(gnx_state* h, const uint64_t* geno /*[N][2][W64]*/);
/* Species._set_genomes_and_tables + _make_starting_mutations
 * (structs/species.py:956-967,1087; structs/genome.py:1108-1157):
 * exactly n_per_site[l] of the 2N homologues carry a 1 at site l.  The k-th
 * genome drawn goes to the individual with the k-th smallest id (the order the
 * reference walks its individuals in), whatever order the slots are in.     */
int gnx_assign_genomes(gnx_state* h, const int32_t* n_per_site /*[L]*/);
/* recompute all phenotypes (Species._set_z, structs/species.py:925)         */
int gnx_set_z(gnx_state* h);
/* phenotypes of slots [first, first+n) only (Species._set_z_individ, :929)   */
int gnx_set_z_range(gnx_state* h, int64_t first, int64_t n);

/* ---- one time step ------------------------------------------------------- */
/* Species._set_age_stage (structs/species.py:567)                           */
int gnx_age(gnx_state* h);
/* Species._do_movement (structs/species.py:582-585; ops/movement.py:34-95)  */
int gnx_move(gnx_state* h);
/* Species._do_pop_dynamics (structs/species.py:822; ops/demography.py:183):
 * pairs -> n_pairs density -> mating (births, dispersal, crossover,
 * phenotype) -> N density -> d -> death probabilities -> mortality.
 * burn != 0: no genomes/selection (burn-in).  Appends to Nt/births/deaths
 * counters readable with gnx_counts().                                      */
int gnx_pop_dynamics(gnx_state* h, int32_t burn, int32_t with_selection);
/* the same in two halves, so that the host can apply this step's mutations to
 * the new offspring in between, where the reference does
 * (structs/species.py:807-809): _mate = pairs, n_pairs density, births;
 * _die = N density, d, death probabilities, mortality.  After _mate the
 * offspring occupy slots [N_before, N_before + births).                     */
int gnx_pop_dynamics_mate(gnx_state* h, int32_t burn);
int gnx_pop_dynamics_die(gnx_state* h, int32_t burn, int32_t with_selection);
/* whole fn-queue entry for one step: age, move (if params.move), pop dynamics
 * (sim/model.py:603-667)                                                    */
int gnx_step(gnx_state* h, int32_t burn, int32_t with_selection);
/* gnx_step in three parts - _begin: age, movement, cell sort, mate search, pair list
 * enqueued; _mid: pair count read, births, densities, death probabilities, death draws,
 * compaction and crossover enqueued; _end: survivor counts read - and gnx_step_many: one
 * step of n INDEPENDENT handles (the iterations of a model, sim/model.py:866-953, whose
 * TODO at :924-925 wants them farmed out), all first parts, then all second, then all
 * third, so that the handles' kernels run side by side on their own streams while one
 * host thread drives them.  Same results as gnx_step on each handle.                     */
int gnx_step_begin(gnx_state* h, int32_t burn);
int gnx_step_mid(gnx_state* h, int32_t burn, int32_t with_selection);
int gnx_step_end(gnx_state* h, int32_t burn);
int gnx_step_many(gnx_state** hs, int32_t n, int32_t burn, int32_t with_selection);
/* T time steps without the host in the loop - Model.walk(T) of the reference
 * (sim/model.py:966-1161: T times _do_timestep over the function queue, :699-744).
 * gnx_step reads the pair count and the survivor count back in every step and sizes the
 * next kernels with them; gnx_walk keeps every count of the step in device memory, sizes
 * the grids by the handle's capacity and replays one captured HIP graph per step: one
 * runtime call and no read-back per step (at 10^5 individuals - BASELINE configs[1], [2] -
 * the host-driven step is bound by the ~45 runtime calls it makes, not by its kernels).
 * Same draws, same canonical orders, same kernels: the population equals the one T calls of
 * gnx_step leave, id by id.  A handle the device-driven step does not cover (tiles,
 * panmixia, Poisson births, no movement, profiling on; GNX_DD=0) walks through gnx_step.
 * The population must fit the capacity throughout: a step whose offspring do not fit is
 * reported as an error when the walk ends.
 * gnx_walk_many: the same for n INDEPENDENT handles (the iterations of one model,
 * sim/model.py:866-953, TODO at :924-925), step t of every handle enqueued before step
 * t + 1 of any, so that their kernels share the chip.
 * gnx_walk_history: (N at the start, births, deaths) of the last max_steps steps of the
 * last walk - Species.Nt / n_births / n_deaths (structs/species.py:374-380, 554) - returns
 * how many were written.                                                                  */
int gnx_walk(gnx_state* h, int64_t T, int32_t burn, int32_t with_selection);
int gnx_walk_many(gnx_state** hs, int32_t n, int64_t T, int32_t burn, int32_t with_selection);
int64_t gnx_walk_history(gnx_state* h, int64_t max_steps, int64_t* n_start, int64_t* births,
                         int64_t* deaths);
int gnx_counts(gnx_state* h, int64_t* N, int64_t* births, int64_t* deaths);
/* Running totals over the gnx_step calls since the last gnx_reset_totals (what Species.Nt /
 * n_births / n_deaths accumulate step by step, structs/species.py:554,  kept in the library
 * so that a driver loop need not call back between steps): out[6] = steps, sum of N at the
 * START of each step (the metric's individual-timesteps), births, deaths, births whose
 * genomes the crossover wrote, steps that gnx_walk took the device-driven way.  Host-side
 * bookkeeping only: no device access.                                                       */
int gnx_totals(gnx_state* h, int64_t* out);
int gnx_reset_totals(gnx_state* h);
/* Which code paths the host-driven steps took since the handle was created or since the last
 * gnx_reset_path_counts - so that a test can prove it reached the path it means to check.
 * out[0 .. n) of: mortalities that left the dead in their slots (gnx_walk: every step but the
 * last); pending crossovers launched from launch policy 2's site (behind the next step's pair
 * list: capacities above 600 000 slots); pending crossovers launched by anybody else (a join,
 * a genome access); job-builder launches of the 256-thread and of the 512-thread
 * instantiation; cell sorts whose first pass gathered through the id-ordered index with the
 * digit counts of the movement; block collections that ran while a crossover was built but
 * not yet joined; uncompacted populations gathered back after a walk that was cut short;
 * movements of the next step launched beside the job builder (gnx_walk of one handle, every
 * step but the last).
 * Returns how many counters there are.  Host-side integers only: no device access, no
 * effect on any result (gnx_totals is separate).  Steps of the device-driven walk are
 * captured once into a graph and replayed: they are not counted.                         */
int gnx_path_counts(gnx_state* h, int64_t* out, int32_t n);
int gnx_reset_path_counts(gnx_state* h);
/* Where the new offspring's genomes are cut (ops/mating.py:130-214, the crossover).
 * on (default, one GPU): after the step's death draws, for the offspring that survive
 * them only, on a second HIP stream under the next step's kernels - offspring that die at
 * age 0 (structs/species.py:822-833 kills them in the same _do_pop_dynamics call) never
 * get a genome.  off: for every birth, inside gnx_pop_dynamics_mate.  Same results either
 * way (draws are keyed by id); any genome access in between triggers the off path.      */
int gnx_set_defer_crossover(gnx_state* h, int32_t on);
/* How the deferred crossover shares the GPU with the next step's kernels.  0 (default):
 * it runs at full width beside the compaction, the sort index's compaction and the next
 * movement; the next cell sort waits for it.  1: a narrow crossover runs beside the
 * WHOLE next step.  2: nothing runs beside it (the kernel's own rate; a slower step).
 * Results do not depend on the mode.                                                   */
int gnx_set_crossover_overlap(gnx_state* h, int32_t mode);
/* Split every deferred crossover launch: wide_per_1024 / 1024 of its jobs at full width
 * (the next cell sort waits for them), the rest as a narrow launch that shares the chip
 * with the sort and the kernels after it.  0 or 1024 = one launch.  Results do not depend
 * on it. */
int gnx_set_crossover_split(gnx_state* h, int32_t wide_per_1024);
/* Bookkeeping of the shared genome blocks (where a gamete's path has no switch point the
 * child refers to the parent's block instead of copying it; blocks nobody alive refers to
 * are found by a mark-and-sweep collection when the free stack runs low).  Runs a
 * collection, then out[6] = logical blocks of the individuals that have a genome row / 2,
 * broken references, collections so far, physical blocks in use, free physical blocks,
 * physical blocks in all.  Consistent iff out[1] == 0 and out[3] + out[4] == out[5]. */
int gnx_debug_halves(gnx_state* h, int64_t* out);
/* The same bookkeeping as the host sees it, WITHOUT touching the device (no join of a
 * crossover in flight, no collection): out[8] = blocks per homologue, words per block,
 * collections so far, row spread, sparse paths (0 / 1), free blocks the host counts on,
 * free logical rows, 1 while offspring still wait for their deferred crossover.        */
int gnx_genome_info(gnx_state* h, int64_t* out);
/* measurement: the job list of the last crossover, 16 bytes per copied block {the
 * parent's two physical blocks, the block written, (path * 2 + start homologue) | block
 * index << 24} (csrc/gnx_xo.h); blocks without a switch point are not in it            */
int gnx_last_crossover_jobs(gnx_state* h, void* dst, int64_t max_jobs, int64_t* n_jobs);
/* births whose genomes the last crossover wrote (== births when not deferred)          */
int64_t gnx_last_crossover_births(gnx_state* h);
int64_t gnx_step_index(gnx_state* h);
int gnx_set_step_index(gnx_state* h, int64_t step);

/* mutation (ops/mutation.py:62-131): set bit (locus, hom) of listed slots   */
int gnx_mutate(gnx_state* h, int32_t n, const int64_t* slot,
               const int32_t* locus, const uint8_t* hom);

/* ---- read-back ------------------------------------------------------------ */
/* slot order == ascending id order is NOT guaranteed; download GNX_F_ID and
 * sort on the host (geonomics_amd does).                                    */
int gnx_download(gnx_state* h, int32_t field, void* dst, int64_t dst_bytes);
/* genotypes of selected slots: uint64 [n][2][W64]                           */
/* new coordinates of all N individuals, slot order (Individual.x / .y assigned by a
 * script + Species._set_coords_and_cells, structs/species.py:937-939); e follows */
int gnx_set_positions(gnx_state* h, const float* x /*[N]*/, const float* y /*[N]*/);
/* slots in use = rows of a gnx_download (the tile's ghosts included while they are
 * resident, i.e. between gnx_tile_import_ghosts and gnx_tile_die)              */
int64_t gnx_n_slots(gnx_state* h);
int gnx_download_genomes(gnx_state* h, int64_t n, const int64_t* slots,
                         uint64_t* dst);
/* double [H][W]: N (Species.N), n_pairs, K, d as of the last pop_dynamics;
 * GNX_R_COUNTS = individuals per cell (sim/burnin.py:44-59)                 */
int gnx_download_raster(gnx_state* h, int32_t which, double* dst);
/* burn-in spatial tester (sim/burnin.py:44-59): updates the per-cell count
 * raster and returns mean and std of (counts_now - counts_prev)             */
int gnx_spatial_diff_stats(gnx_state* h, double* mean, double* std);
/* the same update, returning the sums behind them (integers: sum of the per-cell count
 * differences and of their squares), which add exactly over the tiles of a tiled run  */
int gnx_spatial_diff_sums(gnx_state* h, double* sum, double* sum_sq);

/* ---- operator-level entry points (parity tests; explicit random inputs) -- */
/* ops/movement.py:74-92 with injected direction/distance draws              */
int gnx_op_move(gnx_state* h, const float* theta, const float* dist);
/* draws only: what gnx_move would draw for the current population           */
int gnx_op_move_draws(gnx_state* h, float* theta, float* dist);
/* structs/species.py:2157-2215 + ops/mating.py:24-117.  Outputs mate slot
 * per individual (-1 none) and the final pair list; keep == NULL => draw
 * Bernoulli(b) from the device stream.                                      */
int gnx_op_find_pairs(gnx_state* h, const uint8_t* keep, int32_t* mate,
                      int32_t* pairs /*[cap][2]*/, int64_t* n_pairs);
/* ops/mating.py:130-214: B offspring from parent slots, path keys and start
 * homologues; children are appended to the population (rows allocated).     */
int gnx_op_crossover(gnx_state* h, int64_t B, const int32_t* parent_slots,
                     const int32_t* keys, const uint8_t* start_homs);
/* ops/movement.py:98-141: offspring positions from A attempts of draws      */
int gnx_op_dispersal(gnx_state* h, int64_t B, int32_t A, const float* mid_x,
                     const float* mid_y, const float* theta,
                     const float* dist, float* out_x, float* out_y,
                     int32_t* attempt_used);
/* utils/spatial.py:73-146: density raster of arbitrary points               */
int gnx_op_density(gnx_state* h, int64_t n, const float* x, const float* y,
                   double* node_vals /*[Jy][Jx] or NULL*/, double* raster);
int gnx_density_lattice_dims(gnx_state* h, int32_t* Jx, int32_t* Jy);
/* ops/demography.py:116: N.max(), the maximum of the individuals' density raster
 * the last death probabilities (gnx_step, gnx_pop_dynamics_*, gnx_op_death_probs)
 * clipped dNdt with; waits for the handle's stream                            */
int gnx_density_nmax(gnx_state* h, double* nmax);
/* ops/demography.py:253-321 + ops/selection.py:119-125: death probabilities
 * of the current population given node densities for N and n_pairs          */
int gnx_op_death_probs(gnx_state* h, int32_t with_selection,
                       const double* nodes_N, const double* nodes_pairs,
                       double* p_death, double* d_at_cell);
/* ops/demography.py:175-180 with an injected death mask (by slot); the survivors
 * keep their order.  (The mortality of gnx_step / gnx_pop_dynamics_die leaves the
 * survivors of the first N - deaths slots where they are and moves the others
 * into the slots of the dead: slot order carries no meaning between steps.) */
int gnx_op_mortality(gnx_state* h, const uint8_t* dead);

/* ---- spatial tiling over several GPUs ---------------------------
 * The reference has no distributed mode; these entry points are new.  One
 * process/GPU owns one tile of a uniform R x C grid and the individuals inside
 * it; the host layer (geonomics_amd/parallel.py) moves the staged buffers with
 * torch.distributed (RCCL).  Step order on a tiled landscape:
 *   gnx_age / gnx_move -> export_migrants + import -> export_halo +
 *   import_ghosts -> tile_pairs -> [all-gather pair_info, all-reduce bins 1] ->
 *   tile_offspring -> [requests -> serve_gametes -> put_gametes] ->
 *   tile_finish_births -> [all-reduce bins 0] -> tile_die.                      */
typedef struct {
  float x, y;
  int32_t age, sex;
  int64_t id;
  float fit;
  int32_t nbr_mask;   /* halo: bit (dy+1)*3+(dx+1) = neighbour tile that needs it */
} gnx_ind_rec;

int gnx_tile_set(gnx_state* h, int32_t R, int32_t C, int32_t r, int32_t c);
int gnx_tile_export_migrants(gnx_state* h, int64_t* n_out);
/* halo = whole hash cells: every individual whose cell lies within 2 cells of a
 * neighbour tile's cell range (complete candidate lists for the neighbour's own
 * focal individuals and for the ghosts they can choose)                        */
int gnx_tile_export_halo(gnx_state* h, int64_t* n_out);
int gnx_tile_get_staged(gnx_state* h, gnx_ind_rec* rec, float* z /*[n][n_traits]*/,
                        uint64_t* geno /*[n][2][W64]*/);
int gnx_tile_import(gnx_state* h, int64_t n, const gnx_ind_rec* rec, const float* z,
                    const uint64_t* geno);
int gnx_tile_import_ghosts(gnx_state* h, int64_t n, const gnx_ind_rec* rec);
int gnx_tile_pairs(gnx_state* h, int32_t burn, int64_t* n_pairs, int64_t* n_births);
int gnx_tile_pair_info(gnx_state* h, int64_t* focal_ids /*[P] order keys (cell << 40 | id), ascending*/,
                       int32_t* n_births /*[P]*/);
int gnx_density_bin_count(gnx_state* h);
/* which: 0 = individuals, 1 = pair midpoints; int32 [bin_count]             */
int gnx_get_bins(gnx_state* h, int32_t which, int32_t* out);
int gnx_set_bins(gnx_state* h, int32_t which, const int32_t* in);
int gnx_tile_offspring(gnx_state* h, int32_t burn, int64_t id_base,
                       const int64_t* pair_goff /*[P]*/, int64_t* n_requests);
int gnx_tile_get_requests(gnx_state* h, int64_t* parent_id, int32_t* child_k, int32_t* key,
                          uint8_t* start, float* px, float* py);
int gnx_tile_serve_gametes(gnx_state* h, int64_t n, const int64_t* parent_ids,
                           const int32_t* keys, const uint8_t* starts,
                           uint64_t* out /*[n][W64]*/);
int gnx_tile_put_gametes(gnx_state* h, int64_t n, const int32_t* child_k,
                         const uint64_t* data /*[n][W64]*/);
int gnx_tile_finish_births(gnx_state* h, int32_t burn);
int gnx_tile_die(gnx_state* h, int32_t burn, int32_t with_selection, int32_t have_pairs);
int gnx_set_max_id(gnx_state* h, int64_t max_id);

/* ---- the device-driven tile protocol ("tile2"): the host waits for the device three
 * times per step - for the routing counts, for the pair / request counts and for the
 * survivor count - and every payload stays in device memory.  Entry points marked (no
 * wait) only enqueue work on the handle's stream (gnx_stream_ptr: the host layer orders
 * its collectives behind it with stream dependencies, never with a host synchronisation);
 * buffers the caller hands in must stay alive until gnx_tile2_die returns.
 *   gnx_tile2_move_route -> [counts all-gather, ONE batch of sends: migrants + ghosts] ->
 *   gnx_tile2_import -> gnx_tile2_pairs -> [counts all-gather, pair keys all-gather] ->
 *   gnx_tile2_offspring -> [requests] -> gnx_tile2_serve -> [gametes] -> gnx_tile2_put ->
 *   gnx_tile2_finish_births -> [ONE all-reduce: both bin fields + counters] -> gnx_tile2_die */
typedef struct {
  int64_t parent_id;
  int32_t key;      /* recombination path */
  int32_t start;    /* starting homologue, 0 / 1 */
  float px, py;     /* the parent's position (its hash cell locates it on the owning tile) */
} gnx_gamete_req2;
/* the HIP stream the handle enqueues on (torch.cuda.ExternalStream)                       */
int gnx_stream_ptr(gnx_state* h, void** stream);
/* age (+ movement), then the route of every individual: one that left the tile goes to
 * the tile that owns its new position, with its genome, and every individual in a hash
 * cell within two cells of a neighbour tile goes there as a ghost - emigrants included
 * (relative to their NEW tile; this tile can be among the receivers), so the halo does not
 * wait for the migrants' arrival.  Grouped by destination rank on the device.
 * counts[2 * R*C] = migrants per rank, ghosts per rank.  Emigrants stay in their slots
 * until the cell sort of gnx_tile2_pairs moves them behind the population.  One wait.     */
int gnx_tile2_move_route(gnx_state* h, int32_t move, int64_t* counts);
/* ... in two halves, for a caller that exchanges the counts itself (gnx_tile_step: the wait for
 * this tile's counts is the count exchange's): _begin enqueues age + movement + the counting
 * pass, *counts_dev = int32[2 * R*C] in device memory (no wait); _finish takes this tile's counts
 * from the host and enqueues the pass that fills the staging buffers (no wait).              */
int gnx_tile2_route_begin(gnx_state* h, int32_t move, void** counts_dev);
int gnx_tile2_route_finish(gnx_state* h, const int64_t* counts);
/* gnx_tile2_pairs leaves its gamete-request counts in device memory (*counts_dev, int32[R*C])
 * instead of waiting for them (on != 0); the caller hands them back once they have reached the
 * host with its own exchange (gnx_tile2_set_requests) before gnx_tile2_offspring.             */
int gnx_tile2_requests_dev(gnx_state* h, int32_t on, void** counts_dev);
int gnx_tile2_set_requests(gnx_state* h, const int64_t* req);
/* gnx_tile_step on several tiles, a fixed number of births per pair: gnx_tile2_pairs does not
 * wait for the pair count either (mode 1: counts[0] = counts[1] = -1) - the pairs' density bins
 * and the request counts read it on the device - and _settle does the host's bookkeeping once
 * the count has arrived with the caller's own exchange (births: fixed lambda x P).            */
int gnx_tile2_pairs_mode(gnx_state* h, int32_t nowait);
int gnx_tile2_pairs_settle(gnx_state* h, int32_t burn, int64_t n_pairs, int64_t* births);
/* the offspring that took a remote gamete re-read their alleles at the selected loci and their
 * phenotype from their finished rows (gnx_tile2_finish_births does it unless this has)        */
int gnx_tile2_settle_births(gnx_state* h, int32_t burn);
/* Tile-major offspring ids (gnx_set_id_order 1) through a caller-driven protocol
 * (TiledStepper._step_v2): counts[64] = this tile's births per virtual tile (one wait; the
 * classification rode with gnx_tile2_pairs), then bases[64] = the virtual tiles' global base
 * offsets in births (the exclusive sums of every tile's counts) before gnx_tile2_offspring,
 * which is then handed no offsets.                                                           */
int gnx_tile2_vt_counts(gnx_state* h, int64_t* counts);
int gnx_tile2_vt_bases(gnx_state* h, const int64_t* bases);
int gnx_tile2_route_ptrs(gnx_state* h, void** mig_rec, void** mig_z, void** mig_geno,
                         void** ghost_rec);
/* arrivals (device buffers): migrants rec / z / geno [n_mig], ghosts rec [n_ghost]; (no wait).
 * Capacity: the emigrants of this step still hold their slots and genome rows when the
 * arrivals are appended (they leave with the cell sort of gnx_tile2_pairs), so cap_inds must
 * hold residents + emigrants + immigrants + ghosts (+ the step's births) and cap_rows
 * residents + emigrants + immigrants; "capacity exceeded importing ..." otherwise.          */
int gnx_tile2_import(gnx_state* h, int64_t n_mig, const void* rec, const void* z,
                     const void* geno, int64_t n_ghost, const void* ghost_rec);
/* cell sort (emigrants leave, their genome rows return to the free stack), mate search, pair
 * list, births.  counts[2 + R*C] = pairs, births, gamete requests per owning rank.  One
 * wait (two more with Poisson-distributed births).                                      */
int gnx_tile2_pairs(gnx_state* h, int32_t burn, int64_t* counts);
/* the local pair list in device memory: order keys (cell << 40 | focal id) int64[P] ascending;
 * n_births int32[P], or NULL when every pair has the fixed number of births; (no wait)      */
int gnx_tile_pair_ptrs_nosync(gnx_state* h, int64_t* n_pairs, void** focal_ids, void** n_births);
/* offspring; *req_dev = gnx_gamete_req2[] grouped by owning rank as counted by
 * gnx_tile2_pairs; (no wait)                                                             */
int gnx_tile2_offspring(gnx_state* h, int32_t burn, int64_t id_base,
                        const void* pair_goff_dev /*int64[P]*/, void** req_dev);
/* gametes for n requests of other tiles: *out_dev = u64[n][W64]; (no wait)                */
int gnx_tile2_serve(gnx_state* h, int64_t n, const void* req_dev, void** out_dev);
/* the answers to this tile's requests, in the grouped request order; (no wait)          */
int gnx_tile2_put(gnx_state* h, int64_t n, const void* data_dev);
/* phenotypes of the offspring, bins of the tile's own individuals; *reduce_dev = int32
 * [2 * bin_count + 4]: both bin fields, then this tile's N, births, deaths of the PREVIOUS
 * step and 0 - one all-reduce(sum) in place for all of it; (no wait)                     */
int gnx_tile2_finish_births(gnx_state* h, int32_t burn, void** reduce_dev, int64_t* n_words);
/* densities from the reduced bins, death probabilities, mortality; checks what the
 * (no wait) calls could not report (records off the landscape, unknown parents).  One wait.
 * totals[3] = the all-reduced N, births, deaths-of-the-previous-step words.              */
int gnx_tile2_die(gnx_state* h, int32_t burn, int32_t with_selection, int32_t have_pairs,
                  int64_t* totals);

/* ---- one tiled time step per call, the exchanges issued by the library (csrc/gnx_comm.hip).
 * The tile2 protocol above composed in C: grouped ncclSend / ncclRecv to the neighbour tiles
 * on the handle's own stream (RCCL over xGMI), two KB-sized ncclAllGather for the counts (the
 * second carries the 64 virtual-tile birth counts the offspring ids are numbered from and the
 * pair count), ONE ncclAllReduce for both density fields and the counters - no torch.distributed
 * call, no Python between the phases of a step.  The reference has no counterpart (one process;
 * sim/model.py:924-925 is a TODO).
 *   gnx_comm_unique_id: rank 0 makes the id (ncclGetUniqueId, 128 bytes) and hands it to the
 *     other ranks by whatever channel the launcher has (bench.py: torch.distributed broadcast);
 *   gnx_comm_init_rccl: every rank joins (ncclCommInitRank; world 1 is allowed);
 *   gnx_comm_init_single: one tile, no communicator at all;
 *   gnx_comm_local_*: the tiles are handles of ONE process driven by one host thread each and
 *     the exchanges are device-to-device copies behind a barrier of the threads - the tests of
 *     the one-GPU box, where RCCL refuses two ranks on one device; everything but the nccl*
 *     calls themselves is the same code;
 *   gnx_tile_step: one step.  out[3]: exact != 0 -> the global (N after the step, births,
 *     deaths), one more KB-sized collective; else what rode on the step's own all-reduce:
 *     (N at the START of the step, births, deaths of the PREVIOUS step).  Poisson births
 *     (ops/mating.py:120-126) are numbered like fixed ones: the virtual tiles' BIRTH counts travel.
 *   gnx_tile_step_begin / _end: the same step in two calls, split where the reference's
 *     _do_pop_dynamics has its host work on the newborns - mutation (ops/mutation.py:169-206) and
 *     pedigree rows (structs/species.py:692-736) sit between the births and the deaths: after
 *     _begin every offspring of the step has its record, its alleles at the selected loci and
 *     its phenotype (gnx_last_births, gnx_mutate work there); gnx_tile_step_births tells the first
 *     id and the number of the step's offspring over ALL tiles; _end takes the densities' one
 *     all-reduce, the death probabilities and the mortality.  gnx_tile_step = both.
 *   gnx_comm_probe: librccl can be loaded and has every entry point the transport uses - what
 *     the ranks tell each other (over the launcher's CPU group) BEFORE any of them enters
 *     gnx_comm_init_rccl, whose ncclCommInitRank nobody can be called back from; the init itself
 *     carries a deadline (GNX_COMM_INIT_TIMEOUT_S, default 180 s): past it the rank says why on
 *     stderr and ends the process with code 86.
 *   The global maximum id (gnx_set_max_id) must be the same on every rank before the first
 *   step; the library keeps it.                                                             */
/* 0 (default): offspring ids in the canonical (hash cell, focal id) order of the pairs over the
 * whole landscape; 1: virtual tile by virtual tile (a fixed 8 x 8 blocking of the landscape, every
 * tile grid that divides it is a union of), inside one in that canonical order - what
 * gnx_tile_step hands out, since the tiles then only have to tell each other 64 birth counts
 * instead of every pair's order key; a one-device run in this order reproduces a tiled run id by
 * id.  The reference's own order is that of a Python set (ops/mating.py:63): unspecified.      */
int gnx_set_id_order(gnx_state* h, int32_t mode);
int gnx_comm_unique_id(uint8_t* out128);
int gnx_comm_init_rccl(gnx_state* h, const uint8_t* id128, int32_t rank, int32_t world);
int gnx_comm_init_single(gnx_state* h);
int gnx_comm_local_create(int32_t world, void** group);
int gnx_comm_local_join(gnx_state* h, void* group, int32_t rank);
int gnx_comm_local_abort(void* group);
int gnx_comm_local_destroy(void* group);
int gnx_comm_free(gnx_state* h);
int64_t gnx_comm_bytes_sent(gnx_state* h);
/* Known words through every operation of the handle's transport (the gather of host and device
 * words, a ragged two-part exchange with every rank including itself, the in-place sum), checked
 * on the host; collective: every rank of the communicator calls it.  Nonzero and gnx_last_error
 * when anything arrives wrong.  geonomics_amd.parallel.TiledStepper runs it once after the ranks
 * have joined.  (GNX_COMM_FORCE_RCCL=1 in the environment of gnx_comm_init_rccl makes a ONE-rank
 * communicator use the RCCL calls themselves instead of the one-rank shortcuts.) */
int gnx_comm_selftest(gnx_state* h);
int gnx_tile_step(gnx_state* h, int32_t burn, int32_t with_selection, int32_t exact, int64_t* out);
int gnx_tile_step_begin(gnx_state* h, int32_t burn);
int gnx_tile_step_births(gnx_state* h, int64_t* first_id, int64_t* total);
int gnx_tile_step_end(gnx_state* h, int32_t burn, int32_t with_selection, int32_t exact,
                      int64_t* out);
int gnx_comm_probe(void);
/* gnx_tile_step_abort: leave the state between _begin and _end without the density all-reduce and
 * the mortality - what every rank calls when the host's work on the newborns (the reference's
 * mutation / pedigree hooks, ops/mutation.py:169-206, structs/species.py:692-736) failed on ANY
 * rank, so that all of them raise instead of the others waiting inside the all-reduce.
 * gnx_comm_info: int64 out[16] - [0] transport (0 one rank, 1 RCCL, 2 local), [1] rank, [2] world,
 * [3] ncclCommCount, [4] ncclCommUserRank, [5] ncclCommCuDevice (-1 without an RCCL communicator),
 * [6] HIP device ordinal, [7] tiled steps taken, [8..12] host wall time of the step's phases summed
 * over them in microseconds (routing + count exchange; migrant / ghost exchange + import; cell
 * sort + pairs + second count exchange; births + gamete service; all-reduce + deaths), [13] bytes
 * sent, [14] collections of the genome blocks so far (also without a communicator).  No reference
 * counterpart (sim/model.py:924-925 is a TODO): it lets bench.py certify the ranks it ran on.    */
int gnx_tile_step_abort(gnx_state* h);
/* gnx_tile_walk: T tiled steps in one call with nothing between them (the tiles' gnx_walk; reference
 * Model.walk -> _do_timestep T times, sim/model.py:966-1161, on every rank).  Between two of its
 * steps the dead stay in their slots - no compaction: the next step's movement and routing skip
 * them, the imports go behind, the cell sort removes them with the emigrants - the last step
 * compacts.  out[5]: the last step's triple as gnx_tile_step reports it (exact as there), then
 * the sums over the T steps of the global population at the start of the step and of the births. */
int gnx_tile_walk(gnx_state* h, int64_t T, int32_t burn, int32_t with_selection, int32_t exact,
                  int64_t* out /*[5]*/);
int gnx_comm_info(gnx_state* h, int64_t* out /*[16]*/);

/* ---- pedigree (reference structs/species.py:692-736: rows of the tskit tables) --
 * the offspring of the last gnx_pop_dynamics_mate, in birth order; call it before
 * gnx_pop_dynamics_die.  keys / starts: recombination path and start homologue of
 * the gamete from parent 0 and from parent 1 (NULL to skip; burn-in has none)   */
int gnx_last_births(gnx_state* h, int64_t* child_id /*[B]*/, int64_t* parent_id /*[B][2]*/,
                    int32_t* keys /*[B][2]*/, uint8_t* starts /*[B][2]*/, float* xy /*[B][2]*/);

/* ---- statistics (reference sim/stats.py:359-435) ---------- */
/* per-locus count of 1-alleles over the 2N chromosomes and of heterozygous
 * individuals: het = cnt_het / N (_calc_het), f1 = cnt1 / 2N (_calc_maf)     */
int gnx_stats_locus_counts(gnx_state* h, int32_t* cnt1 /*[L]*/, int32_t* cnt_het /*[L]*/);
/* the same two counts per group of individuals (csrc/gnx_group_counts.hip): what Fst between
 * groups, per-group diversity and the site-frequency spectrum are host arithmetic on
 * (geonomics_amd/sim/fst.py).  It replaces the reference's method, which downloads every
 * genotype and loops in Python over loci x pairs of islands
 * (tests/validation/island/island_test.py:70-115).
 * slots[group_start[g] .. group_start[g + 1]) are the slots of group g's individuals; a group
 * may be empty, and individuals in no group are absent.  cnt1[g][l] = 1-alleles of group g at
 * locus l over both homologues, cnt_het[g][l] = its heterozygotes; with G = 1 and all living
 * slots the outputs equal gnx_stats_locus_counts'.  Refused before anything is launched
 * (return 1): no genomes; ghost records (a tile); G outside 1..1024; G * L above 2^26 counts per table; group_start
 * not starting at 0, decreasing, or not ending at n; a slot outside [0, gnx_n_slots); a group
 * of 2^30 individuals or more.  A pending crossover is cut first, and an uncompacted
 * population would be gathered (the order of the slots may change then, no result does):
 * no individual, genome or later draw is changed.                                        */
int gnx_stats_group_counts(gnx_state* h, int64_t n, const int32_t* slots /*[n], grouped*/,
                           int32_t G, const int64_t* group_start /*[G + 1]*/,
                           int32_t* cnt1 /*[G][L]*/, int32_t* cnt_het /*[G][L]*/);
/* moving-window diversity sums over a map grid (csrc/gnx_divmap.hip; geonomics_amd/sim/divmap.py
 * holds the definition and the host arithmetic): the landscape cut into nx x ny map cells
 * (cell iy * nx + ix), slots[cell_start[c] .. cell_start[c + 1]) the slots of the individuals
 * in map cell c, as gnx_stats_group_counts takes its groups.  The window of map cell (iy, ix)
 * is every map cell within Chebyshev distance r, clipped at the map's edge.  Per window, over
 * the loci of locus_mask (u64 [W64], NULL: all L; L' of them), rasters [ny][nx] on the HOST:
 *   out_n    individuals n                          out_S    loci with 0 < c_l < 2n
 *   out_het  sum over loci of the heterozygotes h_l  out_cc   sum over loci of c_l (2n - c_l)
 * c_l: the window's 1-alleles at locus l over both homologues.  Exact integers, independent of
 * the schedule and of the tile size.  The genome is processed in locus tiles of whole 64-locus
 * words, sized so that one [cell][tile loci] table holds at most max_counts int32 entries
 * (<= 0: 2^26), at least one word; four such tables are the call's scratch.
 * Refused before anything is launched (return 1): no genomes; ghost records (a tile); nx or
 * ny < 1; nx * ny above 2^20; r < 0; a null argument or n < 0; cell_start not starting at 0,
 * decreasing, or not ending at n; a window of 2^30 individuals or more; L' * n_max^2 >= 2^63
 * (out_cc is int64; n_max: the largest window); a slot outside [0, gnx_n_slots).  A pending
 * crossover is cut first and an uncompacted population would be gathered, as there.
 * gnx_divmap_info: the locus tiles, the chunks (runs of at most 511 individuals of one map
 * cell) and the kernel launches of the last call.                                         */
int gnx_divmap_sums(gnx_state* h, int64_t n, const int32_t* slots /*[n], grouped by map cell*/,
                    int32_t nx, int32_t ny, const int64_t* cell_start /*[nx * ny + 1]*/,
                    int32_t r, const uint64_t* locus_mask /*[W64] or NULL*/, int64_t max_counts,
                    int32_t* out_n, int32_t* out_S, int64_t* out_het, int64_t* out_cc);
int gnx_divmap_info(gnx_state* h, int64_t* tiles, int64_t* chunks, int64_t* launches);
/* r^2 between the listed loci (_calc_ld); double [n][n], NaN on the diagonal */
int gnx_stats_ld(gnx_state* h, int32_t n_loci, const int32_t* loci, double* r2);
/* the counts behind r^2, which add over tiles: c[i] 1-alleles at locus i, cc[i][j]
 * chromosomes carrying 1 at both i and j                                        */
int gnx_stats_ld_counts(gnx_state* h, int32_t n_loci, const int32_t* loci, int64_t* c /*[n]*/,
                        int64_t* cc /*[n][n]*/);

/* ---- genetic PCA and distances (reference sim/model.py:2031-2041 plot_genetic_PCA,
 *      demos/_IBD_IBE.py:38-192 calc_dists) ---------------------------------------
 * D = dosages d = a + b in {0, 1, 2} of the individuals in `slots` (rows in that order;
 * slots == NULL: all living slots [0, N), and n must equal N).  Every call refuses a handle
 * without genomes or with ghost records (tiles), cuts a pending crossover first and gathers
 * an uncompacted population before it reads.  The padding bits past L never count.       */
/* G = D D^T, exact, int64 [n][n] on the HOST, n <= 8192; locus_mask: u64 [W64] bit mask of
 * the loci to use (NULL: all L)                                                         */
int gnx_geno_gram(gnx_state* h, int64_t n, const int64_t* slots, const uint64_t* locus_mask,
                  int64_t* G);
/* Y = D M: M fp32 [L][k] and Y fp32 [n][k] are DEVICE pointers (e.g. torch tensors on the
 * handle's device), 1 <= k <= 64.  The caller's writes of M must be complete (synchronise its
 * stream); the call returns when Y is complete, and any stream may read it.               */
int gnx_geno_matmul(gnx_state* h, int32_t k, const float* M, float* Y, int64_t n,
                    const int64_t* slots);
/* Z = D^T Y: Y fp32 [n][k] and Z fp32 [L][k] DEVICE pointers, as gnx_geno_matmul         */
int gnx_geno_rmatmul(gnx_state* h, int32_t k, const float* Y, float* Z, int64_t n,
                     const int64_t* slots);
/* Weighted relationship matrix (csrc/gnx_grm.hip): G_ij = sum over the loci l of the mask of
 * val[l][d_il] * val[l][d_jl], double [n][n] on the HOST, 1 <= n <= 8192; val: fp32 [L][3] on
 * the HOST, the value of locus l at dosage 0, 1, 2 (the host folds centring, weights and
 * sqrt(w) into it; geonomics_amd/sim/quantgen.py).  n, slots, locus_mask and the preconditions
 * as gnx_geno_gram.  f32 MFMA: every fp32 accumulation chain holds at most 1024 products and the
 * chains are added in fp64 in locus order, so |G_ij - exact| <= (1024 * 2^-24 + L * 2^-53) *
 * sum_l |val[l][d_il] val[l][d_jl]| to first order; G == G^T exactly and a repeated call is
 * bit-equal.  Rows past n of a partial tile and loci outside the mask contribute exactly 0.
 * gnx_grm_info: the 128 x 128 tiles, the fp32 chains behind each entry and the HIP-event time
 * of the last call's kernels (each may be NULL).                                           */
int gnx_grm(gnx_state* h, int64_t n, const int64_t* slots, const uint64_t* locus_mask,
            const float* val, double* G);
int gnx_grm_info(gnx_state* h, int64_t* tiles, int64_t* k_chunks, double* kernel_ms);
/* A measuring switch (tools/grm_bench.py): mode 1 runs the kernel's expansion of the bits
 * alone, mode 2 its MFMAs alone; gnx_grm then returns zeros and only its kernel time means
 * anything.  Mode 0 (the default) is the kernel.                                         */
int gnx_grm_probe(gnx_state* h, int32_t mode);

/* ---- genotype-environment association (reference sim/model.py:2717-2780 Model.run_gea ->
 *      structs/species.py:2218-2355 _make_gea_df / _run_cca: the N x L table of mean
 *      genotypes with env, lat, long on the host, then sklearn's CCA) ------------------------
 * The cross-products over the individuals that the fit needs (geonomics_amd/sim/gea.py), of
 * the dosages D at the listed loci (1..8192 of them, ascending and distinct) of the
 * individuals in `slots` (NULL: all living slots, and n must equal N).  Preconditions as the
 * calls above.  Outputs are HOST buffers.                                                  */
/* C = D^T D, int64 [n_loci][n_loci], and s = D^T 1, int64 [n_loci], exact; n <= 2^29
 * (replaces the genotype columns of _make_gea_df, structs/species.py:2252-2255)           */
int gnx_geno_locus_gram(gnx_state* h, int32_t n_loci, const int32_t* loci, int64_t n,
                        const int64_t* slots, int64_t* C, int64_t* s);
/* D^T Z double [n_loci][3], Z^T Z double [3][3], Z^T 1 double [3] with Z = [e of layer lyr,
 * x, y] read from the device's own columns (_make_gea_df's env, lat, long,
 * structs/species.py:2258-2264) and summed in fp64 in a fixed order                        */
int gnx_geno_locus_cross(gnx_state* h, int32_t n_loci, const int32_t* loci, int32_t lyr,
                         int64_t n, const int64_t* slots, double* DtZ, double* ZtZ,
                         double* Zt1);

/* ---- isolation by distance and by environment (csrc/gnx_mantel.hip; reference
 *      demos/_IBD_IBE.py:195-330 -> data/IBD_IBE_demo/MMRR.py:7-74, which refits an OLS on the
 *      n (n - 1) / 2 unfolded pairs once per permutation, and data/IBD_IBE_demo/run_mantel.R,
 *      vegan's mantel.partial) -------------------------------------------------------------
 * The cross-sums of the genetic distance matrix Y with n_pred predictor distance matrices
 * under row-and-column permutation of Y, from which every statistic of both tests follows
 * (geonomics_amd/sim/mmrr.py).  n, slots, locus_mask and the preconditions as gnx_geno_gram
 * (1..8192 individuals); Y[a][b] = 0.5 sqrt(G_aa + G_bb - 2 G_ab) of that call's exact G, which
 * stays on the device.  Predictor k is the Euclidean distance over columns pred_off[k] ..
 * pred_off[k + 1] - 1 (pred_off int32 [n_pred + 1], from 0; 1..4 predictors, at most 8 columns
 * together) of pred_cols int32 [columns][2] = {field, index}: {GNX_F_X, 0}, {GNX_F_Y, 0},
 * {GNX_F_E, layer} or {GNX_F_Z, trait}, read as the device holds them.  perm int32
 * [n_perm][n] (1..2^20 permutations): individual i of the sample takes the columns of individual
 * perm[p][i]; an entry outside 0..n-1 is an error before anything is launched.  HOST outputs,
 * fp64 throughout, summed in a fixed order (a call repeated is bit-equal):
 * sums [n_perm][n_pred]: S_k(p) = sum over pairs a > b of Y[a][b] x_k[perm[p][a]][perm[p][b]];
 * moments [3 + 2 n_pred + n_pred (n_pred + 1) / 2] of the unpermuted sample over the pairs:
 * their number, sum y, sum y^2, sum x_k, sum y x_k, sum x_k x_l (k <= l, row-major).        */
int gnx_dist_perm_sums(gnx_state* h, int64_t n, const int64_t* slots, const uint64_t* locus_mask,
                       int32_t n_pred, const int32_t* pred_off, const int32_t* pred_cols,
                       int32_t n_perm, const int32_t* perm, double* sums, double* moments);
/* The same with n x n predictor matrices behind the column predictors: predictor n_pred + k is
 * x[a][b] = mats[k][a][b] (mats double [n_mat][n][n], HOST), 0..4 column predictors (pred_off and
 * pred_cols may be NULL without any), 0..4 matrices, 1..4 predictors together.  Every matrix must
 * be finite, exactly symmetric and zero on its diagonal: anything else is an error before anything
 * is launched (checked on the host).  sums and moments as above with n_pred + n_mat predictors,
 * the columns first: sums[p][k] = sum over a > b of Y[a][b] x_k[perm[p][a]][perm[p][b]], fp64,
 * fixed order (a call repeated is bit-equal).  Without a matrix (n_mat = 0) the call is
 * gnx_dist_perm_sums: the same bits.  In front of a matrix the column predictors have the terms
 * of gnx_dist_perm_sums, added in stripes of 8 columns of the sample where that call takes 16
 * with 4 predictor columns or fewer: their sums are the bits of its sums with 5..8 predictor
 * columns, and within its summation bound of them with fewer.  A matrix entry is gathered
 * (perm a fixed over the inner loop: one row of the matrix at a time).                         */
int gnx_dist_perm_sums_mat(gnx_state* h, int64_t n, const int64_t* slots,
                           const uint64_t* locus_mask, int32_t n_pred, const int32_t* pred_off,
                           const int32_t* pred_cols, int32_t n_mat,
                           const double* mats /*[n_mat][n][n]*/, int32_t n_perm,
                           const int32_t* perm, double* sums, double* moments);

/* ---- least-cost distances over the landscape (csrc/gnx_cost.hip; the reference has no such
 *      analysis: its Species move along conductance surfaces, but nothing measures the cost of
 *      travelling through them) ----------------------------------------------------------------
 * The graph (geonomics_amd/sim/cost.py restates it with scipy's Dijkstra).  Nodes: the H x W
 * cells of the handle's landscape, cell = y * W + x.  Every cell is joined to its 8 neighbours.
 * R double [H][W] (HOST): every entry > 0, or +inf where the cell is impassable (anything else,
 * nan included, is an error).  The edge between passable cells u, v costs
 *   w = (0.5 * (R[u] + R[v])) * len,
 * evaluated in that order in fp64 without contraction, len = res_x for a step along x, res_y along
 * y and sqrt(res_x res_x + res_y res_y) for a diagonal one (res_x, res_y > 0, finite); an edge
 * exists iff both ends are passable, and a diagonal step does not look at the two cells it passes
 * between.  d(s, t) = the cost of the cheapest path, the fp64 sum of its edges from s on;
 * d(s, s) = 0, also on an impassable cell; d = +inf where there is no path, so an impassable
 * source is at +inf from every other cell.  The distances are the unique fixed point of
 * d[v] = min_u (d[u] + w_uv) below d[s] = 0 and do not depend on the order of relaxation: a call
 * repeated, or made under another gnx_cost_budget, is bit-equal.
 * Refused (return 1) by all four entry points, before any other check: ghost records (a tile).
 * Refused before anything is launched: a bad R entry or res,
 * a cell outside 0..H W - 1, a budget below one source's raster; gnx_cost_matrix: a cell listed
 * twice, n_cells outside 1..32768.  A solve that has not settled after H W + 2 rounds ends with
 * the error "did not converge" (it cannot on a valid graph).  Nothing of the handle changes.
 * gnx_cost_surfaces: out double [n_src][H][W] (HOST), the accumulated-cost raster of every
 * source (sources may repeat).                                                               */
int gnx_cost_surfaces(gnx_state* h, const double* R /*[H][W]*/, double res_x, double res_y,
                      int32_t n_src, const int32_t* src /*cell = y * W + x*/,
                      double* out /*[n_src][H][W]*/);
/* gnx_cost_matrix: D double [n_cells][n_cells] (HOST) of distinct cells.  Every cell is solved
 * as a source and its raster is gathered at the listed cells on the device: only D crosses the
 * bus.  D is exactly symmetric: for a > b, D[a][b] = D[b][a] = the distance computed from source
 * cells[b] (the lower index) at cells[a]; the diagonal is 0.                                   */
int gnx_cost_matrix(gnx_state* h, const double* R /*[H][W]*/, double res_x, double res_y,
                    int32_t n_cells, const int32_t* cells /*distinct*/,
                    double* D /*[n_cells][n_cells]*/);
/* bytes of distance rasters (H W 8 per source) one batch of sources may take: more sources are
 * worked off batch by batch (0: the default, 2 GiB).  Negative, or positive and below one
 * source's raster: an error                                                                    */
int gnx_cost_budget(gnx_state* h, int64_t bytes);
/* of the last gnx_cost_surfaces / gnx_cost_matrix: its kernels' HIP-event time (ms), their
 * number, the rounds (one launch over the active (tile, source) pairs each, summed over the
 * batches) and the batches of sources; each may be NULL                                        */
int gnx_cost_info(gnx_state* h, double* kernel_ms, int64_t* launches, int64_t* rounds,
                  int64_t* batches);

/* ---- circuit-theory resistance distances and current maps (csrc/gnx_circuit.hip; the reference
 *      has no such analysis) --------------------------------------------------------------------
 * The graph is the one of the least-cost distances above (geonomics_amd/sim/circuit.py restates
 * what follows with scipy's splu): R, res_x, res_y and cell = y * W + x as there; the edge between
 * passable cells u, v is a resistor of w ohms, g = 1.0 / w its conductance in fp64, and
 * L = diag(sum g) - G the Laplacian, component by component.
 *   reff(s, t) = (e_s - e_t)' L+ (e_s - e_t)  for two passable cells of one connected component;
 *   reff(s, s) = 0, also on an impassable cell; reff = +inf between components and from or to an
 *   impassable cell.
 * The first listed cell of every component is its anchor a; every other passable listed cell i
 * is one system L x_i = e_i - e_a, solved from x = 0 by Jacobi-preconditioned conjugate gradients
 * in fp64 (x_a = 0; only differences of x_i inside the component mean anything).  A system stops
 * when the recurrence residual is at most tol sqrt(2) (sqrt(2) = the norm of the right-hand side;
 * tol > 0, finite); then the true residual b - L x is recomputed, and a system above the
 * threshold restarts from it, at most 3 times.  max_iter: the iterations one batch of systems may
 * take in all (0: twice the passable cells of the largest component).  Running out of iterations
 * or restarts is an error that names the system and its residual.  No floating-point atomics: a
 * call repeated, or made under another gnx_circuit_budget, is bit-equal.
 * Refused (return 1) by all five entry points, before any other check: ghost records (a tile).
 * Refused before anything is launched: n outside 1..8192 (gnx_circuit_matrix) or 1..128 (the other
 * two), a bad R entry, res or tol, max_iter < 0, a cell outside 0..H W - 1, a cell listed twice, a
 * budget below one system's rasters.  Nothing of the handle changes.
 * gnx_circuit_matrix: out double [n][n] (HOST), exactly symmetric with a zero diagonal,
 *   reff(i, j) = (x_i[c_i] - x_j[c_i]) - (x_i[c_j] - x_j[c_j]) evaluated once for i < j.  The
 *   systems are solved batch by batch under the budget; of a batch only x at the listed cells is
 *   kept.                                                                                       */
int gnx_circuit_matrix(gnx_state* h, const double* R /*[H][W]*/, double res_x, double res_y,
                       int32_t n, const int32_t* cells /*distinct*/, double tol,
                       int64_t max_iter, double* out /*[n][n]*/);
/* gnx_circuit_current: out double [H][W] (HOST) = the sum over all unordered pairs (s, t) of
 *   listed cells that share a component of the node current
 *   c(u) = 0.5 (sum_k g_uk |v_u - v_k| + |b_u|), v = x_s - x_t, b = +1 at s, -1 at t, 0 elsewhere
 *   (the source and the sink carry 1; a cell of a 1-wide corridor between them carries 1);
 *   impassable cells hold 0.  counts[0] = the pairs used, counts[1] = the pairs skipped (across
 *   components, or with an impassable cell).  The work is pairs x cells x 8 edges, hence at most
 *   128 cells.  The potentials of all systems must be resident (H W 8 bytes each, beside the
 *   4 H W 8 of one system's work): above the budget the call is refused with the bytes needed. */
int gnx_circuit_current(gnx_state* h, const double* R /*[H][W]*/, double res_x, double res_y,
                        int32_t n, const int32_t* cells /*distinct*/, double tol,
                        int64_t max_iter, double* out /*[H][W]*/, int64_t* counts /*[2]*/);
/* gnx_circuit_potentials: out double [n][H][W] (HOST) = x_i as the solver left it (all 0 for an
 *   anchor and for an impassable cell); anchor int32 [n] = the index in cells of cell i's anchor
 *   (i itself for an anchor, -1 for an impassable cell).  Resident as gnx_circuit_current.       */
int gnx_circuit_potentials(gnx_state* h, const double* R /*[H][W]*/, double res_x, double res_y,
                           int32_t n, const int32_t* cells /*distinct*/, double tol,
                           int64_t max_iter, int32_t* anchor /*[n]*/, double* out /*[n][H][W]*/);
/* bytes of solver rasters one batch of systems may take (5 rasters of H W 8 bytes per system:
 * x, r, two p, L p); more systems are worked off batch by batch (0: the default, 4 GiB).
 * Negative, or positive and below one system's rasters: an error                                */
int gnx_circuit_budget(gnx_state* h, int64_t bytes);
/* of the last gnx_circuit_matrix / current / potentials: its kernels' HIP-event time (ms), their
 * number, the CG iterations summed over the batches, the restarts, and the worst true residual
 * norm of a system; each may be NULL                                                            */
int gnx_circuit_info(gnx_state* h, double* kernel_ms, int64_t* launches, int64_t* iterations,
                     int64_t* restarts, double* worst_residual);

/* ---- fine-scale spatial genetic structure (csrc/gnx_sgs.hip; the reference has no such
 *      analysis: its IBD demo, demos/_IBD_IBE.py, ends at MMRR on a sample) ----------------
 * The sums over the pairs of individuals closer than the largest distance class, from which mean
 * kinship per class, its slope on ln(distance), Sp and the neighbourhood size follow
 * (geonomics_amd/sim/sgs.py).  n, slots, locus_mask and the preconditions as gnx_geno_gram, but
 * no n x n matrix is formed: 1..2^24 individuals.  edges double [n_bins + 1], finite, strictly
 * ascending, edges[0] >= 0; 1..32 classes.  For a pair a != b of the sample, dx and dy are the
 * fp64 differences of the device's fp32 x and y, r = sqrt(dx dx + dy dy) in fp64 without
 * contraction (IEEE sqrt); the pair is in class k when edges[k] <= r < edges[k + 1]; pairs with
 * r == 0 are in no class and are counted in *n_zero; every unordered pair is visited once.  d is
 * the dosage (0, 1, 2) at the masked loci; with perm int32 [n] sample index i stands at its own
 * position with the genome of sample index perm[i].  dot_ab = sum_l d_al d_bl, self_a = sum_l
 * d_al^2, w_a = sum_l locus_weight[l] d_al (double [L]; fp64, loci ascending; NULL: 0).
 * HOST outputs:  isums int64 [n_bins][3] = {pairs, sum dot_ab, sum (self_a + self_b)}, exact;
 * fsums double [n_bins][7] = {sum r, sum ln r, sum ln^2 r, sum dot_ab ln r,
 * sum (self_a + self_b) ln r, sum (w_a + w_b), sum (w_a + w_b) ln r}.  The fp64 sums are taken
 * without atomics in an order that the sample, the edges and the landscape fix (they do depend
 * on that order, within the usual m 2^-53 sum |term|): a call repeated is bit-equal in all
 * outputs.  *work = the candidate pairs (every pair of individuals in the same or adjacent cells
 * of a grid whose side is just above edges[n_bins], larger where the landscape would have more
 * than 2^22 cells) times the number of words the mask touches; it is known after the cell sort
 * and before the operand is gathered.  max_work <= 0: only *work is written (isums, fsums and
 * n_zero may be NULL).  Refused (return 1) before anything is launched: bad edges, n_bins or n,
 * a slot out of range, a perm entry outside 0..n-1, n (n - 1) / 2 * 8 L >= 2^63; after the cell
 * sort and before anything else: *work > max_work.  Nothing of the handle changes.          */
int gnx_sgs_sums(gnx_state* h, int64_t n, const int64_t* slots, const uint64_t* locus_mask,
                 int32_t n_bins, const double* edges /*[n_bins + 1]*/,
                 const double* locus_weight /*[L] or NULL*/, const int32_t* perm /*[n] or NULL*/,
                 int64_t max_work, int64_t* work, int64_t* isums /*[n_bins][3]*/,
                 double* fsums /*[n_bins][7]*/, int64_t* n_zero);

/* ---- genome-wide linkage disequilibrium (csrc/gnx_ld.hip; the reference's _calc_ld,
 *      sim/stats.py:359-390, is gnx_stats_ld above: an L x L matrix, at most 8192 loci) --------
 * Per bin of the distance between two loci: the number of locus pairs and the sums of r^2, r^4,
 * the distance and Weir & Hill's drift weight, from which the decay of r^2 with distance and the
 * LD estimate of N_e follow (geonomics_amd/sim/ld.py).  Nothing n_loci x n_loci is formed.
 * n, slots as gnx_geno_gram (1..2^25 individuals; slots distinct); the sample's chromosomes are
 * 2 * sample index + homologue, N = 2 n of them.  loci int32 [n_loci], distinct, in any order of
 * locus number; pos double [n_loci], finite and non-decreasing: the coordinate of loci[j] (the
 * caller's unit).  edges double [n_edges], 2..65 of them, strictly ascending, finite but for the
 * last, which may be +inf.  c1[j] = the 1-alleles of loci[j] over the N chromosomes; a locus is
 * KEPT iff min(c1, N - c1) >= max(1, min_minor).  For kept loci i < j (indices of the request),
 * c_ij = the chromosomes carrying 1 at both, in fp64 without contraction:
 *   Dn = N c_ij - c_i c_j (int64, exact);  r2 = (Dn Dn) / ((c_i (N - c_i)) (c_j (N - c_j))), each
 *   bracket exact, three IEEE roundings;  d = pos[j] - pos[i];  the pair is in bin b when
 *   edges[b] <= d < edges[b + 1], in no bin otherwise;  with morgans != 0:
 *   c = 0.5 |expm1(-2 d)| (= -0.5 expm1(-2 d), and +0 at d = 0 whatever zero expm1 returns),
 *   w = ((1 - c)(1 - c) + c c) / ((2 c)(2 - c)), else w = 0.
 * A pair at d = 0 has w = +inf under morgans, and so has the sum of its bin: not special-cased.
 * HOST outputs: c1 int64 [n_loci], pairs int64 [n_edges - 1], fsums double [n_edges - 1][4] =
 * {sum r2, sum r2 r2, sum d, sum w}.  The fp64 sums are taken without atomics in an order fixed
 * by the arguments and gnx_ld_budget: a call repeated is bit-equal in all outputs.  *work = the
 * 64 x 64-locus tiles whose distance range meets [edges[0], edges[last]) times the chromosome
 * words ceil(N / 64); max_work <= 0: only *work is written (the outputs may be NULL).  Refused
 * (return 1) before anything is launched: no genomes, ghost records, n out of range, a slot or
 * locus out of range or listed twice, pos not non-decreasing, bad edges, *work > max_work.
 * Nothing of the handle changes.                                                            */
int gnx_ld_bins(gnx_state* h, int64_t n, const int64_t* slots, int32_t n_loci,
                const int32_t* loci, const double* pos /*[n_loci]*/, int32_t n_edges,
                const double* edges /*[n_edges]*/, int32_t min_minor, int32_t morgans,
                int64_t max_work, int64_t* work, int64_t* c1 /*[n_loci]*/,
                int64_t* pairs /*[n_edges - 1]*/, double* fsums /*[n_edges - 1][4]*/);
/* bytes of transposed bit rows (loci rounded up to 64 x ceil(N / 64) rounded up to 16 x 8)
 * gnx_ld_bins keeps resident: above it
 * the loci are worked off in blocks of whole 64-locus tiles, two blocks at a time (0: the
 * default, 256 MiB)                                                                          */
int gnx_ld_budget(gnx_state* h, int64_t bytes);
/* of the last gnx_ld_bins: its kernels' HIP-event time (ms), their number and the number of
 * locus blocks; each may be NULL                                                             */
int gnx_ld_info(gnx_state* h, double* kernel_ms, int64_t* launches, int64_t* locus_blocks);

/* ---- identity tracts of the phased genomes (csrc/gnx_tracts.hip; the reference has no such
 *      analysis) -----------------------------------------------------------------------------
 * Runs of homozygosity per individual and tracts shared between the haplotypes of two
 * individuals (geonomics_amd/sim/tracts.py).  Definitions:
 * A *haplotype pair* is two bit rows a, b of L loci.  D_l = a_l xor b_l for 0 <= l < L.  Padding
 * bits past L never count and never extend a tract.
 * `brk` is a bit mask over loci.  Bit l set means that a tract cannot continue from locus l-1
 * into locus l, i.e. a chromosome boundary.  Bit 0 is ignored.  NULL means no breaks.
 * A *tract* is a maximal stretch s..e with D_l = 0 for all s <= l <= e and brk_l = 0 for all
 * s < l <= e.  A locus with D_l = 0 and brk_l = 1 ends one tract at l-1 and starts the next at l.
 * `pos` is int64 [L], non-decreasing.  It is the locus coordinate in an integer unit chosen by
 * the caller.
 *   The tract's *locus count* is e - s + 1.
 *   Its *length* is pos[e] - pos[s].
 *   It *qualifies* iff count >= max(1, min_loci) and length >= min_len.
 * Everything the device returns is an integer function of the qualifying tracts.  Every output is
 * therefore exact, independent of order (integer atomics are fine), and bit-equal to the
 * restatement.
 * Masking loci is deliberately left out.  A monomorphic locus has D = 0 for every pair, so
 * skipping it would change no tract's extent, only its locus count.
 *
 * gnx_tracts_self scans each listed individual's homologue 0 against its homologue 1, for
 * 1..2^25 individuals (n, slots as gnx_geno_gram; slots distinct).  HOST outputs:
 *   per[i] = {qualifying tracts, sum of their locus counts, sum of their lengths, the largest
 *   length (0 without a tract)};
 *   hist[b] = {tracts, sum of length} over all listed individuals; a tract is in bin b when
 *   edges[b] <= length < edges[b + 1], in no bin otherwise; edges int64, 2..65 of them, strictly
 *   ascending (hist NULL: n_edges = 0 and no edges);
 *   cover[l] = the number of listed individuals with a qualifying tract that contains locus l.
 * Refused (return 1) before anything is launched: no genomes, ghost records, n out of range, a
 * slot out of range or listed twice, pos decreasing, bad edges, min_len < 0.  Nothing of the
 * handle changes.                                                                             */
int gnx_tracts_self(gnx_state* h, int64_t n, const int64_t* slots /*NULL: all living, n == N*/,
                    const int64_t* pos /*[L]*/, const uint64_t* brk /*[W64] or NULL*/,
                    int32_t min_loci, int64_t min_len, int32_t n_edges,
                    const int64_t* edges /*[n_edges] or NULL*/, int64_t* per /*[n][4]*/,
                    int64_t* hist /*[n_edges - 1][2] or NULL*/, int64_t* cover /*[L] or NULL*/);
/* gnx_tracts_pairs takes a sample of 1..4096 individuals.  For a != b the unit is the four
 * haplotype pairs (a_h, b_g): cnt (qualifying tracts), len (the sum of their lengths) and longest
 * are summed (max for longest) over the four; they are symmetric, and each may be NULL.  The
 * diagonal [a][a] is the individual's own pair (a_0, a_1), i.e. what gnx_tracts_self reports for
 * it.  hist and cover are taken over the off-diagonal unordered pairs only; each haplotype pair
 * counts once, so cover[l] <= 2 n (n - 1).  *work = (2 n (n - 1) + n) ceil(L / 64) word steps;
 * max_work <= 0: only *work is written; *work > max_work is refused before the gather.  Other
 * refusals as gnx_tracts_self.                                                                 */
int gnx_tracts_pairs(gnx_state* h, int64_t n, const int64_t* slots, const int64_t* pos,
                     const uint64_t* brk, int32_t min_loci, int64_t min_len, int32_t n_edges,
                     const int64_t* edges, int64_t max_work, int64_t* work,
                     int32_t* cnt /*[n][n]*/, int64_t* len /*[n][n]*/, int64_t* longest /*[n][n]*/,
                     int64_t* hist, int64_t* cover);
/* of the last gnx_tracts_self / gnx_tracts_pairs: its kernels' HIP-event time (ms), their number
 * and the genome bytes the scan loaded (gnx_tracts_self: blocks that both homologues share are
 * not read; gnx_tracts_pairs: the gather's); each may be NULL                                  */
int gnx_tracts_info(gnx_state* h, double* kernel_ms, int64_t* launches, int64_t* bytes_read);

/* ---- close-kin pairs (csrc/gnx_kin.hip; the reference has no such analysis) ----------------
 * Who is related to whom: KING-robust kinship (Manichaikul et al. 2010) and the IBS0 count of
 * pairs of individuals, from which parent-offspring, full-sib and second-degree pairs are named
 * (geonomics_amd/sim/kin.py).  Definitions, for individual a with homologue bits a0, a1 at the
 * masked loci:
 *   O_a = a0 | a1,  P_a = a0 & a1 (homozygous 1),  het_a = O_a ^ P_a;
 *   nhet_a = popcount(het_a);
 *   hh_ab = popcount(het_a & het_b)                              (both heterozygous);
 *   ibs0_ab = popcount(P_a & ~O_b) + popcount(P_b & ~O_a)        (opposite homozygotes);
 *   kinship_ab = (hh_ab - 2 ibs0_ab) / (nhet_a + nhet_b), in fp64, ON THE HOST ONLY; a zero
 *   denominator gives NaN in the matrix, and such a pair is never kept in the list.
 * Everything the device returns is an integer per individual or per pair: exact, independent of
 * order (integer atomics are fine), and bit-equal to the numpy restatement (sim/kin.py).
 * n, slots, locus_mask and the preconditions as gnx_geno_gram.
 *
 * gnx_kin_matrix: 1..8192 individuals.  HOST outputs, int32: nhet [n], hh [n][n], ibs0 [n][n],
 * symmetric, with hh[a][a] = nhet_a and ibs0[a][a] = 0.                                        */
int gnx_kin_matrix(gnx_state* h, int64_t n, const int64_t* slots, const uint64_t* locus_mask,
                   int32_t* nhet /*[n]*/, int32_t* hh /*[n][n]*/, int32_t* ibs0 /*[n][n]*/);
/* gnx_kin_pairs: the list of kept pairs of 1..2^24 individuals, no n x n matrix.  For a pair
 * a != b of the sample r is taken as gnx_sgs_sums takes it (fp64 from the device's fp32 x and y,
 * without contraction).  With 0 < max_dist < inf a pair is a CANDIDATE iff r < max_dist - pairs at
 * r == 0 are candidates, unlike in gnx_sgs_sums - and only the pairs of individuals in the same
 * or adjacent cells of gnx_sgs_sums' grid (side just above max_dist, at most 2^22 cells) are
 * looked at; max_dist <= 0 or infinite: every pair is a candidate (one cell).  A candidate is KEPT
 * iff nhet_a + nhet_b > 0 and (hh - 2 ibs0) 2^20 >= T (nhet_a + nhet_b) in int64; the host passes
 * T = ceil(min_kinship 2^20), -2^20 <= T <= 2^19.  *work = the pairs of individuals in the same
 * or adjacent cells times the number of words the mask touches; it is known after the cell sort
 * and before the operand is gathered.  max_work <= 0: only *work is written (every other output
 * may be NULL).  HOST outputs otherwise: *n_candidates, *n_found (the kept pairs), nhet int32 [n]
 * and, for k < *n_found, the sample indices pa[k] < pb[k] with hh[k] and ibs0[k], int32
 * [max_pairs] each, sorted by (pa, pb): a call repeated is byte-equal.  max_pairs in 1..2^26.
 * Refused (return 1) before anything is launched: n, T or max_pairs out of range, max_dist NaN,
 * a slot out of range; after the cell sort and before the gather: *work > max_work (*work is
 * written); after the pair kernel: *n_found > max_pairs, with a message containing "exceed
 * max_pairs" - *work and *n_found are written, nothing else.  Nothing of the handle changes.  */
int gnx_kin_pairs(gnx_state* h, int64_t n, const int64_t* slots, const uint64_t* locus_mask,
                  double max_dist, int64_t T, int64_t max_pairs, int64_t max_work, int64_t* work,
                  int64_t* n_candidates, int64_t* n_found, int32_t* pa /*[max_pairs]*/,
                  int32_t* pb /*[max_pairs]*/, int32_t* hh /*[max_pairs]*/,
                  int32_t* ibs0 /*[max_pairs]*/, int32_t* nhet /*[n]*/);
/* of the last gnx_kin_matrix / gnx_kin_pairs: its kernels' HIP-event time (ms), their number and
 * its 64 x 64 tiles of pairs; each may be NULL                                                 */
int gnx_kin_info(gnx_state* h, double* kernel_ms, int64_t* launches, int64_t* tasks);

/* ---- haplotype sweep scans (csrc/gnx_sweeps.hip; the reference has no such analysis) -----------
 * Extended haplotype homozygosity around core loci of the phased genomes, from which EHH, iHS,
 * nSL and XP-EHH follow on the host (geonomics_amd/sim/sweeps.py).  Definitions:
 * Sample.  n individuals in the order of `slots` (n, slots as gnx_geno_gram; slots distinct).
 *   Chromosome 2 i + h is homologue h of sample i.  N = 2 n, with 1 <= n <= 2048.
 * Request.  loci int32 [n_loci], distinct, in any order of locus number.  pos int64 [n_loci],
 *   non-decreasing: the coordinate of loci[j] in an integer unit of the caller's.  brk uint8
 *   [n_loci]: brk[j] != 0 means no scan passes between request index j - 1 and j (a chromosome
 *   boundary); brk[0] is ignored; NULL means no breaks.
 * Kept loci.  c1[j] = the sampled chromosomes that carry 1 at loci[j].  Locus j is KEPT iff
 *   min(c1, N - c1) >= max(2, min_minor).  A locus that is not kept does not exist for the scan:
 *   it is neither a core nor a step.  Its break is inherited by the next kept locus: a break
 *   anywhere between two consecutive kept loci separates them.
 * Classes.  cls == NULL: the class of a chromosome at core j is its allele at j (0 ancestral, 1
 *   derived).  Otherwise cls is uint8 [N] of 0, 1 or 255, the same for every core; 255: the
 *   chromosome is in neither class and is ignored (XP-EHH's two populations).  m_c = the size of
 *   class c, T_c = m_c (m_c - 1) / 2.
 * Scan of (core j, direction d: 0 left, 1 right, class c).  k_0 = j and P_0 = T_c.  Step s goes
 *   from kept locus k_{s-1} to the next kept locus k_s in direction d.  P_s = the unordered pairs
 *   of class-c chromosomes identical at every kept locus from j to k_s inclusive - the core itself
 *   only when cls == NULL, where that is vacuous: with a class row two chromosomes of a class may
 *   differ at the core; P_0 = T_c still and the core's own column is not compared.
 * Status.  Before step s the scan stops, in this order of tests: status 1: there is no next kept
 *   locus, or a break lies between; status 2: max_gap > 0 and |pos[k_s] - pos[k_{s-1}]| > max_gap;
 *   status 3: max_extent > 0 and |pos[k_s] - pos[j]| > max_extent; after computing P_s, status 0:
 *   P_s cut_den < cut_num T_c (the cutoff: the step that falls below is not integrated).  A class
 *   with m_c < 2 has status 4, area 0 and steps 0; a locus that is not kept, or not among cores,
 *   has status 5, area 0 and steps 0.
 * Integration.  Every completed step s adds (P_{s-1} + P_s) |pos[k_s] - pos[k_{s-1}]| to area,
 *   so iHH = area / (2 T_c) in the caller's unit.  steps = the completed steps.
 * Everything the device returns is an integer function of the sample: every output is exact,
 * order-free, and bit-equal to the restatement (sim/sweeps.brute_scan) and to a repeated call.
 * cores int32 [n_cores]: request indices of the loci to scan, distinct (NULL: every kept locus).
 * HOST outputs: c1 int64 [n_loci]; area int64, steps int32, status uint8 [n_loci][2][2], indexed
 * [direction][class]; curve int64 [2][2][n_loci] or NULL, accepted only with n_cores == 1:
 * curve[d][c][s] = P_s of the single core for s = 0 and every step whose P_s was computed (the
 * one that fell below the cutoff included), -1 past that and for a scan with status 4 or 5.
 * *work = scanned cores (the listed ones that are kept) x 4 x ceil(N / 64) x (kept loci - 1).
 * max_work <= 0: only *work and c1 are written (the other outputs may be NULL); *work > max_work
 * is refused after c1 is taken and before the scan.  Refused (return 1) before anything is
 * launched: no genomes, ghost records, n outside 1..2048, a slot or locus out of range or listed
 * twice, pos decreasing, a core out of range or listed twice, cut_num < 0, cut_den <= 0,
 * cut_num > cut_den, N (N - 1) (pos[last] - pos[0]) >= 2^62 (below it no area can overflow),
 * curve with n_cores != 1, a cls value other than 0, 1 or 255.  Nothing of the handle changes.  */
int gnx_sweeps_scan(gnx_state* h, int64_t n, const int64_t* slots, int32_t n_loci,
                    const int32_t* loci, const int64_t* pos /*[n_loci]*/,
                    const uint8_t* brk /*[n_loci] or NULL*/, const uint8_t* cls /*[2 n] or NULL*/,
                    int32_t n_cores, const int32_t* cores /*[n_cores] or NULL*/, int32_t min_minor,
                    int32_t cut_num, int32_t cut_den, int64_t max_gap, int64_t max_extent,
                    int64_t max_work, int64_t* work, int64_t* c1 /*[n_loci]*/,
                    int64_t* area /*[n_loci][2][2]*/, int32_t* steps /*[n_loci][2][2]*/,
                    uint8_t* status /*[n_loci][2][2]*/, int64_t* curve /*[2][2][n_loci] or NULL*/);
/* of the last gnx_sweeps_scan: its kernels' HIP-event time (ms), their number (the transpose's
 * two, then one per batch of cores) and the completed steps summed over its scans; each may be
 * NULL                                                                                         */
int gnx_sweeps_info(gnx_state* h, double* kernel_ms, int64_t* launches, int64_t* steps_total);

/* ---- model-based ancestry (csrc/gnx_admix.hip; the reference has no such analysis) -------------
 * One EM sweep of the admixture model of STRUCTURE / ADMIXTURE: individual i draws each of its
 * two alleles at locus l from ancestral population k with probability q_ik, and that allele is 1
 * with probability f_kl.  The sweep returns the numerators of the FRAPPE / ADMIXTURE EM update
 * and the log-likelihood; the update, its clamps and the acceleration are the caller's
 * (geonomics_amd/sim/ancestry.py).
 * Inputs: the sample of n individuals (n, slots as in the genetic PCA calls above); the loci of
 * locus_mask (u64 [W64], NULL: all L), L_u of them - padding bits past L, masked-out loci and
 * the zero words of the padding contribute to nothing; dosages d_il in {0, 1, 2}; 1 <= K <= 16;
 * Q fp64 [n][K] with positive rows; F fp64 [K][L] in [eps, 1 - eps], indexed by genome locus
 * (entries of unused loci are never read into a result); g_kl = 1 - f_kl rounded to fp64.
 * Per genotype of a used locus:
 *   p_il = sum_k q_ik f_kl,   r_il = sum_k q_ik g_kl,   u = d / p,   v = (2 - d) / r.
 * Outputs, fp64:
 *   A[i][k]  = sum over used l of (u f_kl + v g_kl)         the ancestry numerators
 *   B1[k][l] = sum_i u q_ik,   B0[k][l] = sum_i v q_ik        the frequency numerators; 0 at
 *                                                             every unused locus
 *   *loglik  = sum_il d ln p + (2 - d) ln r                   only when loglik != NULL (the two
 *                                                             logarithms cost as much as the rest)
 * The EM update is q'_ik = q_ik A_ik / (2 L_u) and f'_kl = f_kl B1 / (f_kl B1 + g_kl B0), f'
 * clamped to [eps, 1 - eps], q' clamped below at eps and its rows renormalised, eps = 1e-6.
 * For every valid input sum_k q_ik A_ik = 2 L_u.
 * The device takes p and r by K FMAs each and u, v from ONE division: t = 1 / (p r),
 * u = d (r t), v = (2 - d) (p t), three roundings beside those of p (r), and one logarithm
 * per genotype: 2 ln r, ln(p r) or 2 ln p for d = 0, 1, 2; its sums are taken in
 * an order fixed by the arguments and the budget, without floating-point atomics, so a call
 * repeated is bit-equal in every output.  Error bounds: tests/test_gpu_ancestry.py.
 * Q, F, A, B1, B0 are DEVICE pointers with the synchronisation contract of gnx_geno_matmul;
 * loglik is a HOST double.  skip_b != 0: B1 and B0 are not computed and may be NULL (F held
 * fixed: projection).  budget: bytes of partial sums one chunk of individuals may take (0: the
 * default, 256 MiB); above it the individuals are worked off in chunks of whole 64-row tiles,
 * one after the other (at least one tile per chunk).  Preconditions as the genetic PCA calls; a
 * pending crossover is cut first and an uncompacted population gathered; no individual, genome
 * or later draw is changed.  Refused (return 1) before anything is launched: no genomes, ghost
 * records, K outside 1..16, n < 1, an empty locus set, a null pointer, budget < 0, a slot out
 * of range.                                                                                   */
int gnx_admix_sweep(gnx_state* h, int64_t n, const int64_t* slots /*NULL: all living*/,
                    const uint64_t* locus_mask, int32_t K, const double* Q /*[n][K]*/,
                    const double* F /*[K][L]*/, double* A /*[n][K]*/, double* B1 /*[K][L]*/,
                    double* B0 /*[K][L]*/, double* loglik /*host, or NULL*/, int32_t skip_b,
                    int64_t budget);
/* of the last gnx_admix_sweep: its kernels' HIP-event time (ms), their number, the chunks over
 * the individuals and the template instance that ran (its K); each may be NULL               */
int gnx_admix_info(gnx_state* h, double* kernel_ms, int64_t* launches, int64_t* chunks,
                   int32_t* instance);

/* ---- local ancestry along the genome (csrc/gnx_lai.hip; the reference has no such analysis) ----
 * The linkage model of Falush, Stephens & Pritchard (2003) with fixed frequencies and one
 * admixture time, painted along every phased haplotype of the sample by forward-backward.  The
 * hidden state of haplotype t = 2 i + homologue at used locus j is its ancestry z in 0..K-1.
 * Inputs, all HOST buffers: the sample of n individuals (n, slots as in the genetic PCA calls, in
 * the order given); 1 <= K <= 8; the L_u used loci, ascending (loci NULL: all, L_u = L);
 * F fp64 [L_u][K] = P(allele 1 | ancestry k) strictly inside (0, 1); sw, stay fp64 [L_u], the
 * probabilities that the ancestry is drawn anew from the prior between used loci j - 1 and j, and
 * kept (sw[0] = 1, stay[0] = 0); Q fp64 [n][K], the prior of individual i (both homologues);
 * by int32 [n] labels in -1..max(n_groups, 1)-1 (-1: left out of anc_locus) or NULL (one group),
 * n_groups <= 64.  g = 1 - f rounded to fp64; E_k = f[j][k] if the haplotype's bit is 1, else
 * g[j][k].  Forward, j = 0 .. L_u - 1, alpha_{-1} = q:
 *   b_k = (stay_j alpha_{j-1,k} + sw_j q_k) E_k,  c = b_0 + b_1 + ..,  alpha_{j,k} = b_k / c,
 *   ll += ln c
 * Backward, beta_{L_u-1,k} = 1, j = L_u - 1 .. 0:
 *   p_k = alpha_{j,k} beta_{j,k},  gamma_{j,k} = p_k / (p_0 + p_1 + ..)
 *   j > 0: w_k = beta_{j,k} E_k,  u = q_0 w_0 + q_1 w_1 + ..,  b'_k = stay_j w_k + sw_j u,
 *          beta_{j-1,k} = b'_k / (b'_0 + b'_1 + ..)
 * Every operation is one IEEE fp64 +, * or / (no contraction), every sum over k runs left to
 * right; the logarithm is the device library's.  Outputs, HOST buffers:
 *   loglik    fp64 [2n]        the sum of ln c in ascending j
 *   anc_hap   fp64 [2n][K]     the sum of gamma over j, in descending j        (want_post)
 *   anc_locus fp64 [max(n_groups, 1)][L_u][K]  the sum of gamma over the haplotypes of the
 *             group, one after the other in ascending t                        (want_post)
 *   switches  int32 [2n]       the j >= 1 whose call differs from that of j - 1; the call is the
 *             smallest k of largest gamma                                      (want_post)
 *   calls     uint8 [2n][L_u]                                    (want_post and want_calls)
 * want_post == 0: only the forward pass runs, nothing is stored and only loglik is written.
 * budget: bytes of device scratch the posteriors (8 K L_u per haplotype, and 2 L_u with
 * want_calls) of one batch of haplotypes may take (0: the default, 4 GiB); the haplotypes are
 * worked off in batches of a multiple of 64.  No output depends on the budget, and a call repeated
 * is bit-equal in every output: no floating-point atomics.  *batches (may be NULL): the batches;
 * *kernel_ms (may be NULL): the HIP-event time of the call's kernels.  Preconditions as the
 * genetic PCA calls; no individual, genome or later draw is changed.  Refused (return 1) before
 * anything is launched: no genomes, ghost records, K outside 1..8, n < 1, L_u outside 1..L, loci
 * not ascending or outside 0..L-1, n_groups outside 0..64, a label outside -1..max(n_groups,1)-1,
 * a null pointer, budget < 0, a budget that cannot hold 64 haplotypes (want_post), a slot out of
 * range.                                                                                       */
int gnx_lai_paint(gnx_state* h, int64_t n, const int64_t* slots /*NULL: all living*/, int32_t K,
                  int32_t L_u, const int32_t* loci /*[L_u] or NULL*/, const double* F,
                  const double* sw, const double* stay, const double* Q, const int32_t* by,
                  int32_t n_groups, int64_t budget, int32_t want_post, int32_t want_calls,
                  double* loglik, double* anc_hap, double* anc_locus, int32_t* switches,
                  uint8_t* calls, int64_t* batches, double* kernel_ms);

/* ---- per-locus association scans (csrc/gnx_assoc.hip; the reference has no such analysis) ----
 * The cross-products of the dosages d = a + b in {0, 1, 2} (a, b the bits of the two homologues)
 * of the sample with a HOST matrix Y fp64 [n][m], 1 <= m <= 32 (n, slots as in the genetic PCA
 * calls, rows of Y in the order of the slots), and the integer moments of d per locus, from one
 * pass over the packed genomes.  Outputs, HOST buffers:
 *   DtY fp64 [L][m]   DtY[l][j] = sum over i of d_il Y_ij
 *   s1  int64 [L]     sum over i of d_il        (exact: counted bits)
 *   s2  int64 [L]     sum over i of d_il^2      (exact: s1 + 2 * the individuals with both bits)
 * Order of the fp64 sums, fixed by (n, L) alone.  The individuals 0 .. n - 1 (positions in the
 * sample) are cut into stretches of `*stretch` consecutive ones, the last one ragged:
 *   tiles = ceil(n / 64), lines = gnx_words_per_hom(L) / 16,
 *   want = min(tiles, 32, max(1, 2048 / lines))   (integer division),
 *   *stretch = 64 ceil(tiles / want),  *stretches = ceil(n / *stretch).
 * Within a stretch acc = fma(d, y, acc) from +0 over ascending individuals (d y is exact, so this
 * is the rounded acc + d y, the same with or without a fused multiply-add); the stretches' sums
 * are then added left to right from the first.  No atomics: a repeated call is byte-equal, and a
 * column's sums do not depend on m or on its position in Y.  The partial sums take
 * 8 m L *stretches bytes of device scratch, under 0.6 GB for L <= 2^21 and 8 m L beyond.
 * *stretch, *stretches, *kernel_ms (each may be NULL): the rule's result and the HIP-event time of
 * the call's kernels.  Preconditions as the genetic PCA calls; no individual, genome or later
 * draw is changed.  Refused (return 1) before anything is launched: no genomes, ghost records, m
 * outside 1..32, n outside 1..2^30, a null pointer, a NaN or infinity in Y, a slot out of range,
 * n != N with slots NULL.                                                                      */
int gnx_assoc_cross(gnx_state* h, int64_t n, const int64_t* slots /*NULL: all living*/, int32_t m,
                    const double* Y, double* DtY, int64_t* s1, int64_t* s2, int64_t* stretch,
                    int64_t* stretches, double* kernel_ms);

/* The quadratic forms of a mixed-model scan (csrc/gnx_quad.hip): for the loci l of the mask
 *   q[l] = sum over k < m of ( sum over i < n of M[k][i] * val[l][d_il] )^2,   0 elsewhere,
 * double [L] on the HOST.  val: fp32 [L][3] on the HOST, the value of locus l at dosage 0, 1, 2,
 * as gnx_grm's (the host writes the centring into it; the kernel only selects).  M: fp32 [m][n]
 * on the HOST, 1 <= m <= 8192, columns in the order of the slots: the n x n rotation
 * diag((lambda + delta)^-1/2) U^T of a relationship matrix gives z_l^T (G + delta I)^-1 z_l
 * (geonomics_amd/sim/assoc.py, lmm_*), its top rows alone the communality of every locus.
 * 1 <= n <= 8192; n, slots, locus_mask and the preconditions as gnx_geno_gram.  f32 MFMA over
 * the individuals under gnx_grm's contract (chains of at most 1024 products, added in fp64),
 * so with C_kl = sum_i M_ki z_il and S_kl = sum_i |M_ki z_il|
 *   |dC_kl| <= e_kl := (1.01 * min(n, 1024) * 2^-24 + n * 2^-53) * S_kl,
 *   |dq_l|  <= sum_k (2 |C_kl| e_kl + e_kl^2) + m * 2^-53 * q_l.
 * The squares are added in one fixed order without atomics: a repeated call is bit-equal.
 * Individuals past n of a partial stage, padding rows of M and loci outside the mask contribute
 * exactly 0.  *kernel_ms (may be NULL): the HIP-event time of the call's kernels.  Refused
 * (return 1) before anything is launched: no genomes, ghost records, n or m outside 1..8192, a
 * null pointer, a NaN or infinity in val or M, a slot out of range, n != N with slots NULL.  */
int gnx_assoc_quad(gnx_state* h, int64_t n, const int64_t* slots /*NULL: all living*/,
                   const uint64_t* locus_mask, const float* val, int32_t m, const float* M,
                   double* q, double* kernel_ms);

/* ---- lineages through the recorded pedigree (csrc/gnx_lineage.hip; reference
 *      structs/genome.py:1638-1782 _get_lineage_dicts, structs/species.py:1242-1343) ---------
 * The pedigree is recorded on the host (geonomics_amd/structs/pedigree.py, TreeTables.
 * node_table): node_tab int32 [2 n_rows][2], node 2 row + h -> {row of the parent that gave the
 * gamete (-1: a founder node), path key * 2 + start homologue}; birth_t int32 [n_rows], the
 * nodes table's times (founders +1, offspring of main step t: -t).  The parent homologue at
 * locus l is start ^ bit l of the handle's path `key` (gnx_set_recomb_paths).  A node is KEPT
 * (structs/genome.py:1747, 1720-1729) if (!drop_before_sim or birth_t < 0) and
 * min_ago <= birth_t + t_curr <= max_ago.  All pointers are HOST buffers; the calls return when
 * the outputs are complete.  The table is uploaded, or the device copy of the last call is
 * used again when n_rows and a checksum of the table's last rows are unchanged; it is freed
 * with the handle.  Refused: a handle without genomes, without paths or with ghost records
 * (tiles); a table whose parent rows are not earlier rows or whose keys are not cached paths;
 * sample nodes outside the table; loci outside 0..L-1 - all before anything is launched.   */
/* per (locus, sample node), int32 [n_loci][n_nodes], each may be NULL: root = the founder node
 * reached, first / last = the youngest / oldest kept node (-1: none), n_kept.  locus_lo /
 * locus_hi int32 [n_loci] (both or neither): min and max of `last` over the sample nodes - the
 * sample has coalesced inside the simulation at a locus iff lo == hi >= 0.  The loci are
 * worked off in launches whose outputs stay under gnx_lineage_budget.                       */
int gnx_lineage_trace(gnx_state* h, int64_t n_rows, const int32_t* node_tab,
                      const int32_t* birth_t, int64_t n_nodes, const int32_t* nodes,
                      int32_t n_loci, const int32_t* loci, int32_t t_curr,
                      int32_t drop_before_sim, int32_t min_ago, int32_t max_ago, int32_t* root,
                      int32_t* first, int32_t* last, int32_t* n_kept, int32_t* locus_lo,
                      int32_t* locus_hi);
/* the same walk writing every kept node, youngest first, at chain_nodes[offsets[q] ...], q =
 * locus index * n_nodes + node index; offsets int64 [n_loci * n_nodes + 1] = the exclusive scan
 * of a gnx_lineage_trace's n_kept for the same request (anything else is an error, and never
 * a write outside a chain's own stretch)                                                     */
int gnx_lineage_chains(gnx_state* h, int64_t n_rows, const int32_t* node_tab,
                       const int32_t* birth_t, int64_t n_nodes, const int32_t* nodes,
                       int32_t n_loci, const int32_t* loci, int32_t t_curr,
                       int32_t drop_before_sim, int32_t min_ago, int32_t max_ago,
                       const int64_t* offsets, int32_t* chain_nodes);
/* bytes of output one launch of the two calls above may produce (0: the default, 256 MiB) */
int gnx_lineage_budget(gnx_state* h, int64_t bytes);
/* of the last lineage call: its kernels' HIP-event time (ms), their number, and whether the
 * node table was uploaded (1) or the resident copy used (0); each may be NULL              */
int gnx_lineage_info(gnx_state* h, double* kernel_ms, int64_t* launches, int64_t* uploaded);

/* ---- simplification of the recorded pedigree (csrc/gnx_simplify.hip; reference
 *      structs/species.py:1107-1142 _sort_and_simplify_table_collection, run every
 *      tskit_simp_interval main steps: sim/model.py:756-768) ------------------------------
 * A node is ANCESTRAL at locus l if the lineage at l of some sample node passes through it; the
 * sample is both nodes of every row in sample_rows (the living).  node_loci int32 [2 n_rows]:
 * the number of loci at which the node is ancestral (0: at none; a row both of whose nodes have
 * 0 carries no lineage of the sample and can be dropped).  req_masks uint64 [n_req][W64] (NULL
 * with n_req = 0): the ancestral loci of the nodes in req_nodes as bit masks in the layout of
 * the recombination paths, bits at or above L zero.  node_tab / birth_t as for
 * gnx_lineage_trace, taken through the same resident copy; one launch per birth cohort
 * (youngest first) and, when the masks of all nodes exceed gnx_lineage_budget, per block of
 * mask words.  gnx_lineage_info reports the call.  Refused before anything is launched, beside
 * what gnx_lineage_trace refuses: birth_t ascending somewhere along the rows, a parent row that
 * is not of an earlier birth cohort than its child, sample rows out of range or repeated,
 * requested nodes out of range.                                                            */
int gnx_pedigree_reach(gnx_state* h, int64_t n_rows, const int32_t* node_tab,
                       const int32_t* birth_t, int64_t n_samples, const int32_t* sample_rows,
                       int32_t* node_loci, int64_t n_req, const int32_t* req_nodes,
                       uint64_t* req_masks);
/* drop the resident copy of the node table: the next lineage call uploads its table (after the
 * host has renumbered the rows, the reuse check's row count and checksum mean nothing)      */
int gnx_lineage_forget(gnx_state* h);

/* ---- pairwise coalescence through the recorded pedigree (csrc/gnx_coal.hip; the reference has
 *      no such analysis: what tskit's divergence(mode='branch'), pair_coalescence_counts and
 *      ibd_segments answer) ------------------------------------------------------------------
 * Tables: node_tab, birth_t and the handle's paths as for gnx_lineage_trace, taken with every
 * call through the same resident copy.  anc(v, l) is the parent node of v at locus l,
 * 2 prow + (start ^ bit l of the path); it is undefined for a founder node.  chain(v, l) = v,
 * anc(v, l), ... down to a founder node.  Parent rows are smaller than child rows, so node ids
 * strictly decrease along a chain.
 * MRCA.  For sample nodes a != b, mrca(a, b, l) is the largest node id that lies on both chains,
 * or -1 if there is none (the chains end in different founder nodes).  From their first common
 * node on two chains are equal, so the largest common node is the most recent one; a itself is
 * the MRCA when it lies on b's chain (a living parent and its living offspring both sampled).
 * Age.  ago(v) = birth_t[v >> 1] + t_curr.  A pair COALESCES at l iff m = mrca(a, b, l) >= 0 and
 * ago(m) <= max_ago (max_ago < 0: no limit); T(a, b, l) = ago(m) then.
 * Everything the device returns is an integer function of mrca and ago.  Every output is
 * therefore exact, independent of order (integer atomics are fine), and bit-equal to the
 * restatement (geonomics_amd/sim/coal.py).  All pointers are HOST buffers.
 * Refused (return 1) before anything is launched: what gnx_lineage_trace refuses; fewer than 2
 * or more than 4096 sample nodes; a sample node listed twice; bad edges; *work > max_work; and
 * for gnx_coal_segments loci not strictly ascending, pos decreasing, min_len < 0.  Nothing of the
 * handle changes.  *work = n_pairs n_loci, n_pairs = n_nodes (n_nodes - 1) / 2; max_work <= 0:
 * only *work is written.  gnx_lineage_info reports the call.
 *
 * gnx_coal_times: loci in any order, repeats allowed.  Each output may be NULL and is then not
 * computed:
 *   pair_sum int64 [n][n], pair_cnt int32 [n][n]: the sum of T over the loci at which the pair
 *   coalesces, and their number; symmetric, the diagonal zero;
 *   locus_sum, locus_cnt int64 [n_loci], locus_max int32 [n_loci]: the same over the unordered
 *   pairs per listed locus, and the largest T; locus_max is -1 where no pair coalesces;
 *   thist int64 [n_tedges - 1]: the unordered (pair, locus) cells with tedges[k] <= T <
 *   tedges[k + 1]; tedges int32, 2..65 of them, strictly ascending (thist NULL: n_tedges = 0 and
 *   no edges);
 *   mrca int32 [n_loci][n_pairs], the pairs in row-major upper-triangle order ((0,1), (0,2), ..,
 *   (1,2), ..): the MRCA where the pair coalesces, -1 where it does not.  With mrca the loci are
 *   worked off in launches whose MRCAs stay under gnx_lineage_budget.                          */
int gnx_coal_times(gnx_state* h, int64_t n_rows, const int32_t* node_tab, const int32_t* birth_t,
                   int64_t n_nodes, const int32_t* nodes, int32_t n_loci, const int32_t* loci,
                   int32_t t_curr, int32_t max_ago, int32_t n_tedges, const int32_t* tedges,
                   int64_t max_work, int64_t* work, int64_t* pair_sum, int32_t* pair_cnt,
                   int64_t* locus_sum, int64_t* locus_cnt, int32_t* locus_max, int64_t* thist,
                   int32_t* mrca);
/* gnx_coal_segments: loci strictly ascending; q is a position in that list.  pos int64 [n_loci]
 * is non-decreasing, in an integer unit the caller chooses.  brk uint8 [n_loci] or NULL: when
 * brk[q] is set no segment continues from q - 1 into q (brk[0] is ignored).
 * A SEGMENT of the pair is a maximal stretch s..e of list positions over which the pair
 * coalesces with the same MRCA node and no break lies in s < q <= e.  Its count is e - s + 1,
 * its length pos[e] - pos[s]; it QUALIFIES iff count >= max(1, min_loci) and length >= min_len:
 * the tract of gnx_tracts_*, with "same MRCA within max_ago" in place of "D_l = 0".
 *   cnt int32, len, longest int64 [n][n]: the qualifying segments of the pair, the sum of their
 *   lengths, the largest length; symmetric, the diagonal zero; each may be NULL;
 *   hist int64 [n_edges - 1][2] = {segments, sum of length} and cover int64 [n_loci] (the pairs
 *   with a qualifying segment over list position q) as in gnx_tracts_pairs, over the unordered
 *   node pairs; each may be NULL (hist NULL: n_edges = 0 and no edges).                       */
int gnx_coal_segments(gnx_state* h, int64_t n_rows, const int32_t* node_tab,
                      const int32_t* birth_t, int64_t n_nodes, const int32_t* nodes,
                      int32_t n_loci, const int32_t* loci, const int64_t* pos,
                      const uint8_t* brk /*[n_loci] or NULL*/, int32_t t_curr, int32_t max_ago,
                      int32_t min_loci, int64_t min_len, int32_t n_edges, const int64_t* edges,
                      int64_t max_work, int64_t* work, int32_t* cnt, int64_t* len,
                      int64_t* longest, int64_t* hist, int64_t* cover);

/* ---- introductions (csrc/gnx_transplant.hip) ------------------------------------------ */
/* Species._add_individuals with a Species as the source (structs/species.py:1631-2077):
 * n individuals of src, in the order of src_slots, appended to dst at (x[i], y[i]) with ids
 * first_id + i; age and sex travel, genomes travel bit for bit, e / selected-locus tables /
 * phenotype / fitness are recomputed from dst's rasters and traits.
 * out[4] = first new slot, distinct physical blocks copied, logical blocks linked,
 * collections run in dst.  Returns 2 (dst unchanged) when slots, rows or blocks do not fit.
 * Both handles live on one device, hold no ghosts, have the same L and block geometry and
 * (L > 0) assigned genomes; first_id > dst's largest id; slots are distinct living slots of
 * src; coordinates lie on dst's landscape.  A block that several newcomers share in src is
 * copied once and shared in dst; src is only read.                                        */
int gnx_transplant(gnx_state* dst, gnx_state* src, int64_t n, const int64_t* src_slots,
                   const float* x, const float* y, int64_t first_id, int64_t* out);

/* ---- measurement ------------------------------------------------------------ */
int gnx_profiling(gnx_state* h, int32_t on);
/* accumulated HIP-event time (ms) and launch count of one kernel family,
 * measured on the handle's stream; resets the accumulator                   */
int gnx_kernel_time(gnx_state* h, int32_t kernel, double* ms, int64_t* launches,
                    double* algorithmic_bytes);
/* The box's own streaming rate, for the roofline line ("a measured
 * device-to-device copy"): a hand-written copy kernel, 16 bytes per lane and access,
 * grid-stride, over two buffers of `bytes` bytes each, `reps` launches timed with HIP
 * events on the current device; *gbps = (read + written bytes) / mean launch time.      */
int gnx_measure_copy(int64_t bytes, int32_t reps, double* gbps);

#ifdef __cplusplus
}
#endif
#endif /* GNX_HIP_H */
