"""Model: the driver API kept from the reference (geonomics/sim/model.py:47-1182
and the accessors at :2787-3147).  It builds the Landscape and Community, the
burn-in and main function queues, and runs them; the queue entries call the
device-backed Species methods (geonomics_amd/structs/species.py), which call
libgnxhip.so.

Kept: make_model -> Model.walk(T, mode) / Model.run() / Model.burn(); attributes
t, burn_t, it, T, burn_T, comm, land, its; the queue order _set_t, _set_comm_t,
_set_spp_t, _set_age_stage, _do_movement, _do_pop_dynamics, _set_Nt
(sim/model.py:603-667); ValueError when walking 'main' before burn-in (:1087);
exceptions inside run() are caught per iteration (:938-953).
Fixed: queue lambdas bind their own species; both
params.model.seed.num and params.model.num seed the model.
Statistics (params.model.stats), data sampling / writers (params.model.data) and
change events run from the main queue after the hot path (sim/stats.py,
sim/data.py, ops/change.py).  Out of scope here: plotting.
"""
import copy
import os
import random
import sys
import traceback
import warnings

import numpy as np

from ..structs.landscape import _make_landscape
from ..structs.community import _make_community
from ..structs import genome as _genome
from .stats import _StatsCollector
from .data import (_DataCollector, _get_adhoc_sample, _format_vcf, _format_fasta, _write_csv,
                   _write_file)


import threading as _threading

# per-thread communicator override for the in-process rehearsals of a run over several ranks
_rehearsal = _threading.local()


class Model:
    def __init__(self, name, params, verbose=False, device=None):
        self.params = copy.deepcopy(params)
        m_params = self.params.model
        self.name = 'unnamed_model' if name is None else name
        self._pid = os.getpid()
        self._verbose = verbose
        self.__term_width__ = 80
        self.__tab_len__ = len('\t'.expandtabs())
        if verbose:
            print('\nMAKING MODEL...\n', flush=True)
        # seeds: params.model.seed.num (code) or params.model.num (documented)
        self.seed = None
        if 'seed' in [*m_params] and m_params.seed is not None:
            sd = m_params.seed
            self.seed = sd.num if hasattr(sd, 'keys') else sd
        if self.seed is None and m_params.get('num', None) is not None:
            self.seed = m_params.num
        self._set_seeds()
        self.burn_T = m_params.burn_T
        self.burn_t = -1
        self.T = m_params.T
        self.t = -1
        self.n_its = m_params.its.n_its
        self.its = [*range(self.n_its)][::-1]
        self.it = -1
        if device is None:
            device = int(os.environ.get('LOCAL_RANK', '0'))
        self._device = device
        self._comm = self._make_comm()
        self._rank = 0 if self._comm is None else self._comm.rank
        self.land = self._make_landscape(self._verbose)
        self.comm = self._make_community(self._verbose)
        self._never_been_run = True
        self._data_collector = None
        self._stats_collector = None
        if 'stats' in [*m_params]:
            self._stats_collector = self._make_stats_collector()
        if 'data' in [*m_params]:
            self._data_collector = self._make_data_collector()
        self.reassign_genomes = None
        self.rand_genarch = m_params.its.rand_genarch
        self.rand_landscape = m_params.its.rand_landscape
        self.rand_comm = m_params.its.rand_comm
        self.repeat_burn = m_params.its.repeat_burn
        # snapshots replace the reference's deepcopy(comm); only taken when a
        # later iteration can need them
        self.orig_land = None if self.rand_landscape else self.land
        # a changing landscape is restored from a copy at every new iteration
        self._orig_land_copy = (copy.deepcopy(self.land)
                                if (self.land._changer is not None and not self.rand_landscape)
                                else None)
        self._orig_comm_snap = None
        if not self.rand_comm and self.n_its > 1:
            self._orig_comm_snap = self._snapshot_comm()
        self.burn_fn_queue = None
        self.main_fn_queue = None
        self._lanes_active = False
        self.iteration_log = {}
        self.iteration_times = {}       # it -> wall-clock (start, end) of its main phase

    def __str__(self):
        return ('%s\nModel name: %s\nLayers: %s\nSpecies: %s\nNumber of iterations: %i\n'
                'Number of burn-in timesteps (minimum): %i\nNumber of main timesteps: %i'
                % (str(type(self)), self.name,
                   ', '.join("%i: '%s'" % (i, l.name) for i, l in self.land.items()),
                   ', '.join("%i: '%s'" % (i, s.name) for i, s in self.comm.items()),
                   self.n_its, self.burn_T, self.T))

    __repr__ = __str__

    # -- helpers --------------------------------------------------------------
    def _get_lyr_num(self, lyr_id):
        return self.land._get_lyr_num(lyr_id)

    def _get_spp_num(self, spp_id):
        if isinstance(spp_id, int):
            assert spp_id in self.comm.keys(), (
                'A Species with numeric spp_id %s does not exist.' % str(spp_id))
            return spp_id
        if isinstance(spp_id, str):
            nums = [k for k, spp in self.comm.items() if spp.name == spp_id]
            assert len(nums) == 1, ("Expected to find a single Species with a name "
                                    "matching the name provided (%s). Instead found %i."
                                    % (spp_id, len(nums)))
            return nums[0]
        raise ValueError("The Species identifier must be either a str or an int. "
                         "Instead, a %s was provided." % str(type(spp_id)))

    def _get_trt_num(self, spp, trt_id):
        if isinstance(trt_id, int) or trt_id is None:
            return trt_id
        nums = [k for k, trt in spp.gen_arch.traits.items() if trt.name == trt_id]
        assert len(nums) == 1
        return nums[0]

    def _set_seeds(self):
        """reference sim/model.py:364-366; the device streams are keyed by the
        same seed (one 64-bit Philox key)."""
        self._rng = np.random.RandomState(self.seed if self.seed is not None else None)
        if self.seed is not None:
            random.seed(self.seed)
            np.random.seed(self.seed)
            self._dev_seed = int(self.seed)
        else:
            self._dev_seed = int(np.random.randint(0, 2 ** 31 - 1))

    def _set_it(self):
        # (a lane of a concurrent run has already taken its iteration off the shared list)
        nxt = self.__dict__.pop('_next_it', None)
        self.it = self.its.pop() if nxt is None else nxt

    def _set_t(self):
        self.t += 1

    def _reset_t(self):
        self.t = -1

    def _set_burn_t(self):
        self.burn_t += 1

    def _reset_burn_t(self):
        self.burn_t = -1

    def _set_reassign_genomes(self):
        self.reassign_genomes = bool(np.any([spp.gen_arch is not None
                                             for spp in self.comm.values()]))

    def _make_comm(self):
        """Several GPUs: when the script runs under torch.distributed
        (WORLD_SIZE > 1; `python -m torch.distributed.run --nproc-per-node N script.py`)
        every rank builds the same Model and each Species is tiled over the ranks
        (structs/tiled.py).  Backend: RCCL ("nccl") unless GNX_DIST_BACKEND says
        otherwise (CPU rehearsals use "gloo")."""
        # (rehearsals on a one-GPU box: the ranks are threads of one process, each building its
        # Model with the communicator it was handed - tests/_local_comm.py - instead of a
        # torch.distributed group; RCCL refuses two ranks on one device)
        injected = getattr(_rehearsal, 'comm', None)
        if injected is not None:
            if injected.rank != 0:
                self._verbose = False
            return injected
        if int(os.environ.get('WORLD_SIZE', '1')) <= 1:
            return None
        import torch
        import torch.distributed as dist
        from ..parallel import Comm
        if not dist.is_initialized():
            backend = os.environ.get('GNX_DIST_BACKEND', 'nccl')
            if backend == 'nccl':
                torch.cuda.set_device(self._device)
                dist.init_process_group('nccl', device_id=torch.device('cuda', self._device))
            else:
                dist.init_process_group(backend)
        comm = Comm(dist)
        if self.seed is None:            # one device seed for all ranks
            self._dev_seed = int(comm.allgather_i64(np.array([self._dev_seed]))[0][0])
            self._rng = np.random.RandomState(self._dev_seed)
        # every rank prints nothing but rank 0; files are written by rank 0
        if comm.rank != 0:
            self._verbose = False
        return comm

    def _make_landscape(self, verbose=False):
        return _make_landscape(mod=self, params=self.params, verbose=verbose)

    def _make_community(self, verbose=False):
        comm = _make_community(self.land, self.params, burn=True, verbose=verbose,
                               seed=self._dev_seed, device=self._device, rng=self._rng,
                               comm=self._comm)
        return comm

    def _make_land_change(self):
        """reference sim/model.py:397-398, plus the device mirrors of the changed layers"""
        self.land._make_change(t=self.t, verbose=self._verbose)
        self._sync_changed_layers()

    def _sync_changed_layers(self):
        for lyr_num in sorted(self.land._changed_lyrs):
            for spp in self.comm.values():
                spp._dev.upload_layer(lyr_num, self.land[lyr_num].rast)
        self.land._changed_lyrs.clear()

    def _make_data_collector(self):
        """reference sim/model.py:515-523"""
        dc = _DataCollector(self.name, self.params, rng=self._rng)
        dc.writer = self._rank == 0
        return dc

    def _write_data(self):
        """reference sim/model.py:1185-1186"""
        self._data_collector._write_data(self.comm, self.land, self.it)

    def remove_individuals(self, spp=0, n=None, n_left=None, individs=None):
        """remove n random individuals, all but n_left, or the listed ids
        (reference sim/model.py:3179-3225)"""
        spp = self.comm[self._get_spp_num(spp)]
        spp._remove_individuals(individs=individs, n=n, n_left=n_left,
                                verbose=self._rank == 0)

    def add_individuals(self, n, coords, recip_spp=0, source_spp=None,
                        source_msprime_params=None, individs=None):
        """add Individuals of another Species - of this Model (int or str) or of another
        Model in this process (its Species object) - to `recip_spp` at `coords`: n of them
        (those with the smallest ids) or the listed `individs` (reference
        sim/model.py:3228-3335; structs/species.py:1631-2077).  `coords`: one x,y pair for
        everybody, or n x 2.  An msprime source (`source_msprime_params`) is not part of
        this build."""
        import warnings
        from ..structs.species import Species
        warnings.warn("add_individuals is new: checked, not yet widely used. Please report "
                      "anything that looks wrong.")
        if isinstance(recip_spp, (int, str)):
            recip_spp = self.comm[self._get_spp_num(recip_spp)]
        assert recip_spp.burned, ("Individuals cannot be added to a Species that has not "
                                  "been burned in yet.")
        assert (source_spp is None) != (source_msprime_params is None), (
            "the source population is either a Species ('source_spp') or a set of msprime "
            "arguments ('source_msprime_params'): exactly one of them must be given.")
        if source_spp is not None:
            assert isinstance(source_spp, (Species, int, str)) and \
                not isinstance(source_spp, bool), (
                    "'source_spp' must be a Species object, or the int or str that names a "
                    "Species of this Model.")
            if isinstance(source_spp, (int, str)):
                source_spp = self.comm[self._get_spp_num(source_spp)]
        recip_spp._add_individuals(n=n, coords=coords, land=self.land, source_spp=source_spp,
                                   source_msprime_params=source_msprime_params,
                                   individs=individs, verbose=self._rank == 0)

    def write_tskit_table_collection(self, file_basename, spp=0, sep=','):
        """the spatial pedigree as <basename>_{NODES,EDGES,SITES,MUTATIONS,INDIVIDUALS}.csv
        (reference sim/model.py:3449-3486) and, beside them, tskit's text format
        (<basename>.nodes.txt ..., readable with tskit.load_text)"""
        spp = self.comm[self._get_spp_num(spp)]
        if spp._tt is None:
            raise ValueError("no pedigree was recorded for this Species ('use_tskit' False, "
                             "not yet burned in, or the model is too large)")
        spp._tt.write_csv(file_basename, sep=sep)
        spp._tt.write_text(file_basename)

    def get_tree_sequence(self, spp=0):
        """tskit.TreeSequence of the recorded pedigree (needs tskit on this machine;
        reference sim/model.py get_tree_sequence)"""
        import io
        import tempfile
        try:
            import tskit
        except ImportError:
            raise ImportError('get_tree_sequence needs the tskit package; '
                              'write_tskit_table_collection writes the tables without it')
        spp = self.comm[self._get_spp_num(spp)]
        with tempfile.TemporaryDirectory() as d:
            base = os.path.join(d, 'ts')
            spp._tt.write_text(base)
            args = {k: io.StringIO(open('%s.%s.txt' % (base, k)).read())
                    for k in ('nodes', 'edges', 'sites', 'mutations', 'individuals')}
            return tskit.load_text(sequence_length=spp.gen_arch.L, strict=False, **args)

    def write_gendata(self, filepath, spp=0, n=None, include_fixed_sites=True):
        """VCF / FASTA (by extension) of all or n random individuals
        (reference sim/model.py:3342-3396)"""
        extension = filepath.split('.')[-1].lower()
        assert extension in ['vcf', 'fasta'], ('Must provide valid file extension. Valid '
                                               'extensions include ".vcf" and ".fasta".')
        spp = self.comm[self._get_spp_num(spp)]
        sample = _get_adhoc_sample(spp, n, rng=self._rng)
        gts = spp._get_genotypes(individs=[*sample], as_dict=True)
        if extension == 'vcf':
            text = _format_vcf(sample, gts, spp.gen_arch,
                               include_fixed_sites=include_fixed_sites)
        else:
            text = _format_fasta(sample, gts)
        _write_file(filepath, text)

    def write_geodata(self, filepath, spp=0, n=None):
        """CSV of all or n random individuals (reference sim/model.py:3399-3446;
        shapefile / GeoJSON need geopandas and are not written by this build)"""
        extension = filepath.split('.')[-1].lower()
        assert extension in ['csv', 'shp', 'json'], (
            'Must provide valid file extension. Valid extensions include ".csv", ".shp", '
            'and ".json".')
        if extension != 'csv':
            raise NotImplementedError('shapefile / GeoJSON output needs geopandas')
        spp = self.comm[self._get_spp_num(spp)]
        _write_csv(filepath, _get_adhoc_sample(spp, n, rng=self._rng))

    def _make_stats_collector(self):
        """reference sim/model.py:527-535"""
        sc = _StatsCollector(self.name, self.params)
        sc.writer = self._rank == 0
        return sc

    def calc_stats(self):
        """reference sim/model.py:1190-1191"""
        self._stats_collector._calc_stats(self.comm, self.t, self.it)

    def _snapshot_comm(self):
        return {k: spp._snapshot() for k, spp in self.comm.items()}

    def _restore_comm(self, snap):
        for k, spp in self.comm.items():
            spp._restore(snap[k])
        self.comm.burned = bool(np.all([spp.burned for spp in self.comm.values()]))

    def _reset_community(self, rand_comm=True):
        """reference sim/model.py:457-512"""
        if not rand_comm and self._orig_comm_snap is not None:
            if self._verbose:
                print('Copying the original community for iteration %i...\n\n' % self.it,
                      flush=True)
            self._restore_comm(self._orig_comm_snap)
            if self.rand_genarch:
                for spp in self.comm.values():
                    if spp.gen_arch is not None:
                        spp.gen_arch = _genome._make_genomic_architecture(
                            spp_params=self.params['comm']['species'][spp.name],
                            land=self.land, rng=self._rng)
                        spp._upload_gen_arch()
                        if not self.repeat_burn and spp.burned:
                            spp._set_genomes_and_tables(self.burn_T, self.T)
        else:
            if self._verbose:
                print('Creating new community for iteration %i...\n\n' % self.it,
                      flush=True)
            for spp in self.comm.values():
                spp._dev.close()
            self.comm = self._make_community(self._verbose)

    def _reset(self, rand_landscape=None, rand_comm=None, rand_genarch=None,
               repeat_burn=None):
        """reference sim/model.py:540-593"""
        rand_landscape = self.rand_landscape if rand_landscape is None else rand_landscape
        rand_comm = self.rand_comm if rand_comm is None else rand_comm
        repeat_burn = self.repeat_burn if repeat_burn is None else repeat_burn
        if not self._never_been_run:
            if rand_landscape:
                self.land = self._make_landscape()
            elif self._orig_land_copy is not None:
                self.land = copy.deepcopy(self._orig_land_copy)
                for spp in self.comm.values():
                    spp._land_ref = self.land
                    spp._dev.upload_rasters(self.land._stack())
                    spp._set_K(self.land)
            self._reset_community(rand_comm)
        else:
            self._never_been_run = False
        self._reset_t()
        if self._stats_collector is not None:
            self._stats_collector = self._make_stats_collector()
        if self._data_collector is not None:
            self._data_collector = self._make_data_collector()
        if repeat_burn:
            self._reset_burn_t()
        self.comm._reset_t()
        for spp in self.comm.values():
            spp._reset_t()
        self._set_reassign_genomes()
        # (a Community made anew for this iteration needs a queue bound to ITS Species:
        # the reference's condition - repeat_burn or the first iteration - leaves the old
        # queue in place, whose entries here would call into a closed device)
        if repeat_burn or self.it <= 0 or rand_comm or self.burn_fn_queue is None:
            self.burn_fn_queue = self._make_fn_queue(burn=True)
        self.main_fn_queue = self._make_fn_queue(burn=False)

    # -- function queue (reference sim/model.py:603-667) ----------------------------
    def _make_fn_queue(self, burn=False):
        queue = []
        if burn:
            queue.append(self._set_burn_t)
        else:
            queue.append(self._set_t)
            queue.append(self.comm._set_t)
            for spp in self.comm.values():
                queue.append(spp._set_t)
        for spp in self.comm.values():
            queue.append(spp._set_age_stage)
        for spp in self.comm.values():
            if spp._move:
                queue.append(lambda spp=spp: spp._do_movement(self.land))
        for spp in self.comm.values():
            queue.append(lambda spp=spp: spp._do_pop_dynamics(self.land))
        for spp in self.comm.values():
            queue.append(spp._set_Nt)
        if not burn:
            # change events, then statistics (reference sim/model.py:644-662)
            if self.land._changer is not None:
                queue.append(self._make_land_change)
                for spp in self.comm.values():
                    queue.append(lambda spp=spp: spp._set_K(self.land))
            for spp in self.comm.values():
                if spp._changer is not None:
                    queue.append(lambda spp=spp: spp._make_change(verbose=self._verbose))
            if self._data_collector is not None:
                queue.append(self._write_data)
            if self._stats_collector is not None:
                queue.append(self.calc_stats)
        if burn:
            queue.append(self._check_comm_burned)
        return queue

    def _check_comm_burned(self):
        self.comm._check_burned(burn_T=self.burn_T, params=self.params)

    def _print_timestep_info(self, mode):
        msg = '%s:\tit=%i:\tt=%i\n' % (mode, self.it,
                                       self.burn_t if mode == 'burn' else self.t)
        for spp in self.comm.values():
            Nt = spp.Nt[-1] if spp.Nt else np.nan
            nb = spp.n_births[-1] if spp.n_births else np.nan
            nd = spp.n_deaths[-1] if spp.n_deaths else np.nan
            msg += '\tspecies: %s%sN=%s\t(births=%s\tdeaths=%s)\n' % (
                spp.name, ' ' * (30 - len(spp.name)), Nt, nb, nd)
        print(msg)
        print('\t' + '.' * (self.__term_width__ - self.__tab_len__), flush=True)

    def _do_timestep(self, mode):
        """reference sim/model.py:699-787"""
        queue = self.burn_fn_queue if mode == 'burn' else self.main_fn_queue
        for fn in queue:
            if True not in [spp.extinct for spp in self.comm.values()]:
                fn()
            else:
                break
        if self._verbose:
            self._print_timestep_info(mode)
        if mode == 'main':
            self._simplify_pedigrees()
        if mode == 'burn' and np.all([spp.burned for spp in self.comm.values()]):
            if self.reassign_genomes:
                for spp in self.comm.values():
                    if spp.gen_arch is not None:
                        if self._verbose:
                            print('\nAssigning genomes for species "%s"...\n\n' % spp.name,
                                  flush=True)
                        spp._set_genomes_and_tables(self.burn_T, self.T)
                self.reassign_genomes = False
            self.comm.burned = True
            if self._verbose:
                print('Burn-in complete.\n\n', flush=True)
        extinct = bool(np.any([spp.extinct for spp in self.comm.values()]))
        if extinct and self._verbose:
            print('XXXX     Species %s went extinct. Iteration %i aborting.\n\n' % (
                ' & '.join('"' + spp.name + '"' for spp in self.comm.values()
                           if spp.extinct), self.it), flush=True)
        return extinct

    def _simplify_pedigrees(self):
        """at the end of every tskit_simp_interval-th main step, simplify the recorded pedigree
        of each Species that keeps one (reference sim/model.py:756-768); an interval of None:
        never.  A Species tiled over several GPUs is skipped (structs/tiled.py)."""
        for spp in self.comm.values():
            if spp._tt is None or spp.extinct or getattr(spp, '_comm', None) is not None:
                continue
            interval = getattr(spp.gen_arch, 'tskit_simp_interval', None)
            if isinstance(interval, bool) or not isinstance(interval, (int, np.integer)) \
                    or interval < 1 or self.t == -1 or (self.t + 1) % interval != 0:
                continue
            if self._verbose:
                print("\n\nnow sorting and simplifying tskit tables for Species: '%s'"
                      % spp.name)
                print('\tNUMBER EDGES BEFORE SIMPLIFICATION:', spp._tt._edges_count())
                print('\tNUMBER INDIVIDS BEFORE SIMPLIFICATION:', spp._tt.ids.size)
            spp._sort_and_simplify_table_collection()
            if self._verbose:
                print('\n\tNUMBER EDGES AFTER SIMPLIFICATION: ', spp._tt._edges_count())
                print('\tNUMBER INDIVIDS AFTER SIMPLIFICATION: ', spp._tt.ids.size, '\n',
                      flush=True)

    def _iter_seed(self, it):
        """the host-side random stream of iteration it >= 1 (community / genomic
        architecture / mutation / sampling draws).  The reference draws every iteration from
        one global stream in turn (sim/model.py:364-366), which chains them; here each
        iteration starts its own stream, so iterations can run in any order - and side by
        side (GNX_CONCURRENT_ITS=K) - with the results of a sequential run."""
        return (int(self._dev_seed) * 1000003 + 7919 * int(it) + 12345) % (2 ** 32)

    def _set_next_iteration(self):
        self._set_it()
        if self.it > 0:
            self._rng.seed(self._iter_seed(self.it))
        if self._verbose:
            print('~' * self.__term_width__ + '\n\n')
            print('Setting up iteration %i...\n\n' % self.it, flush=True)
        self._reset(rand_landscape=self.rand_landscape, rand_comm=self.rand_comm,
                    rand_genarch=self.rand_genarch, repeat_burn=self.repeat_burn)

    def _do_next_iteration(self):
        """reference sim/model.py:808-858"""
        self._iteration_burn()
        self._iteration_main()

    def _iteration_burn(self):
        """set the next iteration up and burn it in (when this iteration has a burn-in of
        its own: reference sim/model.py:808-840)"""
        self._set_next_iteration()
        if self.rand_comm or (not self.rand_comm and self.repeat_burn) or self.it == 0:
            if self._verbose:
                print('Running burn-in, iteration %i...\n\n' % self.it, flush=True)
            while not np.all([spp.burned for spp in self.comm.values()]):
                if self._do_timestep(mode='burn'):
                    break
            if not self.rand_comm and not self.repeat_burn and self.n_its > 1:
                self._orig_comm_snap = self._snapshot_comm()

    def _walk_main_on_device(self, T):
        """T main timesteps without the function queue, when nothing in it needs the host
        between two steps (one Species that neither mutates nor records a pedigree; no change
        events, no data or statistics collection, no per-step printing): the queue's
        _set_t / _set_age_stage / _do_movement / _do_pop_dynamics / _set_Nt entries
        (reference sim/model.py:603-667) T times in one call into the library.  Returns the
        number of timesteps taken, or None when the queue has to be walked."""
        if os.environ.get('GNX_MODEL_WALK', '1') == '0' or self._verbose or T < 2:
            return None
        # (lanes of a concurrent run share the process: while one host thread captures a step's
        # graph, HIP refuses the other threads' plain hipMemcpy / hipMemset calls)
        if getattr(self, '_is_lane', False) and self._lanes_active:
            return None
        if len(self.comm) != 1 or self.land._changer is not None:
            return None
        if self._data_collector is not None or self._stats_collector is not None:
            return None
        spp = self.comm[0]
        if not (self.comm.burned and spp._move and spp._can_walk_on_device()):
            return None
        done = spp._walk_on_device(T)
        self.t += done
        self.comm.t += done
        return done

    def _iteration_main(self):
        """the T main timesteps of the iteration (reference sim/model.py:841-858)"""
        if self._verbose:
            print('Running main model, iteration %i...\n\n' % self.it, flush=True)
        if np.any([spp.extinct for spp in self.comm.values()]):
            if self._verbose:
                print("WARNING: At least one Species went extinct during the burn-in. "
                      "Cannot run main phase for iteration %i.\n\n" % self.it, flush=True)
            return
        import time
        t0 = time.perf_counter()
        done = self._walk_main_on_device(self.T) or 0
        for _ in range(self.T - done):
            if np.any([spp.extinct for spp in self.comm.values()]) or self._do_timestep('main'):
                break
        self.iteration_times[self.it] = (t0, time.perf_counter())
        self._log_iteration()

    def _log_iteration(self):
        """per-iteration record (shared by the lanes of a concurrent run): population
        sizes, births and deaths of every Species over the whole iteration"""
        self.iteration_log[self.it] = {
            spp.name: {'Nt': list(spp.Nt), 'n_births': list(spp.n_births),
                       'n_deaths': list(spp.n_deaths), 'extinct': bool(spp.extinct)}
            for spp in self.comm.values()}
        hook = getattr(self, '_on_iteration_end', None)
        if hook is not None:
            hook(self)

    # -- iterations side by side on one GPU ---------------------------------------------
    # The reference walks its n_its iterations one after another and notes that they could
    # be farmed out (sim/model.py:866-953, TODO at :924-925).  A model of 10^5 individuals
    # fills a tenth of an MI355X: K iterations run as K "lanes" - clones of this Model, each
    # with its own Community (device handle, three HIP streams of its own), landscape
    # copy where the landscape changes, collectors and random stream - on K host threads;
    # every call into libgnxhip.so releases the interpreter lock, so while one lane waits for
    # a count its siblings enqueue, and the lanes' kernels share the chip.
    def _concurrency(self):
        """lanes of run(): GNX_CONCURRENT_ITS, else 1.  An experiment kept behind the environment,
        not part of run()'s signature (which is the reference's): on ROCm 7.2 kernels of different
        handles barely overlap and the lanes' runtime calls contend - measured 0.4-1.1 x the
        sequential rate, tools/its_bench.py, DESIGN 4.4."""
        k = max(1, min(int(os.environ.get('GNX_CONCURRENT_ITS', '1')), len(self.its)))
        if self._comm is not None or self._device != 0:
            k = 1           # tiles: one Species already spans the GPUs
        return k

    def _spawn_lane(self, template_comm, share_comm=False):
        lane = copy.copy(self)
        lane._is_lane = True
        lane._verbose = False
        lane._never_been_run = self._never_been_run if share_comm else False
        if share_comm:
            return lane           # the first iteration runs on the Community of make_model
        # a random stream of its own (seeded per iteration, _set_next_iteration); everything
        # the lane builds draws from it
        lane._rng = np.random.RandomState(0)
        if self._orig_land_copy is not None:
            lane.land = copy.deepcopy(self._orig_land_copy)
        if self.rand_comm:
            lane.comm = {}        # _reset_community makes the iteration's Community
        else:
            # a Community of its own to restore the snapshot into; the genomic architecture
            # persists across iterations (unless rand_genarch), so it is the template's
            lane.comm = lane._make_community(False)
            for k, spp in lane.comm.items():
                src = template_comm[k]
                if src.gen_arch is not None:
                    spp.gen_arch = copy.deepcopy(src.gen_arch)
                    spp._upload_gen_arch()
        return lane

    def _lane_loop(self, first_main_only=False):
        """what run() does, on this lane, until the shared list of iterations is empty"""
        first = first_main_only
        while first or self.__dict__.get('_next_it') is not None or len(self.its) > 0:
            try:
                if first:
                    first = False
                    self._iteration_main()
                else:
                    if self.__dict__.get('_next_it') is None:    # (else: handed one by _run_concurrent)
                        try:
                            self._next_it = self.its.pop()
                        except IndexError:          # a sibling took the last iteration
                            break
                    self._iteration_burn()
                    self._iteration_main()
            except Exception as e:
                msg = ('XXXX\tAn error occurred during iteration %i, timestep %i.\n'
                       % (self.it, self.t if getattr(self.comm, 'burned', False)
                          else self.burn_t))
                print(msg)
                print('Error message:\n\t%s\n\n' % e)
                traceback.print_exc(file=sys.stdout)

    def _run_concurrent(self, k):
        import threading
        last_it = max(self.its)
        lanes = [self._spawn_lane(self.comm, share_comm=True)]
        # the burned-in Community every later iteration starts from is a product of the
        # first iteration's burn-in: that part runs before the siblings exist
        first_main_only = False
        if 0 in self.its and not self.rand_comm and not self.repeat_burn:
            lanes[0]._iteration_burn()
            self._orig_comm_snap = lanes[0]._orig_comm_snap
            self._never_been_run = False
            first_main_only = True
        elif self.its and self.its[-1] == 0:
            # iteration 0 is the one that is not reseeded: it belongs to the lane that carries the
            # model's own random stream and original Community, whichever thread runs first
            lanes[0]._next_it = self.its.pop()
        for _ in range(k - 1):
            lanes.append(self._spawn_lane(lanes[0].comm))
        for lane in lanes:
            lane._lanes_active = True
        threads = [threading.Thread(target=lane._lane_loop,
                                    args=(first_main_only and n == 0,))
                   for n, lane in enumerate(lanes)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        # the model is left as the sequential run leaves it: in the state of the last iteration
        keep = [lane for lane in lanes if lane.it == last_it]
        keep = keep[0] if keep else lanes[0]
        for lane in lanes:
            if lane is not keep:
                for spp in (lane.comm.values() if lane.comm else []):
                    if not any(spp is s for s in keep.comm.values()):
                        spp._dev.close()
        keep._lanes_active = False
        for name in ('comm', 'land', 't', 'burn_t', 'it', '_rng', '_stats_collector',
                     '_data_collector', 'reassign_genomes', '_orig_comm_snap',
                     '_orig_land_copy', 'orig_land'):
            setattr(self, name, getattr(keep, name))
        self._never_been_run = False
        self.burn_fn_queue = self._make_fn_queue(burn=True)
        self.main_fn_queue = self._make_fn_queue(burn=False)

    # -- public API ---------------------------------------------------------------------
    def run(self, verbose=False):
        """Run all iterations: burn-in then T main timesteps each
        (reference sim/model.py:866-961)."""
        self._verbose = verbose and self._rank == 0
        if self._verbose:
            print('\n\n' + '#' * self.__term_width__ + '\n\n')
            print('Running model "%s"...\n\n' % self.name, flush=True)
        k = self._concurrency()
        if k > 1:
            self._run_concurrent(k)
        while len(self.its) > 0:
            try:
                self._do_next_iteration()
            except Exception as e:
                msg = ('XXXX\tAn error occurred during iteration %i, timestep %i.\n'
                       % (self.it, self.t if self.comm.burned else self.burn_t))
                print(msg)
                print('Error message:\n\t%s\n\n' % e)
                traceback.print_exc(file=sys.stdout)
        if self._verbose:
            print('\n\nModel "%s" is complete.\n' % self.name, flush=True)
        self._verbose = False

    def walk(self, T=1, mode='main', verbose=True, animate=False):
        """Run T timesteps in 'burn' or 'main' mode
        (reference sim/model.py:966-1161)."""
        assert isinstance(T, (int, float)), "'T' must be a numeric data type."
        T = int(T)
        if mode not in ('burn', 'main'):
            raise ValueError("mode must be 'burn' or 'main'")
        if mode == 'main' and not self.comm.burned:
            raise ValueError("The Model.walk method cannot be run in 'main' mode if the "
                             "Model's Community has not yet been burned in (i.e. if "
                             "Model.comm.burned is False).")
        if animate not in (False, None):
            raise NotImplementedError('plotting is outside the GPU hot path (SURVEY 2)')
        old_verbose = self._verbose
        self._verbose = verbose and self._rank == 0
        if self._verbose:
            print('\n')
        if mode == 'main' and self.main_fn_queue is not None:
            T -= self._walk_main_on_device(T) or 0
            if np.any([spp.extinct for spp in self.comm.values()]):
                T = 0
        for _ in range(T):
            if mode == 'burn' and self.comm.burned:
                break
            if self.burn_fn_queue is None:
                if self._verbose:
                    print('No mod.burn_fn_queue was found. Running mod.reset()...\n\n',
                          flush=True)
                self._reset()
            if self._do_timestep(mode=mode):
                break
        self._verbose = old_verbose

    def burn(self):
        """reference sim/model.py:1166-1181"""
        if self.comm.burned:
            print('\nModel has already been burned in.\n')
        else:
            while not self.comm.burned:
                self.walk(10, 'burn')
                if np.any([spp.extinct for spp in self.comm.values()]):
                    break
            print('\nModel has now been burned in.\n')

    # -- accessors (reference sim/model.py:2787-3147): rows sorted by individual id -----
    def get_coords(self, spp=0, individs=None):
        spp = self.comm[self._get_spp_num(spp)]
        return spp._get_coords(individs=None if individs is None else np.sort(individs))

    def get_x(self, spp=0, individs=None):
        spp = self.comm[self._get_spp_num(spp)]
        return spp._get_x(individs=None if individs is None else np.sort(individs))

    def get_y(self, spp=0, individs=None):
        spp = self.comm[self._get_spp_num(spp)]
        return spp._get_y(individs=None if individs is None else np.sort(individs))

    def get_cells(self, spp=0, individs=None):
        spp = self.comm[self._get_spp_num(spp)]
        return spp._get_cells(individs=None if individs is None else np.sort(individs))

    def get_random_individs(self, n, spp=0):
        spp = self.comm[self._get_spp_num(spp)]
        ids = np.array([*spp])
        return self._rng.choice(ids, n, replace=False)

    def get_e(self, spp=0, lyr_num=None, individs=None):
        spp = self.comm[self._get_spp_num(spp)]
        return spp._get_e(lyr_num=lyr_num,
                          individs=None if individs is None else np.sort(individs))

    def get_z(self, spp=0, trt=None, individs=None):
        spp = self.comm[self._get_spp_num(spp)]
        trt = self._get_trt_num(spp, trt)
        return spp._get_z(trait_num=trt,
                          individs=None if individs is None else np.sort(individs))

    def get_fitness(self, spp=0, trt=None, individs=None):
        """overall fitness, or that of one trait (reference sim/model.py get_fitness)"""
        spp = self.comm[self._get_spp_num(spp)]
        if trt is None:
            return spp._get_fit(individs=None if individs is None else np.sort(individs))
        w = spp._calc_fitness(trait_num=self._get_trt_num(spp, trt))
        if individs is None:
            return w
        ids = np.array([*spp])
        return w[np.searchsorted(ids, np.sort(individs))]

    def get_genotypes(self, spp=0, loci=None, individs=None, biallelic=False):
        spp = self.comm[self._get_spp_num(spp)]
        return spp._get_genotypes(loci=loci, individs=individs, biallelic=biallelic)

    def calc_genetic_PCA(self, n_pcs=3, spp=0, individs=None, loci=None, method='auto',
                         n_iter=8, oversample=10, seed=0):
        """genetic PCA of the mean genotypes (reference Model.plot_genetic_PCA,
        sim/model.py:2031-2041, without the plot) computed on the device:
        -> (ids ascending, scores [n][n_pcs], explained_variance_ratio [n_pcs]).
        The products run on torch buffers: initialise torch's device (torch.cuda.init())
        before the model is made, or torch may not see the GPU the library holds."""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_genetic_PCA(n_pcs=n_pcs, individs=individs, loci=loci, method=method,
                                     n_iter=n_iter, oversample=oversample, seed=seed)

    def get_genetic_distances(self, spp=0, individs=None, loci=None):
        """Euclidean distances between mean genotypes (reference demos/_IBD_IBE.py calc_dists,
        dist_type='gen', biallelic=False) computed on the device: -> (ids, dist [n][n])"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_genetic_distances(individs=individs, loci=loci)

    def run_gea(self, method='cca', spp=0, trt=0, plot=True, plot_sd=True, scale=3, sd=3,
                individs=None, loci=None, gea_df=False):
        """genotype-environment association (reference sim/model.py:2717-2780): for
        method 'cca', the only one, the canonical correlation analysis genotype ~ env + lat +
        long of Species._run_cca, computed from cross-products taken on the device.
        -> dict(ind_df [n][3], loci_df [n_loci][3], var_df [3][3], trait_loci, ids), numpy
        arrays where the reference has DataFrames; rows of ind_df in ascending-id order (ids).
        individs and loci (extensions) restrict the analysis; more than 8192 loci need loci.
        gea_df=True adds the reference's 'gea_df' table ([n][n_loci + 3]: mean genotypes, env,
        lat, long) - the one thing here that downloads N x L genotypes to the host.
        This build does not plot: a truthy plot warns and the results are returned all the
        same; plot_sd, scale and sd only ever shaped the reference's plot.  Initialise torch's
        device (torch.cuda.init()) before the model is made, as for calc_genetic_PCA."""
        if not isinstance(method, str) or method.lower() != 'cca':
            raise ValueError('Invalid GEA method. Valid methods include: cca')
        spp = self.comm[self._get_spp_num(spp)]
        trt_num = self._get_trt_num(spp, trt)
        results = spp._run_cca(trt_num=trt_num, individs=individs, loci=loci)
        if gea_df:
            gts = spp._get_genotypes(loci=None if loci is None else np.unique(loci),
                                     individs=individs, biallelic=False)
            ids = None if individs is None else np.sort(individs)
            lyr = spp.gen_arch.traits[trt_num].lyr_num
            results['gea_df'] = np.column_stack([gts, spp._get_e(lyr_num=lyr, individs=ids),
                                                 spp._get_coords(individs=ids)])
        if plot:
            warnings.warn('run_gea: this build does not plot (plotting is outside the GPU hot '
                          'path); pass plot=False.  The results are returned.', stacklevel=2)
        return results

    def run_gwas(self, trt=0, spp=0, y=None, covars=(), n_pcs=0, individs=None, n=None,
                 loci=None, min_maf=0.01, calibrate=False):
        """genome-wide association scan (an extension: the reference has no such analysis):
        for every locus the regression of the response - the phenotype z of Trait trt, or y [n]
        in ascending-id order - on the dosage, given the covariates and an intercept, over the
        whole population by default, computed on the device in fp64 (gnx_assoc_cross; the
        statistics are sim/assoc.py's).  covars: any of 'env' (the layers the Traits are tied
        to), ('env', lyr), 'x', 'y', or an array [n][c] in ascending-id order; n_pcs > 0 appends
        the first genetic PCs (calc_genetic_PCA, with its limits).  individs, or a random sample
        of n, restrict the rows; loci selects rows of the result after the full scan.  Loci that
        are monomorphic, below min_maf or collinear with the covariates are not tested (NaN).
        calibrate: p from t^2 / gif against chi-square with 1 df.  At most 32 covariates and
        responses together.
        -> dict: loci, beta, se, t, p, q [n_loci][r], maf, tested, gif [r], df, ids, trait_loci,
        pcs [n][n_pcs], kernel_ms"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._run_gwas(trt_num=self._get_trt_num(spp, trt), y=y, covars=covars,
                             n_pcs=n_pcs, individs=self._test_sample(spp, individs, n),
                             loci=loci, min_maf=min_maf, calibrate=calibrate)

    def run_lfmm(self, K, spp=0, env_lyrs=None, lam=1e-5, individs=None, n=None, loci=None,
                 min_maf=0.01, calibrate=True):
        """genotype-environment association scan with K latent factors (LFMM2, Caye et al.
        2019; an extension: the reference has no such analysis): for every locus the regression
        of the dosage on each environmental layer (env_lyrs; default: the layers the Traits are
        tied to, or all) given the other layers and the latent factors of the ridge estimate with
        penalty lam, computed on the device in fp64.  K = 0 is the plain linear model.  At most
        8192 individuals (the factors come from the n x n Gram matrix): individs, or a random
        sample of n, restrict the rows; loci selects rows of the result after the full scan.
        calibrate: p from t^2 / gif against chi-square with 1 df (LFMM's usual calibration).
        -> dict: loci, beta, se, t, p, q [n_loci][layers], maf, tested, gif [layers], df, ids,
        trait_loci (per layer), U [n][K], kernel_ms"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._run_lfmm(K, env_lyrs=env_lyrs, lam=lam,
                             individs=self._test_sample(spp, individs, n), loci=loci,
                             min_maf=min_maf, calibrate=calibrate)

    def run_logistic_gea(self, spp=0, env_lyrs=None, env=None, covars=(), n_pcs=0, individs=None,
                         n=None, loci=None, min_maf=0.01, calibrate=False, tol=1e-8, max_iter=25):
        """logistic genotype-environment association scan (Sambada: Joost et al. 2007, Stucki et
        al. 2017; an extension: the reference has no such analysis): for every locus the binomial
        model dosage ~ Binomial(2, mu), logit mu = intercept + covariates + environment, so that
        an effect is a log-odds of the allele per unit of environment and the fitted frequency
        stays inside 0..1.  The tested columns are the layers env_lyrs (default: the layers the
        Traits are tied to, or all) or a table env [n][r] in ascending-id order; they are tested
        together by the likelihood ratio (the G score, on r degrees of freedom) and each by Wald.
        covars and n_pcs as run_gwas; at most 7 columns beside the intercept, and none may be
        constant or a combination of the others.  The genomes are read once on the device
        (gnx_assoc_cross: X^T D in fp64); every Newton step of the fits that have not converged
        is one device sweep over the design (gnx_glm_sweep), the 2 x 2 .. 8 x 8 solves run on the
        host.  individs, or a random sample of n, restrict the rows; loci selects rows of the
        result after the full scan.  Loci that are monomorphic or below min_maf are not fitted
        (NaN); a locus that has not converged after max_iter steps (separation: the allele is
        absent on one side of a threshold) is reported with converged False, not raised.
        calibrate: p from lrt / gif
        -> dict: loci, beta, se, z, p_wald [n_loci][r], lrt, p, q, maf, tested, converged, n_iter
        [n_loci], gif, df, ids, trait_loci (per layer), kernel_ms, n_sweeps, seconds"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._run_logistic_gea(env_lyrs=env_lyrs, env=env, covars=covars, n_pcs=n_pcs,
                                     individs=self._test_sample(spp, individs, n), loci=loci,
                                     min_maf=min_maf, calibrate=calibrate, tol=tol,
                                     max_iter=max_iter)

    def calc_clines(self, spp=0, axis='x', covars=(), individs=None, n=None, loci=None,
                    min_maf=0.01, sigma=None, tol=1e-8, max_iter=25):
        """the sigmoid cline of every locus along a transect (an extension: the reference has no
        such analysis): p(x) = 1 / (1 + exp(-4 (x - c) / w)) fitted by maximum likelihood as the
        binomial model of run_logistic_gea with the axis as its one tested column, centre
        c = -b0 / b1 and width w = 4 / |b1| with delta-method standard errors.  axis: 'x', 'y',
        ('env', lyr), an angle in degrees (the coordinates projected on that direction), or
        values [n] in ascending-id order; covars as run_gwas (centred: the cline at their means).
        Concordant centres and narrow widths mark the loci under selection along a gradient or
        across a secondary contact (add_individuals, calc_local_ancestry); with the dispersal
        distance sigma (find_kin estimates it) a width becomes s_hat = 8 sigma^2 / w^2.
        individs, n, loci, min_maf, tol, max_iter as run_logistic_gea
        -> dict: loci, centre, width, se_centre, se_width, beta [n_loci][2 + c], delta_p,
        in_range, slope_sign, lrt, p, q, maf, tested, converged [n_loci], axis_range, ids,
        trait_loci, concordance (the median and MAD of centre and width over the loci that are
        tested, converged, in range and have q <= 0.05), kernel_ms, n_sweeps, s_hat (with sigma)"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_clines(axis=axis, covars=covars,
                                individs=self._test_sample(spp, individs, n), loci=loci,
                                min_maf=min_maf, sigma=sigma, tol=tol, max_iter=max_iter)

    def calc_grm(self, spp=0, individs=None, n=None, loci=None, kind='additive', method='gcta',
                 alpha=-1.0, min_maf=0.01, weights=None):
        """the standardised genomic relationship matrix of at most 8192 individuals (an
        extension: the reference has no such analysis), summed on the device from the packed
        genomes (gnx_grm: f32 matrix cores, fp64 sums): G_ij = sum_l v_l(d_il) v_l(d_jl), every
        locus centred by the sample's allele frequency p and scaled.  kind 'additive' with method
        'gcta' ((d - 2p) / sqrt(2pq m), Yang et al. 2011), 'vanraden' ((d - 2p) / sqrt(sum 2pq))
        or 'alpha' ((d - 2p) (2pq)^(alpha/2), normalised; Speed et al. 2012), or kind 'dominance'
        (Zhu et al. 2015).  Loci monomorphic in the sample or below min_maf are left out;
        weights [L] multiplies each locus' values (LD-weighted matrices).  individs, or a random
        sample of n, and loci restrict the analysis
        -> dict: G [n][n] float64 (symmetric; mean diagonal about 1), ids, loci_used, n_loci, p,
        kernel_ms, kind, method"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_grm(individs=self._test_sample(spp, individs, n), loci=loci, kind=kind,
                             method=method, alpha=alpha, min_maf=min_maf, weights=weights)

    def calc_heritability(self, trt=0, spp=0, y=None, covars=(), n_pcs=0, individs=None, n=None,
                          loci=None, method='gcta', alpha=-1.0, min_maf=0.01, grm=None):
        """the SNP heritability of a response among at most 8192 individuals (an extension: the
        reference has no such analysis): the mixed model y = X b + g + e with g ~ N(0, Vg G), G
        the additive relationship matrix of calc_grm, fitted by restricted maximum likelihood in
        the eigenbasis of G.  The response is the phenotype z of Trait trt or y [n] in
        ascending-id order.  A Trait's z carries no environmental deviation in Geonomics (it is a
        function of the genotype alone), so its h2 measures how much of z the additive matrix
        captures and approaches 1; give y - fitness, or z plus noise - for a response with
        environmental variance.  covars and n_pcs as run_gwas; an intercept is always fitted.
        grm takes a previous calc_grm result (of the same individuals), so that several
        responses share one matrix and its eigendecomposition
        -> dict: h2, se_h2, Vg, Ve, beta, logL, logL0, lrt_p, delta, at_boundary, he_h2 (the
        Haseman-Elston estimate, a non-iterative check), ids, n_loci, seconds"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_heritability(trt_num=self._get_trt_num(spp, trt), y=y, covars=covars,
                                      n_pcs=n_pcs, individs=self._test_sample(spp, individs, n),
                                      loci=loci, method=method, alpha=alpha, min_maf=min_maf,
                                      grm=grm)

    def run_lmm(self, trt=0, spp=0, y=None, covars=(), n_pcs=0, individs=None, n=None, loci=None,
                grm=None, grm_loci=None, method='gcta', alpha=-1.0, min_maf=0.01, delta=None,
                calibrate=False, collinear_tol=1e-8):
        """mixed-model genome-wide association scan among at most 8192 individuals (an
        extension: the reference has no such analysis): run_gwas' regression with a random effect
        u ~ N(0, Vg G) against population structure and relatedness, y = X b + g beta + u + e, G
        the additive relationship matrix of calc_grm over the loci grm_loci (all by default;
        leave a region out by hand - there is no automatic leave-one-chromosome-out).  The ratio
        delta = Ve / Vg is calc_heritability's REML estimate of the model without a locus, or
        the given delta, and stays fixed over the scan (EMMAX / P3D / FaST-LMM with a fixed
        delta; it is not refitted per locus as exact GEMMA does); the per-locus quadratic forms
        g^T (G + delta I)^-1 g run on the matrix cores (gnx_assoc_quad), the cross-products in
        fp64 (gnx_assoc_cross).  The response is the phenotype z of Trait trt or one y [n] in
        ascending-id order (several responses: one call each, with grm= shared).  covars, n_pcs,
        individs, n, loci, min_maf, calibrate as run_gwas; grm, method, alpha as
        calc_heritability.  A locus whose whitened dosage keeps no more than collinear_tol of
        its squared length beside the covariates is not tested
        -> dict: loci, beta, se, t, p, q [n_loci][1], maf, tested, gif [1], df, ids, trait_loci,
        kernel_ms, delta, h2, Vg, Ve, at_boundary, n_loci_grm, seconds (grm, eigh, reml, quad,
        cross)"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._run_lmm(trt_num=self._get_trt_num(spp, trt), y=y, covars=covars, n_pcs=n_pcs,
                            individs=self._test_sample(spp, individs, n), loci=loci, grm=grm,
                            grm_loci=grm_loci, method=method, alpha=alpha, min_maf=min_maf,
                            delta=delta, calibrate=calibrate, collinear_tol=collinear_tol)

    def predict_breeding_values(self, trt=0, spp=0, y=None, covars=(), n_pcs=0, train=None,
                                individs=None, n=None, loci=None, method='gcta', alpha=-1.0,
                                min_maf=0.01, grm=None):
        """genomic BLUP of the breeding values of at most 8192 individuals (an extension: the
        reference has no such analysis): the model of calc_heritability is fitted on the
        individuals of train (ids; default: everybody) and predicts g_hat for every individual
        of the sample, the untrained ones from their relationships with the trained; y of the
        untrained is not read
        -> dict: g_hat, y_hat [n], ids, train, beta, delta, h2, Vg, Ve, and for a Trait response
        accuracy: the correlation of g_hat with the Trait's true z over the individuals that
        were not trained on (NaN when there are none)"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._predict_breeding_values(
            trt_num=self._get_trt_num(spp, trt), y=y, covars=covars, n_pcs=n_pcs, train=train,
            individs=self._test_sample(spp, individs, n), loci=loci, method=method, alpha=alpha,
            min_maf=min_maf, grm=grm)

    def _test_sample(self, spp, individs, n):
        """the ids a Mantel / MMRR call analyses: individs, or a random n of the living drawn
        as write_gendata draws its sample, or everybody"""
        if n is None:
            return individs
        if individs is not None:
            raise ValueError('give individs or n, not both')
        if isinstance(n, bool) or int(n) != n or n < 1:
            raise ValueError('n: a positive number of individuals (got %r)' % (n,))
        return np.array([*_get_adhoc_sample(spp, int(n), rng=self._rng)], dtype=np.int64)

    def run_mmrr(self, spp=0, predictors=('geo', 'env'), env_lyrs=None, trts=None,
                 individs=None, n=None, loci=None, nperm=999, seed=None):
        """multiple matrix regression with randomization (reference
        data/IBD_IBE_demo/MMRR.py, the last step of demos/_IBD_IBE.py): the genetic distances
        between the individuals (get_genetic_distances) regressed on the distances of the
        predictors - 'geo' (x, y), 'env' (the layers env_lyrs; default: the layers the Traits
        are tied to, or all), 'phn' (the Traits trts; default: all), 'cost' (least-cost
        distances as calc_cost_distances, or ('cost', dict(lyr=, kind=, barrier=, cost=, name=));
        the key is the name, default 'cost') and 'circuit' (resistance distances as
        calc_resistance_distances, or ('circuit', dict(...)) with the options of 'cost' and tol=,
        max_iter=; default name 'circuit') - with nperm row-and-column
        permutations of the genetic matrix, computed on the device.  individs, or a random
        sample of n, and loci restrict the analysis; at most 8192 individuals.  seed: the
        permutations of np.random.seed(seed) followed by the reference's shuffles (default: the
        model's own generator).
        -> the reference's OrderedDict: 'R^2', 'Intercept', the predictors, '<name>(t)',
        '<name>(p)', 'F-statistic', 'F p-value'"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._run_mmrr(predictors=predictors, env_lyrs=env_lyrs, trts=trts,
                             individs=self._test_sample(spp, individs, n), loci=loci,
                             nperm=nperm, seed=seed)

    def run_mantel(self, x='geo', given=None, spp=0, env_lyrs=None, trts=None, individs=None,
                   n=None, loci=None, nperm=999, seed=None):
        """Mantel test of the genetic distances against the distances of predictor x ('geo',
        'env', 'phn', 'cost' or 'circuit', as run_mmrr), or the partial test given another predictor (reference
        data/IBD_IBE_demo/run_mantel.R: vegan's mantel.partial(gen, env, geo), the genetic
        matrix permuted), computed on the device.
        -> dict(r, p = (1 + #{r_perm >= r}) / (nperm + 1), nperm, perm_r [nperm])"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._run_mantel(x=x, given=given, env_lyrs=env_lyrs, trts=trts,
                               individs=self._test_sample(spp, individs, n), loci=loci,
                               nperm=nperm, seed=seed)

    def calc_cost_distances(self, spp=0, lyr=None, kind='conductance', barrier=None, cost=None,
                            individs=None, n=None):
        """least-cost distances between the living individuals (an extension: isolation by
        resistance; sim/cost.py states the graph): the cost of the cheapest path over the
        landscape's cells, 8 neighbours each, a step between cells u, v costing
        0.5 (R[u] + R[v]) times its length in units of the landscape's res, solved on the device.
        R comes from Layer lyr (number or name; default: the Layer of the Species' move_surf):
        kind='conductance': R = 1 / value, cells with value <= barrier (default 0) impassable;
        kind='resistance': R = value, cells with value >= barrier impassable when barrier is
        given; or cost=: an explicit [H][W] raster of R (inf / nan: impassable).  individs, or a
        random sample of n, as run_mmrr; at most 8192 individuals.  An individual stands on the
        cell get_cells reports; two on one cell are at cost 0; inf: no path
        -> dict(ids, cells [n][2], dist float64 [n][n])"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_cost_distances(lyr=lyr, kind=kind, barrier=barrier, cost=cost,
                                        individs=self._test_sample(spp, individs, n))

    def calc_cost_surface(self, x, y, spp=0, lyr=None, kind='conductance', barrier=None,
                          cost=None):
        """the accumulated-cost raster of k points (x, y: scalars or arrays in landscape
        coordinates, floored to cells as get_cells does) over the resistance raster that
        calc_cost_distances describes -> float64 [k][H][W] (inf: not reachable)"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_cost_surface(x, y, lyr=lyr, kind=kind, barrier=barrier, cost=cost)

    def calc_resistance_distances(self, spp=0, lyr=None, kind='conductance', barrier=None,
                                  cost=None, individs=None, n=None, tol=None, max_iter=None):
        """circuit-theory resistance distances between the living individuals (an extension:
        isolation by resistance in McRae's sense; sim/circuit.py states the definition): the
        effective resistance between the individuals' cells when the raster is read as a
        resistor network - the graph, R and lyr / kind / barrier / cost of calc_cost_distances,
        an edge between cells u, v being a resistor of 0.5 (R[u] + R[v]) times its length - so
        that every additional route lowers the distance.  One linear system per distinct cell,
        solved on the device by conjugate gradients to the relative residual tol (default
        1e-10) within max_iter iterations (default: twice the cells of the largest connected
        component).  individs, or a random sample of n, as run_mmrr; at most 8192 individuals.
        Two on one cell are at 0; inf: different components, or an impassable cell
        -> dict(ids, cells [n][2], dist float64 [n][n], info: the solver's kernel_ms, launches,
        iterations, restarts, worst_residual)"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_resistance_distances(lyr=lyr, kind=kind, barrier=barrier, cost=cost,
                                              individs=self._test_sample(spp, individs, n),
                                              tol=tol, max_iter=max_iter)

    def calc_current_map(self, x=None, y=None, spp=0, individs=None, n=None, lyr=None,
                         kind='conductance', barrier=None, cost=None, tol=None, max_iter=None):
        """the cumulative current map of circuit theory (corridors and pinch points): one
        ampere is sent between every unordered pair of the distinct cells of the points (x, y)
        - or of the individuals individs, or of a random sample of n, or of everyone - over the
        resistor network calc_resistance_distances describes, and the currents through every
        cell are added up (Circuitscape's node current: the two ends of a pair carry 1).  At
        most 128 distinct cells per call: the work is pairs x cells x 8 edges.  Pairs in
        different components or with an impassable cell are skipped and counted
        -> dict(current float64 [H][W] (0 on impassable cells), cells (y * W + x), n_pairs,
        n_skipped)"""
        spp = self.comm[self._get_spp_num(spp)]
        if x is None and y is None:
            individs = self._test_sample(spp, individs, n)
        elif n is not None:
            raise ValueError('calc_current_map: points (x, y) or a sample of n, not both')
        return spp._calc_current_map(x=x, y=y, individs=individs, lyr=lyr, kind=kind,
                                     barrier=barrier, cost=cost, tol=tol, max_iter=max_iter)

    def calc_spatial_structure(self, spp=0, edges=None, n_classes=10, max_dist=None,
                               individs=None, n=None, loci=None, nperm=0, seed=None,
                               fit_range=None, max_work=None):
        """fine-scale spatial genetic structure (an extension: the reference's IBD demo ends at
        MMRR on a sample): Loiselle's kinship averaged over the pairs of each distance class,
        its slope on ln(distance), Sp = -slope / (1 - F of the first class) and Wright's
        neighbourhood size 1 / Sp, computed on the device from the pairs closer than the largest
        class only, so the whole population can be analysed.  edges: the classes' bounds
        (default: n_classes classes of equal width in ln r from one landscape cell to max_dist;
        default a quarter of the shorter side).  individs, or a random sample of n, and loci
        restrict the analysis.  nperm > 0 adds permutation tests (genomes shuffled over the
        positions; seed as run_mantel's).  fit_range: (first class, one past the last) the slope
        is fitted over.  max_work bounds the pair-words (candidate pairs x genome words) of one
        device call; a request above it raises ValueError.
        -> dict: edges, pairs, mean_r, mean_lnr, F, dist2 (arrays over the classes), slope, F1,
        Sp, Nb, n, n_zero, work, ids; with nperm: nperm, perm_slope, p_slope, perm_F, p_F"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_spatial_structure(
            edges=edges, n_classes=n_classes, max_dist=max_dist,
            individs=self._test_sample(spp, individs, n), loci=loci, nperm=nperm, seed=seed,
            fit_range=fit_range, max_work=max_work)

    def calc_relatedness(self, spp=0, individs=None, n=None, loci=None):
        """KING-robust kinship between every two of at most 8192 individuals (an extension: the
        reference has no relatedness analysis), from integer counts taken on the device:
        kinship = (hh - 2 ibs0) / (nhet_a + nhet_b) with hh the loci at which both are
        heterozygous, ibs0 those at which they are opposite homozygotes and nhet each one's
        heterozygous loci (Manichaikul et al. 2010).  It uses no allele frequencies: about 1/4
        for first-degree relatives, 1/8 for second-degree ones, 0 for unrelated individuals of
        one population and negative across population structure.  individs, or a random sample
        of n, and loci restrict the analysis
        -> dict: ids, kinship [n][n] (0.5 on the diagonal; NaN where neither individual has a
        heterozygous locus), ibs0, hh [n][n], nhet [n]"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_relatedness(individs=self._test_sample(spp, individs, n), loci=loci)

    def find_kin(self, spp=0, max_dist=None, min_kinship=2 ** -3.5, individs=None, n=None,
                 loci=None, max_pairs=1 << 22, max_work=None, po_max_ibs0=0):
        """the pairs of close relatives in the population (an extension: the reference has no
        such analysis): every two individuals closer than max_dist (None: every pair) whose
        KING-robust kinship (calc_relatedness) is at least min_kinship, found on the device
        without an n x n matrix, so the whole population can be searched - the parent-offspring
        pairs whose distances are the dispersal kernel, the parent-offspring and half-sib
        counts of close-kin mark-recapture, and the relatives to prune from a sample.  Each
        pair is named by KING's cutoffs: 'dup', 'PO', 'FS', '2nd', '3rd' or 'un'; a first-degree
        pair is 'PO' iff its ibs0 <= po_max_ibs0 (a parent and its child are never opposite
        homozygotes).  With a recorded pedigree ('use_tskit': True) the truth stands beside it.
        individs, or a random sample of n, and loci restrict the search.  max_pairs bounds the
        list and max_work the pair-words of the device call; a request above either raises
        ValueError
        -> dict: ids_a, ids_b, kinship, ibs0, hh, dist, relationship (per pair, sorted by ids_a,
        ids_b), n_candidates, work, ids, nhet; with a pedigree also true_relationship ('PO',
        'FS', 'HS' or '')"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_kin_pairs(max_dist=max_dist, min_kinship=min_kinship,
                                   individs=self._test_sample(spp, individs, n), loci=loci,
                                   max_pairs=max_pairs, max_work=max_work,
                                   po_max_ibs0=po_max_ibs0)

    def get_pedigree_parents(self, spp=0, individs=None):
        """the recorded parents of the living individuals asked for (all by default), from the
        spatial pedigree of a 'use_tskit': True Species
        -> (ids ascending, int64 [n][2]: the ids of the parents that gave homologues 0 and 1;
        -1 for the founders)"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._get_pedigree_parents(individs=individs)

    def calc_ld_decay(self, spp=0, edges=None, n_bins=20, unit='c', max_dist=None,
                      individs=None, n=None, loci=None, min_maf=0.05, max_work=None):
        """the decay of linkage disequilibrium with distance, genome-wide (an extension: the
        reference's 'ld' statistic is an L x L matrix): mean r^2 over the pairs of loci in each
        bin of recombination fraction (unit 'c', from the architecture's recombination rates),
        map distance ('morgans') or locus separation ('loci'), computed on the device for any
        number of loci.  edges: the bins' bounds (default n_bins bins up to max_dist).
        individs, or a random sample of n, and loci restrict the analysis; loci below min_maf
        in the sample are left out.  max_work bounds the tile-words of the device call; a
        request above it raises ValueError.
        -> dict: edges, pairs, mean_r2, sd_r2, mean_dist, mean_c, expected_w (arrays over the
        bins; E[mean_r2] ~ expected_w / N_e + 1 / n_chrom), n_chrom, n_loci_kept, c1, loci,
        ids, work"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_ld_decay(edges=edges, n_bins=n_bins, unit=unit, max_dist=max_dist,
                                  individs=self._test_sample(spp, individs, n), loci=loci,
                                  min_maf=min_maf, max_work=max_work)

    def calc_ne(self, spp=0, method='ld', min_c=0.05, min_maf=0.05, individs=None, n=None,
                loci=None):
        """the linkage-disequilibrium estimate of the effective population size (Waples 2006;
        Weir & Hill 1980) from every pair of loci at recombination fraction >= min_c, computed
        on the device.  No confidence interval.
        -> dict: Ne, mean_r2, r2_drift, pairs, n_chrom, n_loci_kept, min_c"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_ne(method=method, min_c=min_c, min_maf=min_maf,
                            individs=self._test_sample(spp, individs, n), loci=loci)

    def prune_ld(self, spp=0, r2=0.2, window=50, unit='loci', min_maf=0.05, individs=None,
                 n=None, loci=None, max_edges=None, max_work=None):
        """loci in approximate linkage equilibrium (an extension: the reference has no such
        analysis; PLINK's --indep-pairwise), the list that calc_genetic_PCA, calc_ancestry,
        calc_grm, calc_relatedness and find_kin expect as loci=: among the loci with a
        minor-allele frequency of at least min_maf, no two within `window` of each other keep
        an r^2 of r2 or more.  unit as calc_ld_decay: 'loci' (locus numbers), 'morgans' or 'c'.
        The pairs above r2 are found on the device (gnx_ld_window, no L x L matrix); the greedy
        choice - the commonest locus first, each claiming its later neighbours - runs on the
        host.  individs, or a random sample of n, and loci restrict the analysis; max_edges
        bounds the pair list and max_work the tile-words of the device call, a request above
        either raises ValueError
        -> dict: loci (kept, ascending), removed, claimed_by, n_edges, c1, n_chrom, ids, work,
        kernel_ms"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._prune_ld(r2=r2, window=window, unit=unit, min_maf=min_maf,
                             individs=self._test_sample(spp, individs, n), loci=loci,
                             max_edges=max_edges, max_work=max_work)

    def clump(self, result, r=0, p1=1e-4, p2=1e-2, r2=0.5, window=250, unit='loci', spp=0,
              individs=None, max_edges=None, max_work=None):
        """the hits of run_gwas, run_lmm, run_lfmm or run_logistic_gea as independent signals (an
        extension; PLINK's --clump): the tested loci with p <= p2 (column r of p) in the order
        of p, each unclaimed one claiming the later ones within `window` of it with r^2 >= r2
        among the scan's individuals (or individs); index loci above p1 are dropped with their
        members.  The pairs come from the device (gnx_ld_window), the greedy step runs on the
        host
        -> dict: index_loci, index_p, members (a list of arrays), n_clumps, n_candidates,
        n_edges, work, kernel_ms, and trait_loci_hit (which clumps hold a causal locus) when
        the result carries trait_loci"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._clump(result, r=r, p1=p1, p2=p2, r2=r2, window=window, unit=unit,
                          individs=individs, max_edges=max_edges, max_work=max_work)

    def calc_ld_scores(self, spp=0, window=100, unit='loci', min_maf=0.05, adjust=True,
                       individs=None, n=None, loci=None, max_work=None):
        """the LD score of every locus (an extension; Bulik-Sullivan et al. 2015): 1 + the sum
        of its r^2 with the loci within `window` of it (unit as calc_ld_decay), adjusted for the
        sample's size when adjust, summed on the device (gnx_ld_window).  weights is 1 /
        max(ld_score, 1) over the whole genome, the weights= of calc_grm; with run_ldsc the
        scores tell inflation by structure from polygenic signal.  individs, or a random sample
        of n, and loci restrict the analysis; loci below min_maf are left out
        -> dict: ld_score, partners, score [n_loci], weights [L], loci, c1, n_chrom, ids, work,
        kernel_ms"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_ld_scores(window=window, unit=unit, min_maf=min_maf, adjust=adjust,
                                   individs=self._test_sample(spp, individs, n), loci=loci,
                                   max_work=max_work)

    def run_ldsc(self, result, scores, r=0, n_blocks=200, spp=0):
        """LD-score regression on the host (an extension; Bulik-Sullivan et al. 2015): the
        chi-square of an association scan (result: t^2 of column r, or lrt) regressed on the LD
        scores of calc_ld_scores with LDSC's two weights, standard errors by a jackknife over
        n_blocks contiguous blocks of loci (at most the loci there are)
        -> dict: intercept, slope, h2, intercept_se, slope_se, h2_se, ratio, mean_chi2, n_loci,
        n_blocks"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._run_ldsc(result, scores, r=r, n_blocks=n_blocks)

    def calc_ancestry(self, K, spp=0, individs=None, n=None, loci=None, init='pca', seed=None,
                      accelerate=True, tol=1e-4, max_sweeps=2000, fixed_F=None):
        """model-based ancestry (an extension: the reference has no such analysis): the
        admixture model of STRUCTURE / ADMIXTURE with K ancestral populations (1..16), fitted
        by EM with every sweep computed on the device from the packed genomes - individual
        ancestry proportions Q and ancestral allele frequencies F, the description of clines,
        contact zones and introductions (add_individuals) and the usual covariate beside PCs
        in a GEA.  individs, or a random sample of n, and loci (a list, or 'neutral': the loci
        under no selection) restrict the analysis.  init: 'pca' (Q from the first K - 1 genetic
        PCs, min-max scaled; no clustering), 'random' (from seed) or a pair of arrays (Q, F).
        accelerate: SQUAREM extrapolation, each accepted only if it does not lower the
        log-likelihood.  The fit stops when an accepted step gains less than tol in
        log-likelihood, or after max_sweeps sweeps.
        fixed_F [K][loci used] holds the frequencies and fits Q alone (projection).  For a large
        population fit on a sample first, res = calc_ancestry(K, n=2000), then project
        everybody onto its frequencies: calc_ancestry(K, fixed_F=res['F']) - one pass over the
        genomes per sweep and no frequency update.
        -> dict: Q [n][K] (rows: individs, ascending ids; components by decreasing mean
        ancestry, under fixed_F in its order), F [K][loci used], loci, individs, loglik (the
        trace of accepted log-likelihoods), n_sweeps, converged, n_params, aic, bic"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_ancestry(K, individs=self._test_sample(spp, individs, n), loci=loci,
                                  init=init, seed=seed, accelerate=accelerate, tol=tol,
                                  max_sweeps=max_sweeps, fixed_F=fixed_F)

    def calc_local_ancestry(self, spp=0, ancestry=None, F=None, loci=None, panels=None,
                            prior='fit', gens=10.0, individs=None, n=None, by=None, eps=1e-3,
                            calls=False, budget=None):
        """local ancestry (an extension: the reference has no such analysis): where on the
        genome the ancestry that calc_ancestry measures lies - after introductions, assisted
        gene flow, secondary contact or genetic rescue (add_individuals) - from the linkage
        model of Falush et al. (2003) with fixed frequencies and one admixture time, painted
        along both phased haplotypes of every individual on the device with the architecture's
        recombination map.  The frequencies come from exactly one of: ancestry (the dict
        calc_ancestry returned), F [K][loci used] with loci (None: all; 'neutral'; an ascending
        list), or panels (a label 0..K-1 per living individual in ascending-id order, -1: in no
        panel; reference-panel frequencies (ones + 0.5) / (2 n_k + 1)); K <= 8; they are
        clipped to [eps, 1 - eps].  prior: 'fit' (calc_ancestry's Q under those frequencies),
        'uniform' or rows [n][K].  gens: the generations since admixture, or 'fit'.  individs,
        or a random sample of n, restrict the analysis; by: a label 0..63 per analysed
        individual (-1: left out) for per-group summaries.  calls: also the hard calls and
        their tracts.  budget: bytes of device scratch per batch of haplotypes
        -> dict: ids, loci, K, gens, gens_trace (when fitted: rows (gens, loglik)), loglik,
        loglik_hap [2n] (haplotype 2 i + homologue), Q_local [n][K] (the share of the genome
        per ancestry), Q_prior, anc_locus [L_u][K] (mean posterior per locus; [G][L_u][K] with
        by), switches [2n], calls [2n][L_u] and tracts (if asked), map_len"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_local_ancestry(ancestry=ancestry, F=F, loci=loci, panels=panels,
                                        prior=prior, gens=gens,
                                        individs=self._test_sample(spp, individs, n), by=by,
                                        eps=eps, calls=calls, budget=budget)

    def calc_roh(self, spp=0, min_len=0.01, min_loci=50, unit='morgans', individs=None, n=None,
                 edges=None, cover=False):
        """runs of homozygosity and the genomic inbreeding coefficient F_ROH per individual (an
        extension: the reference has no haplotype-tract analysis), scanned on the device from
        the phased genomes: the tracts, at least min_len long (in the unit: 'morgans' on the
        map of the architecture's recombination rates, or 'loci') and min_loci loci, over which
        the two homologues are identical.  A rate of 0.5 or more is a chromosome boundary; under
        the template's free recombination every locus is a break, so every tract is one locus
        long.  individs, or a random sample of n, restrict the analysis.  edges: a histogram of
        tract lengths; cover: per locus the individuals with a run over it
        -> dict: ids, n_roh, roh_loci, roh_len, longest, f_roh, mean_f_roh, genome_len, hist (if
        edges), cover (if asked), unit"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_roh(min_len=min_len, min_loci=min_loci, unit=unit,
                             individs=self._test_sample(spp, individs, n), edges=edges,
                             cover=cover)

    def calc_ibs_sharing(self, spp=0, min_len=0.02, min_loci=50, unit='morgans', individs=None,
                         n=None, edges=None, n_classes=10, max_dist=None, tract_edges=None,
                         cover=False, max_work=None):
        """long haplotype tracts shared between individuals by geographic distance (an
        extension; the recent-dispersal signal that complements calc_spatial_structure): for
        every two of at most 4096 individuals (individs, or a random sample of n) the tracts at
        least min_len (in the unit) and min_loci loci long over which a haplotype of the one is
        identical to a haplotype of the other, scanned on the device, and their summary per
        distance class (edges, or n_classes classes up to max_dist as calc_spatial_structure).
        Under the template's free recombination every locus is a break, so every tract is one
        locus long.  max_work bounds the word steps of the device call; a request above it raises
        ValueError
        -> dict: ids, n_tracts, shared_len, longest ([n][n]), by_dist (the per-class table),
        hist, cover, work, unit"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_ibs_sharing(min_len=min_len, min_loci=min_loci, unit=unit,
                                     individs=self._test_sample(spp, individs, n), edges=edges,
                                     n_classes=n_classes, max_dist=max_dist,
                                     tract_edges=tract_edges, cover=cover, max_work=max_work)

    def calc_tmrca(self, spp=0, individs=None, n=None, loci=None, max_time_ago=None,
                   time_edges=None, n_time_bins=20, dist_edges=None, n_classes=10, max_dist=None,
                   groups=None, return_mrca=False, max_work=None):
        """pairwise coalescence times from the recorded spatial pedigree ('use_tskit': True; an
        extension: what tskit's divergence(mode='branch') and pair_coalescence_counts answer),
        merged on the device: for every two sample nodes - both homologues of at most 2048 living
        individuals (individs, or a random sample of n) - and every locus (loci: default all) the
        most recent common ancestor in the local tree and its age T in steps.  A pair coalesces
        at a locus when that ancestor is no older than max_time_ago (None: anywhere in the
        tables).  Means are over the (pair, locus) cells that coalesce.  time_edges: whole-step
        bounds of the histogram of T (default n_time_bins bins); dist_edges, n_classes,
        max_dist: distance classes as calc_spatial_structure; groups as calc_fst.  max_work
        bounds the look-up chains (pairs x loci) of the device call; a request above it raises
        ValueError
        -> dict: ids, nodes, loci, tmrca [n_nodes][n_nodes] (mean T per pair, NaN where it never
        coalesces), n_coalesced, per_locus (mean, share_coalesced, max), diversity_branch (2 x
        mean T), by_group (within, between), by_dist (mean T per distance class over pairs of
        different individuals), coal_times (edges, counts, at_risk, ne: the inverse coalescence
        rate per bin - the population-size history that calc_ne estimates), share_coalesced,
        mrca (if return_mrca), work"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_tmrca(individs=self._test_sample(spp, individs, n), loci=loci,
                               max_time_ago=max_time_ago, time_edges=time_edges,
                               n_time_bins=n_time_bins, dist_edges=dist_edges,
                               n_classes=n_classes, max_dist=max_dist, groups=groups,
                               return_mrca=return_mrca, max_work=max_work)

    def calc_ibd(self, spp=0, max_time_ago=None, min_len=0.02, min_loci=50, unit='morgans',
                 individs=None, n=None, edges=None, n_classes=10, max_dist=None,
                 tract_edges=None, cover=False, max_work=None):
        """segments shared identical by descent, from the recorded spatial pedigree
        ('use_tskit': True; an extension: what tskit's ibd_segments answers), merged on the
        device: for every two haplotypes of at most 2048 living individuals (individs, or a
        random sample of n) the stretches of loci, at least min_len (in the unit) and min_loci
        loci long, inherited from one common ancestor no older than max_time_ago steps (None:
        anywhere in the tables).  The truth beside calc_ibs_sharing, calc_roh and
        calc_relatedness, which estimate it from identity by state; lengths, breaks, distance
        classes and the histogram are calc_ibs_sharing's
        -> dict: ids, n_tracts, shared_len, longest ([n][n]; the diagonal the individual's own
        two haplotypes), by_dist, hist, cover, work, unit, f_ibd (the realised autozygosity per
        individual), genome_len"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_ibd(max_time_ago=max_time_ago, min_len=min_len, min_loci=min_loci,
                             unit=unit, individs=self._test_sample(spp, individs, n),
                             edges=edges, n_classes=n_classes, max_dist=max_dist,
                             tract_edges=tract_edges, cover=cover, max_work=max_work)

    def calc_ihs(self, spp=0, unit='morgans', min_maf=0.05, cutoff=0.05, max_gap=None,
                 max_extent=None, individs=None, n=None, loci=None, n_freq_bins=20,
                 keep_edge=False, max_work=None):
        """the integrated haplotype score iHS of every locus (an extension: the reference has no
        haplotype-based scan for selection), from the phased genomes of at most 2048
        individuals (individs, or a random sample of n), scanned on the device: the haplotypes
        carrying the derived allele (1) at a core locus and those carrying the ancestral one are
        followed outwards until their EHH falls below cutoff; iHH is the area under each curve
        and ihs_unstd = ln(iHH_1 / iHH_0), large where the derived allele sits on unusually long
        haplotypes - a sweep in progress.  unit: 'morgans' (the architecture's map), 'loci' or
        'sites' (nSL).  Loci below min_maf in the sample are left out.  A rate of 0.5 or more is
        a chromosome boundary; under the template's free recombination every scan ends at once.
        max_gap, max_extent (in the unit) bound a step and the whole scan; keep_edge keeps the
        loci whose scans reached an edge before the cutoff.  max_work bounds the word steps of
        the device call; a request above it raises ValueError
        -> dict: loci, pos, freq, ihh1, ihh0, ihs_unstd, ihs (standardised within n_freq_bins
        bins of the derived-allele frequency), status, steps ([n_loci][2][2]: direction,
        class), kept, c1, n_chrom, work, ids, unit"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_ihs(unit=unit, min_maf=min_maf, cutoff=cutoff, max_gap=max_gap,
                             max_extent=max_extent, individs=self._test_sample(spp, individs, n),
                             loci=loci, n_freq_bins=n_freq_bins, keep_edge=keep_edge,
                             max_work=max_work)

    def calc_nsl(self, spp=0, min_maf=0.05, cutoff=0.05, max_gap=None, max_extent=None,
                 individs=None, n=None, loci=None, n_freq_bins=20, keep_edge=False,
                 max_work=None):
        """nSL (Ferrer-Admetlla et al. 2014): calc_ihs with unit='sites', distances counted in
        kept (segregating) loci, which needs no map -> as calc_ihs"""
        return self.calc_ihs(spp=spp, unit='sites', min_maf=min_maf, cutoff=cutoff,
                             max_gap=max_gap, max_extent=max_extent, individs=individs, n=n,
                             loci=loci, n_freq_bins=n_freq_bins, keep_edge=keep_edge,
                             max_work=max_work)

    def calc_xpehh(self, groups, spp=0, unit='morgans', min_maf=0.05, cutoff=0.05, max_gap=None,
                   max_extent=None, individs=None, n=None, loci=None, keep_edge=False,
                   max_work=None):
        """XP-EHH of every locus between two groups of individuals (an extension; groups as
        calc_fst takes them, exactly two, at most 2048 individuals together: individs, or a
        random sample of n of the living, restrict them): iHH of all haplotypes of each group
        around each core locus, scanned on the device, and xpehh_unstd = ln(iHH_a / iHH_b) -
        positive where a sweep is complete or nearly so in group a and not in group b.  One
        departure from selscan: each population is scanned to its own cutoff, not to the cutoff
        of the pooled EHH.  The other arguments as calc_ihs
        -> dict: loci, pos, ihh_a, ihh_b, xpehh_unstd, xpehh (standardised over all defined
        loci), status, steps, kept, c1, names, n_a, n_b, work, ids, unit"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_xpehh(groups, unit=unit, min_maf=min_maf, cutoff=cutoff,
                               max_gap=max_gap, max_extent=max_extent,
                               individs=self._test_sample(spp, individs, n), loci=loci,
                               keep_edge=keep_edge, max_work=max_work)

    def calc_ehh(self, locus, spp=0, unit='morgans', min_maf=0.05, cutoff=0.05, max_gap=None,
                 max_extent=None, individs=None, n=None, loci=None, max_work=None):
        """the decay of extended haplotype homozygosity around one core locus (an extension):
        per locus the scan reached, the share of pairs of haplotypes carrying the derived
        (ehh1) or ancestral allele (ehh0) at the core that are identical from the core to there,
        scanned on the device.  The arguments as calc_ihs
        -> dict: locus, loci, pos, ehh1, ehh0 (NaN at loci not kept and past the scan's end),
        status, steps ([2][2]: direction, class), c1, n_chrom, ids, unit"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_ehh(locus, unit=unit, min_maf=min_maf, cutoff=cutoff, max_gap=max_gap,
                             max_extent=max_extent, individs=self._test_sample(spp, individs, n),
                             loci=loci, max_work=max_work)

    # -- Fst, diversity and the SFS of groups of individuals (sim/fst.py) ----------------
    def calc_fst(self, groups, spp=0, loci=None, method='HsHt', mean=True, est_Hs=False,
                 include_zeros=False):
        """Fst between groups of individuals (reference tests/validation/island/island_test.py,
        calc_Fsts_mod), from per-group locus counts taken on the device.  groups: a dict
        name -> ids, or integer labels aligned with the living in id order (group_by_layer,
        group_by_grid; negative: left out).  method 'HsHt' (the reference's) or 'hudson'
        -> {(name_a, name_b): mean over loci, or with mean=False the per-locus array};
        'var' -> one array over all groups, or its mean"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_fst(groups, loci=loci, method=method, mean=mean, est_Hs=est_Hs,
                             include_zeros=include_zeros)

    def calc_diversity(self, groups=None, spp=0, loci=None):
        """per group (default: everybody as one group): n, S, pi, theta_w, tajima_d, Ho, He, Fis"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_diversity(groups=groups, loci=loci)

    def calc_sfs(self, groups=None, spp=0, loci=None, folded=False):
        """site-frequency spectrum, one row per group -> (names, sfs)"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_sfs(groups=groups, loci=loci, folded=folded)

    def calc_diversity_map(self, spp=0, grid=None, win=3, min_n=2, loci=None, individs=None):
        """moving-window diversity rasters (sim/divmap.py): the landscape cut into grid =
        (nx, ny) map cells (default: (min(dim_x, 64), min(dim_y, 64))), a window of win x win
        map cells (win odd) around each, clipped at the edges -> dict with 'n' and 'S' (int
        rasters [ny][nx]), 'pi', 'theta_w', 'tajima_d', 'Ho', 'He', 'Fis' (float64 rasters, NaN
        where a window holds fewer than min_n individuals), 'grid', 'win', 'n_loci'"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._calc_diversity_map(grid=grid, win=win, min_n=min_n, loci=loci,
                                       individs=individs)

    def group_by_layer(self, lyr, edges, spp=0):
        """labels of the living in id order: np.digitize(e on Layer lyr, edges) - 1, -1 outside"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._group_by_layer(self._get_lyr_num(lyr), edges)

    def group_by_grid(self, nx, ny, spp=0):
        """labels of the living in id order: the landscape cut into nx x ny rectangles"""
        spp = self.comm[self._get_spp_num(spp)]
        return spp._group_by_grid(nx, ny)
