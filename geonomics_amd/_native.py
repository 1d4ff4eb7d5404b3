"""ctypes binding of libgnxhip.so (include/gnx_hip.h).

The product has no CPU fallback: loading fails loudly if the shared library is
missing, and creating a device state fails if there is no HIP device.
"""
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (GNX_LIB: another build of the same library - A/B runs of two builds on one box, tools/)
LIB_PATH = os.environ.get('GNX_LIB') or os.path.join(_HERE, 'libgnxhip.so')

# enums (include/gnx_hip.h)
DIST = {'lognormal': 0, 'wald': 1, 'levy': 2}
MATE_UNIFORM, MATE_NEAREST, MATE_INVERSE = 0, 1, 2
SURF_NONE, SURF_MIXTURE, SURF_UNIMODAL = 0, 1, 2
(F_X, F_Y, F_AGE, F_SEX, F_ID, F_E, F_Z, F_FIT, F_GROW, F_GENO) = range(10)
(R_N, R_NPAIRS, R_K, R_D, R_COUNTS) = range(5)
KERNELS = ['move', 'sort', 'permute', 'find_mates', 'pairs', 'offspring',
           'crossover', 'phenotype', 'density', 'death', 'compact', 'crossover_tail']

class Config(C.Structure):
    _fields_ = [('W', C.c_int32), ('H', C.c_int32), ('n_layers', C.c_int32),
                ('L', C.c_int32), ('n_traits', C.c_int32),
                ('cap_inds', C.c_int64), ('cap_rows', C.c_int64),
                ('seed', C.c_uint64), ('device', C.c_int32),
                ('reserved', C.c_int32)]


class SpeciesParams(C.Structure):
    _fields_ = [
        ('b', C.c_double), ('R', C.c_double), ('n_births_lambda', C.c_double),
        ('n_births_fixed', C.c_int32), ('sexed', C.c_int32),
        ('p_male', C.c_double), ('mating_radius', C.c_double),
        ('mate_mode', C.c_int32), ('repro_age', C.c_int32 * 2),
        ('max_age', C.c_int32), ('d_min', C.c_double), ('d_max', C.c_double),
        ('window_width', C.c_double), ('move', C.c_int32),
        ('dir_mu', C.c_double), ('dir_kappa', C.c_double),
        ('move_distr', C.c_int32), ('move_p1', C.c_double),
        ('move_p2', C.c_double), ('disp_distr', C.c_int32),
        ('disp_p1', C.c_double), ('disp_p2', C.c_double),
        ('move_surf', C.c_int32), ('move_surf_layer', C.c_int32),
        ('move_surf_kappa', C.c_double), ('disp_surf', C.c_int32),
        ('disp_surf_layer', C.c_int32), ('disp_surf_kappa', C.c_double),
        ('res_ratio', C.c_double * 2), ('K_layer', C.c_int32),
        ('pad0', C.c_int32), ('K_factor', C.c_double)]


# gnx_ind_rec (include/gnx_hip.h) as a numpy record dtype (32 bytes)
IND_REC = np.dtype([('x', np.float32), ('y', np.float32), ('age', np.int32),
                    ('sex', np.int32), ('id', np.int64), ('fit', np.float32),
                    ('nbr_mask', np.int32)], align=True)
assert IND_REC.itemsize == 32

# -- the signatures, read from include/gnx_hip.h: the header is the one place that says them ----
_SCALARS = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64,
            'uint8_t': C.c_uint8, 'float': C.c_float, 'double': C.c_double}
# every type the header uses, `const` dropped: scalars are exact, pointers to scalars are typed
# (ctypes checks them), handles and records are opaque
_CTYPES = {'void': None, 'int': C.c_int, 'char*': C.c_char_p,
           'int32_t': C.c_int32, 'int64_t': C.c_int64, 'double': C.c_double,
           'void*': C.c_void_p, 'gnx_state*': C.c_void_p, 'gnx_ind_rec*': C.c_void_p,
           'void**': C.POINTER(C.c_void_p), 'gnx_state**': C.POINTER(C.c_void_p),
           'gnx_config*': C.POINTER(Config), 'gnx_species_params*': C.POINTER(SpeciesParams)}
_CTYPES.update((t + '*', C.POINTER(c)) for t, c in _SCALARS.items())
_NP_PTR = {np.dtype(c): C.POINTER(c) for c in _SCALARS.values()}


def parse_prototypes(text, header='include/gnx_hip.h'):
    """{name: (restype, [argtypes])} of every `ret gnx_name(args);` in the header `text`;
    a type outside _CTYPES raises, naming the header and the prototype"""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r'^[ \t]*([\w \t*]+?)\b(gnx_\w+)\s*\(([^)]*)\)\s*;', text,
                                      flags=re.M):
        args = [] if args.strip() in ('', 'void') else args.split(',')
        types = []
        for k, decl in enumerate([ret + ' _'] + args):
            m = re.fullmatch(r'\s*(\w+)\s*(\**)\s*\w*\s*', re.sub(r'\bconst\b', ' ', decl))
            if not m or m.group(1) + m.group(2) not in _CTYPES:
                raise TypeError('%s, %s: no ctypes type for "%s"'
                                % (header, name, ' '.join(decl.split()) if k else ret.strip()))
            types.append(_CTYPES[m.group(1) + m.group(2)])
        protos[name] = (types[0], types[1:])
    return protos


with open(os.path.join(_HERE, '..', 'include', 'gnx_hip.h')) as _f:
    PROTOTYPES = parse_prototypes(_f.read())
EXPORTS = list(PROTOTYPES)
# the entry points declared in headers of their own (include/gnx_glm.h), read the same way
with open(os.path.join(_HERE, '..', 'include', 'gnx_glm.h')) as _f:
    PROTOTYPES_EXT = parse_prototypes(_f.read(), 'include/gnx_glm.h')
# (include/gnx_ldwin.h)
with open(os.path.join(_HERE, '..', 'include', 'gnx_ldwin.h')) as _f:
    PROTOTYPES_LDWIN = parse_prototypes(_f.read(), 'include/gnx_ldwin.h')

_lib = None


def load():
    """Load libgnxhip.so and declare every prototype of the headers on it; raises if it has
    not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            'geonomics_amd: %s is missing - build it with '
            '`python -m geonomics_amd.build` (hipcc, gfx950). There is no CPU '
            'fallback.' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**PROTOTYPES, **PROTOTYPES_EXT, **PROTOTYPES_LDWIN}.items():
        fn = getattr(lib, name, None)       # (None: an older build behind GNX_LIB lacks it)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _ptr(a):
    """a numpy array as the typed pointer its dtype says (None: NULL)"""
    if a is None:
        return None
    return a.ctypes.data_as(_NP_PTR[a.dtype])


def _dev_ptr(t):
    """a torch tensor's device address as the typed pointer its dtype says (None or an empty
    tensor: NULL)"""
    if t is None or not t.data_ptr():
        return None
    ctype = {'torch.float32': C.c_float, 'torch.float64': C.c_double}[str(t.dtype)]
    return C.cast(t.data_ptr(), C.POINTER(ctype))


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


class GnxError(RuntimeError):
    """a call into libgnxhip.so failed; `code` is its return code where the caller of the
    binding kept it (2: slots, genome rows or blocks did not fit)"""
    code = None


class Device:
    """One device-resident Species state (opaque gnx_state handle)."""

    def __init__(self, W, H, n_layers, L=0, n_traits=0, cap_inds=1024,
                 cap_rows=None, seed=0, device=0):
        self.lib = load()
        self.cfg = Config(W=W, H=H, n_layers=n_layers, L=L, n_traits=n_traits,
                          cap_inds=int(cap_inds),
                          cap_rows=int(cap_inds if cap_rows is None else cap_rows),
                          seed=int(seed) & 0xFFFFFFFFFFFFFFFF, device=device)
        self.W, self.H, self.n_layers, self.L = W, H, n_layers, L
        self.n_traits = n_traits
        self.W64 = self.lib.gnx_words_per_hom(L) if L > 0 else 0
        h = C.c_void_p()
        rc = self.lib.gnx_create(C.byref(self.cfg), C.byref(h))
        if rc:
            raise GnxError(self.lib.gnx_last_error().decode())
        self.h = h

    @property
    def blocks_per_hom(self):
        """blocks a homologue is stored in (the crossover copies or shares whole blocks)"""
        return int(self.lib.gnx_blocks_per_hom(self.h))

    @property
    def h(self):
        """the opaque handle; a Device that was closed raises instead of handing the
        library a null pointer"""
        h = self.__dict__.get('_h')
        if h is None or not h:
            raise GnxError('this Device was closed (gnx_destroy): no device state behind it')
        return h

    @h.setter
    def h(self, v):
        self.__dict__['_h'] = v

    def close(self):
        h = self.__dict__.get('_h')
        if h is not None and h:
            self.lib.gnx_destroy(h)
            self.__dict__['_h'] = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise GnxError(self.lib.gnx_last_error().decode())

    def _outs(self, fn, names, *args):
        """fn(h, *args, &out...) with one out scalar per name, of the types of fn's trailing
        pointer parameters -> {name: value}, int or float"""
        outs = [t._type_() for t in fn.argtypes[-len(names):]]
        self._chk(fn(self.h, *args, *map(C.byref, outs)))
        return {k: o.value for k, o in zip(names, outs)}

    # -- setup ---------------------------------------------------------------
    def upload_rasters(self, rasts):
        r = _arr(rasts, np.float32)
        assert r.shape == (self.n_layers, self.H, self.W), r.shape
        self._chk(self.lib.gnx_upload_rasters(self.h, _ptr(r)))

    def upload_layer(self, layer, rast):
        r = _arr(rast, np.float32)
        assert r.shape == (self.H, self.W)
        self._chk(self.lib.gnx_upload_layer(self.h, int(layer), _ptr(r)))

    def set_K_raster(self, K):
        """explicit K raster (float64 [H][W]) or None for rast[K_layer] * K_factor"""
        if K is None:
            self._chk(self.lib.gnx_set_k_raster(self.h, None))
            return
        k = _arr(K, np.float64)
        assert k.shape == (self.H, self.W), k.shape
        self._chk(self.lib.gnx_set_k_raster(self.h, _ptr(k)))

    @property
    def births_fixed_lambda(self):
        """births per pair when n_births_fixed (structs/species.py:604-609), else 0"""
        sp = getattr(self, '_sp', None)
        return int(sp.n_births_lambda) if (sp is not None and sp.n_births_fixed) else 0

    def set_species_params(self, sp):
        self._sp = sp
        self.sp = sp
        self._chk(self.lib.gnx_set_species_params(self.h, C.byref(sp)))

    def upload_population(self, x, y, age, sex, ids):
        x = _arr(x, np.float32)
        n = x.size
        y = _arr(y, np.float32)
        age = _arr(age, np.int32)
        sex = _arr(sex, np.uint8)
        ids = _arr(ids, np.int64)
        assert y.size == n and age.size == n and sex.size == n and ids.size == n
        self._chk(self.lib.gnx_upload_population(
            self.h, n, _ptr(x), _ptr(y), _ptr(age), _ptr(sex), _ptr(ids)))

    def set_positions(self, x, y):
        x, y = _arr(x, np.float32), _arr(y, np.float32)
        assert x.size == self.N and y.size == self.N
        self._chk(self.lib.gnx_set_positions(self.h, _ptr(x), _ptr(y)))

    def init_population(self, n):
        self._chk(self.lib.gnx_init_population(self.h, n))

    def set_recomb_paths(self, paths_packed):
        p = _arr(paths_packed, np.uint64)
        assert p.ndim == 2 and p.shape[1] == self.W64, (p.shape, self.W64)
        self._chk(self.lib.gnx_set_recomb_paths(self.h, p.shape[0], _ptr(p)))

    def set_trait(self, t, loci, alpha, layer, phi, gamma, univ_adv):
        loci = _arr(loci, np.int32)
        alpha = _arr(alpha, np.float64)
        assert loci.size == alpha.size
        phi_rast = None
        phi_s = 0.0
        if np.ndim(phi) == 2:
            phi_rast = _arr(phi, np.float32)
            assert phi_rast.shape == (self.H, self.W)
        else:
            phi_s = float(phi)
        self._chk(self.lib.gnx_set_trait(
            self.h, int(t), int(loci.size), _ptr(loci), _ptr(alpha), int(layer), phi_s,
            _ptr(phi_rast), float(gamma), int(bool(univ_adv))))

    def set_dominance(self, dom):
        d = None if dom is None else _arr(dom, np.uint8)
        self._chk(self.lib.gnx_set_dominance(self.h, _ptr(d)))

    def set_deleterious(self, loci, s):
        loci = _arr(loci, np.int32)
        s = _arr(s, np.float64)
        self._chk(self.lib.gnx_set_deleterious(self.h, int(loci.size), _ptr(loci), _ptr(s)))

    def upload_genomes(self, geno):
        g = _arr(geno, np.uint64)
        assert g.shape == (self.N, 2, self.W64), (g.shape, self.N, self.W64)
        self._chk(self.lib.gnx_upload_genomes(self.h, _ptr(g)))

    def assign_genomes(self, n_per_site):
        n = _arr(n_per_site, np.int32)
        assert n.size == self.L
        self._chk(self.lib.gnx_assign_genomes(self.h, _ptr(n)))

    def set_z(self):
        self._chk(self.lib.gnx_set_z(self.h))

    # -- stepping ------------------------------------------------------------
    def age(self):
        self._chk(self.lib.gnx_age(self.h))

    def move(self):
        self._chk(self.lib.gnx_move(self.h))

    def pop_dynamics(self, burn, with_selection):
        self._chk(self.lib.gnx_pop_dynamics(self.h, int(bool(burn)),
                                            int(bool(with_selection))))

    def pop_dynamics_mate(self, burn):
        self._chk(self.lib.gnx_pop_dynamics_mate(self.h, int(bool(burn))))

    def pop_dynamics_die(self, burn, with_selection):
        self._chk(self.lib.gnx_pop_dynamics_die(self.h, int(bool(burn)),
                                                int(bool(with_selection))))

    def set_z_range(self, first, n):
        self._chk(self.lib.gnx_set_z_range(self.h, first, n))

    def step(self, burn, with_selection):
        self._chk(self.lib.gnx_step(self.h, int(bool(burn)),
                                    int(bool(with_selection))))

    def walk(self, T, burn, with_selection):
        """T time steps in one call, counts kept on the device (gnx_walk): no read-back and
        one graph launch per step"""
        self._chk(self.lib.gnx_walk(self.h, int(T), int(bool(burn)), int(bool(with_selection))))

    def walk_history(self, max_steps=1 << 16):
        """(N at the start, births, deaths) of the last walk's steps, int64 arrays"""
        n = np.zeros(max_steps, np.int64)
        b = np.zeros(max_steps, np.int64)
        d = np.zeros(max_steps, np.int64)
        k = self.lib.gnx_walk_history(self.h, max_steps, _ptr(n), _ptr(b), _ptr(d))
        return n[:k], b[:k], d[:k]

    # -- one tiled step per call, exchanges issued by the library (csrc/gnx_comm.hip) -------
    def comm_init_rccl(self, unique_id, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self.lib.gnx_comm_init_rccl(self.h, buf, int(rank), int(world)))

    def comm_init_single(self):
        self._chk(self.lib.gnx_comm_init_single(self.h))

    def comm_local_join(self, group, rank):
        self._chk(self.lib.gnx_comm_local_join(self.h, group, int(rank)))

    def set_id_order(self, mode):
        """0: offspring ids in (hash cell, focal id) order (default); 1: virtual-tile-major"""
        self._chk(self.lib.gnx_set_id_order(self.h, int(mode)))
        self._id_order = int(mode)

    @property
    def id_order(self):
        return getattr(self, '_id_order', 0)

    def comm_selftest(self):
        """known words through every operation of the transport (collective); raises GnxError"""
        self._chk(self.lib.gnx_comm_selftest(self.h))

    def comm_free(self):
        self._chk(self.lib.gnx_comm_free(self.h))

    @property
    def comm_bytes_sent(self):
        return int(self.lib.gnx_comm_bytes_sent(self.h))

    def comm_info(self):
        """what the handle's tile communicator says about itself (gnx_comm_info): transport, rank,
        world, ncclCommCount / UserRank / CuDevice, device ordinal, steps, per-phase host ms per step"""
        out = np.zeros(16, np.int64)
        self._chk(self.lib.gnx_comm_info(self.h, _ptr(out)))
        steps = max(int(out[7]), 1)
        names = ('route_and_count_exchange', 'migrant_ghost_exchange_import',
                 'sort_pairs_second_count_exchange', 'births_gamete_service',
                 'allreduce_deaths')
        return {'transport': ('single', 'rccl', 'local')[int(out[0])], 'rank': int(out[1]),
                'world': int(out[2]), 'nccl_comm_count': int(out[3]),
                'nccl_comm_user_rank': int(out[4]), 'nccl_comm_device': int(out[5]),
                'hip_device': int(out[6]), 'tile_steps': int(out[7]),
                'phase_ms_per_step': {n: float(out[8 + k]) / 1e3 / steps
                                      for k, n in enumerate(names)},
                'bytes_sent': int(out[13]), 'gc_runs': int(out[14])}

    def tile_step_abort(self):
        self._chk(self.lib.gnx_tile_step_abort(self.h))

    def tile_step(self, burn, with_selection, exact=True):
        """one time step of this tile and, through its communicator, of the whole tiled
        landscape (gnx_tile_step) -> (N, births, deaths), see include/gnx_hip.h"""
        out = np.zeros(3, np.int64)
        self._chk(self.lib.gnx_tile_step(self.h, int(bool(burn)), int(bool(with_selection)),
                                         int(bool(exact)), _ptr(out)))
        self._id_order = 1          # (the library numbers a tiled step's offspring tile-major)
        return int(out[0]), int(out[1]), int(out[2])

    def tile_walk(self, T, burn, with_selection, exact=True):
        """T tiled steps in one call, no compaction between them (gnx_tile_walk) -> ((N, births,
        deaths) of the last step as tile_step reports them, sum of the global N at the start of
        every step, sum of the global births)"""
        out = np.zeros(5, np.int64)
        self._chk(self.lib.gnx_tile_walk(self.h, int(T), int(bool(burn)), int(bool(with_selection)),
                                         int(bool(exact)), _ptr(out)))
        self._id_order = 1
        return (int(out[0]), int(out[1]), int(out[2])), int(out[3]), int(out[4])

    def tile_step_begin(self, burn):
        """the tiled step up to and including the births (gnx_tile_step_begin) -> (first id,
        number) of the step's offspring over ALL tiles; the host's work on the newborns
        (mutations, pedigree rows) goes between this and tile_step_end"""
        self._chk(self.lib.gnx_tile_step_begin(self.h, int(bool(burn))))
        self._id_order = 1
        return tuple(self._outs(self.lib.gnx_tile_step_births, ('first_id', 'total')).values())

    def tile_step_end(self, burn, with_selection, exact=True):
        out = np.zeros(3, np.int64)
        self._chk(self.lib.gnx_tile_step_end(self.h, int(bool(burn)), int(bool(with_selection)),
                                             int(bool(exact)), _ptr(out)))
        return int(out[0]), int(out[1]), int(out[2])

    def tile2_vt_counts(self):
        """tile-major offspring ids: this tile's births per virtual tile, int64 [64]"""
        cnt = np.zeros(64, np.int64)
        self._chk(self.lib.gnx_tile2_vt_counts(self.h, _ptr(cnt)))
        return cnt

    def tile2_vt_bases(self, bases):
        b = _arr(bases, np.int64)
        assert b.size == 64
        self._chk(self.lib.gnx_tile2_vt_bases(self.h, _ptr(b)))

    def step_begin(self, burn):
        self._chk(self.lib.gnx_step_begin(self.h, int(bool(burn))))

    def step_mid(self, burn, with_selection):
        self._chk(self.lib.gnx_step_mid(self.h, int(bool(burn)), int(bool(with_selection))))

    def step_end(self, burn):
        self._chk(self.lib.gnx_step_end(self.h, int(bool(burn))))

    def counts(self):
        return tuple(self._outs(self.lib.gnx_counts, ('N', 'births', 'deaths')).values())

    def totals(self):
        """dict(steps, ind_steps, births, deaths, xo_births, dd_steps) summed over the gnx_step calls
        since reset_totals() - host-side bookkeeping of the library, no device access"""
        out = np.zeros(6, np.int64)
        self._chk(self.lib.gnx_totals(self.h, _ptr(out)))
        return dict(zip(('steps', 'ind_steps', 'births', 'deaths', 'xo_births', 'dd_steps'),
                        (int(v) for v in out)))

    def reset_totals(self):
        self._chk(self.lib.gnx_reset_totals(self.h))

    PATH_COUNTS = ('lazy_mortalities', 'xo_launch_p2', 'xo_flush', 'jobs_lanes_256',
                   'jobs_lanes_512', 'sort_hist_gather', 'gc_with_pending_xo', 'make_dense',
                   'moves_ahead')

    def path_counts(self):
        """dict of how often the host-driven steps took each path since the handle was made or
        reset_path_counts() (gnx_path_counts) - host-side bookkeeping, no device access"""
        out = np.zeros(len(self.PATH_COUNTS), np.int64)
        n = self.lib.gnx_path_counts(self.h, _ptr(out), len(out))
        assert n == len(out), 'gnx_path_counts: the library has %d counters' % n
        return dict(zip(self.PATH_COUNTS, (int(v) for v in out)))

    def reset_path_counts(self):
        self._chk(self.lib.gnx_reset_path_counts(self.h))

    @property
    def N(self):
        return self.counts()[0]

    @property
    def step_index(self):
        return self.lib.gnx_step_index(self.h)

    @step_index.setter
    def step_index(self, v):
        self._chk(self.lib.gnx_set_step_index(self.h, int(v)))

    def synchronize(self):
        self._chk(self.lib.gnx_synchronize(self.h))

    def set_defer_crossover(self, on):
        """cut the offspring's genomes after the death draws, survivors only (default)"""
        self._chk(self.lib.gnx_set_defer_crossover(self.h, int(bool(on))))

    def set_crossover_overlap(self, mode):
        """0 / False (default): full-width crossover beside the compaction and the next
        movement, the next cell sort waits for it; 1 / True: a narrow crossover beside the whole
        next step; 2: nothing runs beside the crossover"""
        self._chk(self.lib.gnx_set_crossover_overlap(self.h, int(mode)))

    def debug_halves(self):
        """(logical blocks in use / 2, broken references, collections so far, physical blocks
        in use, free blocks, blocks in all) of the shared genome blocks, after a collection"""
        out = np.zeros(6, np.int64)
        self._chk(self.lib.gnx_debug_halves(self.h, _ptr(out)))
        return out

    def genome_info(self):
        """host-side view of the genome blocks, no device access: dict(NB, BW, gc_runs,
        row_spread, sparse, free_blocks_est, free_rows, deferred)"""
        out = np.zeros(8, np.int64)
        self._chk(self.lib.gnx_genome_info(self.h, _ptr(out)))
        return dict(zip(('NB', 'BW', 'gc_runs', 'row_spread', 'sparse', 'free_blocks_est',
                         'free_rows', 'deferred'), (int(v) for v in out)))

    def set_crossover_split(self, wide_per_1024):
        """share (/1024) of a deferred crossover's jobs that runs at full width before the next
        cell sort; the rest runs narrow beside the sort and the kernels after it"""
        self._chk(self.lib.gnx_set_crossover_split(self.h, int(wide_per_1024)))

    def last_crossover_jobs(self):
        """int32 [n, 4]: the parent's two physical blocks, the block written,
        (path * 2 + start homologue) | block index << 24"""
        n = C.c_int64()
        self._chk(self.lib.gnx_last_crossover_jobs(self.h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 4), np.int32)
        if n.value:
            self._chk(self.lib.gnx_last_crossover_jobs(self.h, _ptr(out), n.value, C.byref(n)))
        return out

    @property
    def last_crossover_births(self):
        return self.lib.gnx_last_crossover_births(self.h)

    def set_stream(self, stream_ptr):
        self._chk(self.lib.gnx_set_stream(self.h, stream_ptr))

    def mutate(self, slots, loci, homs):
        slots = _arr(slots, np.int64)
        loci = _arr(loci, np.int32)
        homs = _arr(homs, np.uint8)
        self._chk(self.lib.gnx_mutate(self.h, int(slots.size), _ptr(slots), _ptr(loci), _ptr(homs)))

    # -- read-back -----------------------------------------------------------
    _FIELD_DT = {F_X: np.float32, F_Y: np.float32, F_AGE: np.int32,
                 F_SEX: np.uint8, F_ID: np.int64, F_FIT: np.float32,
                 F_GROW: np.int32}

    def download(self, field):
        n = int(self.lib.gnx_n_slots(self.h))     # = N, plus the ghosts while a tiled step runs
        if field == F_E:
            out = np.empty((self.n_layers, n), dtype=np.float32)
        elif field == F_Z:
            out = np.empty((self.n_traits, n), dtype=np.float32)
        elif field == F_GENO:
            out = np.empty((n, 2, self.W64), dtype=np.uint64)
        else:
            out = np.empty(n, dtype=self._FIELD_DT[field])
        if out.size:
            self._chk(self.lib.gnx_download(self.h, field, out.ctypes.data_as(C.c_void_p),
                                            out.nbytes))
        return out

    def download_genomes(self, slots):
        slots = _arr(slots, np.int64)
        out = np.empty((slots.size, 2, self.W64), dtype=np.uint64)
        if slots.size:
            self._chk(self.lib.gnx_download_genomes(self.h, slots.size, _ptr(slots), _ptr(out)))
        return out

    def download_raster(self, which):
        out = np.empty((self.H, self.W), dtype=np.float64)
        self._chk(self.lib.gnx_download_raster(self.h, which, _ptr(out)))
        return out

    def spatial_diff_stats(self):
        return tuple(self._outs(self.lib.gnx_spatial_diff_stats, ('mean', 'std')).values())

    def spatial_diff_sums(self):
        return tuple(self._outs(self.lib.gnx_spatial_diff_sums, ('sum', 'sum_sq')).values())

    # -- operator-level (tests) ----------------------------------------------
    def op_move(self, theta, dist):
        t = _arr(theta, np.float32)
        d = _arr(dist, np.float32)
        assert t.size == self.N and d.size == self.N
        self._chk(self.lib.gnx_op_move(self.h, _ptr(t), _ptr(d)))

    def op_move_draws(self):
        n = self.N
        t = np.empty(n, np.float32)
        d = np.empty(n, np.float32)
        self._chk(self.lib.gnx_op_move_draws(self.h, _ptr(t), _ptr(d)))
        return t, d

    def op_find_pairs(self, keep=None):
        n = self.N
        k = None if keep is None else _arr(keep, np.uint8)
        mate = np.empty(n, np.int32)
        pairs = np.empty((max(n, 1), 2), np.int32)
        npairs = C.c_int64()
        self._chk(self.lib.gnx_op_find_pairs(self.h, _ptr(k), _ptr(mate), _ptr(pairs),
                                             C.byref(npairs)))
        return mate, pairs[:npairs.value].copy()

    def op_crossover(self, parent_slots, keys, start_homs):
        p = _arr(parent_slots, np.int32)
        k = _arr(keys, np.int32)
        s = _arr(start_homs, np.uint8)
        B = p.shape[0]
        assert p.shape == (B, 2) and k.shape == (B, 2) and s.shape == (B, 2)
        self._chk(self.lib.gnx_op_crossover(self.h, B, _ptr(p), _ptr(k), _ptr(s)))

    def op_dispersal(self, mid_x, mid_y, theta, dist):
        mx = _arr(mid_x, np.float32)
        my = _arr(mid_y, np.float32)
        th = _arr(theta, np.float32)
        ds = _arr(dist, np.float32)
        A, B = th.shape
        ox = np.empty(B, np.float32)
        oy = np.empty(B, np.float32)
        used = np.empty(B, np.int32)
        self._chk(self.lib.gnx_op_dispersal(
            self.h, B, int(A), _ptr(mx), _ptr(my), _ptr(th), _ptr(ds), _ptr(ox), _ptr(oy),
            _ptr(used)))
        return ox, oy, used

    def lattice_dims(self):
        return tuple(self._outs(self.lib.gnx_density_lattice_dims, ('Jx', 'Jy')).values())

    def density_nmax(self):
        """N.max() of the last death probabilities' density raster (ops/demography.py:116)"""
        return self._outs(self.lib.gnx_density_nmax, ('nmax',))['nmax']

    def op_density(self, x, y, want_raster=True):
        x = _arr(x, np.float32)
        y = _arr(y, np.float32)
        jx, jy = self.lattice_dims()
        nodes = np.empty((jy, jx), np.float64)
        rast = np.empty((self.H, self.W), np.float64) if want_raster else None
        self._chk(self.lib.gnx_op_density(self.h, x.size, _ptr(x), _ptr(y), _ptr(nodes),
                                          _ptr(rast)))
        return nodes, rast

    def op_death_probs(self, with_selection, nodes_N, nodes_pairs=None):
        nN = _arr(nodes_N, np.float64)
        nP = None if nodes_pairs is None else _arr(nodes_pairs, np.float64)
        n = self.N
        p = np.empty(n, np.float64)
        d = np.empty(n, np.float64)
        self._chk(self.lib.gnx_op_death_probs(self.h, int(bool(with_selection)), _ptr(nN), _ptr(nP),
                                              _ptr(p), _ptr(d)))
        return p, d

    def op_mortality(self, dead):
        d = _arr(dead, np.uint8)
        assert d.size == self.N
        self._chk(self.lib.gnx_op_mortality(self.h, _ptr(d)))

    # -- spatial tiling (geonomics_amd/parallel.py) ---------------------------------
    def tile_set(self, R, C, r, c):
        self._chk(self.lib.gnx_tile_set(self.h, int(R), int(C), int(r), int(c)))
        self._n_tiles = int(R) * int(C)

    def _get_staged(self, n, with_z, with_geno):
        rec = np.zeros(n, dtype=IND_REC)
        z = np.zeros((n, self.n_traits), np.float32) if (with_z and self.n_traits) else None
        geno = np.zeros((n, 2, self.W64), np.uint64) if with_geno else None
        if n:
            self._chk(self.lib.gnx_tile_get_staged(
                self.h, rec.ctypes.data_as(C.c_void_p), _ptr(z), _ptr(geno)))
        return rec, z, geno

    def tile_export_migrants(self, with_geno):
        n = self._outs(self.lib.gnx_tile_export_migrants, ('n',))['n']
        return self._get_staged(n, True, with_geno and self.L > 0)

    def tile_export_halo(self):
        n = self._outs(self.lib.gnx_tile_export_halo, ('n',))['n']
        return self._get_staged(n, False, False)[0]

    def tile_import(self, rec, z=None, geno=None):
        rec = np.ascontiguousarray(rec, dtype=IND_REC)
        z = None if z is None else _arr(z, np.float32)
        geno = None if geno is None else _arr(geno, np.uint64)
        self._chk(self.lib.gnx_tile_import(self.h, rec.size, rec.ctypes.data_as(C.c_void_p),
                                           _ptr(z), _ptr(geno)))

    def tile_import_ghosts(self, rec):
        rec = np.ascontiguousarray(rec, dtype=IND_REC)
        self._chk(self.lib.gnx_tile_import_ghosts(self.h, rec.size, rec.ctypes.data_as(C.c_void_p)))

    def tile_pairs(self, burn):
        p, b = self._outs(self.lib.gnx_tile_pairs, ('n_pairs', 'n_births'),
                          int(bool(burn))).values()
        self._n_pairs = p
        return p, b

    def tile_pair_info(self):
        P = self._n_pairs
        ids = np.zeros(P, np.int64)
        nb = np.zeros(P, np.int32)
        if P:
            self._chk(self.lib.gnx_tile_pair_info(self.h, _ptr(ids), _ptr(nb)))
        return ids, nb

    def get_bins(self, which):
        out = np.zeros(self.lib.gnx_density_bin_count(self.h), np.int32)
        self._chk(self.lib.gnx_get_bins(self.h, int(which), _ptr(out)))
        return out

    def set_bins(self, which, bins):
        b = _arr(bins, np.int32)
        assert b.size == self.lib.gnx_density_bin_count(self.h)
        self._chk(self.lib.gnx_set_bins(self.h, int(which), _ptr(b)))

    def tile_offspring(self, burn, id_base, pair_goff):
        """pair_goff None: tile-major offspring ids (tile2_vt_counts / tile2_vt_bases came first)"""
        g = None if pair_goff is None else _arr(pair_goff, np.int64)
        assert g is None or g.size == self._n_pairs
        n = C.c_int64()
        self._chk(self.lib.gnx_tile_offspring(self.h, int(bool(burn)), int(id_base), _ptr(g),
                                              C.byref(n)))
        self._n_req = n.value
        return n.value

    def tile_get_requests(self):
        n = self._n_req
        pid = np.zeros(n, np.int64)
        ck = np.zeros(n, np.int32)
        key = np.zeros(n, np.int32)
        st = np.zeros(n, np.uint8)
        px = np.zeros(n, np.float32)
        py = np.zeros(n, np.float32)
        if n:
            self._chk(self.lib.gnx_tile_get_requests(
                self.h, _ptr(pid), _ptr(ck), _ptr(key), _ptr(st), _ptr(px), _ptr(py)))
        return pid, ck, key, st, px, py

    def tile_serve_gametes(self, pids, keys, starts):
        pids = _arr(pids, np.int64)
        keys = _arr(keys, np.int32)
        starts = _arr(starts, np.uint8)
        out = np.zeros((pids.size, self.W64), np.uint64)
        if pids.size:
            self._chk(self.lib.gnx_tile_serve_gametes(
                self.h, pids.size, _ptr(pids), _ptr(keys), _ptr(starts), _ptr(out)))
        return out

    def tile_put_gametes(self, child_k, data):
        ck = _arr(child_k, np.int32)
        d = _arr(data, np.uint64)
        if ck.size:
            assert d.shape == (ck.size, self.W64)
            self._chk(self.lib.gnx_tile_put_gametes(self.h, ck.size, _ptr(ck), _ptr(d)))

    def tile_finish_births(self, burn):
        self._chk(self.lib.gnx_tile_finish_births(self.h, int(bool(burn))))

    def tile_die(self, burn, with_selection, have_pairs):
        self._chk(self.lib.gnx_tile_die(self.h, int(bool(burn)), int(bool(with_selection)),
                                        int(bool(have_pairs))))

    def set_max_id(self, v):
        self._chk(self.lib.gnx_set_max_id(self.h, int(v)))

    # -- tile2: the device-driven protocol (include/gnx_hip.h); addresses are plain ints
    # (device memory) --------------------------------------------------------------------
    def tile_pair_ptrs_nosync(self):
        """-> P, order keys address (int64[P], ascending), n_births address (int32[P]) or 0,
        without waiting for the stream (the consumer is ordered behind the library's stream)"""
        n, a, b = C.c_int64(), C.c_void_p(), C.c_void_p()
        self._chk(self.lib.gnx_tile_pair_ptrs_nosync(self.h, C.byref(n), C.byref(a), C.byref(b)))
        return n.value, a.value or 0, b.value or 0

    def stream_ptr(self):
        a = C.c_void_p()
        self._chk(self.lib.gnx_stream_ptr(self.h, C.byref(a)))
        return a.value or 0

    def tile2_move_route(self, move):
        """-> counts int64 [2][R*C]: migrants per rank, ghosts per rank (one host wait)"""
        T = max(getattr(self, '_n_tiles', 1), 1)
        cnt = np.zeros(2 * T, np.int64)
        self._chk(self.lib.gnx_tile2_move_route(self.h, int(bool(move)), _ptr(cnt)))
        return cnt.reshape(2, T)

    def tile2_route_ptrs(self):
        a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self.lib.gnx_tile2_route_ptrs(self.h, C.byref(a), C.byref(b), C.byref(c),
                                                C.byref(d)))
        return a.value or 0, b.value or 0, c.value or 0, d.value or 0

    def tile2_import(self, n_mig, rec, z, geno, n_ghost, ghost_rec):
        self._chk(self.lib.gnx_tile2_import(
            self.h, int(n_mig), rec or None, z or None, geno or None, int(n_ghost),
            ghost_rec or None))

    def tile2_pairs(self, burn):
        """-> P, births, gamete requests per owning rank int64 [R*C]"""
        T = max(getattr(self, '_n_tiles', 1), 1)
        cnt = np.zeros(2 + T, np.int64)
        self._chk(self.lib.gnx_tile2_pairs(self.h, int(bool(burn)), _ptr(cnt)))
        self._n_pairs = int(cnt[0])
        return int(cnt[0]), int(cnt[1]), cnt[2:]

    def tile2_offspring(self, burn, id_base, goff_ptr):
        a = C.c_void_p()
        self._chk(self.lib.gnx_tile2_offspring(self.h, int(bool(burn)), int(id_base),
                                               goff_ptr or None, C.byref(a)))
        return a.value or 0

    def tile2_serve(self, n, req_ptr):
        a = C.c_void_p()
        self._chk(self.lib.gnx_tile2_serve(self.h, int(n), req_ptr or None, C.byref(a)))
        return a.value or 0

    def tile2_put(self, n, data_ptr):
        self._chk(self.lib.gnx_tile2_put(self.h, int(n), data_ptr or None))

    def tile2_finish_births(self, burn):
        a, n = C.c_void_p(), C.c_int64()
        self._chk(self.lib.gnx_tile2_finish_births(self.h, int(bool(burn)), C.byref(a),
                                                   C.byref(n)))
        return a.value or 0, n.value

    def tile2_die(self, burn, with_selection, have_pairs):
        """-> the all-reduced (N before this step's deaths, births, deaths of the previous step)"""
        tot = np.zeros(3, np.int64)
        self._chk(self.lib.gnx_tile2_die(self.h, int(bool(burn)), int(bool(with_selection)),
                                         int(bool(have_pairs)), _ptr(tot)))
        return int(tot[0]), int(tot[1]), int(tot[2])

    def last_births(self, with_gametes=True):
        """offspring of the last pop_dynamics_mate (call before pop_dynamics_die):
        child ids [B], parent ids [B,2], path keys [B,2], start homologues [B,2], xy [B,2]"""
        B = self.counts()[1]
        child = np.zeros(B, np.int64)
        par = np.zeros((B, 2), np.int64)
        keys = np.zeros((B, 2), np.int32)
        starts = np.zeros((B, 2), np.uint8)
        xy = np.zeros((B, 2), np.float32)
        if B:
            self._chk(self.lib.gnx_last_births(
                self.h, _ptr(child), _ptr(par), _ptr(keys) if with_gametes else None,
                _ptr(starts) if with_gametes else None, _ptr(xy)))
        return child, par, keys, starts, xy

    # -- statistics ------------------------------------------------------------------
    def stats_locus_counts(self):
        c1 = np.zeros(self.L, np.int32)
        ch = np.zeros(self.L, np.int32)
        self._chk(self.lib.gnx_stats_locus_counts(self.h, _ptr(c1), _ptr(ch)))
        return c1, ch

    def stats_group_counts(self, slots, group_start):
        """per-group, per-locus counts: slots[group_start[g]:group_start[g + 1]] are the slots of
        group g -> (cnt1 [G][L] int32 1-alleles, cnt_het [G][L] int32 heterozygotes)"""
        s = _arr(slots, np.int64).ravel()
        if s.size and (s.min() < -2 ** 31 or s.max() >= 2 ** 31):
            raise GnxError('gnx_stats_group_counts: slot out of range')
        s = s.astype(np.int32)
        gs = _arr(group_start, np.int64).ravel()
        G = int(gs.size) - 1
        # (the library refuses G outside 1..1024 before it writes: no G x L buffer for that)
        shape = (G, self.L) if 1 <= G <= 1024 and G * self.L <= 2 ** 26 else (0, 0)
        c1 = np.zeros(shape, np.int32)
        ch = np.zeros(shape, np.int32)
        self._chk(self.lib.gnx_stats_group_counts(
            self.h, int(s.size), _ptr(s), max(G, -1),
            _ptr(gs if gs.size else np.zeros(1, np.int64)), _ptr(c1), _ptr(ch)))
        return c1, ch

    # -- moving-window diversity sums (csrc/gnx_divmap.hip; sim/divmap.py) -----------------
    def divmap_sums(self, slots, cell_start, nx, ny, r, locus_mask=None, max_counts=0):
        """the four integers per window of an nx x ny map (gnx_divmap_sums): slots grouped by
        map cell iy * nx + ix, cell_start [nx * ny + 1], windows of Chebyshev radius r
        -> dict n, S (int32), sum_het, sum_cc (int64), each [ny][nx]"""
        s = _arr(slots, np.int64).ravel()
        if s.size and (s.min() < -2 ** 31 or s.max() >= 2 ** 31):
            raise GnxError('gnx_divmap_sums: slot out of range')
        s = s.astype(np.int32)
        cs = _arr(cell_start, np.int64).ravel()
        nx, ny, r = int(nx), int(ny), int(r)
        if not -2 ** 31 <= min(nx, ny, r) <= max(nx, ny, r) < 2 ** 31:
            raise ValueError('nx, ny, r: 32-bit integers')
        cells = nx * ny if nx >= 1 and ny >= 1 and nx * ny <= 2 ** 20 else 0
        if cells and cs.size != cells + 1:
            raise ValueError('cell_start: %d entries, not nx * ny + 1 = %d' % (cs.size, cells + 1))
        m = self._locus_mask_words(locus_mask)
        # (the library refuses a map outside 1..2^20 cells before it writes: no raster for that)
        shape = (ny, nx) if cells else (0, 0)
        out = dict(n=np.zeros(shape, np.int32), S=np.zeros(shape, np.int32),
                   sum_het=np.zeros(shape, np.int64), sum_cc=np.zeros(shape, np.int64))
        self._chk(self.lib.gnx_divmap_sums(
            self.h, int(s.size), _ptr(s), nx, ny, _ptr(cs if cs.size else np.zeros(1, np.int64)),
            r, _ptr(m), int(max_counts), _ptr(out['n']), _ptr(out['S']), _ptr(out['sum_het']),
            _ptr(out['sum_cc'])))
        return out

    def divmap_info(self):
        """locus tiles, chunks and kernel launches of the last divmap_sums"""
        return self._outs(self.lib.gnx_divmap_info, ('tiles', 'chunks', 'launches'))

    def stats_ld(self, loci):
        loci = _arr(loci, np.int32)
        out = np.zeros((loci.size, loci.size), np.float64)
        self._chk(self.lib.gnx_stats_ld(self.h, int(loci.size), _ptr(loci), _ptr(out)))
        return out

    def stats_ld_counts(self, loci):
        loci = _arr(loci, np.int32)
        c = np.zeros(loci.size, np.int64)
        cc = np.zeros((loci.size, loci.size), np.int64)
        self._chk(self.lib.gnx_stats_ld_counts(self.h, int(loci.size), _ptr(loci), _ptr(c),
                                               _ptr(cc)))
        return c, cc

    # -- genetic PCA and distances (csrc/gnx_geno.hip) ---------------------------------
    def _geno_slots(self, slots):
        if slots is None:
            return None, int(self.N)
        s = _arr(slots, np.int64)
        return s, int(s.size)

    def _locus_mask_words(self, locus_mask):
        if locus_mask is None:
            return None
        m = _arr(locus_mask, np.uint64)
        if m.size != self.W64:
            raise ValueError('locus_mask: %d words, not %d' % (m.size, self.W64))
        return m

    def geno_gram(self, slots=None, locus_mask=None):
        """G = D D^T of the dosages of `slots` (all living slots by default), exact int64
        [n][n]; locus_mask: uint64 [W64] bit mask of the loci to use (None: all)"""
        s, n = self._geno_slots(slots)
        m = self._locus_mask_words(locus_mask)
        # (the library refuses n outside 1..8192 before it writes: no n x n buffer for that)
        out = np.zeros((n, n) if 1 <= n <= 8192 else (0, 0), np.int64)
        self._chk(self.lib.gnx_geno_gram(self.h, n, _ptr(s), _ptr(m), _ptr(out)))
        return out

    def _val_table(self, val):
        """the table of grm and assoc_quad: fp32 [L][3], the value of each locus at dosage 0, 1, 2"""
        v = _arr(val, np.float32)
        if v.shape != (self.L, 3):
            raise ValueError('val: shape %s, not (L = %d, 3)' % (v.shape, self.L))
        return v

    def grm(self, val, slots=None, locus_mask=None):
        """G_ij = sum over the masked loci of val[l][d_il] val[l][d_jl] for `slots` (all living
        slots by default; at most 8192): val fp32 [L][3], the value of each locus at dosage 0, 1,
        2 (include/gnx_hip.h, gnx_grm) -> G float64 [n][n], symmetric"""
        s, n = self._geno_slots(slots)
        m = self._locus_mask_words(locus_mask)
        v = self._val_table(val)
        # (the library refuses n outside 1..8192 before it writes: no n x n buffer for that)
        out = np.zeros((n, n) if 1 <= n <= 8192 else (0, 0), np.float64)
        self._chk(self.lib.gnx_grm(self.h, n, _ptr(s), _ptr(m), _ptr(v), _ptr(out)))
        return out

    def grm_probe(self, mode):
        """a measuring switch (tools/grm_bench.py): 1 = grm runs its expansion alone, 2 = its
        MFMAs alone (zeros come back; only grm_info's kernel_ms means anything), 0 = the kernel"""
        self._chk(self.lib.gnx_grm_probe(self.h, int(mode)))

    def grm_info(self):
        """of the last grm: dict(tiles, k_chunks, kernel_ms)"""
        return self._outs(self.lib.gnx_grm_info, ('tiles', 'k_chunks', 'kernel_ms'))

    @staticmethod
    def _f32_dev(t, name):
        import torch
        if not torch.cuda.is_available():
            raise GnxError('torch sees no HIP device: initialise it (torch.cuda.init()) before '
                           'the first Device is created, as bench.py does')
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2:
            raise ValueError('%s: a 2-d torch tensor on the device' % name)
        return t.to(torch.float32).contiguous()

    def geno_matmul(self, M, slots=None):
        """Y = D M: M torch fp32 [L][k] on the handle's device -> Y torch fp32 [n][k] (rows in
        the order of `slots`, all living slots by default).  The call waits for the current
        torch stream before it reads M and returns with Y complete."""
        import torch
        M = self._f32_dev(M, 'M')
        if M.shape[0] != self.L:
            raise ValueError('M: %d rows, not L = %d' % (M.shape[0], self.L))
        s, n = self._geno_slots(slots)
        Y = torch.empty((n, M.shape[1]), dtype=torch.float32, device=M.device)
        torch.cuda.current_stream(M.device).synchronize()
        self._chk(self.lib.gnx_geno_matmul(self.h, int(M.shape[1]), _dev_ptr(M), _dev_ptr(Y), n,
                                           _ptr(s)))
        return Y

    def geno_rmatmul(self, Y, slots=None):
        """Z = D^T Y: Y torch fp32 [n][k] on the handle's device -> Z torch fp32 [L][k]"""
        import torch
        Y = self._f32_dev(Y, 'Y')
        s, n = self._geno_slots(slots)
        if Y.shape[0] != n:
            raise ValueError('Y: %d rows, not n = %d' % (Y.shape[0], n))
        Z = torch.empty((self.L, Y.shape[1]), dtype=torch.float32, device=Y.device)
        torch.cuda.current_stream(Y.device).synchronize()
        self._chk(self.lib.gnx_geno_rmatmul(self.h, int(Y.shape[1]), _dev_ptr(Y), _dev_ptr(Z), n,
                                            _ptr(s)))
        return Z

    # -- genotype-environment association (csrc/gnx_gea.hip) ----------------------------
    def geno_locus_gram(self, loci, slots=None):
        """C = D^T D (int64 [n_loci][n_loci]) and s = D^T 1 (int64 [n_loci]) of the dosages
        of `slots` (all living slots by default) at `loci` (ascending, distinct, up to
        8192), exact"""
        loci = _arr(loci, np.int32).ravel()
        s, n = self._geno_slots(slots)
        m = int(loci.size) if 1 <= loci.size <= 8192 else 0    # the library refuses the rest
        Cm = np.zeros((m, m), np.int64)
        cs = np.zeros(m, np.int64)
        self._chk(self.lib.gnx_geno_locus_gram(self.h, int(loci.size), _ptr(loci), n, _ptr(s),
                                               _ptr(Cm), _ptr(cs)))
        return Cm, cs

    def geno_locus_cross(self, loci, lyr, slots=None):
        """D^T Z [n_loci][3], Z^T Z [3][3], Z^T 1 [3] in fp64, Z = [e[:, lyr], x, y] of
        `slots` as the device holds them (nothing is uploaded)"""
        loci = _arr(loci, np.int32).ravel()
        s, n = self._geno_slots(slots)
        m = int(loci.size) if 1 <= loci.size <= 8192 else 0
        DtZ = np.zeros((m, 3), np.float64)
        ZtZ = np.zeros((3, 3), np.float64)
        Zt1 = np.zeros(3, np.float64)
        self._chk(self.lib.gnx_geno_locus_cross(self.h, int(loci.size), _ptr(loci), int(lyr), n,
                                                _ptr(s), _ptr(DtZ), _ptr(ZtZ), _ptr(Zt1)))
        return DtZ, ZtZ, Zt1

    # -- Mantel tests and MMRR (csrc/gnx_mantel.hip) --------------------------------------
    def dist_perm_sums(self, predictors, perm, slots=None, locus_mask=None):
        """the cross-sums of the genetic distances of `slots` (all living slots by default)
        with the predictors' distances under the permutations `perm` int32 [n_perm][n]
        (individual i takes the columns of individual perm[p][i]).  predictors: a list of lists
        of (field, index) columns, e.g. [[(F_X, 0), (F_Y, 0)], [(F_E, 1)]], read as the device
        holds them.  -> sums float64 [n_perm][n_pred], dict(m, sy, syy, sx [n_pred],
        sxy [n_pred], sxx [n_pred][n_pred]) of the unpermuted pairs"""
        return self._dist_perm_sums(predictors, None, perm, slots, locus_mask)

    def dist_perm_sums_mat(self, predictors, mats, perm, slots=None, locus_mask=None):
        """dist_perm_sums with n x n predictor matrices `mats` (float64 [n_mat][n][n], rows and
        columns in the order of `slots`; finite, symmetric, zero diagonal) behind the column
        predictors (which may be empty): sums float64 [n_perm][n_pred + n_mat] and the moments,
        the columns first"""
        return self._dist_perm_sums(predictors, mats, perm, slots, locus_mask)

    def _dist_perm_sums(self, predictors, mats, perm, slots, locus_mask):
        """both calls above; mats None: gnx_dist_perm_sums, which takes no matrices"""
        s, n = self._geno_slots(slots)
        m = self._locus_mask_words(locus_mask)
        predictors = list(predictors)
        off = np.cumsum([0] + [len(p) for p in predictors]).astype(np.int32)
        cols = _arr([c for p in predictors for c in p], np.int32).reshape(-1, 2)
        k = len(predictors)
        if mats is not None:
            mats = _arr(mats, np.float64)
            mats = mats.reshape((0, n, n)) if mats.size == 0 else mats
            if mats.ndim != 3 or mats.shape[1:] != (n, n):
                raise ValueError('mats: [n_mat][%d][%d], not %s' % (n, n, mats.shape))
            k += mats.shape[0]
        perm = _arr(perm, np.int32)
        if perm.ndim != 2 or perm.shape[1] != n:
            raise ValueError('perm: [n_perm][%d], not %s' % (n, perm.shape))
        sums = np.zeros((perm.shape[0], k), np.float64)
        mom = np.zeros(3 + 2 * k + k * (k + 1) // 2, np.float64)
        head = (self.h, n, _ptr(s), _ptr(m), len(predictors), _ptr(off),
                _ptr(cols if cols.size else None))
        tail = (int(perm.shape[0]), _ptr(perm), _ptr(sums), _ptr(mom))
        if mats is None:
            self._chk(self.lib.gnx_dist_perm_sums(*head, *tail))
        else:
            self._chk(self.lib.gnx_dist_perm_sums_mat(
                *head, int(mats.shape[0]), _ptr(mats if mats.size else None), *tail))
        sxx = np.zeros((k, k))
        sxx[np.triu_indices(k)] = mom[3 + 2 * k:]
        sxx = sxx + np.triu(sxx, 1).T
        return sums, dict(m=mom[0], sy=mom[1], syy=mom[2], sx=mom[3:3 + k].copy(),
                          sxy=mom[3 + k:3 + 2 * k].copy(), sxx=sxx)

    # -- least-cost distances over the landscape (csrc/gnx_cost.hip) -----------------------
    def _cost_raster(self, R):
        R = _arr(R, np.float64)
        if R.shape != (self.cfg.H, self.cfg.W):
            raise ValueError('R: [%d][%d], not %s' % (self.cfg.H, self.cfg.W, R.shape))
        return R

    def cost_surfaces(self, R, res, src):
        """the accumulated-cost raster of every source cell (y * W + x) over the resistance
        raster R float64 [H][W] (inf: impassable) with cell size res = (res_x, res_y)
        (include/gnx_hip.h, gnx_cost_surfaces) -> float64 [n_src][H][W]"""
        R = self._cost_raster(R)
        src = _arr(src, np.int32).ravel()
        out = np.zeros((src.size, self.cfg.H, self.cfg.W), np.float64)
        self._chk(self.lib.gnx_cost_surfaces(
            self.h, _ptr(R), float(res[0]), float(res[1]), int(src.size),
            _ptr(src if src.size else None), _ptr(out if out.size else None)))
        return out

    def cost_matrix(self, R, res, cells):
        """the pairwise least-cost distances of distinct cells (y * W + x), exactly symmetric
        (include/gnx_hip.h, gnx_cost_matrix) -> float64 [n_cells][n_cells]"""
        R = self._cost_raster(R)
        cells = _arr(cells, np.int32).ravel()
        n = int(cells.size) if 1 <= cells.size <= 32768 else 0   # the library refuses the rest
        D = np.zeros((n, n), np.float64)
        self._chk(self.lib.gnx_cost_matrix(
            self.h, _ptr(R), float(res[0]), float(res[1]), int(cells.size),
            _ptr(cells if cells.size else None), _ptr(D if D.size else None)))
        return D

    def cost_budget(self, n_bytes):
        """bytes of distance rasters one batch of sources may take (0: the default, 2 GiB)"""
        self._chk(self.lib.gnx_cost_budget(self.h, int(n_bytes)))

    def cost_info(self):
        """of the last cost_surfaces / cost_matrix: dict(kernel_ms, launches, rounds, batches)"""
        return self._outs(self.lib.gnx_cost_info, ('kernel_ms', 'launches', 'rounds', 'batches'))

    # -- circuit-theory resistances and current maps (csrc/gnx_circuit.hip) ----------------
    def _circuit_args(self, R, res, cells, tol, max_iter):
        R = self._cost_raster(R)
        cells = _arr(cells, np.int32).ravel()
        return R, cells, (
            self.h, _ptr(R), float(res[0]), float(res[1]), int(cells.size),
            _ptr(cells if cells.size else None), 1e-10 if tol is None else float(tol),
            0 if max_iter is None else int(max_iter))

    def circuit_matrix(self, R, res, cells, tol=None, max_iter=None):
        """the pairwise effective resistances of distinct cells (y * W + x) over the resistance
        raster R float64 [H][W] (inf: impassable), exactly symmetric; tol: the relative residual
        every system is solved to (default 1e-10), max_iter: the CG iterations a batch may take
        (default: twice the cells of the largest component)
        (include/gnx_hip.h, gnx_circuit_matrix) -> float64 [n][n]"""
        R, cells, args = self._circuit_args(R, res, cells, tol, max_iter)
        n = int(cells.size) if 1 <= cells.size <= 8192 else 0     # the library refuses the rest
        D = np.zeros((n, n), np.float64)
        self._chk(self.lib.gnx_circuit_matrix(*args, _ptr(D if D.size else None)))
        return D

    def circuit_current(self, R, res, cells, tol=None, max_iter=None):
        """the cumulative node-current map of all pairs of at most 128 distinct cells
        (include/gnx_hip.h, gnx_circuit_current)
        -> (float64 [H][W], pairs used, pairs skipped)"""
        R, cells, args = self._circuit_args(R, res, cells, tol, max_iter)
        out = np.zeros((self.cfg.H, self.cfg.W), np.float64)
        counts = np.zeros(2, np.int64)
        self._chk(self.lib.gnx_circuit_current(*args, _ptr(out), _ptr(counts)))
        return out, int(counts[0]), int(counts[1])

    def circuit_potentials(self, R, res, cells, tol=None, max_iter=None):
        """the potentials x_i of L x_i = e_i - e_anchor of at most 128 distinct cells as the
        solver left them (include/gnx_hip.h, gnx_circuit_potentials)
        -> (float64 [n][H][W], anchor int32 [n])"""
        R, cells, args = self._circuit_args(R, res, cells, tol, max_iter)
        n = int(cells.size) if 1 <= cells.size <= 128 else 0      # the library refuses the rest
        out = np.zeros((n, self.cfg.H, self.cfg.W), np.float64)
        anchor = np.full(n, -1, np.int32)
        self._chk(self.lib.gnx_circuit_potentials(
            *args, _ptr(anchor if n else None), _ptr(out if out.size else None)))
        return out, anchor

    def circuit_budget(self, n_bytes):
        """bytes of solver rasters one batch of systems may take (0: the default, 4 GiB)"""
        self._chk(self.lib.gnx_circuit_budget(self.h, int(n_bytes)))

    def circuit_info(self):
        """of the last circuit_matrix / circuit_current / circuit_potentials:
        dict(kernel_ms, launches, iterations, restarts, worst_residual)"""
        return self._outs(self.lib.gnx_circuit_info, ('kernel_ms', 'launches', 'iterations',
                                                      'restarts', 'worst_residual'))

    # -- fine-scale spatial genetic structure (csrc/gnx_sgs.hip) ---------------------------
    def sgs_sums(self, edges, slots=None, locus_mask=None, locus_weight=None, perm=None,
                 max_work=0):
        """the per-class sums over the pairs of `slots` (all living slots by default) closer
        than edges[-1] (include/gnx_hip.h, gnx_sgs_sums).  edges float64 [n_bins + 1];
        locus_weight float64 [L] or None; perm int32 [n] or None (individual i stands where it
        is with the genome of individual perm[i]).  max_work <= 0: only the work is computed.
        -> dict(work, isums int64 [n_bins][3], fsums float64 [n_bins][7], n_zero); isums,
        fsums and n_zero are None when max_work <= 0"""
        s, n = self._geno_slots(slots)
        m = self._locus_mask_words(locus_mask)
        e = _arr(edges, np.float64).ravel()
        nb = int(e.size) - 1
        wt = None
        if locus_weight is not None:
            wt = _arr(locus_weight, np.float64).ravel()
            if wt.size != self.L:
                raise ValueError('locus_weight: %d entries, not L = %d' % (wt.size, self.L))
        p = None
        if perm is not None:
            p = _arr(perm, np.int32).ravel()
            if p.size != n:
                raise ValueError('perm: [%d], not %s' % (n, p.shape))
        # (the library refuses n_bins outside 1..32 before it writes)
        rows = nb if 1 <= nb <= 32 else 0
        isums = np.zeros((rows, 3), np.int64)
        fsums = np.zeros((rows, 7), np.float64)
        work = np.zeros(1, np.int64)
        nz = np.zeros(1, np.int64)
        self._chk(self.lib.gnx_sgs_sums(
            self.h, n, _ptr(s), _ptr(m), max(nb, -1), _ptr(e if e.size else np.zeros(1)), _ptr(wt),
            _ptr(p), int(max_work), _ptr(work), _ptr(isums), _ptr(fsums), _ptr(nz)))
        if max_work <= 0:
            return dict(work=int(work[0]), isums=None, fsums=None, n_zero=None)
        return dict(work=int(work[0]), isums=isums, fsums=fsums, n_zero=int(nz[0]))

    # -- genome-wide linkage disequilibrium (csrc/gnx_ld.hip) ------------------------------
    def ld_bins(self, loci, pos, edges, slots=None, min_minor=1, morgans=False, max_work=0):
        """per bin of pos[j] - pos[i] the locus pairs and the sums of r^2, r^4, the distance and
        the drift weight over the kept pairs of `loci` (include/gnx_hip.h, gnx_ld_bins).  loci
        int32 [n_loci] distinct; pos float64 [n_loci] non-decreasing; edges float64 [2..65]
        ascending, the last may be inf.  max_work <= 0: only the work is computed.
        -> dict(work, c1 int64 [n_loci], pairs int64 [n_bins], sum_r2, sum_r4, sum_d, sum_w
        float64 [n_bins]); all but work are None when max_work <= 0"""
        s, n = self._geno_slots(slots)
        loci = _arr(loci, np.int32).ravel()
        pos = _arr(pos, np.float64).ravel()
        if pos.size != loci.size:
            raise ValueError('pos: %d entries for %d loci' % (pos.size, loci.size))
        e = _arr(edges, np.float64).ravel()
        nb = int(e.size) - 1
        rows = nb if 1 <= nb <= 64 else 0         # (the library refuses the rest before it writes)
        c1 = np.zeros(loci.size, np.int64)
        pairs = np.zeros(rows, np.int64)
        fs = np.zeros((rows, 4), np.float64)
        work = np.zeros(1, np.int64)
        self._chk(self.lib.gnx_ld_bins(
            self.h, n, _ptr(s), int(loci.size), _ptr(loci if loci.size else np.zeros(1, np.int32)),
            _ptr(pos if pos.size else np.zeros(1)), int(e.size), _ptr(e if e.size else np.zeros(1)),
            int(min_minor), int(bool(morgans)), int(max_work), _ptr(work), _ptr(c1), _ptr(pairs),
            _ptr(fs)))
        if max_work <= 0:
            return dict(work=int(work[0]), c1=None, pairs=None, sum_r2=None, sum_r4=None,
                        sum_d=None, sum_w=None)
        return dict(work=int(work[0]), c1=c1, pairs=pairs, sum_r2=fs[:, 0].copy(),
                    sum_r4=fs[:, 1].copy(), sum_d=fs[:, 2].copy(), sum_w=fs[:, 3].copy())

    def ld_budget(self, n_bytes):
        """bytes of transposed bit rows ld_bins keeps resident (0: the default, 256 MiB)"""
        self._chk(self.lib.gnx_ld_budget(self.h, int(n_bytes)))

    def ld_info(self):
        """of the last ld_bins: dict(kernel_ms, launches, locus_blocks)"""
        return self._outs(self.lib.gnx_ld_info, ('kernel_ms', 'launches', 'locus_blocks'))

    # -- windowed linkage disequilibrium (csrc/gnx_ldwin.hip) --------------------------------
    def ld_window(self, loci, pos, window, slots=None, min_minor=1, r2_min=0.0, max_edges=0,
                  max_work=0, scores=True):
        """per locus of `loci` the kept loci within `window` of it (partners) and the sum of its
        r^2 with them (score), and with max_edges > 0 the in-window pairs with r^2 >= r2_min,
        sorted by (ei, ej) (include/gnx_ldwin.h, gnx_ld_window).  loci int32 [n_loci] distinct;
        pos float64 [n_loci] non-decreasing; window >= 0, inf allowed.  scores=False: the edges
        only.  max_work <= 0: only the work is computed.  More pairs than max_edges: GnxError
        with the attribute n_found
        -> dict(work, c1, partners int64 [n_loci], score float64 [n_loci], n_edges, ei, ej int32
        [n_edges], er2 float64 [n_edges]); partners and score are None without scores, the edge
        entries None with max_edges = 0, all but work None when max_work <= 0"""
        s, n = self._geno_slots(slots)
        loci = _arr(loci, np.int32).ravel()
        pos = _arr(pos, np.float64).ravel()
        if pos.size != loci.size:
            raise ValueError('pos: %d entries for %d loci' % (pos.size, loci.size))
        max_edges = int(max_edges)
        run = max_work > 0
        edges = run and 0 < max_edges <= 2 ** 26      # (the library refuses the rest)
        c1 = np.zeros(loci.size, np.int64)
        partners = np.zeros(loci.size, np.int64) if scores else None
        score = np.zeros(loci.size, np.float64) if scores else None
        k = max_edges if edges else 1
        ei, ej, er2 = np.empty(k, np.int32), np.empty(k, np.int32), np.empty(k, np.float64)
        work, nf = np.zeros(1, np.int64), np.zeros(1, np.int64)
        try:
            self._chk(self.lib.gnx_ld_window(
                self.h, n, _ptr(s), int(loci.size),
                _ptr(loci if loci.size else np.zeros(1, np.int32)),
                _ptr(pos if pos.size else np.zeros(1)), float(window), int(min_minor),
                float(r2_min), max_edges, int(max_work), _ptr(work), _ptr(c1), _ptr(partners),
                _ptr(score), _ptr(nf), _ptr(ei), _ptr(ej), _ptr(er2)))
        except GnxError as err:
            if 'exceed max_edges' in str(err):
                err.n_found = int(nf[0])
            raise
        out = dict(work=int(work[0]), c1=None, partners=None, score=None, n_edges=None, ei=None,
                   ej=None, er2=None)
        if not run:
            return out
        out.update(c1=c1, partners=partners, score=score)
        if edges:
            k = int(nf[0])
            out.update(n_edges=k, ei=ei[:k].copy(), ej=ej[:k].copy(), er2=er2[:k].copy())
        return out

    def ld_window_info(self):
        """of the last ld_window: dict(kernel_ms, launches, locus_blocks)"""
        return self._outs(self.lib.gnx_ld_window_info, ('kernel_ms', 'launches', 'locus_blocks'))

    # -- model-based ancestry (csrc/gnx_admix.hip) -------------------------------------------
    def admix_sweep(self, Q, F, slots=None, locus_mask=None, want_loglik=True, budget=None,
                    want_B=True):
        """one EM sweep of the admixture model (include/gnx_hip.h, gnx_admix_sweep): Q torch
        fp64 [n][K] and F torch fp64 [K][L] on the handle's device -> dict(A [n][K], B1 [K][L],
        B0 [K][L] torch fp64 on the device, loglik float or None).  want_B=False (F held fixed)
        skips B1 and B0 (None); budget: bytes of partial sums per chunk of individuals (None:
        the default).  The call waits for the current torch stream before it reads Q and F and
        returns with the outputs complete."""
        import torch
        for t, name in ((Q, 'Q'), (F, 'F')):
            if not torch.cuda.is_available():
                raise GnxError('torch sees no HIP device: initialise it (torch.cuda.init()) '
                               'before the first Device is created, as bench.py does')
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2:
                raise ValueError('%s: a 2-d torch tensor on the device' % name)
        Q = Q.to(torch.float64).contiguous()
        F = F.to(torch.float64).contiguous()
        s, n = self._geno_slots(slots)
        K = int(Q.shape[1])
        if Q.shape[0] != n:
            raise ValueError('Q: %d rows, not n = %d' % (Q.shape[0], n))
        if F.shape[0] != K or F.shape[1] != self.L:
            raise ValueError('F: %s, not (K, L) = (%d, %d)' % (tuple(F.shape), K, self.L))
        m = self._locus_mask_words(locus_mask)
        A = torch.empty((n, K), dtype=torch.float64, device=Q.device)
        B1 = B0 = None
        if want_B:
            B1 = torch.empty((K, self.L), dtype=torch.float64, device=Q.device)
            B0 = torch.empty((K, self.L), dtype=torch.float64, device=Q.device)
        ll = C.c_double(0.0)
        torch.cuda.current_stream(Q.device).synchronize()
        self._chk(self.lib.gnx_admix_sweep(
            self.h, n, _ptr(s), _ptr(m), K, _dev_ptr(Q), _dev_ptr(F), _dev_ptr(A), _dev_ptr(B1),
            _dev_ptr(B0), C.byref(ll) if want_loglik else None, 0 if want_B else 1,
            int(budget or 0)))
        return dict(A=A, B1=B1, B0=B0, loglik=float(ll.value) if want_loglik else None)

    def admix_info(self):
        """of the last admix_sweep: dict(kernel_ms, launches, chunks (over the individuals),
        instance (the K of the template instance that ran))"""
        return self._outs(self.lib.gnx_admix_info, ('kernel_ms', 'launches', 'chunks', 'instance'))

    # -- local ancestry along the genome (csrc/gnx_lai.hip) ------------------------------------
    def lai_paint(self, F, sw, stay, Q, slots=None, loci=None, by=None, n_groups=0, budget=None,
                  want_post=True, want_calls=False):
        """the linkage model painted along every haplotype of `slots` (all living slots by
        default, in the order given; include/gnx_hip.h, gnx_lai_paint): F fp64 [L_u][K], sw and
        stay fp64 [L_u], Q fp64 [n][K]; loci int32 [L_u] ascending (None: all L); by int32 [n]
        labels in -1..n_groups-1 or None; budget: bytes of device scratch per batch of
        haplotypes (None: the default)
        -> dict(loglik fp64 [2n], anc_hap fp64 [2n][K], anc_locus fp64 [max(n_groups, 1)][L_u][K],
        switches int32 [2n], calls uint8 [2n][L_u] or None, batches, kernel_ms); with
        want_post=False only loglik (the others None)"""
        s, n = self._geno_slots(slots)
        F = _arr(F, np.float64)
        if F.ndim != 2:
            raise ValueError('F: an array [L_u][K]')
        L_u, K = int(F.shape[0]), int(F.shape[1])
        sw, stay, Q = _arr(sw, np.float64).ravel(), _arr(stay, np.float64).ravel(), \
            _arr(Q, np.float64)
        if sw.size != L_u or stay.size != L_u:
            raise ValueError('sw, stay: %d and %d entries, not L_u = %d' % (sw.size, stay.size,
                                                                           L_u))
        if Q.shape != (n, K):
            raise ValueError('Q: %s, not (n, K) = (%d, %d)' % (Q.shape, n, K))
        lo = None
        if loci is not None:
            lo = _arr(loci, np.int32).ravel()
            if lo.size != L_u:
                raise ValueError('loci: %d entries, not L_u = %d' % (lo.size, L_u))
        b = None
        if by is not None:
            b = _arr(by, np.int32).ravel()
            if b.size != n:
                raise ValueError('by: %d labels, not n = %d' % (b.size, n))
        post, wc = bool(want_post), bool(want_calls)
        n_g = max(int(n_groups), 1)
        # (the library refuses n < 1 and K outside 1..8 before it writes)
        T = 2 * max(n, 0)
        ll = np.zeros(max(T, 1))
        ah = np.zeros((T, K)) if post else None
        al = np.zeros((n_g, L_u, K)) if post else None
        sn = np.zeros(max(T, 1), np.int32) if post else None
        calls = np.zeros((T, L_u), np.uint8) if post and wc else None
        nb, ms = C.c_int64(0), C.c_double(0.0)
        self._chk(self.lib.gnx_lai_paint(
            self.h, n, _ptr(s), K, L_u, _ptr(lo), _ptr(F), _ptr(sw), _ptr(stay), _ptr(Q), _ptr(b),
            int(n_groups), int(budget or 0), int(post), int(wc), _ptr(ll), _ptr(ah), _ptr(al),
            _ptr(sn), _ptr(calls), C.byref(nb), C.byref(ms)))
        return dict(loglik=ll[:T], anc_hap=ah, anc_locus=al,
                    switches=None if sn is None else sn[:T], calls=calls,
                    batches=int(nb.value), kernel_ms=ms.value)

    # -- per-locus association scans (csrc/gnx_assoc.hip) --------------------------------------
    def assoc_cross(self, Y, slots=None):
        """D^T Y in fp64 and the integer moments of the dosages of `slots` (all living slots by
        default, in the order given; include/gnx_hip.h, gnx_assoc_cross): Y fp64 [n][m] (or [n])
        on the host, finite, 1 <= m <= 32
        -> dict(DtY fp64 [L][m], s1 int64 [L] = sum d, s2 int64 [L] = sum d^2, stretch,
        stretches (the summation order: sim/assoc.stretch_rule), kernel_ms)"""
        s, n = self._geno_slots(slots)
        Y = _arr(Y, np.float64)
        if Y.ndim == 1:
            Y = Y[:, None]
        if Y.ndim != 2 or Y.shape[0] != n:
            raise ValueError('Y: %s, not [n = %d][m]' % (Y.shape, n))
        m = int(Y.shape[1])
        # (the library refuses m outside 1..32 before it writes)
        mo = m if 1 <= m <= 32 else 0
        out = np.zeros((self.L, mo))
        s1, s2 = np.zeros(self.L, np.int64), np.zeros(self.L, np.int64)
        per, cnt, ms = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        self._chk(self.lib.gnx_assoc_cross(
            self.h, n, _ptr(s), m, _ptr(Y), _ptr(out), _ptr(s1), _ptr(s2), C.byref(per),
            C.byref(cnt), C.byref(ms)))
        return dict(DtY=out, s1=s1, s2=s2, stretch=int(per.value), stretches=int(cnt.value),
                    kernel_ms=ms.value)

    def assoc_quad(self, val, M, slots=None, locus_mask=None):
        """q[l] = sum over the rows k of M of (sum_i M[k][i] val[l][d_il])^2 for the dosages of
        `slots` (all living slots by default, in the order given; at most 8192) at the loci of the
        mask (include/gnx_hip.h, gnx_assoc_quad): val fp32 [L][3] as grm's, M fp32 [m][n] on the
        host, finite, 1 <= m <= 8192 -> dict(q fp64 [L], 0 outside the mask; kernel_ms)"""
        s, n = self._geno_slots(slots)
        mk = self._locus_mask_words(locus_mask)
        v = self._val_table(val)
        M = _arr(M, np.float32)
        if M.ndim != 2 or M.shape[1] != n:
            raise ValueError('M: %s, not [m][n = %d]' % (M.shape, n))
        out = np.zeros(self.L, np.float64)
        ms = C.c_double(0.0)
        self._chk(self.lib.gnx_assoc_quad(
            self.h, n, _ptr(s), _ptr(mk), _ptr(v), int(M.shape[0]), _ptr(M), _ptr(out),
            C.byref(ms)))
        return dict(q=out, kernel_ms=ms.value)

    # -- the sums of a Newton step of m logistic fits (csrc/gnx_glm.hip) ---------------------
    def glm_sweep(self, X, B, info=False):
        """per fit k the sums [s, A, I] of a binomial GLM with the logit link at the coefficients
        B[k] over the design X (include/gnx_glm.h, gnx_glm_sweep): X fp64 [n][p], B fp64 [m][p]
        on the host, finite, 1 <= p <= 8 -> (sums fp64 [m][1 + p + p (p + 1) / 2], kernel_ms);
        info: a dict(sums, kernel_ms, stretch, stretches (the summation order:
        sim/glm.stretch_rule)) instead"""
        X = _arr(X, np.float64)
        B = _arr(B, np.float64)
        if X.ndim != 2 or B.ndim != 2 or X.shape[1] != B.shape[1]:
            raise ValueError('X [n][p] and B [m][p] (got %s and %s)' % (X.shape, B.shape))
        (n, p), m = X.shape, int(B.shape[0])
        # (the library refuses p outside 1..8 before it writes)
        out = np.zeros((m, 1 + p + p * (p + 1) // 2 if 1 <= p <= 8 else 0))
        per, cnt, ms = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        self._chk(self.lib.gnx_glm_sweep(self.h, n, p, _ptr(X), m, _ptr(B), _ptr(out),
                                         C.byref(per), C.byref(cnt), C.byref(ms)))
        if info:
            return dict(sums=out, kernel_ms=ms.value, stretch=int(per.value),
                        stretches=int(cnt.value))
        return out, ms.value

    def glm_budget(self, n_bytes):
        """bytes of device scratch one batch of fits of glm_sweep may take (0: the default)"""
        self._chk(self.lib.gnx_glm_budget(self.h, int(n_bytes)))

    # -- identity tracts of the phased genomes (csrc/gnx_tracts.hip) ------------------------
    def _tract_args(self, pos, brk, edges):
        pos = _arr(pos, np.int64).ravel()
        if pos.size != self.L:
            raise ValueError('pos: %d entries, not L = %d' % (pos.size, self.L))
        b = None
        if brk is not None:
            b = _arr(brk, np.uint64).ravel()
            if b.size != self.W64:
                raise ValueError('brk: %d words, not %d' % (b.size, self.W64))
        e, hist = None, None
        if edges is not None:
            e = _arr(edges, np.int64).ravel()
            # (the library refuses fewer than 2 and more than 65 edges before it writes)
            hist = np.zeros((e.size - 1 if 2 <= e.size <= 65 else 1, 2), np.int64)
            if e.size == 0:
                e = np.zeros(1, np.int64)
        return pos, b, e, hist

    def tracts_self(self, pos, brk=None, min_loci=1, min_len=0, edges=None, slots=None,
                    cover=False):
        """runs of homozygosity: the tracts over which homologue 0 and homologue 1 of each of
        `slots` (all living slots by default) are identical (include/gnx_hip.h,
        gnx_tracts_self).  pos int64 [L] non-decreasing; brk uint64 [W64] or None; edges int64
        [2..65] ascending or None
        -> dict(per int64 [n][4] = {tracts, loci, length, longest}, hist int64 [n_bins][2] or
        None, cover int64 [L] or None)"""
        s, n = self._geno_slots(slots)
        pos, b, e, hist = self._tract_args(pos, brk, edges)
        # (the library refuses n outside 1..2^25 before it writes)
        per = np.zeros((n if 1 <= n <= 2 ** 25 else 1, 4), np.int64)
        cov = np.zeros(self.L, np.int64) if cover else None
        self._chk(self.lib.gnx_tracts_self(
            self.h, n, _ptr(s), _ptr(pos), _ptr(b), int(min_loci), int(min_len),
            0 if edges is None else int(np.size(edges)), _ptr(e), _ptr(per), _ptr(hist), _ptr(cov)))
        return dict(per=per, hist=hist, cover=cov)

    def tracts_pairs(self, pos, brk=None, min_loci=1, min_len=0, edges=None, slots=None,
                     cover=False, max_work=0):
        """tracts shared between the haplotypes of every two of `slots` (at most 4096;
        include/gnx_hip.h, gnx_tracts_pairs); the diagonal is the individual's own pair.
        max_work <= 0: only the work is computed
        -> dict(work, cnt int32 [n][n], len, longest int64 [n][n], hist, cover); all but work
        are None when max_work <= 0"""
        s, n = self._geno_slots(slots)
        pos, b, e, hist = self._tract_args(pos, brk, edges)
        run = max_work > 0 and 1 <= n <= 4096
        m = n if run else 1
        cnt = np.zeros((m, m), np.int32)
        tot = np.zeros((m, m), np.int64)
        longest = np.zeros((m, m), np.int64)
        cov = np.zeros(self.L, np.int64) if cover else None
        work = np.zeros(1, np.int64)
        self._chk(self.lib.gnx_tracts_pairs(
            self.h, n, _ptr(s), _ptr(pos), _ptr(b), int(min_loci), int(min_len),
            0 if edges is None else int(np.size(edges)), _ptr(e), int(max_work), _ptr(work),
            _ptr(cnt), _ptr(tot), _ptr(longest), _ptr(hist), _ptr(cov)))
        if max_work <= 0:
            return dict(work=int(work[0]), cnt=None, len=None, longest=None, hist=None,
                        cover=None)
        return dict(work=int(work[0]), cnt=cnt, len=tot, longest=longest, hist=hist, cover=cov)

    def tracts_info(self):
        """of the last tracts_self / tracts_pairs: dict(kernel_ms, launches, bytes_read)"""
        return self._outs(self.lib.gnx_tracts_info, ('kernel_ms', 'launches', 'bytes_read'))

    # -- close-kin pairs (csrc/gnx_kin.hip) ---------------------------------------------------
    def kin_matrix(self, slots=None, locus_mask=None):
        """the integers of KING-robust kinship for every two of `slots` (at most 8192;
        include/gnx_hip.h, gnx_kin_matrix)
        -> dict(nhet int32 [n], hh int32 [n][n], ibs0 int32 [n][n])"""
        s, n = self._geno_slots(slots)
        m = self._locus_mask_words(locus_mask)
        # (the library refuses n outside 1..8192 before it writes: no n x n buffer for that)
        k = n if 1 <= n <= 8192 else 0
        nhet = np.zeros(max(k, 1), np.int32)
        hh = np.zeros((k, k), np.int32)
        ib = np.zeros((k, k), np.int32)
        self._chk(self.lib.gnx_kin_matrix(
            self.h, n, _ptr(s), _ptr(m), _ptr(nhet), _ptr(hh if k else None),
            _ptr(ib if k else None)))
        return dict(nhet=nhet[:k], hh=hh, ibs0=ib)

    def kin_pairs(self, T, max_dist=None, slots=None, locus_mask=None, max_pairs=1 << 22,
                  max_work=0, out=None):
        """the pairs of `slots` (all living slots by default) closer than max_dist (None: every
        pair) that the integer rule keeps at threshold T = sim/kin.threshold(min_kinship)
        (include/gnx_hip.h, gnx_kin_pairs), sorted by (pa, pb).  max_work <= 0: only the work is
        computed.  out: (pa, pb, hh, ibs0 int32 [max_pairs], nhet int32 [n]) to write into.
        More kept pairs than max_pairs: GnxError with the attribute n_found
        -> dict(work, n_candidates, n_found, pa, pb, hh, ibs0 int32 [n_found], nhet int32 [n]);
        all but work are None when max_work <= 0"""
        s, n = self._geno_slots(slots)
        m = self._locus_mask_words(locus_mask)
        max_pairs = int(max_pairs)
        run = max_work > 0 and 1 <= n <= 2 ** 24 and 1 <= max_pairs <= 2 ** 26
        if out is None:
            k = max_pairs if run else 1
            out = tuple(np.empty(k, np.int32) for _ in range(4)) + \
                (np.zeros(n if run else 1, np.int32),)
        pa, pb, hh, ib, nhet = out
        for a, size in ((pa, max_pairs), (pb, max_pairs), (hh, max_pairs), (ib, max_pairs),
                        (nhet, n)):
            if run and (a.dtype != np.int32 or a.size < size or not a.flags.c_contiguous):
                raise ValueError('out: contiguous int32 arrays of max_pairs (nhet: n) entries')
        work, nc, nf = (np.zeros(1, np.int64) for _ in range(3))
        try:
            self._chk(self.lib.gnx_kin_pairs(
                self.h, n, _ptr(s), _ptr(m), 0.0 if max_dist is None else float(max_dist), int(T),
                max_pairs, int(max_work), _ptr(work), _ptr(nc), _ptr(nf), _ptr(pa), _ptr(pb),
                _ptr(hh), _ptr(ib), _ptr(nhet)))
        except GnxError as err:
            if 'exceed max_pairs' in str(err):
                err.n_found = int(nf[0])
            raise
        if max_work <= 0:
            return dict(work=int(work[0]), n_candidates=None, n_found=None, pa=None, pb=None,
                        hh=None, ibs0=None, nhet=None)
        k = int(nf[0])
        return dict(work=int(work[0]), n_candidates=int(nc[0]), n_found=k, pa=pa[:k].copy(),
                    pb=pb[:k].copy(), hh=hh[:k].copy(), ibs0=ib[:k].copy(), nhet=nhet[:n])

    def kin_info(self):
        """of the last kin_matrix / kin_pairs: dict(kernel_ms, launches, tasks)"""
        return self._outs(self.lib.gnx_kin_info, ('kernel_ms', 'launches', 'tasks'))

    # -- haplotype sweep scans (csrc/gnx_sweeps.hip) -------------------------------------------
    def sweeps_scan(self, loci, pos, brk=None, cls=None, cores=None, slots=None, min_minor=2,
                    cut_num=0, cut_den=1, max_gap=0, max_extent=0, max_work=0, curve=False):
        """the area under the curve of identical haplotype pairs around core loci
        (include/gnx_hip.h, gnx_sweeps_scan).  loci int32 [n_loci] distinct; pos int64 [n_loci]
        non-decreasing; brk uint8 [n_loci] or None; cls uint8 [2 n] of 0 / 1 / 255 or None (the
        class is the allele at the core); cores: request indices or None (every kept locus).
        max_work <= 0: only the work and c1 are computed
        -> dict(work, c1 int64 [n_loci], area int64, steps int32, status uint8 [n_loci][2][2],
        curve int64 [2][2][n_loci] or None); all but work and c1 are None when max_work <= 0"""
        s, n = self._geno_slots(slots)
        loci = _arr(loci, np.int32).ravel()
        pos = _arr(pos, np.int64).ravel()
        if pos.size != loci.size:
            raise ValueError('pos: %d entries for %d loci' % (pos.size, loci.size))
        b = None
        if brk is not None:
            b = _arr(np.asarray(brk) != 0, np.uint8).ravel()
            if b.size != loci.size:
                raise ValueError('brk: %d entries for %d loci' % (b.size, loci.size))
        k = None
        if cls is not None:
            k = _arr(cls, np.uint8).ravel()
            if k.size != 2 * n:
                raise ValueError('cls: %d entries for %d chromosomes' % (k.size, 2 * n))
        co, n_cores = None, 0
        if cores is not None:
            co = _arr(cores, np.int32).ravel()
            n_cores = int(co.size)
            if n_cores == 0:
                co = np.zeros(1, np.int32)
        m = max(1, int(loci.size))
        c1 = np.zeros(m, np.int64)
        area = np.zeros((m, 2, 2), np.int64)
        steps = np.zeros((m, 2, 2), np.int32)
        status = np.zeros((m, 2, 2), np.uint8)
        cv = np.zeros((2, 2, m), np.int64) if curve else None
        work = np.zeros(1, np.int64)
        self._chk(self.lib.gnx_sweeps_scan(
            self.h, n, _ptr(s), int(loci.size), _ptr(loci if loci.size else np.zeros(1, np.int32)),
            _ptr(pos if pos.size else np.zeros(1, np.int64)), _ptr(b), _ptr(k), n_cores, _ptr(co),
            int(min_minor), int(cut_num), int(cut_den), int(max_gap), int(max_extent),
            int(max_work), _ptr(work), _ptr(c1), _ptr(area), _ptr(steps), _ptr(status), _ptr(cv)))
        if max_work <= 0:
            return dict(work=int(work[0]), c1=c1, area=None, steps=None, status=None, curve=None)
        return dict(work=int(work[0]), c1=c1, area=area, steps=steps, status=status, curve=cv)

    def sweeps_info(self):
        """of the last sweeps_scan: dict(kernel_ms, launches, steps_total)"""
        return self._outs(self.lib.gnx_sweeps_info, ('kernel_ms', 'launches', 'steps_total'))

    # -- lineages through the recorded pedigree (csrc/gnx_lineage.hip) -------------------
    @staticmethod
    def _ago(v, default, up):
        """a time-window bound as the int32 the library compares integers with"""
        if v is None:
            return default
        v = float(v)
        if v != v:
            raise ValueError('a time-window bound is NaN')
        v = np.ceil(v) if up else np.floor(v)
        return int(min(max(v, -2 ** 31), 2 ** 31 - 1))

    def _lineage_args(self, node_tab, birth_t, nodes, loci, t_curr, drop_before_sim,
                      min_time_ago, max_time_ago):
        tab = _arr(node_tab, np.int32)
        bt = _arr(birth_t, np.int32).ravel()
        if tab.ndim != 2 or tab.shape != (2 * bt.size, 2):
            raise ValueError('node_tab: int32 [2 n_rows][2] with birth_t [n_rows]')
        nodes = _arr(nodes, np.int32).ravel()
        loci = _arr(loci, np.int32).ravel()
        keep = (tab, bt, nodes, loci)
        args = (self.h, bt.size, _ptr(tab), _ptr(bt), nodes.size, _ptr(nodes), int(loci.size),
                _ptr(loci), int(t_curr), int(bool(drop_before_sim)),
                self._ago(min_time_ago, -2 ** 31, True), self._ago(max_time_ago, 2 ** 31 - 1, False))
        return keep, args, (int(loci.size), int(nodes.size))

    def lineage_trace(self, node_tab, birth_t, nodes, loci, t_curr, drop_before_sim=True,
                      min_time_ago=None, max_time_ago=None,
                      want=('root', 'first', 'last', 'n_kept'), locus_range=True):
        """gnx_lineage_trace: the lineages of the sample `nodes` at `loci` through the pedigree
        (TreeTables.node_table()).  -> dict of the int32 [n_loci][n_nodes] arrays named in
        `want`, plus 'locus_lo' / 'locus_hi' int32 [n_loci] (min / max of `last` over the
        sample) if locus_range"""
        bad = set(want) - {'root', 'first', 'last', 'n_kept'}
        if bad:
            raise ValueError('want: unknown output %s' % sorted(bad))
        keep, args, shape = self._lineage_args(node_tab, birth_t, nodes, loci, t_curr,
                                               drop_before_sim, min_time_ago, max_time_ago)
        out = {k: np.full(shape, -1, np.int32) for k in ('root', 'first', 'last', 'n_kept')
               if k in want}
        if locus_range:
            out['locus_lo'] = np.zeros(shape[0], np.int32)
            out['locus_hi'] = np.zeros(shape[0], np.int32)
        self._chk(self.lib.gnx_lineage_trace(
            *args, *[_ptr(out.get(k))
                     for k in ('root', 'first', 'last', 'n_kept', 'locus_lo', 'locus_hi')]))
        return out

    def lineage_chains(self, node_tab, birth_t, nodes, loci, t_curr, drop_before_sim=True,
                       min_time_ago=None, max_time_ago=None, n_kept=None):
        """gnx_lineage_chains: every kept node of every lineage, youngest first, in CSR form
        (offsets int64 [n_loci * n_nodes + 1], nodes int32); n_kept: that of a lineage_trace
        of the same request (taken here if not given)"""
        if n_kept is None:
            n_kept = self.lineage_trace(node_tab, birth_t, nodes, loci, t_curr, drop_before_sim,
                                        min_time_ago, max_time_ago, want=('n_kept',),
                                        locus_range=False)['n_kept']
        keep, args, shape = self._lineage_args(node_tab, birth_t, nodes, loci, t_curr,
                                               drop_before_sim, min_time_ago, max_time_ago)
        n_kept = np.asarray(n_kept)
        if n_kept.shape != shape:
            raise ValueError('n_kept: shape %s, not %s' % (n_kept.shape, shape))
        offsets = np.zeros(n_kept.size + 1, np.int64)
        np.cumsum(n_kept.ravel(), dtype=np.int64, out=offsets[1:])
        chain = np.zeros(int(offsets[-1]), np.int32)
        self._chk(self.lib.gnx_lineage_chains(*args, _ptr(offsets), _ptr(chain)))
        return offsets, chain

    def lineage_budget(self, n_bytes):
        """bytes of output per launch of the lineage calls (0: the default, 256 MiB)"""
        self._chk(self.lib.gnx_lineage_budget(self.h, int(n_bytes)))

    def lineage_info(self):
        """of the last lineage call: dict(kernel_ms, launches, uploaded)"""
        info = self._outs(self.lib.gnx_lineage_info, ('kernel_ms', 'launches', 'uploaded'))
        return dict(info, uploaded=bool(info['uploaded']))

    # -- simplification of the recorded pedigree (csrc/gnx_simplify.hip) ------------------
    def pedigree_reach(self, node_tab, birth_t, sample_rows, masks_of=None):
        """gnx_pedigree_reach: node_loci int32 [2 n_rows], the number of loci at which each node
        of the pedigree (TreeTables.node_table()) is an ancestor of the sample - both nodes of
        every row in `sample_rows`; 0: at none.  With masks_of (node ids) -> (node_loci, uint64
        [n][W64]): those nodes' ancestral loci as bit masks in the paths' layout"""
        tab = _arr(node_tab, np.int32)
        bt = _arr(birth_t, np.int32).ravel()
        if tab.ndim != 2 or tab.shape != (2 * bt.size, 2):
            raise ValueError('node_tab: int32 [2 n_rows][2] with birth_t [n_rows]')
        rows = _arr(sample_rows, np.int32).ravel()
        node_loci = np.zeros(2 * bt.size, np.int32)
        req = masks = None
        if masks_of is not None:
            req = _arr(masks_of, np.int32).ravel()
            masks = np.zeros((req.size, self.W64), np.uint64)
        n_req = 0 if req is None else int(req.size)
        self._chk(self.lib.gnx_pedigree_reach(
            self.h, bt.size, _ptr(tab), _ptr(bt), rows.size, _ptr(rows), _ptr(node_loci), n_req,
            _ptr(req if n_req else None), _ptr(masks if n_req else None)))
        return node_loci if masks_of is None else (node_loci, masks)

    def lineage_forget(self):
        """drop the device's copy of the node table: the next lineage call uploads its own"""
        self._chk(self.lib.gnx_lineage_forget(self.h))

    # -- pairwise coalescence through the recorded pedigree (csrc/gnx_coal.hip) -------------
    COAL_TIMES_OUT = ('pair_sum', 'pair_cnt', 'locus_sum', 'locus_cnt', 'locus_max', 'thist',
                      'mrca')

    def _coal_args(self, node_tab, birth_t, nodes, loci):
        tab = _arr(node_tab, np.int32)
        bt = _arr(birth_t, np.int32).ravel()
        if tab.ndim != 2 or tab.shape != (2 * bt.size, 2):
            raise ValueError('node_tab: int32 [2 n_rows][2] with birth_t [n_rows]')
        nodes = _arr(nodes, np.int32).ravel()
        loci = _arr(loci, np.int32).ravel()
        args = (self.h, bt.size, _ptr(tab), _ptr(bt), nodes.size, _ptr(nodes), int(loci.size),
                _ptr(loci))
        # (the library refuses fewer than 2 and more than 4096 nodes before it writes)
        n = int(nodes.size) if 2 <= nodes.size <= 4096 else 1
        return (tab, bt, nodes, loci), args, n, int(loci.size)

    def _coal_max_ago(self, max_time_ago):
        """max_time_ago (None: no limit) as the library's max_ago, where negative means none"""
        if max_time_ago is not None and not float(max_time_ago) >= 0:
            raise ValueError('max_time_ago: >= 0, or None for no limit (got %r)' % (max_time_ago,))
        return self._ago(max_time_ago, -1, False)

    def coal_times(self, node_tab, birth_t, nodes, loci, t_curr, max_time_ago=None,
                   time_edges=None, want=('pair_sum', 'pair_cnt', 'locus_sum', 'locus_cnt',
                                          'locus_max'), max_work=0):
        """gnx_coal_times (include/gnx_hip.h): the coalescence times of every two of the sample
        `nodes` (2..4096, distinct) at `loci` (any order) through the pedigree
        (TreeTables.node_table()).  max_time_ago None: no limit; time_edges int32 [2..65]
        ascending: 'thist' is computed too.  want: the outputs to compute ('mrca' int32
        [n_loci][n_pairs] on request only).  max_work <= 0: only the work is computed
        -> dict(work, and the arrays named in want, 'thist' with time_edges); without the arrays
        when max_work <= 0"""
        bad = set(want) - set(self.COAL_TIMES_OUT) | ({'thist'} & set(want))
        if bad:
            raise ValueError('want: unknown output %s (thist comes with time_edges)'
                             % sorted(bad))
        keep, args, n, nl = self._coal_args(node_tab, birth_t, nodes, loci)
        max_ago = self._coal_max_ago(max_time_ago)
        run = max_work > 0
        e = None
        out = {}
        if time_edges is not None:
            e = _arr(time_edges, np.int32).ravel()
            out['thist'] = np.zeros(e.size - 1 if 2 <= e.size <= 65 else 1, np.int64)
            if e.size == 0:
                e = np.zeros(1, np.int32)
        m, ml = (n, nl) if run else (1, 1)
        shapes = dict(pair_sum=((m, m), np.int64), pair_cnt=((m, m), np.int32),
                      locus_sum=((ml,), np.int64), locus_cnt=((ml,), np.int64),
                      locus_max=((ml,), np.int32), mrca=((ml, m * (m - 1) // 2), np.int32))
        for k in want:
            out[k] = np.zeros(*shapes[k])
        work = np.zeros(1, np.int64)
        self._chk(self.lib.gnx_coal_times(
            *args, int(t_curr), max_ago, 0 if time_edges is None else int(np.size(time_edges)),
            _ptr(e), int(max_work), _ptr(work), *[_ptr(out.get(k)) for k in self.COAL_TIMES_OUT]))
        if not run:
            return dict(work=int(work[0]))
        return dict(out, work=int(work[0]))

    def coal_segments(self, node_tab, birth_t, nodes, loci, pos, t_curr, brk=None,
                      max_time_ago=None, min_loci=1, min_len=0, edges=None, cover=False,
                      max_work=0):
        """gnx_coal_segments (include/gnx_hip.h): the stretches of the strictly ascending `loci`
        over which two of the sample `nodes` keep one most recent common ancestor no older than
        max_time_ago (identity by descent).  pos int64 [n_loci] non-decreasing; brk uint8
        [n_loci] or None; edges int64 [2..65] ascending or None.  max_work <= 0: only the work is
        computed
        -> dict(work, cnt int32 [n][n], len, longest int64 [n][n], hist, cover); all but work
        are None when max_work <= 0"""
        keep, args, n, nl = self._coal_args(node_tab, birth_t, nodes, loci)
        pos = _arr(pos, np.int64).ravel()
        if pos.size != nl:
            raise ValueError('pos: %d entries, not one per listed locus (%d)' % (pos.size, nl))
        b = None
        if brk is not None:
            b = _arr(brk, np.uint8).ravel()
            if b.size != nl:
                raise ValueError('brk: %d entries, not one per listed locus (%d)' % (b.size, nl))
        e, hist = None, None
        if edges is not None:
            e = _arr(edges, np.int64).ravel()
            hist = np.zeros((e.size - 1 if 2 <= e.size <= 65 else 1, 2), np.int64)
            if e.size == 0:
                e = np.zeros(1, np.int64)
        run = max_work > 0
        m = n if run else 1
        cnt = np.zeros((m, m), np.int32)
        tot = np.zeros((m, m), np.int64)
        longest = np.zeros((m, m), np.int64)
        cov = np.zeros(max(nl, 1), np.int64) if cover else None
        work = np.zeros(1, np.int64)
        self._chk(self.lib.gnx_coal_segments(
            *args, _ptr(pos), _ptr(b), int(t_curr), self._coal_max_ago(max_time_ago), int(min_loci),
            int(min_len), 0 if edges is None else int(np.size(edges)), _ptr(e), int(max_work),
            _ptr(work), _ptr(cnt), _ptr(tot), _ptr(longest), _ptr(hist), _ptr(cov)))
        if not run:
            return dict(work=int(work[0]), cnt=None, len=None, longest=None, hist=None,
                        cover=None)
        return dict(work=int(work[0]), cnt=cnt, len=tot, longest=longest, hist=hist, cover=cov)

    # -- introductions (csrc/gnx_transplant.hip) ----------------------------------------
    def transplant(self, src, slots, x, y, first_id):
        """append the individuals in `slots` of Device `src` (same GPU) to this one at
        (x[i], y[i]) with ids first_id + i, genomes block for block on the device
        (gnx_transplant).  -> dict(first_slot, blocks_copied, blocks_linked, collections).
        Raises GnxError with code 2, and changes nothing, when they do not fit."""
        if not isinstance(src, Device):
            raise TypeError('src: a Device')
        slots = _arr(slots, np.int64).ravel()
        x = _arr(x, np.float32).ravel()
        y = _arr(y, np.float32).ravel()
        if not (x.size == slots.size and y.size == slots.size):
            raise ValueError('slots, x and y: one entry per newcomer')
        out = np.zeros(4, np.int64)
        rc = self.lib.gnx_transplant(self.h, src.h, slots.size, _ptr(slots), _ptr(x), _ptr(y),
                                     int(first_id), _ptr(out))
        if rc:
            e = GnxError(self.lib.gnx_last_error().decode())
            e.code = int(rc)
            raise e
        return dict(zip(('first_slot', 'blocks_copied', 'blocks_linked', 'collections'),
                        (int(v) for v in out)))

    # -- measurement ---------------------------------------------------------
    def profiling(self, on):
        """0 off, 1 all kernel families, 2 only the dominant kernel (crossover)"""
        self._chk(self.lib.gnx_profiling(self.h, int(on)))

    def kernel_times(self):
        out = {}
        for k, name in enumerate(KERNELS):
            out[name] = self._outs(self.lib.gnx_kernel_time, ('ms', 'launches', 'bytes'), k)
        return out


def measure_copy(nbytes=8 << 30, reps=5):
    """GB/s (read + written) of the library's own 16-byte-per-lane copy kernel on the current
    device: the box's streaming rate beside the 8 TB/s of the data sheet"""
    lib = load()
    out = C.c_double()
    if lib.gnx_measure_copy(int(nbytes), int(reps), C.byref(out)):
        raise GnxError(lib.gnx_last_error().decode())
    return out.value


def step_many(devs, burn, with_selection):
    """one time step of several independent Devices (the iterations of one model), their
    kernels side by side on the handles' own streams (gnx_step_many)"""
    if not devs:
        return
    arr = (C.c_void_p * len(devs))(*[d.h for d in devs])
    devs[0]._chk(devs[0].lib.gnx_step_many(arr, len(devs), int(bool(burn)),
                                           int(bool(with_selection))))


def comm_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0 makes them, every rank joins with them)"""
    lib = load()
    buf = (C.c_uint8 * 128)()
    if lib.gnx_comm_unique_id(buf):
        raise GnxError(lib.gnx_last_error().decode())
    return bytes(buf)


def comm_probe():
    """librccl can be loaded and has every entry point the tile transport uses (raises GnxError
    otherwise): what the ranks agree on BEFORE any of them enters Device.comm_init_rccl"""
    lib = load()
    if lib.gnx_comm_probe():
        raise GnxError(lib.gnx_last_error().decode())


def comm_local_create(world):
    """meeting point of `world` tiles that live in this process (the one-GPU tests)"""
    lib = load()
    g = C.c_void_p()
    if lib.gnx_comm_local_create(int(world), C.byref(g)):
        raise GnxError(lib.gnx_last_error().decode())
    return g


def comm_local_abort(group):
    load().gnx_comm_local_abort(group)


def comm_local_destroy(group):
    load().gnx_comm_local_destroy(group)


def walk_many(devs, T, burn, with_selection):
    """T time steps of several independent Devices side by side (gnx_walk_many)"""
    if not devs:
        return
    arr = (C.c_void_p * len(devs))(*[d.h for d in devs])
    devs[0]._chk(devs[0].lib.gnx_walk_many(arr, len(devs), int(T), int(bool(burn)),
                                           int(bool(with_selection))))


def default_species_params(**kw):
    """SpeciesParams with the parameters-file template defaults
    (sim/params.py SPP_PARAMS)."""
    sp = SpeciesParams()
    sp.b = 0.2
    sp.R = 0.5
    sp.n_births_lambda = 1
    sp.n_births_fixed = 1
    sp.sexed = 0
    sp.p_male = 0.5
    sp.mating_radius = 10
    sp.mate_mode = MATE_UNIFORM
    sp.repro_age[0] = 0
    sp.repro_age[1] = 0
    sp.max_age = -1
    sp.d_min = 0
    sp.d_max = 1
    sp.window_width = -1
    sp.move = 1
    sp.dir_mu = 0
    sp.dir_kappa = 0
    sp.move_distr = DIST['lognormal']
    sp.move_p1 = 0.01
    sp.move_p2 = 0.5
    sp.disp_distr = DIST['lognormal']
    sp.disp_p1 = -1
    sp.disp_p2 = 0.05
    sp.move_surf = SURF_NONE
    sp.move_surf_layer = 0
    sp.move_surf_kappa = 12
    sp.disp_surf = SURF_NONE
    sp.disp_surf_layer = 0
    sp.disp_surf_kappa = 12
    sp.res_ratio[0] = 1
    sp.res_ratio[1] = 1
    sp.K_layer = 0
    sp.K_factor = 1
    for k, v in kw.items():
        if k == 'repro_age':
            sp.repro_age[0], sp.repro_age[1] = v
        elif k == 'res_ratio':
            sp.res_ratio[0], sp.res_ratio[1] = v
        else:
            if not hasattr(sp, k):
                raise AttributeError(k)
            setattr(sp, k, v)
    return sp
