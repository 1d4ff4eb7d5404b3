"""SpeciesAnalyses: the host side of a Species' analysis calls (the Model's calc_* and run_*
delegate here), as a mixin of structs/species.py's Species.  Each call checks its request,
hands the packed genomes' work to the device and finishes in sim/*.py; none is on the step
path.  The class keeps no state: it reads the Species' handle, architecture, generator and
landscape.  A new analysis takes its request checks from the functions above the class and,
until it works over tiles, gets a line in structs/tiled.py's table of refusals.
"""
import numpy as np

from .. import _native as nat


_COST_OPTS = ('lyr', 'kind', 'barrier', 'cost', 'name')
# the matrix predictors (solved over the landscape's raster, not device columns) and their options
_MATRIX_OPTS = {'cost': _COST_OPTS,
                'circuit': ('lyr', 'kind', 'barrier', 'cost', 'tol', 'max_iter', 'name')}


def _is_cost_spec(p):
    return (isinstance(p, (tuple, list)) and len(p) == 2 and isinstance(p[0], str)
            and p[0] in _MATRIX_OPTS and isinstance(p[1], dict))


def _predictor_list(predictors):
    """the predictors of a Mantel / MMRR request as a list: one name, or one ('cost', opts) or
    ('circuit', opts), stands for itself"""
    if isinstance(predictors, str) or _is_cost_spec(predictors):
        return [predictors]
    return list(predictors)


def _split_predictors(spp, who, predictors, env_lyrs, trts):
    """(names in the caller's order, the device columns of the column predictors in that order
    (Species._dist_predictors), [(name, kind, opts)] of the matrix predictors in that order).  A
    matrix predictor is 'cost' (the defaults of calc_cost_distances) or ('cost', opts) with any
    of lyr, kind, barrier, cost, name, or 'circuit' (the defaults of calc_resistance_distances)
    or ('circuit', opts) with those and tol, max_iter; its name is opts['name'], default its
    kind"""
    names, col_names, costs = [], [], []
    for p in _predictor_list(predictors):
        if isinstance(p, str) and p in _MATRIX_OPTS:
            p = (p, {})
        if _is_cost_spec(p):
            what, opts = p[0], dict(p[1])
            extra = sorted(set(opts) - set(_MATRIX_OPTS[what]))
            if extra:
                raise ValueError("%s: a '%s' predictor takes %s, not %s"
                                 % (who, what, ', '.join(_MATRIX_OPTS[what]), ', '.join(extra)))
            name = str(opts.pop('name', what))
            costs.append((name, what, opts))
            names.append(name)
        else:
            col_names.append(p)
            names.append(p)
    cols = []
    if col_names or not costs:
        _, cols = spp._dist_predictors(who, col_names, env_lyrs, trts)
    if len(set(names)) != len(names):
        raise ValueError('%s: a predictor is listed twice' % who)
    if len(names) > 4:
        raise ValueError('%s: at most 4 predictors and 8 columns (layers, traits, x, y) '
                         'together' % who)
    return names, cols, costs


def _solver_opts(who, tol, max_iter):
    """refuse a tolerance or an iteration limit the circuit solver cannot take"""
    if tol is not None and not (np.isfinite(tol) and tol > 0):
        raise ValueError('%s: tol: a positive relative residual (got %r)' % (who, tol))
    if max_iter is not None and (isinstance(max_iter, bool) or int(max_iter) != max_iter
                                 or max_iter < 1):
        raise ValueError('%s: max_iter: at least 1 iteration (got %r)' % (who, max_iter))


def _newton_opts(who, tol, max_iter):
    """refuse a tolerance or an iteration limit the Newton iteration of sim/glm.fit cannot take"""
    try:
        ok = not isinstance(tol, bool) and 0 < float(tol) < 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('%s: tol: a relative step in (0, 1) (got %r)' % (who, tol))
    try:
        ok = not isinstance(max_iter, bool) and int(max_iter) == max_iter and max_iter >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('%s: max_iter: at least 1 iteration (got %r)' % (who, max_iter))


# -- the request checks the analyses share: functions of the Species like _split_predictors, not
# methods, so that an object that borrows single analysis methods of the class can run them -----
def _need_genomes(spp, who=None, assigned=True):
    """refuse a Species without genomes and, with assigned, one whose genomes the burn-in
    has not assigned yet (looked up in __dict__: Species.__getattr__ falls through to the
    parameter block)"""
    pre = '%s: ' % who if who else ''
    if spp.gen_arch is None or spp._dev.L == 0:
        raise ValueError(pre + 'the Species has no genomes (no gen_arch)')
    if assigned and not spp.__dict__.get('_genomes_assigned', False):
        raise ValueError(pre + 'genomes are assigned at the end of the burn-in; burn the '
                         'model in first')


def _work_limit(who, max_work, default, what):
    """max_work (None: default) as a positive integer of the unit `what`"""
    if max_work is None:
        max_work = default
    if isinstance(max_work, bool) or int(max_work) != max_work or max_work < 1:
        raise ValueError('%s: max_work: a positive number of %s (got %r)'
                         % (who, what, max_work))
    return int(max_work)


def _within_max_work(who, call, advice):
    """call(); the library's refusal of a request above max_work (it comes before anything
    is launched) becomes a ValueError with advice"""
    try:
        return call()
    except nat.GnxError as err:
        if 'exceed max_work' not in str(err):
            raise
        raise ValueError('%s: %s: %s' % (who, err, advice)) from None


def _rec_rates(spp):
    """the architecture's recombination rates as a dense array over the loci"""
    rec = spp.gen_arch.recombinations
    rates = np.zeros(spp._dev.L)
    rates[rec._positions] = rec._rates
    return rates


def _torch_device(spp):
    import torch
    return torch.device('cuda', int(spp._dev.cfg.device))


def _distance_classes(spp, who, edges, n_classes, max_dist):
    """the checked bounds of the distance classes: edges, or n_classes classes of equal
    width in ln r from one landscape cell to max_dist (a quarter of the shorter side)"""
    from ..sim import sgs as _sgs
    if edges is None:
        dim = spp._land_ref.dim
        hi = min(dim) / 4.0 if max_dist is None else float(max_dist)
        edges = _sgs.default_edges(1.0, hi, n_classes)
    elif max_dist is not None:
        raise ValueError('%s: give edges or max_dist, not both' % who)
    return _sgs.check_edges(edges)


def _need_pedigree(spp, who):
    """refuse a Species that recorded no pedigree"""
    if spp._tt is None:
        raise ValueError("%s: no pedigree was recorded for this Species ('use_tskit' False, "
                         "or the genomes were not assigned yet)" % who)


def _tract_hist(edges, hist, unit):
    """the tract-length histogram of a tract call, as the caller gave its edges"""
    from ..sim import tracts as _tr
    return dict(edges=np.asarray(edges, dtype=np.float64).ravel(),
                tracts=hist[:, 0].copy(), sum_len=_tr.from_units(hist[:, 1], unit))


class SpeciesAnalyses:
    # -- genetic PCA and distances (sim/pca.py; csrc/gnx_geno.hip) -----------------------
    def _geno_sample(self, individs):
        """(ids ascending, their slots) of the listed living individuals (all by default)"""
        all_ids = self._field(nat.F_ID)
        order = np.argsort(all_ids, kind='stable')
        srt = all_ids[order]
        if individs is None:
            return srt, order.astype(np.int64)
        ids = np.sort(np.asarray(individs, dtype=np.int64).ravel())
        if (np.diff(ids) == 0).any():
            raise ValueError('individs lists an individual more than once')
        pos = np.searchsorted(srt, ids)
        alive = pos < srt.size
        alive[alive] = srt[pos[alive]] == ids[alive]
        if not alive.all():
            raise ValueError('individuals not alive: %s' % ids[~alive][:10].tolist())
        return ids, order[pos].astype(np.int64)

    def _geno_loci(self, loci):
        """(ascending loci, uint64 [W64] bit mask of them), or (None, None) for all loci"""
        if loci is None:
            return None, None
        L = self._dev.L
        loci = np.unique(np.asarray(loci, dtype=np.int64).ravel())
        if loci.size == 0 or loci[0] < 0 or loci[-1] >= L:
            raise ValueError('loci: a non-empty list of loci in 0..%d' % (L - 1))
        mask = np.zeros(self._dev.W64, np.uint64)
        np.bitwise_or.at(mask, loci >> 6, np.uint64(1) << (loci & 63).astype(np.uint64))
        return loci, mask

    # -- Fst, diversity and the SFS of groups of individuals (sim/fst.py;
    # csrc/gnx_group_counts.hip) --------------------------------------------------------
    def _group_counts(self, groups, loci=None):
        """per-group locus counts taken on the device (gnx_stats_group_counts): groups as
        sim/fst.make_groups takes them (a dict name -> ids, or integer labels aligned with the
        living in id order; negative: left out); loci selects columns on the host
        -> (names, n [G], cnt1 [G][L'], cnt_het [G][L'])"""
        from ..sim import fst as _fst
        _need_genomes(self, assigned=False)
        ids, slots = self._geno_sample(None)
        names, order, group_start = _fst.make_groups(ids, groups)
        if len(names) > 1024:
            raise ValueError('at most 1024 groups per call (got %d)' % len(names))
        cnt1, cnt_het = self._dev.stats_group_counts(slots[order], group_start)
        if loci is not None:
            loci = np.asarray(loci, dtype=np.int64).ravel()
            if loci.size == 0 or loci.min() < 0 or loci.max() >= self._dev.L:
                raise ValueError('loci: a non-empty list of loci in 0..%d' % (self._dev.L - 1))
            cnt1, cnt_het = cnt1[:, loci], cnt_het[:, loci]
        return names, np.diff(group_start), cnt1, cnt_het

    def _everybody(self, groups):
        return np.zeros(len(self), np.int64) if groups is None else groups

    def _calc_fst(self, groups, loci=None, method='HsHt', mean=True, est_Hs=False,
                  include_zeros=False):
        """Fst between groups of individuals from counts taken on the device.  'HsHt' (the
        reference's island validation, tests/validation/island/island_test.py:54-115) and
        'hudson' -> {(name_a, name_b): value}, keyed as calc_Fsts_mod keys its dict; the value
        is the nanmean over loci as there ('hudson': the ratio of averages), or with mean=False
        the per-locus array.  'var' -> one array over all groups, or its mean."""
        from ..sim import fst as _fst
        if method not in ('HsHt', 'hudson', 'var'):
            raise ValueError("method: 'HsHt', 'hudson' or 'var', not %r" % (method,))
        names, n, cnt1, cnt_het = self._group_counts(groups, loci)
        return _fst.calc_fst(names, n, cnt1, cnt_het, method=method, mean=mean, est_Hs=est_Hs,
                             include_zeros=include_zeros)

    def _calc_diversity(self, groups=None, loci=None):
        """per group (None: one group holding everybody): n, S, pi, theta_w, tajima_d, Ho, He,
        Fis (sim/fst.diversity) -> dict of arrays [G], and 'names'"""
        from ..sim import fst as _fst
        names, n, cnt1, cnt_het = self._group_counts(self._everybody(groups), loci)
        out = _fst.diversity(cnt1, cnt_het, n)
        out['names'] = names
        return out

    def _calc_sfs(self, groups=None, loci=None, folded=False):
        """site-frequency spectrum, one row per group (sim/fst.sfs) -> (names, sfs)"""
        from ..sim import fst as _fst
        names, n, cnt1, _ = self._group_counts(self._everybody(groups), loci)
        return names, _fst.sfs(cnt1, n, folded=folded)

    def _group_by_layer(self, lyr_num, edges):
        """labels of the living in id order by their environment on a Layer:
        np.digitize(e, edges) - 1, individuals outside the edges -1"""
        edges = np.asarray(edges, dtype=np.float64).ravel()
        if edges.size < 2 or (np.diff(edges) <= 0).any():
            raise ValueError('edges: at least two ascending values')
        lab = np.digitize(self._get_e(lyr_num=int(lyr_num)), edges) - 1
        lab[lab >= edges.size - 1] = -1
        return lab.astype(np.int64)

    def _group_by_grid(self, nx, ny):
        """labels of the living in id order by the rectangle of the landscape, cut into
        nx x ny by coordinate, they stand in: label = iy * nx + ix"""
        if int(nx) < 1 or int(ny) < 1:
            raise ValueError('nx, ny: at least 1')
        dim = self._land_ref.dim
        xy = self._get_coords()
        ix = np.clip((xy[:, 0] * (int(nx) / dim[0])).astype(np.int64), 0, int(nx) - 1)
        iy = np.clip((xy[:, 1] * (int(ny) / dim[1])).astype(np.int64), 0, int(ny) - 1)
        return iy * int(nx) + ix

    # -- moving-window diversity rasters (sim/divmap.py; csrc/gnx_divmap.hip) ----------------
    def _calc_diversity_map(self, grid=None, win=3, min_n=2, loci=None, individs=None):
        """rasters of n, S, pi, theta_w, tajima_d, Ho, He and Fis over overlapping windows of
        win x win map cells (sim/divmap.py holds the definition): grid (nx, ny) cuts the
        landscape as _group_by_grid does (None: (min(dim_x, 64), min(dim_y, 64))), win is odd,
        windows of fewer than min_n individuals are NaN; loci and individs restrict what is
        counted.  The four integers per window are taken on the device (gnx_divmap_sums)
        -> dict of [ny][nx] rasters, and 'grid', 'win', 'n_loci'"""
        from ..sim import divmap as _divmap
        _need_genomes(self, assigned=False)
        if int(win) != win or int(win) < 1 or int(win) % 2 == 0:
            raise ValueError('win: an odd number of map cells, at least 1 (got %r)' % (win,))
        if int(min_n) != min_n or int(min_n) < 1:
            raise ValueError('min_n: at least 1 (got %r)' % (min_n,))
        dim = self._land_ref.dim
        if grid is None:
            grid = (min(int(dim[0]), 64), min(int(dim[1]), 64))
        if len(grid) != 2 or int(grid[0]) < 1 or int(grid[1]) < 1:
            raise ValueError('grid: (nx, ny), each at least 1 (got %r)' % (grid,))
        nx, ny = int(grid[0]), int(grid[1])
        lab = self._group_by_grid(nx, ny)                 # the living in id order
        ids, slots = self._geno_sample(individs)
        if individs is not None:
            all_ids, _ = self._geno_sample(None)
            lab = lab[np.searchsorted(all_ids, ids)]
        loci, mask = self._geno_loci(loci)
        order = np.argsort(lab, kind='stable')
        cell_start = np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=nx * ny))])
        got = self._dev.divmap_sums(slots[order], cell_start.astype(np.int64), nx, ny,
                                    (int(win) - 1) // 2, locus_mask=mask)
        n_loci = int(self._dev.L if loci is None else loci.size)
        out = {'n': got['n'], 'S': got['S']}
        out.update(_divmap.window_stats(got['n'], got['S'], got['sum_het'], got['sum_cc'],
                                        n_loci, min_n=int(min_n)))
        out.update(grid=(nx, ny), win=int(win), n_loci=n_loci)
        return out

    def _calc_genetic_PCA(self, n_pcs=3, individs=None, loci=None, method='auto', n_iter=8,
                          oversample=10, seed=0):
        """PCA of the mean genotypes of the living individuals asked for (reference
        Model.plot_genetic_PCA, sim/model.py:2031-2041: sklearn PCA of the speciome, ids
        ascending), on the device.  method 'exact': the Gram matrix (gnx_geno_gram, up to
        8192 individuals) and eigh in fp64; 'randomized': subspace iteration over
        gnx_geno_matmul / gnx_geno_rmatmul (the whole population); 'auto': exact for
        n <= 8192.  -> (ids, scores [n][n_pcs], explained_variance_ratio [n_pcs])"""
        from ..sim import pca as _pca
        if method not in ('auto', 'exact', 'randomized'):
            raise ValueError("method: 'auto', 'exact' or 'randomized', not %r" % (method,))
        ids, slots = self._geno_sample(individs)
        if self._dev.L == 0:
            self._dev.geno_gram(slots[:1])            # the library's error: no genomes
        loci, mask = self._geno_loci(loci)
        n = ids.size
        n_pcs = _pca.check_n_pcs(n_pcs, n, self._dev.L if loci is None else loci.size,
                                 oversample)
        if method == 'auto':
            method = 'exact' if n <= 8192 else 'randomized'
        if method == 'randomized':
            if n != len(self):
                raise NotImplementedError(
                    'randomized genetic PCA of a subset of the individuals (its total variance '
                    'needs per-sample locus counts); use the exact method (up to 8192)')
            scores, ratio = _pca.device_randomized_pca(self._dev, n_pcs, loci=loci,
                                                       oversample=oversample, n_iter=n_iter,
                                                       seed=seed)
            return ids, scores[slots], ratio
        if n > 8192:
            raise ValueError('the exact genetic PCA takes at most 8192 individuals (got %d)' % n)
        import torch
        G = self._dev.geno_gram(slots, mask)
        tdev = _torch_device(self)

        def rmatmul(U):
            Z = self._dev.geno_rmatmul(torch.as_tensor(U, dtype=torch.float32, device=tdev),
                                       slots)
            return Z if loci is None else Z[torch.as_tensor(loci, device=tdev)]

        scores, ratio = _pca.pca_from_gram(G, n_pcs, rmatmul=rmatmul)
        return ids, scores, ratio

    def _calc_genetic_distances(self, individs=None, loci=None):
        """Euclidean distances between the mean genotypes of the living individuals asked for
        (reference demos/_IBD_IBE.py calc_dists, dist_type='gen', biallelic=False,
        return_flat=False): 0.5 sqrt(G_ii + G_jj - 2 G_ij) from the exact Gram matrix (up to
        8192 individuals).  -> (ids ascending, dist [n][n])"""
        ids, slots = self._geno_sample(individs)
        if ids.size > 8192:
            raise ValueError('genetic distances of at most 8192 individuals per call (got %d)'
                             % ids.size)
        if self._dev.L == 0:
            self._dev.geno_gram(slots[:1])            # the library's error: no genomes
        loci, mask = self._geno_loci(loci)
        G = self._dev.geno_gram(slots, mask)
        g = np.diag(G)
        return ids, 0.5 * np.sqrt((g[:, None] + g[None, :] - 2 * G).astype(np.float64))

    # -- genotype-environment association (sim/gea.py; csrc/gnx_gea.hip) -----------------
    def _gea_products(self, slots, loci, lyr_num):
        """what sim/gea.cca_from_cross_products takes, from the device: C, s (gnx_geno_locus_gram),
        DtZ, ZtZ, Zt1 (gnx_geno_locus_cross; Z = [e[:, lyr_num], x, y]) of the individuals in
        `slots` at `loci`, and matmul(M [n_loci][3]) -> D M [n][3] (gnx_geno_matmul, fp32)"""
        import torch
        dev = self._dev
        Cm, cs = dev.geno_locus_gram(loci, slots)
        DtZ, ZtZ, Zt1 = dev.geno_locus_cross(loci, lyr_num, slots)
        tdev = _torch_device(self)
        loci_t = torch.as_tensor(loci, device=tdev)

        def matmul(M):
            full = torch.zeros((dev.L, M.shape[1]), dtype=torch.float32, device=tdev)
            full[loci_t] = torch.as_tensor(M, dtype=torch.float32, device=tdev)
            return dev.geno_matmul(full, slots).cpu().numpy().astype(np.float64)

        return Cm, cs, DtZ, ZtZ, Zt1, matmul

    def _run_cca(self, trt_num=0, individs=None, loci=None):
        """Canonical correlation analysis genotype ~ env + lat + long for one Trait (reference
        structs/species.py:2269-2355: sklearn's CCA(n_components=3) on the table of
        _make_gea_df, :2218-2266; env = e of the Trait's Layer, lat = x, long = y), from
        cross-products taken on the device (sim/gea.py): no N x L table leaves the GPU.
        individs and loci (extensions) restrict the rows and the columns; at most 8192 loci.
        -> dict(ind_df [n][3] (rows in ascending-id order), loci_df [n_loci][3], var_df [3][3],
        trait_loci, ids)"""
        from ..sim import gea as _gea
        _need_genomes(self, 'run_gea', assigned=False)
        traits = self.gen_arch.traits
        if not traits:
            raise ValueError('run_gea: the Species has no Traits')
        if isinstance(trt_num, bool) or trt_num not in traits:
            raise ValueError('run_gea: no Trait %r (Traits: %s)' % (trt_num, sorted(traits)))
        _need_genomes(self, 'run_gea')
        trt = traits[trt_num]
        loci_u, _ = self._geno_loci(loci)
        if loci_u is None:
            loci_u = np.arange(self._dev.L, dtype=np.int64)
        if loci_u.size > 8192:
            raise ValueError('run_gea: at most 8192 loci per analysis (the cross-product matrix '
                             'is n_loci x n_loci), got %d: choose them with loci=...' % loci_u.size)
        ids, slots = self._geno_sample(individs)
        prods = self._gea_products(slots, loci_u, int(trt.lyr_num))
        res = _gea.cca_from_cross_products(*prods[:5], ids.size, prods[5])
        return dict(ind_df=res['ind_df'], loci_df=res['loci_df'], var_df=res['var_df'],
                    trait_loci=np.asarray(trt.loci), ids=ids)

    # -- per-locus association scans (sim/assoc.py; csrc/gnx_assoc.hip) ----------------------
    def _env_layers(self, who, env_lyrs):
        """the layers of a request: env_lyrs, or the layers the Traits are tied to, or every
        layer of a Species without Traits (as _dist_predictors)"""
        n_layers = int(self._dev.cfg.n_layers)
        lyrs = env_lyrs
        if lyrs is None:
            traits = self.gen_arch.traits or {}
            lyrs = sorted({int(t.lyr_num) for t in traits.values()}) or range(n_layers)
        lyrs = [int(l) for l in np.atleast_1d(lyrs)]
        if not lyrs or min(lyrs) < 0 or max(lyrs) >= n_layers or len(set(lyrs)) != len(lyrs):
            raise ValueError('%s: env_lyrs: distinct layers in 0..%d' % (who, n_layers - 1))
        return lyrs

    def _assoc_covars(self, who, covars, n):
        """the covariates of run_gwas as [(columns or None, fetch(slots) -> [n][c])]: 'env' (the
        layers the Traits are tied to), ('env', lyr), 'x', 'y', or an array [n][c] in
        ascending-id order; the arrays are counted before the device is asked"""
        if isinstance(covars, (str, np.ndarray)) or (
                isinstance(covars, tuple) and len(covars) == 2 and covars[0] == 'env'
                and not isinstance(covars[1], (str, tuple, list, np.ndarray))):
            covars = [covars]
        out = []
        for c in covars:
            if isinstance(c, str) and c in ('x', 'y'):
                f = nat.F_X if c == 'x' else nat.F_Y
                out.append((1, lambda slots, f=f: self._field(f)[slots].astype(np.float64)[:, None]))
            elif isinstance(c, str) and c == 'env':
                out.append((None, lambda slots: self._field(nat.F_E)[
                    self._env_layers(who, None)][:, slots].T.astype(np.float64)))
            elif isinstance(c, tuple) and len(c) == 2 and c[0] == 'env':
                out.append((1, lambda slots, l=c[1]: self._field(nat.F_E)[
                    self._env_layers(who, [l])][:, slots].T.astype(np.float64)))
            elif isinstance(c, str):
                raise ValueError("%s: covars: 'env', ('env', lyr), 'x', 'y' or an array [n][c] "
                                 "(got %r)" % (who, c))
            else:
                a = np.asarray(c, dtype=np.float64)
                a = a[:, None] if a.ndim == 1 else a
                if a.ndim != 2 or a.shape[0] != n or not np.isfinite(a).all():
                    raise ValueError('%s: covars: a finite array [n = %d][c] in ascending-id '
                                     'order (got %s)' % (who, n, a.shape))
                out.append((a.shape[1], lambda slots, a=a: a))
        return out

    def _assoc_result(self, res, ids, loci, trait_loci, **more):
        """the dict an association scan returns: the scan's arrays at `loci` (all by default;
        chosen on the host after the full scan, so gif and q are those of the whole genome)"""
        loci_u, _ = self._geno_loci(loci)
        if loci_u is None:
            loci_u = np.arange(self._dev.L, dtype=np.int64)
        out = {k: res[k][loci_u] for k in ('beta', 'se', 't', 'p', 'q', 'maf', 'tested')}
        out.update(loci=loci_u, gif=res['gif'], df=res['df'], ids=ids, trait_loci=trait_loci,
                   kernel_ms=res['kernel_ms'], **more)
        return out

    def _run_gwas(self, trt_num=0, y=None, covars=(), n_pcs=0, individs=None, loci=None,
                  min_maf=0.01, calibrate=False, collinear_tol=1e-8):
        """a genome-wide association scan over the living individuals asked for (all by
        default): per locus the regression of the response - the phenotype z of Trait trt_num, or
        y [n] (or [n][r]) in ascending-id order - on the dosage, given an intercept, the covariates
        (_assoc_covars) and the first n_pcs genetic PCs (_calc_genetic_PCA, with its limits).  One
        pass of gnx_assoc_cross over the packed genomes in fp64; the statistics are
        sim/assoc.scan_stats'.  loci selects rows of the result on the host
        -> dict: loci, beta, se, t, p, q [n_loci][r], maf, tested [n_loci], gif [r], df, ids,
        trait_loci (the Trait's loci; None with y), pcs [n][n_pcs], kernel_ms"""
        from ..sim import assoc as _as
        who = 'run_gwas'
        _need_genomes(self, who)
        trait_loci = None
        if y is None:
            traits = self.gen_arch.traits
            if not traits:
                raise ValueError('%s: the Species has no Traits; give y' % who)
            if isinstance(trt_num, bool) or trt_num not in traits:
                raise ValueError('%s: no Trait %r (Traits: %s)' % (who, trt_num, sorted(traits)))
            trait_loci = np.asarray(traits[trt_num].loci)
        if isinstance(n_pcs, bool) or int(n_pcs) != n_pcs or n_pcs < 0:
            raise ValueError('%s: n_pcs: a number of genetic PCs >= 0 (got %r)' % (who, n_pcs))
        ids, slots = self._geno_sample(individs)
        n = int(ids.size)
        if y is not None:
            y = np.asarray(y, dtype=np.float64)
            y = y[:, None] if y.ndim == 1 else y
            if y.ndim != 2 or y.shape[0] != n or y.shape[1] < 1 or not np.isfinite(y).all():
                raise ValueError('%s: y: finite values [n = %d] in ascending-id order (got %s)'
                                 % (who, n, y.shape))
        cov = self._assoc_covars(who, covars, n)
        n_cov = sum(len(self._env_layers(who, None)) if c is None else c for c, _ in cov)
        _as.check_columns(n_cov + int(n_pcs) + (1 if y is None else y.shape[1]), who)
        # ---- from here on the device is asked
        if y is None:
            y = self._field(nat.F_Z)[trt_num][slots].astype(np.float64)[:, None]
        pcs = np.zeros((n, 0))
        if n_pcs:
            pcs = np.asarray(self._calc_genetic_PCA(int(n_pcs), individs=ids)[1], np.float64)
        C = np.column_stack([f(slots) for _, f in cov] + [pcs])
        res = _as.scan(lambda Y: self._dev.assoc_cross(Y, slots), n, y, C, 'gwas', False,
                       min_maf, collinear_tol, calibrate)
        return self._assoc_result(res, ids, loci, trait_loci, pcs=pcs)

    def _run_lfmm(self, K, env_lyrs=None, lam=1e-5, individs=None, loci=None, min_maf=0.01,
                  calibrate=True, collinear_tol=1e-8, env=None):
        """a genotype-environment association scan with latent factors (LFMM2, Caye et al.
        2019): per locus the regression of the dosage on each environmental layer (env_lyrs;
        default: the layers the Traits are tied to, or all; env: a table [n][r] in ascending-id
        order instead of layers), given the other layers and the K latent factors of the ridge
        estimate (sim/assoc.latent_factors, from the exact Gram matrix of gnx_geno_gram: at most
        8192 individuals).  K = 0: the plain linear model.  calibrate: p from t^2 / gif
        -> dict as _run_gwas, with U [n][K] for pcs and trait_loci as a list, per tested layer the
        loci of the Traits tied to it"""
        from ..sim import assoc as _as
        who = 'run_lfmm'
        _need_genomes(self, who)
        if isinstance(K, bool) or int(K) != K or K < 0:
            raise ValueError('%s: K: a number of latent factors >= 0 (got %r)' % (who, K))
        if isinstance(lam, bool) or not lam > 0:
            raise ValueError('%s: lam: a positive ridge penalty (got %r)' % (who, lam))
        ids, slots = self._geno_sample(individs)
        n = int(ids.size)
        if n > _as.GRAM_MAX:
            raise ValueError('%s: at most %d individuals (the latent factors come from the n x n '
                             'Gram matrix), got %d: pass n=... or individs=...'
                             % (who, _as.GRAM_MAX, n))
        if env is not None:
            if env_lyrs is not None:
                raise ValueError('%s: give env_lyrs or env, not both' % who)
            X = np.asarray(env, dtype=np.float64)
            X = X[:, None] if X.ndim == 1 else X
            if X.ndim != 2 or X.shape[0] != n or X.shape[1] < 1 or not np.isfinite(X).all():
                raise ValueError('%s: env: finite values [n = %d][r] in ascending-id order '
                                 '(got %s)' % (who, n, X.shape))
            lyrs, r = None, X.shape[1]
        else:
            lyrs = self._env_layers(who, env_lyrs)
            r = len(lyrs)
        # the columns sent: a basis of the factors and the layers, and the r residuals
        _as.check_columns(int(K) + 2 * r, who)
        if int(K) >= n:
            raise ValueError('%s: K = %d latent factors for %d individuals' % (who, K, n))
        # ---- from here on the device is asked
        trait_loci = None
        if lyrs is not None:
            X = self._field(nat.F_E)[lyrs][:, slots].T.astype(np.float64)
            traits = self.gen_arch.traits or {}
            trait_loci = [np.unique(np.concatenate(
                [np.asarray(t.loci, dtype=np.int64).ravel() for t in traits.values()
                 if int(t.lyr_num) == l] + [np.zeros(0, np.int64)])) for l in lyrs]
        U = _as.latent_factors(self._dev.geno_gram(slots), X, int(K), lam) if K else \
            np.zeros((n, 0))
        res = _as.scan(lambda Y: self._dev.assoc_cross(Y, slots), n, X, U, 'gea', True, min_maf,
                       collinear_tol, calibrate)
        return self._assoc_result(res, ids, loci, trait_loci, U=U)

    # -- per-locus logistic fits (sim/glm.py; csrc/gnx_glm.hip, csrc/gnx_assoc.hip) ----------
    def _logistic_covars(self, who, covars, n_pcs, n, n_other):
        """the covariates of a logistic scan as _run_gwas reads them, counted (with the n_other
        other columns beside the intercept) before the device is asked -> fetch(ids, slots)"""
        from ..sim import glm as _glm
        if isinstance(n_pcs, bool) or int(n_pcs) != n_pcs or n_pcs < 0:
            raise ValueError('%s: n_pcs: a number of genetic PCs >= 0 (got %r)' % (who, n_pcs))
        cov = self._assoc_covars(who, covars, n)
        n_cov = sum(len(self._env_layers(who, None)) if c is None else c for c, _ in cov)
        _glm.check_columns(n_cov + int(n_pcs) + n_other, who)

        def fetch(ids, slots):
            pcs = np.zeros((n, 0))
            if n_pcs:
                pcs = np.asarray(self._calc_genetic_PCA(int(n_pcs), individs=ids)[1], np.float64)
            return np.column_stack([f(slots) for _, f in cov] + [pcs])
        return fetch

    def _logistic_scan(self, who, slots, n, X, C, min_maf, tol, max_iter, calibrate):
        """sim/glm.scan over the device: one gnx_assoc_cross and the sweeps of gnx_glm_sweep"""
        from ..sim import glm as _glm
        return _glm.scan(lambda Y: self._dev.assoc_cross(Y, slots),
                         lambda Z, B: self._dev.glm_sweep(Z, B), n, X, C, min_maf, tol, max_iter,
                         calibrate, who)

    def _run_logistic_gea(self, env_lyrs=None, env=None, covars=(), n_pcs=0, individs=None,
                          loci=None, min_maf=0.01, calibrate=False, tol=1e-8, max_iter=25):
        """a logistic genotype-environment association scan (Sambada: Joost et al. 2007, Stucki
        et al. 2017) over the living individuals asked for (all by default): per locus the
        binomial GLM d_i ~ Binomial(2, mu_i), logit mu_i = b0 + covariates + env_i . beta, fitted
        by Newton's method (sim/glm.fit; tol, max_iter), the tested columns (env_lyrs; default: the
        layers the Traits are tied to, or all; env: a table [n][r] in ascending-id order instead)
        tested together by the likelihood ratio against the model without them and each by Wald.
        Covariates and genetic PCs as _run_gwas; at most 7 columns beside the intercept.  One
        pass of gnx_assoc_cross over the packed genomes (X^T D, s1, s2), then one gnx_glm_sweep
        per Newton step over the fits that have not converged.  loci selects rows of the result on
        the host
        -> dict: loci, beta, se, z, p_wald [n_loci][r], lrt, p, q, maf, tested, converged, n_iter
        [n_loci], gif, df (= r), ids, trait_loci (per layer, as _run_lfmm), kernel_ms (cross and
        sweeps), n_sweeps, seconds"""
        import time
        who = 'run_logistic_gea'
        _need_genomes(self, who)
        _newton_opts(who, tol, max_iter)
        ids, slots = self._geno_sample(individs)
        n = int(ids.size)
        if env is not None:
            if env_lyrs is not None:
                raise ValueError('%s: give env_lyrs or env, not both' % who)
            X = np.asarray(env, dtype=np.float64)
            X = X[:, None] if X.ndim == 1 else X
            if X.ndim != 2 or X.shape[0] != n or X.shape[1] < 1 or not np.isfinite(X).all():
                raise ValueError('%s: env: finite values [n = %d][r] in ascending-id order '
                                 '(got %s)' % (who, n, X.shape))
            lyrs, r = None, X.shape[1]
        else:
            lyrs = self._env_layers(who, env_lyrs)
            r = len(lyrs)
        fetch = self._logistic_covars(who, covars, n_pcs, n, r)
        # ---- from here on the device is asked (sim/glm.scan checks the design's rank first)
        t0 = time.perf_counter()
        trait_loci = None
        if lyrs is not None:
            X = self._field(nat.F_E)[lyrs][:, slots].T.astype(np.float64)
            traits = self.gen_arch.traits or {}
            trait_loci = [np.unique(np.concatenate(
                [np.asarray(t.loci, dtype=np.int64).ravel() for t in traits.values()
                 if int(t.lyr_num) == l] + [np.zeros(0, np.int64)])) for l in lyrs]
        res = self._logistic_scan(who, slots, n, X, fetch(ids, slots), min_maf, tol, max_iter,
                                  calibrate)
        loci_u, _ = self._geno_loci(loci)
        if loci_u is None:
            loci_u = np.arange(self._dev.L, dtype=np.int64)
        out = {k: res[k][loci_u] for k in ('beta', 'se', 'z', 'p_wald', 'lrt', 'p', 'q', 'maf',
                                           'tested', 'converged', 'n_iter')}
        out.update(loci=loci_u, gif=res['gif'], df=res['df'], ids=ids, trait_loci=trait_loci,
                   kernel_ms=res['kernel_ms'], n_sweeps=res['n_sweeps'],
                   seconds=time.perf_counter() - t0)
        return out

    def _calc_clines(self, axis='x', covars=(), individs=None, loci=None, min_maf=0.01,
                     sigma=None, tol=1e-8, max_iter=25):
        """the sigmoid cline of every locus along one axis over the living individuals asked for
        (all by default): p(x) = 1 / (1 + exp(-4 (x - c) / w)), the binomial GLM of
        _run_logistic_gea with the axis as its one tested column (and the covariates, centred, so
        that the cline is the one at their means).  axis: 'x', 'y', ('env', lyr), an angle in
        degrees (the coordinates projected on that direction, 0 = x, 90 = y), or values [n] in
        ascending-id order.  sigma: the dispersal distance per generation (find_kin estimates
        it), which turns a width into a selection coefficient s_hat = 8 sigma^2 / w^2
        -> dict: loci, centre, width, se_centre, se_width, beta [n_loci][2 + c] (intercept, axis,
        covariates), delta_p (the fitted frequency at the upper end of the axis minus that at the
        lower), in_range (the centre lies inside axis_range), slope_sign, lrt, p, q, maf, tested,
        converged [n_loci], axis_range (lo, hi), ids, trait_loci (every Trait's loci),
        concordance (sim/glm.concordance over the loci that are tested, converged, in_range and
        have q <= 0.05), kernel_ms, n_sweeps, and with sigma s_hat [n_loci]"""
        from ..sim import glm as _glm
        who = 'calc_clines'
        _need_genomes(self, who)
        _newton_opts(who, tol, max_iter)
        if sigma is not None and (isinstance(sigma, bool) or not np.isfinite(sigma)
                                  or not sigma > 0):
            raise ValueError('%s: sigma: a positive dispersal distance (got %r)' % (who, sigma))
        ids, slots = self._geno_sample(individs)
        n = int(ids.size)
        bad_axis = ValueError("%s: axis: 'x', 'y', ('env', lyr), an angle in degrees or finite "
                              "values [n = %d] in ascending-id order (got %r)" % (who, n, axis))
        if isinstance(axis, str):
            if axis not in ('x', 'y'):
                raise bad_axis
            get = lambda: self._field(nat.F_X if axis == 'x' else nat.F_Y)[slots]  # noqa: E731
        elif isinstance(axis, tuple) and len(axis) == 2 and axis[0] == 'env':
            lyr = self._env_layers(who, [axis[1]])
            get = lambda: self._field(nat.F_E)[lyr][0][slots]                       # noqa: E731
        elif isinstance(axis, (int, float, np.integer, np.floating)) and \
                not isinstance(axis, bool) and np.isfinite(axis):
            th = np.deg2rad(float(axis))
            get = lambda: (np.cos(th) * self._field(nat.F_X)[slots].astype(np.float64)  # noqa: E731
                           + np.sin(th) * self._field(nat.F_Y)[slots].astype(np.float64))
        else:
            try:
                a = np.asarray(axis, dtype=np.float64)
            except (TypeError, ValueError):
                raise bad_axis from None
            if a.shape != (n,) or not np.isfinite(a).all():
                raise bad_axis
            get = lambda: a                                                         # noqa: E731
        fetch = self._logistic_covars(who, covars, 0, n, 1)
        # ---- from here on the device is asked (sim/glm.scan checks the design's rank first)
        x = np.asarray(get(), np.float64)
        C = fetch(ids, slots)
        C = C - C.mean(axis=0)
        c = C.shape[1]
        res = self._logistic_scan(who, slots, n, x, C, min_maf, tol, max_iter, False)
        lo, hi = float(x.min()), float(x.max())
        ends = [0, 1 + c]                                    # the design is [1, C, x]
        st = _glm.cline_stats(res['coef'][:, ends], res['cov'][:, ends][:, :, ends], lo, hi)
        loci_u, _ = self._geno_loci(loci)
        if loci_u is None:
            loci_u = np.arange(self._dev.L, dtype=np.int64)
        use = res['tested'] & res['converged'] & st['in_range'] & (res['q'] <= 0.05)
        traits = self.gen_arch.traits or {}
        out = {k: st[k][loci_u] for k in st}
        out.update({k: res[k][loci_u] for k in ('lrt', 'p', 'q', 'maf', 'tested', 'converged')})
        out.update(loci=loci_u, beta=res['coef'][:, ends + list(range(1, 1 + c))][loci_u],
                   axis_range=(lo, hi), ids=ids,
                   trait_loci=np.unique(np.concatenate(
                       [np.asarray(t.loci, dtype=np.int64).ravel() for t in traits.values()]
                       + [np.zeros(0, np.int64)])),
                   concordance=_glm.concordance(st['centre'], st['width'], use),
                   kernel_ms=res['kernel_ms'], n_sweeps=res['n_sweeps'])
        if sigma is not None:
            out['s_hat'] = 8.0 * float(sigma) ** 2 / out['width'] ** 2
        return out

    # -- relationship matrices, heritability and breeding values (sim/quantgen.py;
    # csrc/gnx_grm.hip) ---------------------------------------------------------------------
    def _calc_grm(self, individs=None, loci=None, kind='additive', method='gcta', alpha=-1.0,
                  min_maf=0.01, weights=None):
        """the standardised genomic relationship matrix of the living individuals asked for (all
        by default; at most 8192: the matrix is n x n): G_ij = sum_l v_l(d_il) v_l(d_jl) with the
        per-locus values of sim/quantgen.grm_values (additive in GCTA's, VanRaden's or the
        alpha model's weighting, or dominance), written from the sample's exact allele counts
        (gnx_stats_group_counts) and summed on the device (gnx_grm).  weights [L] multiplies the
        values per locus
        -> dict: G float64 [n][n], ids, loci_used, n_loci, p [n_loci] (the sample's frequency of
        the 1-allele at loci_used), kernel_ms, kind, method"""
        from ..sim import quantgen as _qg
        who = 'calc_grm'
        _qg.check_request(who, kind, method, alpha, min_maf)
        _need_genomes(self, who)
        ids, slots = self._geno_sample(individs)
        n = int(ids.size)
        if n > _qg.GRM_MAX:
            raise ValueError('%s: at most %d individuals (the relationship matrix is n x n), got '
                             '%d: pass n=... or individs=...' % (who, _qg.GRM_MAX, n))
        L = self._dev.L
        loci_u, _ = self._geno_loci(loci)
        subset = None
        if loci_u is not None:
            subset = np.zeros(L, bool)
            subset[loci_u] = True
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64)
            if weights.shape != (L,) or not np.isfinite(weights).all():
                raise ValueError('%s: weights: finite values [L = %d] (got %s)'
                                 % (who, L, weights.shape))
        # ---- from here on the device is asked
        c1 = self._dev.stats_group_counts(slots, np.array([0, n], np.int64))[0][0]
        val, used = _qg.grm_values(c1, n, kind, method, alpha, min_maf, subset, weights)
        loci_used = np.flatnonzero(used)
        if loci_used.size == 0:
            raise ValueError('%s: no locus of the request is polymorphic in the sample with a '
                             'minor allele frequency of at least %g' % (who, min_maf))
        _, mask = self._geno_loci(loci_used)
        G = self._dev.grm(val, slots, mask)
        return dict(G=G, ids=ids, loci_used=loci_used, n_loci=int(loci_used.size),
                    p=c1[loci_used] / (2.0 * n), kernel_ms=self._dev.grm_info()['kernel_ms'],
                    kind=kind, method=method)

    def _quantgen_request(self, who, trt_num, y, covars, n_pcs, individs, loci, method, alpha,
                          min_maf, grm, finite=None):
        """what calc_heritability and predict_breeding_values share: the checked request, then
        the response (read as run_gwas reads it), the design matrix [1, covariates, PCs], the
        relationship matrix (grm: a calc_grm result of the same individuals, else computed) and
        its eigendecomposition, kept in the grm dict for the next response
        -> (ids, slots, y [n], X [n][c], grm, z or None, seconds)"""
        import time
        from ..sim import assoc as _as
        from ..sim import quantgen as _qg
        _qg.check_request(who, 'additive', method, alpha, min_maf)
        _need_genomes(self, who)
        if y is None:
            traits = self.gen_arch.traits
            if not traits:
                raise ValueError('%s: the Species has no Traits; give y' % who)
            if isinstance(trt_num, bool) or trt_num not in traits:
                raise ValueError('%s: no Trait %r (Traits: %s)' % (who, trt_num, sorted(traits)))
        if isinstance(n_pcs, bool) or int(n_pcs) != n_pcs or n_pcs < 0:
            raise ValueError('%s: n_pcs: a number of genetic PCs >= 0 (got %r)' % (who, n_pcs))
        if grm is not None:
            if not isinstance(grm, dict) or 'G' not in grm or 'ids' not in grm:
                raise ValueError('%s: grm: the dict calc_grm returns' % who)
            if individs is None:
                individs = grm['ids']
        ids, slots = self._geno_sample(individs)
        n = int(ids.size)
        if n > _qg.GRM_MAX:
            raise ValueError('%s: at most %d individuals (the relationship matrix is n x n), got '
                             '%d: pass n=... or individs=...' % (who, _qg.GRM_MAX, n))
        if grm is not None and not np.array_equal(np.asarray(grm['ids']), ids):
            raise ValueError('%s: grm: its ids are not the individuals of this request' % who)
        if y is not None:
            y = np.asarray(y, dtype=np.float64)
            ok = np.ones(n, bool) if finite is None else finite(ids)
            if y.ndim != 1 or y.shape[0] != n or not np.isfinite(y[ok]).all():
                raise ValueError('%s: y: finite values [n = %d] in ascending-id order (got %s)'
                                 % (who, n, y.shape))
        cov = self._assoc_covars(who, covars, n)
        n_cov = sum(len(self._env_layers(who, None)) if c is None else c for c, _ in cov)
        _as.check_columns(n_cov + int(n_pcs) + 1, who)
        # ---- from here on the device is asked
        z = None
        if y is None:
            y = z = self._field(nat.F_Z)[trt_num][slots].astype(np.float64)
        pcs = np.zeros((n, 0))
        if n_pcs:
            pcs = np.asarray(self._calc_genetic_PCA(int(n_pcs), individs=ids)[1], np.float64)
        X = np.column_stack([np.ones(n)] + [f(slots) for _, f in cov] + [pcs])
        seconds = dict(grm=0.0, eigh=0.0)
        if grm is None:
            t0 = time.perf_counter()
            grm = self._calc_grm(individs=ids, loci=loci, method=method, alpha=alpha,
                                 min_maf=min_maf)
            seconds['grm'] = time.perf_counter() - t0
        if 'eig' not in grm:
            t0 = time.perf_counter()
            grm['eig'] = _qg.eig_grm(grm['G'])
            seconds['eigh'] = time.perf_counter() - t0
        return ids, slots, y, X, grm, z, seconds

    def _calc_heritability(self, trt_num=0, y=None, covars=(), n_pcs=0, individs=None, loci=None,
                           method='gcta', alpha=-1.0, min_maf=0.01, grm=None):
        """the SNP heritability of a response over the living individuals asked for (all by
        default; at most 8192): the mixed model y = X b + g + e, g ~ N(0, Vg G), with G the
        additive relationship matrix (_calc_grm; grm: a previous result of the same individuals,
        which then also keeps its eigendecomposition under 'eig'), X an intercept, the covariates
        (_assoc_covars) and the first n_pcs genetic PCs, fitted by REML (sim/quantgen.reml).  The
        response is the phenotype z of Trait trt_num or y [n] in ascending-id order
        -> reml's dict plus he_h2 (Haseman-Elston), ids, n_loci, seconds (grm, eigh, reml)"""
        import time
        from ..sim import quantgen as _qg
        ids, _, y, X, grm, _, seconds = self._quantgen_request(
            'calc_heritability', trt_num, y, covars, n_pcs, individs, loci, method, alpha,
            min_maf, grm)
        t0 = time.perf_counter()
        out = _qg.reml(grm['eig'][0], grm['eig'][1], y, X)
        seconds['reml'] = time.perf_counter() - t0
        out.update(he_h2=_qg.he_regression(grm['G'], y, X), ids=ids, n_loci=grm['n_loci'],
                   seconds=seconds)
        return out

    def _predict_breeding_values(self, trt_num=0, y=None, covars=(), n_pcs=0, train=None,
                                 individs=None, loci=None, method='gcta', alpha=-1.0,
                                 min_maf=0.01, grm=None):
        """genomic BLUP of the breeding values of the living individuals asked for (all by
        default; at most 8192): the variance components are fitted by REML on the individuals
        of `train` (ids; None: everybody) and g_hat = G[:, train] V_tt^-1 (y_t - X_t b) predicts
        everybody (sim/quantgen.gblup).  y outside `train` is not read and may be NaN
        -> dict: g_hat, y_hat [n], ids, train (ids), beta, delta, h2, Vg, Ve, and for a Trait
        response accuracy: the correlation of g_hat with the Trait's z over the individuals not
        trained on (NaN when there are none)"""
        from ..sim import quantgen as _qg
        who = 'predict_breeding_values'
        tr_ids = None
        if train is not None:
            tr_ids = np.unique(np.asarray(train, dtype=np.int64).ravel())
            if tr_ids.size < 2:
                raise ValueError('%s: train: at least 2 individuals' % who)

        def observed(ids):
            return np.ones(ids.size, bool) if tr_ids is None else np.isin(ids, tr_ids)

        given = y is not None
        ids, _, y, X, grm, z, _ = self._quantgen_request(
            who, trt_num, y, covars, n_pcs, individs, loci, method, alpha, min_maf, grm, observed)
        idx = None
        if tr_ids is not None:
            idx = np.searchsorted(ids, tr_ids)
            if (idx >= ids.size).any() or (ids[np.minimum(idx, ids.size - 1)] != tr_ids).any():
                raise ValueError('%s: train: individuals outside the sample' % who)
        got = _qg.gblup(grm['eig'][0], grm['eig'][1], np.where(observed(ids), y, 0.0), X,
                        train=idx)
        fit = got['fit']
        out = dict(g_hat=got['g_hat'], y_hat=got['y_hat'], ids=ids,
                   train=ids if tr_ids is None else tr_ids, beta=got['beta'], delta=got['delta'],
                   h2=fit['h2'], Vg=fit['Vg'], Ve=fit['Ve'])
        if not given:
            rest = ~observed(ids)
            acc = float('nan')
            if rest.sum() > 1 and np.std(z[rest]) > 0 and np.std(got['g_hat'][rest]) > 0:
                acc = float(np.corrcoef(got['g_hat'][rest], z[rest])[0, 1])
            out['accuracy'] = acc
        return out

    def _run_lmm(self, trt_num=0, y=None, covars=(), n_pcs=0, individs=None, loci=None, grm=None,
                 grm_loci=None, method='gcta', alpha=-1.0, min_maf=0.01, delta=None,
                 calibrate=False, collinear_tol=1e-8):
        """a mixed-model association scan over the living individuals asked for (all by default;
        at most 8192): per locus the test of beta in y = X b + g beta + u + e, u ~ N(0, Vg G),
        with G the additive relationship matrix of the loci grm_loci (_calc_grm; grm: a previous
        result of the same individuals, which keeps its eigendecomposition under 'eig'), X an
        intercept, the covariates and the first n_pcs genetic PCs.  The request, the response and
        G are _calc_heritability's; delta = Ve / Vg is its REML estimate of the model without a
        locus (delta: a given ratio instead) and stays fixed over the scan (sim/assoc.py,
        lmm_scan_stats).  One response per call: delta belongs to the response, so y [n][r] is
        refused.  One pass of gnx_assoc_cross and one of gnx_assoc_quad (f32 matrix cores, fp64
        sums; the rotation is rounded to fp32 once and every term uses the rounded one)
        -> _run_gwas' dict without pcs, plus delta, h2, Vg, Ve, at_boundary (NaN / False with a
        given delta), n_loci_grm, seconds (grm, eigh, reml, quad, cross)"""
        import time
        from ..sim import assoc as _as
        from ..sim import quantgen as _qg
        who = 'run_lmm'
        if y is not None and np.ndim(y) != 1:
            raise ValueError('%s: one response y [n] per call (delta is fitted per response; got '
                             'shape %s)' % (who, np.shape(y)))
        if delta is not None and (isinstance(delta, bool) or not np.isfinite(delta)
                                  or not delta > 0):
            raise ValueError('%s: delta: a positive, finite ratio Ve / Vg (got %r)' % (who, delta))
        trait_loci = None
        if y is None and self.gen_arch.traits and trt_num in self.gen_arch.traits:
            trait_loci = np.asarray(self.gen_arch.traits[trt_num].loci)
        ids, slots, y, X, grm, _, seconds = self._quantgen_request(
            who, trt_num, y, covars, n_pcs, individs, grm_loci, method, alpha, min_maf, grm)
        n = int(ids.size)
        fit = dict(h2=float('nan'), Vg=float('nan'), Ve=float('nan'), at_boundary=False)
        seconds['reml'] = 0.0
        if delta is None:
            t0 = time.perf_counter()
            fit = _qg.reml(grm['eig'][0], grm['eig'][1], y, X)
            seconds['reml'] = time.perf_counter() - t0
            delta = fit['delta']
        M = _as.lmm_rotation(grm['eig'][0], grm['eig'][1], delta).astype(np.float32)

        def quad(val, _, use):               # the device takes the fp32 M itself
            if not use.any():
                return dict(q=np.zeros(self._dev.L), kernel_ms=0.0)
            _, mask = self._geno_loci(np.flatnonzero(use))
            return self._dev.assoc_quad(val, M, slots, mask)

        res = _as.lmm_scan(lambda Y: self._dev.assoc_cross(Y, slots), quad, n, y, X,
                           M.astype(np.float64), min_maf, collinear_tol, calibrate)
        seconds.update(res['seconds'])
        return self._assoc_result(res, ids, loci, trait_loci, delta=float(delta),
                                  h2=fit['h2'], Vg=fit['Vg'], Ve=fit['Ve'],
                                  at_boundary=fit['at_boundary'], n_loci_grm=grm['n_loci'],
                                  seconds=seconds)

    # -- Mantel tests and MMRR (sim/mmrr.py; csrc/gnx_mantel.hip) --------------------------
    def _dist_predictors(self, who, predictors, env_lyrs, trts):
        """the device columns [(field, index), ...] of each named predictor: 'geo' = (x, y),
        'env' = the layers env_lyrs (default: the layers the Traits are tied to, or every layer
        of a Species without Traits), 'phn' = the Traits trts (default: all)"""
        if isinstance(predictors, str):
            predictors = (predictors,)
        predictors = list(predictors)
        if not predictors:
            raise ValueError('%s: no predictors' % who)
        traits = self.gen_arch.traits or {}
        n_layers = int(self._dev.cfg.n_layers)
        cols = []
        for name in predictors:
            if name == 'geo':
                cols.append([(nat.F_X, 0), (nat.F_Y, 0)])
            elif name == 'env':
                lyrs = env_lyrs
                if lyrs is None:
                    lyrs = sorted({int(t.lyr_num) for t in traits.values()}) or range(n_layers)
                lyrs = [int(l) for l in np.atleast_1d(lyrs)]
                if not lyrs or min(lyrs) < 0 or max(lyrs) >= n_layers:
                    raise ValueError('%s: env_lyrs: layers in 0..%d' % (who, n_layers - 1))
                cols.append([(nat.F_E, l) for l in lyrs])
            elif name == 'phn':
                nums = sorted(traits) if trts is None else [int(t) for t in np.atleast_1d(trts)]
                if not nums or any(t not in traits for t in nums):
                    raise ValueError('%s: trts: Traits among %s' % (who, sorted(traits)))
                cols.append([(nat.F_Z, t) for t in nums])
            else:
                raise ValueError("%s: unknown predictor %r ('geo', 'env', 'phn', 'cost' or "
                                 "'circuit')"
                                 % (who, name))
        if len(set(predictors)) != len(predictors):
            raise ValueError('%s: a predictor is listed twice' % who)
        if len(cols) > 4 or sum(len(c) for c in cols) > 8:
            raise ValueError('%s: at most 4 predictors and 8 columns (layers, traits, x, y) '
                             'together' % who)
        return predictors, cols

    # -- least-cost distances (sim/cost.py; csrc/gnx_cost.hip) ------------------------------
    def _cost_raster(self, who, lyr=None, kind='conductance', barrier=None, cost=None):
        """the resistance raster R [H][W] of a request (sim/cost.resistance_raster): an explicit
        cost raster, or the values of Layer lyr (default: the Layer of the move_surf) read as
        kind"""
        from ..sim import cost as _cost
        W, H = self._land_dim
        if cost is not None:
            return _cost.resistance_raster(cost=cost, shape=(H, W))
        land = self._land_ref
        if lyr is None:
            if not self._move_surf:
                raise ValueError('%s: the Species has no move_surf to take the conductance '
                                 'from: pass lyr=... or cost=...' % who)
            lyr = self._spp_params.movement.move_surf['layer']
        if isinstance(lyr, str):
            nums = [k for k, l in land.items() if l.name == lyr]
            if len(nums) != 1:
                raise ValueError('%s: lyr: no single Layer is named %r' % (who, lyr))
            lyr = nums[0]
        if isinstance(lyr, bool) or int(lyr) != lyr or int(lyr) not in land:
            raise ValueError('%s: lyr: a Layer among %s (got %r)' % (who, sorted(land), lyr))
        return _cost.resistance_raster(land[int(lyr)].rast, kind=kind, barrier=barrier,
                                       shape=(H, W))

    def _cost_res(self):
        return abs(float(self._land_res[0])), abs(float(self._land_res[1]))

    def _cost_matrix_of_cells(self, R, cells):
        """least-cost distances [n][n] of individuals standing on cells [n][2] = (x, y): the
        distinct cells' matrix from the device, expanded (two individuals on one cell: 0)"""
        from ..sim import cost as _cost
        cells = np.asarray(cells, np.int64).reshape(-1, 2)
        lin = cells[:, 1] * int(self._land_dim[0]) + cells[:, 0]
        uniq, inverse = np.unique(lin, return_inverse=True)
        return _cost.expand(self._dev.cost_matrix(R, self._cost_res(), uniq), inverse)

    def _calc_cost_distances(self, lyr=None, kind='conductance', barrier=None, cost=None,
                             individs=None):
        """pairwise least-cost distances between the cells of the living individuals asked for
        (all by default; at most 8192) over the resistance raster of the request, solved on the
        device -> dict(ids ascending, cells [n][2], dist float64 [n][n])"""
        who = 'calc_cost_distances'
        ids, _ = self._geno_sample(individs)
        if ids.size > 8192:
            raise ValueError('%s: at most 8192 individuals per call (the distance matrix is '
                             'n x n), got %d: sample them with n=... or individs=...'
                             % (who, ids.size))
        if ids.size < 1:
            raise ValueError('%s: no individuals' % who)
        R = self._cost_raster(who, lyr=lyr, kind=kind, barrier=barrier, cost=cost)
        cells = self._get_cells(individs=ids)
        return dict(ids=ids, cells=cells, dist=self._cost_matrix_of_cells(R, cells))

    def _calc_cost_surface(self, x, y, lyr=None, kind='conductance', barrier=None, cost=None):
        """the accumulated-cost raster float64 [k][H][W] of k points (x, y) in landscape
        coordinates, floored to cells as _get_cells does"""
        who = 'calc_cost_surface'
        x = np.atleast_1d(np.asarray(x, np.float64)).ravel()
        y = np.atleast_1d(np.asarray(y, np.float64)).ravel()
        if x.size != y.size or x.size < 1:
            raise ValueError('%s: as many x as y, at least one point' % who)
        W, H = self._land_dim
        if not (np.isfinite(x).all() and np.isfinite(y).all()):
            raise ValueError('%s: a point is not finite' % who)
        cx, cy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
        if (cx < 0).any() or (cx >= W).any() or (cy < 0).any() or (cy >= H).any():
            raise ValueError('%s: a point lies outside the landscape (0 <= x < %d, 0 <= y < %d)'
                             % (who, W, H))
        R = self._cost_raster(who, lyr=lyr, kind=kind, barrier=barrier, cost=cost)
        return self._dev.cost_surfaces(R, self._cost_res(), cy * int(W) + cx)

    # -- circuit-theory resistances (sim/circuit.py; csrc/gnx_circuit.hip) -------------------
    def _resistance_matrix_of_cells(self, R, cells, tol=None, max_iter=None):
        """effective resistances [n][n] of individuals standing on cells [n][2] = (x, y): the
        distinct cells' matrix from the device, expanded (two individuals on one cell: 0)"""
        from ..sim import circuit as _circuit
        cells = np.asarray(cells, np.int64).reshape(-1, 2)
        lin = cells[:, 1] * int(self._land_dim[0]) + cells[:, 0]
        uniq, inverse = np.unique(lin, return_inverse=True)
        return _circuit.expand(self._dev.circuit_matrix(R, self._cost_res(), uniq, tol, max_iter),
                               inverse)

    def _calc_resistance_distances(self, lyr=None, kind='conductance', barrier=None, cost=None,
                                   individs=None, tol=None, max_iter=None):
        """pairwise effective resistances (circuit theory) between the cells of the living
        individuals asked for (all by default; at most 8192) over the resistance raster of the
        request, solved on the device
        -> dict(ids ascending, cells [n][2], dist float64 [n][n], info: the solver's
        kernel_ms, launches, iterations, restarts, worst_residual)"""
        who = 'calc_resistance_distances'
        ids, _ = self._geno_sample(individs)
        if ids.size > 8192:
            raise ValueError('%s: at most 8192 individuals per call (the distance matrix is '
                             'n x n), got %d: sample them with n=... or individs=...'
                             % (who, ids.size))
        if ids.size < 1:
            raise ValueError('%s: no individuals' % who)
        _solver_opts(who, tol, max_iter)
        R = self._cost_raster(who, lyr=lyr, kind=kind, barrier=barrier, cost=cost)
        cells = self._get_cells(individs=ids)
        dist = self._resistance_matrix_of_cells(R, cells, tol, max_iter)
        return dict(ids=ids, cells=cells, dist=dist, info=self._dev.circuit_info())

    def _calc_current_map(self, x=None, y=None, individs=None, lyr=None, kind='conductance',
                          barrier=None, cost=None, tol=None, max_iter=None):
        """the cumulative current map float64 [H][W] of all pairs of the distinct cells of k
        points (x, y) in landscape coordinates, floored to cells as _calc_cost_surface does, or
        of the cells of the living individuals asked for (all when neither is given).  At most
        128 distinct cells: the work is pairs x cells x 8 edges
        -> dict(current [H][W], cells [m] (y * W + x, ascending), n_pairs, n_skipped)"""
        who = 'calc_current_map'
        W, H = self._land_dim
        if (x is None) != (y is None):
            raise ValueError('%s: x and y, or neither' % who)
        if x is not None:
            if individs is not None:
                raise ValueError('%s: points (x, y) or individs, not both' % who)
            x = np.atleast_1d(np.asarray(x, np.float64)).ravel()
            y = np.atleast_1d(np.asarray(y, np.float64)).ravel()
            if x.size != y.size or x.size < 1:
                raise ValueError('%s: as many x as y, at least one point' % who)
            if not (np.isfinite(x).all() and np.isfinite(y).all()):
                raise ValueError('%s: a point is not finite' % who)
            cx, cy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
            if (cx < 0).any() or (cx >= W).any() or (cy < 0).any() or (cy >= H).any():
                raise ValueError('%s: a point lies outside the landscape (0 <= x < %d, '
                                 '0 <= y < %d)' % (who, W, H))
        else:
            ids, _ = self._geno_sample(individs)
            if ids.size < 1:
                raise ValueError('%s: no individuals' % who)
            cells = np.asarray(self._get_cells(individs=ids), np.int64).reshape(-1, 2)
            cx, cy = cells[:, 0], cells[:, 1]
        uniq = np.unique(cy * int(W) + cx)
        if uniq.size > 128:
            raise ValueError('%s: at most 128 distinct cells per call (the work is pairs x cells '
                             'x 8 edges), got %d: sample them with n=... or individs=...'
                             % (who, uniq.size))
        _solver_opts(who, tol, max_iter)
        R = self._cost_raster(who, lyr=lyr, kind=kind, barrier=barrier, cost=cost)
        cur, used, skipped = self._dev.circuit_current(R, self._cost_res(), uniq, tol, max_iter)
        return dict(current=cur, cells=uniq, n_pairs=used, n_skipped=skipped)

    def _dist_perm_sums(self, who, predictors, env_lyrs, trts, individs, loci, nperm, seed,
                        min_n):
        """(names, permuted cross-sums [nperm][K], moments) of a Mantel / MMRR request:
        the reference's row shuffles drawn from `seed` (or the Species' rng), inverted for the
        library, and gnx_dist_perm_sums on the device columns"""
        from ..sim import mmrr as _mmrr
        _need_genomes(self, who)
        if isinstance(nperm, bool) or int(nperm) != nperm or nperm < 1:
            raise ValueError('%s: nperm: at least 1 permutation (got %r)' % (who, nperm))
        names, cols, costs = _split_predictors(self, who, predictors, env_lyrs, trts)
        ids, slots = self._geno_sample(individs)
        if ids.size > 8192:
            raise ValueError('%s: at most 8192 individuals per test (the distance matrix is '
                             'n x n), got %d: sample them with n=... or individs=...'
                             % (who, ids.size))
        if ids.size < min_n:
            raise ValueError('%s: %d individuals leave the test no degrees of freedom (at least '
                             '%d)' % (who, ids.size, min_n))
        _, mask = self._geno_loci(loci)
        if not costs:
            rows = _mmrr.draw_row_shuffles(ids.size, int(nperm), seed=seed, rng=self._rng)
            sums, mom = self._dev.dist_perm_sums(cols, _mmrr.invert_rows(rows), slots, mask)
            return names, sums, mom
        # the cost matrices of the sample (rows in id order, as slots), built beside the columns
        cells = self._get_cells(individs=ids)
        mats = []
        for name, what, opts in costs:
            if what == 'circuit':
                opts = dict(opts)
                tol, max_iter = opts.pop('tol', None), opts.pop('max_iter', None)
                D = self._resistance_matrix_of_cells(self._cost_raster(who, **opts), cells, tol,
                                                     max_iter)
            else:
                D = self._cost_matrix_of_cells(self._cost_raster(who, **opts), cells)
            n_inf = int(np.isinf(D[np.tril_indices(ids.size, -1)]).sum())
            if n_inf:
                raise ValueError('%s: predictor %r: %d pairs of the sampled individuals are at '
                                 'infinite cost (no path joins them): sample individuals that '
                                 'can reach each other' % (who, name, n_inf))
            mats.append(D)
        rows = _mmrr.draw_row_shuffles(ids.size, int(nperm), seed=seed, rng=self._rng)
        sums, mom = self._dev.dist_perm_sums_mat(cols, np.stack(mats), _mmrr.invert_rows(rows),
                                                 slots, mask)
        # the library's order (columns, then matrices) back to the caller's
        mat_names = [c[0] for c in costs]
        lib = [n for n in names if n not in mat_names] + mat_names
        o = [lib.index(n) for n in names]
        mom = dict(mom, sx=np.asarray(mom['sx'])[o], sxy=np.asarray(mom['sxy'])[o],
                   sxx=np.asarray(mom['sxx'])[np.ix_(o, o)])
        return names, np.ascontiguousarray(np.asarray(sums)[:, o]), mom

    def _run_mmrr(self, predictors=('geo', 'env'), env_lyrs=None, trts=None, individs=None,
                  loci=None, nperm=999, seed=None):
        """multiple matrix regression with randomization of the genetic distances on the
        predictors' distances (reference data/IBD_IBE_demo/MMRR.py, as demos/_IBD_IBE.py calls
        it), every permutation's fit from cross-sums taken on the device
        -> the reference's OrderedDict (sim/mmrr.mmrr)"""
        from ..sim import mmrr as _mmrr
        K = len(_predictor_list(predictors))
        # n (n - 1) / 2 pairs must exceed the K + 1 coefficients
        min_n = 3
        while min_n * (min_n - 1) // 2 < K + 2:
            min_n += 1
        names, sums, mom = self._dist_perm_sums('run_mmrr', predictors, env_lyrs, trts,
                                                individs, loci, nperm, seed, min_n)
        return _mmrr.mmrr(sums, mom, names)

    def _run_mantel(self, x='geo', given=None, env_lyrs=None, trts=None, individs=None,
                    loci=None, nperm=999, seed=None):
        """Mantel test of the genetic distances against predictor x, partial given another
        (reference data/IBD_IBE_demo/run_mantel.R: vegan's mantel.partial with the genetic
        matrix permuted) -> dict(r, p, nperm, perm_r [nperm])"""
        from ..sim import mmrr as _mmrr
        preds = (x,) if given is None else (x, given)
        _, sums, mom = self._dist_perm_sums('run_mantel', preds, env_lyrs, trts, individs,
                                            loci, nperm, seed, 3 if given is None else 4)
        return _mmrr.mantel(sums, mom, 0, None if given is None else 1)

    # -- fine-scale spatial genetic structure (sim/sgs.py; csrc/gnx_sgs.hip) ----------------
    # pair-words (candidate pairs x genome words) one call may take: about ten seconds at the
    # measured rate of the call with cells that fill their tiles
    _SGS_MAX_WORK = 1 << 43

    def _calc_spatial_structure(self, edges=None, n_classes=10, max_dist=None, individs=None,
                                loci=None, nperm=0, seed=None, fit_range=None, max_work=None):
        """kinship by distance class over the pairs of the living individuals asked for (all by
        default; no n x n matrix, so the whole population can be analysed): Loiselle's kinship
        per class, its slope on ln(distance), Sp and Wright's neighbourhood size
        (sim/sgs.spatial_structure), from per-class sums taken on the device (gnx_sgs_sums).
        edges: the classes' bounds, ascending (1..32 classes); default n_classes classes of equal
        width in ln r from the landscape's cell size to max_dist (default: a quarter of the
        shorter landscape side).  nperm > 0: the genomes are permuted over the positions, drawn
        as run_mantel draws its permutations, one device call each.  fit_range: (first class,
        one past the last) of the classes the slope is fitted over.  max_work: the pair-words
        (candidate pairs x genome words) one call may take
        -> dict of arrays and scalars: edges, pairs, mean_r, mean_lnr, F, dist2, slope, F1, Sp,
        Nb, n, n_zero (pairs at distance 0: in no class), work, ids; with nperm: nperm,
        perm_slope, p_slope, perm_F, p_F"""
        from ..sim import mmrr as _mmrr
        from ..sim import sgs as _sgs
        who = 'calc_spatial_structure'
        _need_genomes(self, who)
        if isinstance(nperm, bool) or int(nperm) != nperm or nperm < 0:
            raise ValueError('%s: nperm: a number of permutations >= 0 (got %r)' % (who, nperm))
        edges = _distance_classes(self, who, edges, n_classes, max_dist)
        _sgs._fit_slice(fit_range, edges.size - 1)
        max_work = _work_limit(who, max_work, self._SGS_MAX_WORK, 'pair-words')
        ids, slots = self._geno_sample(individs)
        n = ids.size
        if n < 2:
            raise ValueError('%s: at least 2 individuals (got %d)' % (who, n))
        if n > 2 ** 24:
            raise ValueError('%s: at most 2^24 individuals per call (got %d): sample them with '
                             'n=... or individs=...' % (who, n))
        loci_u, mask = self._geno_loci(loci)
        dev = self._dev
        work = dev.sgs_sums(edges, slots, mask)['work']
        if work > max_work:
            raise ValueError('%s: %d pair-words of work (candidate pairs x genome words) exceed '
                             'max_work = %d: analyse a sample (n=...), fewer loci (loci=...) or a '
                             'smaller max_dist, or raise max_work' % (who, work, max_work))
        cnt1, _ = dev.stats_group_counts(slots, np.array([0, n], np.int64))
        s_l = cnt1[0].astype(np.int64)
        weight = np.zeros(dev.L, np.float64)
        if loci_u is None:
            weight[:] = _sgs.locus_terms(s_l, n)[0]
        else:
            s_l = s_l[loci_u]
            weight[loci_u] = _sgs.locus_terms(s_l, n)[0]
        obs = dev.sgs_sums(edges, slots, mask, weight, None, max_work)
        pI = pS = None
        if nperm:
            rows = _mmrr.draw_row_shuffles(n, int(nperm), seed=seed, rng=self._rng)
            pI = np.empty((int(nperm),) + obs['isums'].shape, np.int64)
            pS = np.empty((int(nperm),) + obs['fsums'].shape, np.float64)
            for p, r in enumerate(rows):                  # position i takes the genome of r[i]
                got = dev.sgs_sums(edges, slots, mask, weight, r.astype(np.int32), max_work)
                pI[p], pS[p] = got['isums'], got['fsums']
        out = _sgs.spatial_structure(obs['isums'], obs['fsums'], s_l, n, fit_range, pI, pS)
        out.update(edges=edges, n_zero=obs['n_zero'], work=work, ids=ids)
        return out

    # -- close-kin pairs (sim/kin.py; csrc/gnx_kin.hip) ----------------------------------------
    def _calc_relatedness(self, individs=None, loci=None):
        """KING-robust kinship (Manichaikul et al. 2010) between every two of the living
        individuals asked for (all by default; at most 8192: the matrices are n x n), from the
        integers the device counts (gnx_kin_matrix): the loci at which both are heterozygous
        (hh), those at which they are opposite homozygotes (ibs0) and each one's heterozygous
        loci (nhet); kinship = (hh - 2 ibs0) / (nhet_a + nhet_b), 0.5 on the diagonal, NaN where
        neither has a heterozygous locus
        -> dict: ids, kinship float64 [n][n], ibs0, hh int32 [n][n], nhet int32 [n]"""
        from ..sim import kin as _kin
        who = 'calc_relatedness'
        _need_genomes(self, who)
        ids, slots = self._geno_sample(individs)
        if ids.size > 8192:
            raise ValueError('relatedness of at most 8192 individuals per call (got %d): '
                             'sample them with n=... or individs=..., or list the close pairs '
                             'with find_kin' % ids.size)
        _, mask = self._geno_loci(loci)
        got = self._dev.kin_matrix(slots, mask)
        nh = got['nhet']
        return dict(ids=ids, kinship=_kin.king(got['hh'], got['ibs0'], nh[:, None], nh[None, :]),
                    ibs0=got['ibs0'], hh=got['hh'], nhet=nh)

    def _calc_kin_pairs(self, max_dist=None, min_kinship=2 ** -3.5, individs=None, loci=None,
                        max_pairs=1 << 22, max_work=None, po_max_ibs0=0):
        """the pairs of close relatives among the living individuals asked for (all by default;
        no n x n matrix, so the whole population can be searched): every pair closer than
        max_dist (None: every pair) whose KING-robust kinship is at least min_kinship (default
        2^-3.5: second degree and closer), found on the device (gnx_kin_pairs), with the
        relationship KING's cutoffs name ('dup', 'PO', 'FS', '2nd', '3rd', 'un'; a first-degree
        pair is 'PO' iff ibs0 <= po_max_ibs0).  max_pairs: the pairs the list may hold;
        max_work: the pair-words (pairs of individuals in the same or adjacent cells of side
        max_dist x genome words) the call may take
        -> dict: ids_a, ids_b (ids_a < ids_b, sorted by both), kinship, ibs0, hh, dist,
        relationship (per pair), n_candidates (pairs closer than max_dist), work, ids, nhet;
        with a recorded pedigree also true_relationship ('PO', 'FS', 'HS' or '')"""
        from ..sim import kin as _kin
        who = 'find_kin'
        _need_genomes(self, who)
        try:
            T = _kin.threshold(min_kinship)
        except (TypeError, ValueError):
            raise ValueError('%s: min_kinship: a finite number in [-1, 0.5] (got %r)'
                             % (who, min_kinship)) from None
        if max_dist is not None and (isinstance(max_dist, bool)
                                     or not 0 < float(max_dist) < np.inf):
            raise ValueError('%s: max_dist: None or a positive finite distance (got %r)'
                             % (who, max_dist))
        if isinstance(max_pairs, bool) or int(max_pairs) != max_pairs or \
                not 1 <= max_pairs <= 1 << 26:
            raise ValueError('%s: max_pairs: a positive integer, at most 2^26 (got %r)'
                             % (who, max_pairs))
        max_work = _work_limit(who, max_work, self._SGS_MAX_WORK, 'pair-words')
        ids, slots = self._geno_sample(individs)
        n = ids.size
        if n < 1 or n > 2 ** 24:
            raise ValueError('%s: 1..2^24 individuals per call (got %d): sample them with '
                             'n=... or individs=...' % (who, n))
        _, mask = self._geno_loci(loci)
        try:
            got = _within_max_work(
                who, lambda: self._dev.kin_pairs(T, max_dist, slots, mask, int(max_pairs),
                                                 max_work),
                'search a sample (n=... or individs=...), fewer loci (loci=...) or a smaller '
                'max_dist, or raise max_work')
        except nat.GnxError as err:
            if 'exceed max_pairs' not in str(err):
                raise
            raise ValueError('%s: n_found = %d kept pairs exceed max_pairs = %d: ask for a '
                             'higher min_kinship, a smaller max_dist, or a larger max_pairs'
                             % (who, getattr(err, 'n_found', -1), max_pairs)) from None
        pa, pb, nh = got['pa'], got['pb'], got['nhet']
        x = self._field(nat.F_X)[slots].astype(np.float64)
        y = self._field(nat.F_Y)[slots].astype(np.float64)
        dx, dy = x[pa] - x[pb], y[pa] - y[pb]
        kinship = _kin.king(got['hh'], got['ibs0'], nh[pa], nh[pb])
        out = dict(ids_a=ids[pa], ids_b=ids[pb], kinship=kinship, ibs0=got['ibs0'],
                   hh=got['hh'], dist=np.sqrt(dx * dx + dy * dy),
                   relationship=_kin.relationship(kinship, got['ibs0'], po_max_ibs0),
                   n_candidates=got['n_candidates'], work=got['work'], ids=ids, nhet=nh)
        if self.__dict__.get('_tt') is not None:
            par = self._tt.parents_of(ids)
            out['true_relationship'] = _kin.pair_truth(ids[pa], ids[pb], par[pa], par[pb])
        return out

    def _get_pedigree_parents(self, individs=None):
        """(ids ascending, int64 [n][2] their recorded parents' ids, -1 for founders) of the
        living individuals asked for (all by default)"""
        if self.__dict__.get('_tt') is None:
            raise ValueError("get_pedigree_parents: no pedigree was recorded for this Species "
                             "('use_tskit' False, or the genomes were not assigned yet)")
        ids, _ = self._geno_sample(individs)
        return ids, self._tt.parents_of(ids)

    # -- genome-wide linkage disequilibrium (sim/ld.py; csrc/gnx_ld.hip) ---------------------
    # tile-words (64 x 64-locus tiles x chromosome words) one call may take; a tile-word is 4096
    # pair-words of the popcount tile, so this is four times _SGS_MAX_WORK
    _LD_MAX_WORK = 1 << 33

    def _ld_request(self, who, individs, loci, unit, min_maf):
        """(ids, slots, loci ascending, their coordinates for the device, min_minor) of an LD
        request"""
        from ..sim import ld as _ld
        _need_genomes(self, who)
        if unit not in ('c', 'morgans', 'loci'):
            raise ValueError("%s: unit: 'c', 'morgans' or 'loci', not %r" % (who, unit))
        ids, slots = self._geno_sample(individs)
        if ids.size < 1 or ids.size > 2 ** 25:
            raise ValueError('%s: 1..2^25 individuals per call (got %d): sample them with n=... '
                             'or individs=...' % (who, ids.size))
        loci_u, _ = self._geno_loci(loci)
        if loci_u is None:
            loci_u = np.arange(self._dev.L, dtype=np.int64)
        if unit == 'loci':
            pos = loci_u.astype(np.float64)
        else:
            pos = _ld.map_positions(_rec_rates(self))[loci_u]
        return ids, slots, loci_u, pos, _ld.min_minor(min_maf, 2 * ids.size)

    def _ld_call(self, who, loci, pos, edges, slots, min_minor, morgans, max_work):
        """one gnx_ld_bins call; the library's refusal of a request above max_work (it comes
        before anything is launched) becomes a ValueError with advice"""
        return _within_max_work(
            who, lambda: self._dev.ld_bins(loci, pos, edges, slots, min_minor, morgans, max_work),
            'analyse a sample (n=...), fewer loci (loci=...) or a smaller max_dist, or raise '
            'max_work')

    def _calc_ld_decay(self, edges=None, n_bins=20, unit='c', max_dist=None, individs=None,
                       loci=None, min_maf=0.05, max_work=None):
        """the decay of linkage disequilibrium with distance: mean r^2 over the pairs of loci in
        each distance bin, for all loci of the living individuals asked for (all by default), on
        the device (gnx_ld_bins: no L x L matrix, any number of loci).  unit: 'c', the
        recombination fraction between the two loci under the architecture's rates (sim/ld.py;
        edges in c, an upper edge >= 0.5 taking in every looser pair); 'morgans', their map
        distance; 'loci', the difference of their locus numbers.  edges: the bins' bounds
        (default sim/ld.default_edges(unit, n_bins, max_dist)).  Loci whose minor-allele
        frequency in the sample is below min_maf are left out.  max_work: the tile-words (tiles
        of 64 x 64 loci x words of 64 chromosomes) the call may take
        -> dict: edges, pairs, mean_r2, sd_r2, mean_dist (Morgans for 'c'), mean_c (c at the mean
        map distance; NaN for 'loci'), expected_w (the mean of Weir & Hill's w(c), so that
        E[mean_r2] ~ expected_w / N_e + 1 / n_chrom; inf in a bin holding a pair at distance 0;
        NaN for 'loci'), n_chrom, n_loci_kept, c1 (1-alleles per locus), loci, ids, work"""
        from ..sim import ld as _ld
        who = 'calc_ld_decay'
        ids, slots, loci_u, pos, mm = self._ld_request(who, individs, loci, unit, min_maf)
        if edges is None:
            edges = _ld.default_edges(unit, n_bins, max_dist, loci_u.size)
        elif max_dist is not None:
            raise ValueError('%s: give edges or max_dist, not both' % who)
        edges = _ld.check_edges(edges)
        dev_edges = _ld.c_to_morgans(edges) if unit == 'c' else edges
        if unit == 'c' and ((edges < 0).any() or (edges[:-1] >= 0.5).any()):
            raise ValueError('%s: edges in c lie in 0..0.5, at most the last at or above 0.5 '
                             '(got %r)' % (who, edges.tolist()))
        max_work = _work_limit(who, max_work, self._LD_MAX_WORK, 'tile-words')
        morgans = unit != 'loci'
        got = self._ld_call(who, loci_u, pos, dev_edges, slots, mm, morgans, max_work)
        work = got['work']
        out = _ld.decay_stats(got['pairs'], got['sum_r2'], got['sum_r4'], got['sum_d'],
                              got['sum_w'], morgans)
        n_chrom = 2 * ids.size
        c1 = got['c1']
        out.update(edges=edges, pairs=got['pairs'], n_chrom=n_chrom,
                   n_loci_kept=int((np.minimum(c1, n_chrom - c1) >= mm).sum()), c1=c1,
                   loci=loci_u, ids=ids, work=work)
        return out

    def _calc_ne(self, method='ld', min_c=0.05, min_maf=0.05, individs=None, loci=None):
        """the linkage-disequilibrium estimate of the effective population size (Waples 2006;
        Weir & Hill 1980) from every pair of loci with recombination fraction >= min_c under the
        architecture's rates (0.5: unlinked pairs only), in one device call:
        N_e = mean w(c) / (mean r^2 - 1 / n_chrom) (sim/ld.ld_ne), for phase-known gametes under
        random mating.  inf when the sample's own 1 / n_chrom explains all the r^2 there is, NaN
        without pairs.  Confidence intervals are out of scope.  The call takes every tile of loci
        at or beyond min_c, up to _LD_MAX_WORK tile-words (above it: ValueError; pass individs
        or loci).
        -> dict: Ne, mean_r2, r2_drift (mean_r2 - 1 / n_chrom), pairs, n_chrom, n_loci_kept,
        min_c"""
        from ..sim import ld as _ld
        who = 'calc_ne'
        if method != 'ld':
            raise ValueError("%s: method: 'ld' (got %r)" % (who, method))
        if not 0.0 <= float(min_c) <= 0.5:
            raise ValueError('%s: min_c: a recombination fraction in 0..0.5 (got %r)'
                             % (who, min_c))
        ids, slots, loci_u, pos, mm = self._ld_request(who, individs, loci, 'c', min_maf)
        # across a break the map puts BREAK_MORGANS: half of it already gives c = 0.5 exactly
        lo = min(float(_ld.c_to_morgans(float(min_c))), _ld.BREAK_MORGANS / 2)
        got = self._ld_call(who, loci_u, pos, np.array([lo, np.inf]), slots, mm, True,
                            self._LD_MAX_WORK)
        n_chrom = 2 * ids.size
        m = int(got['pairs'][0])
        mean = float(got['sum_r2'][0]) / m if m else float('nan')
        c1 = got['c1']
        return dict(Ne=_ld.ld_ne(m, got['sum_r2'][0], got['sum_w'][0], n_chrom), mean_r2=mean,
                    r2_drift=mean - 1.0 / n_chrom, pairs=m, n_chrom=n_chrom,
                    n_loci_kept=int((np.minimum(c1, n_chrom - c1) >= mm).sum()),
                    min_c=float(min_c))

    # -- windowed LD: pruning, clumping, LD scores (sim/ldwin.py; csrc/gnx_ldwin.hip) ---------
    # pairs the edge list of one call may hold by default (16 bytes each on the host)
    _LDW_MAX_EDGES = 1 << 24

    def _ldw_call(self, who, loci, pos, window, slots, min_minor, r2_min, max_edges, max_work,
                  scores):
        """one gnx_ld_window call with its kernel time; the library's refusals of a request
        above max_work or max_edges become ValueErrors with advice"""
        max_work = _work_limit(who, max_work, self._LD_MAX_WORK, 'tile-words')
        if max_edges is None:
            max_edges = self._LDW_MAX_EDGES
        if isinstance(max_edges, bool) or int(max_edges) != max_edges or \
                not (0 if scores else 1) <= max_edges <= 1 << 26:
            raise ValueError('%s: max_edges: a positive integer, at most 2^26 (got %r)'
                             % (who, max_edges))
        try:
            got = _within_max_work(
                who, lambda: self._dev.ld_window(loci, pos, window, slots, min_minor, r2_min,
                                                 int(max_edges), max_work, scores),
                'analyse a sample (n=...), fewer loci (loci=...) or a smaller window, or raise '
                'max_work')
        except nat.GnxError as err:
            if 'exceed max_edges' not in str(err):
                raise
            raise ValueError('%s: n_found = %d pairs of loci above the r2 threshold exceed '
                             'max_edges = %d: ask for a higher r2, a smaller window or fewer '
                             'loci, or a larger max_edges'
                             % (who, getattr(err, 'n_found', -1), max_edges)) from None
        got['kernel_ms'] = self._dev.ld_window_info()['kernel_ms']
        return got

    def _prune_ld(self, r2=0.2, window=50, unit='loci', min_maf=0.05, individs=None, loci=None,
                  max_edges=None, max_work=None):
        """loci in approximate linkage equilibrium (PLINK's --indep-pairwise): of the loci asked
        for (all by default) with a minor-allele frequency of at least min_maf among the living
        individuals asked for, a set no two of which, within `window` of each other (unit as
        _calc_ld_decay), have r^2 >= r2.  The pairs come from the device (gnx_ld_window); the
        choice is greedy on the host (sim/ldwin.greedy_independent) in the order of the
        minor-allele count, the commonest first, ties by locus number
        -> dict: loci (kept, ascending), removed (ascending; the loci below min_maf are in
        neither), claimed_by (per removed locus, the kept locus that removed it), n_edges, c1
        (1-alleles per locus of the request), n_chrom, ids, work, kernel_ms"""
        from ..sim import ldwin as _lw
        who = 'prune_ld'
        r2 = _lw.check_r2(r2, who)
        ids, slots, loci_u, pos, mm = self._ld_request(who, individs, loci, unit, min_maf)
        w = _lw.check_window(window, unit, who)
        got = self._ldw_call(who, loci_u, pos, w, slots, mm, r2, max_edges, max_work, False)
        n_chrom = 2 * ids.size
        c1 = got['c1']
        kept = np.minimum(c1, n_chrom - c1) >= mm
        keep, claimed = _lw.greedy_independent(loci_u.size, got['ei'], got['ej'],
                                               _lw.maf_rank(c1, n_chrom))
        gone = kept & ~keep
        return dict(loci=loci_u[kept & keep], removed=loci_u[gone],
                    claimed_by=loci_u[claimed[gone]], n_edges=got['n_edges'], c1=c1,
                    n_chrom=n_chrom, ids=ids, work=got['work'], kernel_ms=got['kernel_ms'])

    def _clump(self, result, r=0, p1=1e-4, p2=1e-2, r2=0.5, window=250, unit='loci',
               individs=None, max_edges=None, max_work=None):
        """the hits of an association scan as independent signals (PLINK's --clump).  result: a
        dict of _run_gwas, _run_lmm, _run_lfmm or _run_logistic_gea (column r of a two-
        dimensional p).  The tested loci with p <= p2 are visited in the order of p (ties by
        locus number); a locus that no earlier one has claimed becomes an index locus and claims
        every later one within `window` of it (unit as _calc_ld_decay) with r^2 >= r2 among the
        individuals of the scan (or individs); index loci with p > p1 are then dropped with
        their members.  Pairs from the device (gnx_ld_window), the greedy step on the host
        -> dict: index_loci, index_p (ascending p), members (a list of ascending arrays of
        loci, the index locus not among them), n_clumps, n_candidates, n_edges, work,
        kernel_ms, and trait_loci_hit (per clump, whether it holds a locus of
        result['trait_loci']) when the result carries them"""
        from ..sim import ldwin as _lw
        who = 'clump'
        if not isinstance(result, dict) or 'p' not in result or 'loci' not in result:
            raise ValueError("%s: result: the dict of an association scan ('p', 'loci')" % who)
        p = np.asarray(result['p'], dtype=np.float64)
        if p.ndim == 2:
            if isinstance(r, bool) or int(r) != r or not 0 <= r < p.shape[1]:
                raise ValueError('%s: r: a column of p in 0..%d (got %r)'
                                 % (who, p.shape[1] - 1, r))
            p = p[:, int(r)]
        res_loci = np.asarray(result['loci'], dtype=np.int64).ravel()
        if p.ndim != 1 or p.size != res_loci.size:
            raise ValueError('%s: result: p and loci differ in length' % who)
        if not 0.0 <= float(p1) <= float(p2) <= 1.0:
            raise ValueError('%s: 0 <= p1 <= p2 <= 1 (got %r, %r)' % (who, p1, p2))
        r2 = _lw.check_r2(r2, who)
        w = _lw.check_window(window, unit, who)
        tested = np.asarray(result.get('tested', np.isfinite(p)), bool)
        with np.errstate(invalid='ignore'):
            sel = tested & np.isfinite(p) & (p <= p2)
        out = dict(index_loci=np.zeros(0, np.int64), index_p=np.zeros(0), members=[],
                   n_clumps=0, n_candidates=int(sel.sum()), n_edges=0, work=0, kernel_ms=0.0)
        tl = result.get('trait_loci')
        if isinstance(tl, (list, tuple)):
            tl = tl[int(r)] if int(r) < len(tl) else None
        if sel.any():
            if individs is None:
                individs = result.get('ids')
            if (np.diff(res_loci) <= 0).any():
                raise ValueError('%s: result: loci must be ascending' % who)
            # (ascending and distinct: the request's loci are res_loci[sel] in that order)
            ids, slots, loci_u, pos, mm = self._ld_request(who, individs, res_loci[sel], unit,
                                                           0.0)
            pr = p[sel]
            got = self._ldw_call(who, loci_u, pos, w, slots, mm, r2, max_edges, max_work, False)
            keep, claimed = _lw.greedy_independent(loci_u.size, got['ei'], got['ej'],
                                                   _lw.p_rank(pr))
            idx, mem = _lw.clumps(pr, keep, claimed, float(p1))
            out.update(index_loci=loci_u[idx], index_p=pr[idx],
                       members=[loci_u[m] for m in mem], n_clumps=int(idx.size),
                       n_edges=got['n_edges'], work=got['work'], kernel_ms=got['kernel_ms'])
        if tl is not None:
            tl = np.asarray(tl, dtype=np.int64).ravel()
            out['trait_loci_hit'] = np.array(
                [bool(np.isin(np.r_[i, m], tl).any())
                 for i, m in zip(out['index_loci'].tolist(), out['members'])], dtype=bool)
        return out

    def _calc_ld_scores(self, window=100, unit='loci', min_maf=0.05, adjust=True, individs=None,
                        loci=None, max_work=None):
        """the LD score of every locus asked for (all by default): 1 + the sum of its r^2 with
        the loci within `window` of it (unit as _calc_ld_decay) that reach min_maf among the
        living individuals asked for, each r^2 adjusted for the sample's size when adjust
        (sim/ldwin.ld_scores); the counts and the sums come from the device (gnx_ld_window)
        -> dict: ld_score [n_loci] (NaN below min_maf), partners, score (the plain sum), weights
        [L] (1 / max(ld_score, 1), 0 for every other locus: the weights argument of _calc_grm),
        loci, c1, n_chrom, ids, work, kernel_ms"""
        from ..sim import ldwin as _lw
        who = 'calc_ld_scores'
        ids, slots, loci_u, pos, mm = self._ld_request(who, individs, loci, unit, min_maf)
        w = _lw.check_window(window, unit, who)
        n_chrom = 2 * ids.size
        if adjust and n_chrom <= 2:
            raise ValueError('%s: adjust needs at least two individuals' % who)
        got = self._ldw_call(who, loci_u, pos, w, slots, mm, 0.0, 0, max_work, True)
        c1 = got['c1']
        kept = np.minimum(c1, n_chrom - c1) >= mm
        ls = _lw.ld_scores(got['partners'], got['score'], kept, n_chrom, bool(adjust))
        weights = np.zeros(self._dev.L)
        weights[loci_u] = _lw.score_weights(ls)
        return dict(ld_score=ls, partners=got['partners'], score=got['score'], weights=weights,
                    loci=loci_u, c1=c1, n_chrom=n_chrom, ids=ids, work=got['work'],
                    kernel_ms=got['kernel_ms'])

    def _run_ldsc(self, result, scores, r=0, n_blocks=200):
        """LD-score regression (Bulik-Sullivan et al. 2015) on the host: the chi-square of an
        association scan (result: t^2 of column r, or lrt) over its tested loci regressed on
        their LD scores (scores: a dict of _calc_ld_scores), sim/ldwin.ldsc.  An intercept above
        1 is inflation that every locus shares (structure); the slope is polygenic signal
        -> dict: intercept, slope, h2 (slope M / n), intercept_se, slope_se, h2_se, ratio,
        mean_chi2, n_loci, n_blocks"""
        from ..sim import ldwin as _lw
        who = 'run_ldsc'
        if not isinstance(result, dict) or 'loci' not in result or \
                not ('lrt' in result or 't' in result):
            raise ValueError("%s: result: the dict of an association scan ('loci' and 't' or "
                             "'lrt')" % who)
        if not isinstance(scores, dict) or 'ld_score' not in scores or 'loci' not in scores:
            raise ValueError("%s: scores: the dict of calc_ld_scores" % who)
        if 'lrt' in result:
            chi2 = np.asarray(result['lrt'], dtype=np.float64)
        else:
            t = np.asarray(result['t'], dtype=np.float64)
            if t.ndim == 2:
                if isinstance(r, bool) or int(r) != r or not 0 <= r < t.shape[1]:
                    raise ValueError('%s: r: a column of t in 0..%d (got %r)'
                                     % (who, t.shape[1] - 1, r))
                t = t[:, int(r)]
            chi2 = t * t
        res_loci = np.asarray(result['loci'], dtype=np.int64).ravel()
        if chi2.ndim != 1 or chi2.size != res_loci.size:
            raise ValueError('%s: result: the statistic and loci differ in length' % who)
        ls = np.full(self._dev.L, np.nan)
        ls[np.asarray(scores['loci'], dtype=np.int64)] = scores['ld_score']
        x = ls[res_loci]
        use = np.asarray(result.get('tested', np.ones(chi2.size, bool)), bool) & \
            np.isfinite(chi2) & np.isfinite(x)
        n = len(result['ids']) if 'ids' in result else scores['n_chrom'] // 2
        try:
            return _lw.ldsc(chi2[use], x[use], n, int(np.isfinite(scores['ld_score']).sum()),
                            n_blocks)
        except ValueError as err:
            raise ValueError('%s: %s' % (who, err)) from None

    # -- model-based ancestry (sim/ancestry.py; csrc/gnx_admix.hip) ---------------------------
    def _calc_ancestry(self, K, individs=None, loci=None, init='pca', seed=None, accelerate=True,
                       tol=1e-4, max_sweeps=2000, fixed_F=None, budget=None):
        """the admixture model of STRUCTURE / ADMIXTURE fitted by (accelerated) EM to the living
        individuals asked for (all by default) at `loci` (all by default; 'neutral': the loci
        under no selection), every sweep taken on the device from the packed genomes
        (gnx_admix_sweep; sim/ancestry.fit describes the driver, its initialisations and what it
        returns).  fixed_F [K][the loci used]: projection onto held frequencies.  seed None
        with init='random': drawn from the Species' generator.  budget: bytes of partial sums
        per chunk of individuals of one sweep (None: the library's default)
        -> sim/ancestry.fit's dict; individs = the ids (ascending, the rows of Q), loci = the
        loci used (ascending, the columns of F)"""
        import torch
        from ..sim import ancestry as _an
        who = 'calc_ancestry'
        K = _an.check_K(K)
        _need_genomes(self, who)
        ids, slots = self._geno_sample(individs)
        if ids.size < 1:
            raise ValueError('%s: at least one individual' % who)
        if isinstance(loci, str):
            if loci != 'neutral':
                raise ValueError("%s: loci: a list of loci, None or 'neutral' (got %r)"
                                 % (who, loci))
            loci = self.gen_arch.neut_loci
        loci_u, mask = self._geno_loci(loci)
        L_u = self._dev.L if loci_u is None else int(loci_u.size)
        pcs = None
        if isinstance(init, str) and init == 'pca' and K > 1:
            _, pcs, _ = self._calc_genetic_PCA(n_pcs=K - 1, individs=ids, loci=loci_u)
        if seed is None and isinstance(init, str) and init == 'random':
            seed = int(self._rng.randint(0, 2 ** 31 - 1))
        tdev = _torch_device(self)
        sweep = _an.device_sweep(self._dev, slots, loci_u, mask, budget)
        return _an.fit(sweep, ids.size, L_u, K, init=init, seed=seed, accelerate=accelerate,
                       tol=tol, max_sweeps=max_sweeps, fixed_F=fixed_F, pcs=pcs,
                       put=lambda a: torch.as_tensor(np.asarray(a, np.float64), device=tdev),
                       loci=np.arange(L_u, dtype=np.int64) if loci_u is None else loci_u,
                       individs=ids)

    # -- local ancestry along the genome (sim/lai.py; csrc/gnx_lai.hip) ------------------------
    def _calc_local_ancestry(self, ancestry=None, F=None, loci=None, panels=None, prior='fit',
                             gens=10.0, individs=None, by=None, eps=1e-3, calls=False,
                             budget=None):
        """where on the genome the ancestry of the living individuals asked for (all by
        default) lies: the linkage model of Falush et al. (2003) with the frequencies held fixed
        and one admixture time, painted along both haplotypes of every individual on the device
        (gnx_lai_paint; sim/lai.py states the model).  The frequencies come from exactly one of
        ancestry (the dict calc_ancestry returned: its F and loci), F [K][the loci used] with
        loci (None: all; 'neutral'; or an ascending list), or panels (a label 0..K-1 per living
        individual in ascending-id order, -1: in no panel; F = (ones + 0.5) / (2 n_k + 1) of
        each panel's counts).  They are clipped to [eps, 1 - eps].  prior: 'fit' (the Q of
        _calc_ancestry under the held frequencies), 'uniform' or rows [n][K] that sum to 1.
        gens: generations since admixture, or 'fit' (golden-section search on the total
        log-likelihood, forward passes only).  by: a label per analysed individual, 0..63 (-1:
        left out), for anc_locus per group.  calls: also the hard calls and their tracts.
        budget: bytes of device scratch per batch of haplotypes (None: the library's default)
        -> dict: ids, loci, K, gens, gens_trace (when fitted), loglik, loglik_hap [2n], Q_local
        [n][K], Q_prior [n][K], anc_locus [L_u][K] ([G][L_u][K] with by; means over the
        haplotypes), switches [2n], calls uint8 [2n][L_u] and tracts (sim/lai.calls_to_tracts;
        if asked), map_len (Morgans, breaks left out)"""
        import math
        from ..sim import lai as _lai
        from ..sim import ld as _ld
        who = 'calc_local_ancestry'
        _need_genomes(self, who)
        given = [name for name, v in (('ancestry', ancestry), ('F', F), ('panels', panels))
                 if v is not None]
        if len(given) != 1:
            raise ValueError('%s: exactly one of ancestry, F and panels gives the frequencies '
                             '(got %s)' % (who, ', '.join(given) or 'none'))
        if ancestry is not None:
            if loci is not None:
                raise ValueError('%s: ancestry brings its own loci; give no loci' % who)
            try:
                F, loci = ancestry['F'], ancestry['loci']
            except (TypeError, KeyError, IndexError):
                raise ValueError('%s: ancestry: the dict calc_ancestry returned (F and loci)'
                                 % who) from None
        if isinstance(loci, str):
            if loci != 'neutral':
                raise ValueError("%s: loci: a list of loci, None or 'neutral' (got %r)"
                                 % (who, loci))
            loci = self.gen_arch.neut_loci
        if loci is not None and (np.diff(np.asarray(loci, dtype=np.int64).ravel()) <= 0).any():
            raise ValueError('%s: loci: ascending and distinct (they are the columns of F)' % who)
        loci_u, _ = self._geno_loci(loci)
        L_u = self._dev.L if loci_u is None else int(loci_u.size)
        ids, slots = self._geno_sample(individs)
        n = int(ids.size)
        if n < 1:
            raise ValueError('%s: at least one individual' % who)
        if isinstance(eps, bool) or not 0.0 < float(eps) < 0.5:
            raise ValueError('%s: eps: a number in (0, 0.5) (got %r)' % (who, eps))
        if panels is None:
            F = np.array(F, dtype=np.float64)
            if F.ndim != 2 or F.shape[1] != L_u or not np.isfinite(F).all():
                raise ValueError('%s: F: finite frequencies [K][the %d loci used] (got %s)'
                                 % (who, L_u, F.shape))
            K = _lai.check_K(F.shape[0])
        else:
            lab = np.asarray(panels)
            if lab.ndim != 1 or lab.dtype.kind not in 'iu' or lab.size != len(self):
                raise ValueError('%s: panels: one integer label per living individual, in '
                                 'ascending-id order' % who)
            if lab.min() < -1 or lab.max() < 0:
                raise ValueError('%s: panels: labels in -1..K-1 (-1: in no panel)' % who)
            K = _lai.check_K(int(lab.max()) + 1)
            if (np.bincount(lab[lab >= 0], minlength=K) < 1).any():
                raise ValueError('%s: panels: every panel 0..%d holds at least one individual'
                                 % (who, K - 1))
        fit_t = isinstance(gens, str) and gens == 'fit'
        if not fit_t:
            gens = _lai.check_gens(gens)
        fit_q = isinstance(prior, str) and prior == 'fit'
        Q = None if fit_q else _lai.check_prior(prior, n, K)
        by, n_groups = _lai.check_by(by, n)
        if budget is not None and (isinstance(budget, bool) or int(budget) != budget
                                   or budget < 1):
            raise ValueError('%s: budget: a positive number of bytes (got %r)' % (who, budget))
        # ---- from here on the device is asked
        if panels is not None:
            _, n_k, ones, _ = self._group_counts(lab.astype(np.int64), loci_u)
            F = _lai.panel_freqs(ones, n_k)
        F = _lai.clip_freqs(F, eps)
        if fit_q:
            Q = self._calc_ancestry(K, individs=ids, loci=loci_u, fixed_F=F)['Q']
        pos = _ld.map_positions(_rec_rates(self))
        if loci_u is not None:
            pos = pos[loci_u]
        Fd = np.ascontiguousarray(F.T)
        loci_d = None if loci_u is None else loci_u.astype(np.int32)

        def paint(g, post):
            sw, stay = _lai.switch_probs(pos, g)
            return self._dev.lai_paint(Fd, sw, stay, Q, slots, loci_d, by, n_groups, budget,
                                       want_post=post, want_calls=post and bool(calls))

        out = dict(ids=ids, loci=np.arange(L_u, dtype=np.int64) if loci_u is None else loci_u,
                   K=K)
        if fit_t:
            gens, trace = _lai.fit_gens(
                lambda g: math.fsum(paint(g, False)['loglik'].tolist()))
            out['gens_trace'] = np.array(trace)
        got = paint(gens, True)
        ah = got['anc_hap']
        per = np.full(1, 2.0 * n) if by is None else \
            2.0 * np.bincount(by[by >= 0], minlength=n_groups)
        with np.errstate(invalid='ignore', divide='ignore'):
            al = got['anc_locus'] / per[:, None, None]
        d = np.diff(pos)
        brk = np.r_[True, d >= _ld.BREAK_MORGANS / 2]
        out.update(gens=float(gens), loglik=math.fsum(got['loglik'].tolist()),
                   loglik_hap=got['loglik'], Q_local=0.5 * (ah[0::2] + ah[1::2]) / L_u,
                   Q_prior=Q, anc_locus=al[0] if by is None else al, switches=got['switches'],
                   map_len=float(d[~brk[1:]].sum()))
        if calls:
            out['calls'] = got['calls']
            out['tracts'] = _lai.calls_to_tracts(got['calls'], pos, brk, K=K)
        return out

    # -- identity tracts of the phased genomes (sim/tracts.py; csrc/gnx_tracts.hip) -----------
    # word steps (haplotype pairs x genome words) one pair scan may take: 4096 individuals at
    # 10^5 loci are 5.2e10
    _TRACT_MAX_WORK = 1 << 37

    def _tract_request(self, who, individs, unit, min_len, min_loci, n_max, advice):
        """(ids, slots, pos, packed breaks, genome_len, min_len in units, min_loci) of a tract
        request"""
        from ..sim import tracts as _tr
        _need_genomes(self, who)
        if unit not in ('morgans', 'loci'):
            raise ValueError("%s: unit: 'morgans' or 'loci', not %r" % (who, unit))
        if isinstance(min_loci, bool) or int(min_loci) != min_loci or min_loci < 1:
            raise ValueError('%s: min_loci: a number of loci >= 1 (got %r)' % (who, min_loci))
        if isinstance(min_len, bool) or not 0 <= float(min_len) < np.inf:
            raise ValueError('%s: min_len: a finite length >= 0 in %s (got %r)'
                             % (who, unit, min_len))
        ids, slots = self._geno_sample(individs)
        if ids.size < 1 or ids.size > n_max:
            raise ValueError('%s: 1..%d individuals per call (got %d)%s'
                             % (who, n_max, ids.size, advice))
        pos, brk, genome_len = _tr.tract_map(_rec_rates(self), unit)
        return (ids, slots, pos, _tr.pack_breaks(brk, self._dev.W64), genome_len,
                _tr.to_units(min_len, unit), int(min_loci))

    def _tract_edges(self, who, edges, unit):
        from ..sim import tracts as _tr
        if edges is None:
            return None
        e = np.asarray(edges, dtype=np.float64).ravel()
        if not 2 <= e.size <= 65 or np.isnan(e).any() or (e < 0).any() or \
                (np.diff(e) <= 0).any():
            raise ValueError('%s: tract length edges: 2..65 ascending lengths >= 0 (got %r)'
                             % (who, edges))
        return _tr.check_tract_edges([_tr.to_units(v, unit) for v in e])

    def _calc_roh(self, min_len=0.01, min_loci=50, unit='morgans', individs=None, edges=None,
                  cover=False):
        """runs of homozygosity: the tracts over which an individual's two homologues are
        identical, no shorter than min_len (in the unit: Morgans on the architecture's map, or
        loci) and min_loci loci, for the living individuals asked for (all by default), scanned
        on the device (gnx_tracts_self).  A recombination rate of 0.5 or more is a chromosome
        boundary that no tract crosses: under the template's free recombination every locus is
        a break, so every tract is one locus long.  edges: bounds of a histogram of tract
        lengths (in the unit; the last may be inf).  cover: per locus, the individuals with a
        run over it (ROH islands)
        -> dict: ids, n_roh, roh_loci, roh_len, longest (per individual; lengths in the unit),
        f_roh (roh_len / genome_len; for 'loci' roh_loci / L), mean_f_roh, genome_len, hist
        (dict(edges, tracts, sum_len) if edges), cover (if asked), unit"""
        from ..sim import tracts as _tr
        who = 'calc_roh'
        ids, slots, pos, brk, genome_len, ml, mloci = self._tract_request(
            who, individs, unit, min_len, min_loci, 2 ** 25,
            ': sample them with n=... or individs=...')
        e = self._tract_edges(who, edges, unit)
        got = self._dev.tracts_self(pos, brk, mloci, ml, e, slots, bool(cover))
        per = got['per']
        f, mean_f = _tr.roh_stats(per[:, 1], per[:, 2], genome_len, self._dev.L, unit)
        out = dict(ids=ids, n_roh=per[:, 0].copy(), roh_loci=per[:, 1].copy(),
                   roh_len=_tr.from_units(per[:, 2], unit),
                   longest=_tr.from_units(per[:, 3], unit), f_roh=f, mean_f_roh=mean_f,
                   genome_len=float(_tr.from_units(genome_len, unit)), unit=unit)
        if e is not None:
            out['hist'] = _tract_hist(edges, got['hist'], unit)
        if cover:
            out['cover'] = got['cover']
        return out

    def _calc_ibs_sharing(self, min_len=0.02, min_loci=50, unit='morgans', individs=None,
                          edges=None, n_classes=10, max_dist=None, tract_edges=None, cover=False,
                          max_work=None):
        """long tracts shared identical-by-state between individuals as a function of their
        geographic distance (the recent-dispersal signal of Ringbauer et al. 2017): for every
        two of the individuals asked for (at most 4096) the tracts, no shorter than min_len (in
        the unit) and min_loci loci, over which one haplotype of the one equals one haplotype of
        the other (four haplotype pairs), scanned on the device (gnx_tracts_pairs).  Under the
        template's free recombination every locus is a break, so every tract is one locus long.
        edges: the distance classes' bounds (default n_classes classes of equal width in ln r
        from one landscape cell to max_dist; default a quarter of the shorter side).
        tract_edges: bounds of a histogram of tract lengths (in the unit).  cover: per locus, the
        haplotype pairs with a tract over it.  max_work: the word steps (haplotype pairs x
        genome words) the call may take
        -> dict: ids, n_tracts, shared_len, longest ([n][n], the diagonal the individual's own
        runs of homozygosity; lengths in the unit), by_dist (dict: edges, pairs, mean_tracts,
        mean_len, share_with_tract, mean_dist per class), hist (or None), cover (or None), work,
        unit"""
        from ..sim import tracts as _tr
        who = 'calc_ibs_sharing'
        ids, slots, pos, brk, _, ml, mloci = self._tract_request(
            who, individs, unit, min_len, min_loci, 4096,
            ' (the matrices are n x n): sample them with n=... or individs=...')
        edges = _distance_classes(self, who, edges, n_classes, max_dist)
        te = self._tract_edges(who, tract_edges, unit)
        max_work = _work_limit(who, max_work, self._TRACT_MAX_WORK, 'word steps')
        got = _within_max_work(
            who, lambda: self._dev.tracts_pairs(pos, brk, mloci, ml, te, slots, bool(cover),
                                                max_work),
            'analyse a sample (n=... or individs=...), or raise max_work')
        x = self._field(nat.F_X)[slots]
        y = self._field(nat.F_Y)[slots]
        by = _tr.sharing_stats(x, y, got['cnt'], got['len'], edges)
        by['mean_len'] = _tr.from_units(by['mean_len'], unit)
        by['edges'] = edges
        hist = None if te is None else _tract_hist(tract_edges, got['hist'], unit)
        return dict(ids=ids, n_tracts=got['cnt'], shared_len=_tr.from_units(got['len'], unit),
                    longest=_tr.from_units(got['longest'], unit), by_dist=by, hist=hist,
                    cover=got['cover'], work=got['work'], unit=unit)

    # -- haplotype sweep scans (sim/sweeps.py; csrc/gnx_sweeps.hip) ----------------------------
    # word steps (scanned cores x 4 scans x chromosome words x kept loci) one call may take: the
    # bound no scan reaches, since a scan ends at its cutoff
    _SWEEP_MAX_WORK = 1 << 42

    def _sweep_request(self, who, individs, loci, unit, min_maf, cutoff, max_gap, max_extent,
                       max_work):
        """what the sweep calls share: the request checks of _ld_request, the integer map of the
        unit (for 'sites' after a probe call that only counts c1), the thresholds as integers
        -> dict(ids, slots, loci, pos, brk, scale, min_minor, kw), kw the keyword arguments of
        Device.sweeps_scan"""
        from ..sim import sweeps as _sw
        if unit not in ('morgans', 'loci', 'sites'):
            raise ValueError("%s: unit: 'morgans', 'loci' or 'sites', not %r" % (who, unit))
        num, den = _sw.cutoff_fraction(cutoff)
        lim = {}
        for name, v in (('max_gap', max_gap), ('max_extent', max_extent)):
            if v is not None and (isinstance(v, bool) or not 0 < float(v) < np.inf):
                raise ValueError('%s: %s: a positive length in %s, or None (got %r)'
                                 % (who, name, unit, v))
            lim[name] = v
        max_work = _work_limit(who, max_work, self._SWEEP_MAX_WORK, 'word steps')
        ids, slots, loci_u, _, mm = self._ld_request(who, individs, loci, 'loci', min_maf)
        if ids.size > _sw.MAX_N:
            raise ValueError('%s: 1..%d individuals per call (got %d): sample them with n=... or '
                             'individs=...' % (who, _sw.MAX_N, ids.size))
        mm = max(2, mm)
        rates = _rec_rates(self)
        kept = None
        if unit == 'sites':
            probe = self._dev.sweeps_scan(loci_u, loci_u, slots=slots, min_minor=mm, max_work=0)
            kept = np.zeros(self._dev.L, bool)
            kept[loci_u] = _sw.kept_loci(probe['c1'], 2 * ids.size, mm)
        pos, brk, scale = _sw.sweep_map(rates, unit, kept)
        nb = np.cumsum(brk)
        b = np.zeros(loci_u.size, np.uint8)
        b[1:] = nb[loci_u[1:]] > nb[loci_u[:-1]]
        kw = dict(min_minor=mm, cut_num=num, cut_den=den, max_work=int(max_work))
        for name, v in lim.items():
            kw[name] = 0 if v is None else max(1, int(np.floor(float(v) * scale)))
        return dict(ids=ids, slots=slots, loci=loci_u, pos=pos[loci_u], brk=b, scale=scale,
                    min_minor=mm, kw=kw)

    def _sweep_call(self, who, rq, cls=None, cores=None, curve=False):
        """one gnx_sweeps_scan call; the library's refusal of a request above max_work becomes a
        ValueError with advice"""
        return _within_max_work(
            who, lambda: self._dev.sweeps_scan(rq['loci'], rq['pos'], rq['brk'], cls, cores,
                                               rq['slots'], curve=curve, **rq['kw']),
            'analyse a sample (n=...) or fewer loci (loci=...), or raise max_work')

    def _calc_ihs(self, unit='morgans', min_maf=0.05, cutoff=0.05, max_gap=None, max_extent=None,
                  individs=None, loci=None, n_freq_bins=20, keep_edge=False, max_work=None):
        """the integrated haplotype score of every locus (Voight et al. 2006) from the phased
        genomes of the living individuals asked for (at most 2048), scanned on the device
        (gnx_sweeps_scan): around each core locus the haplotypes carrying the derived allele (1)
        and those carrying the ancestral one (0) are followed outwards in both directions until
        their EHH - the share of pairs still identical - falls below cutoff, and the area under
        each curve is iHH.  unit: 'morgans' on the map of the architecture's recombination rates,
        'loci' (locus numbers) or 'sites' (the rank among the loci kept: nSL).  Loci whose
        minor-allele frequency in the sample is below min_maf (or whose minor count is below 2)
        are neither cores nor steps.  A recombination rate of 0.5 or more is a chromosome
        boundary no scan crosses: under the template's free recombination every scan ends at
        once.  max_gap, max_extent (in the unit): a scan stops before a step longer than max_gap
        and before leaving max_extent around the core.  A locus one of whose scans reached an
        edge, a break or a gap before the cutoff has no score unless keep_edge.  ihs is ihs_unstd
        standardised within n_freq_bins bins of the derived-allele frequency.  max_work: the
        word steps (cores x 4 scans x words of 64 chromosomes x kept loci) the call may take
        -> dict: loci, pos (in the unit), freq (of allele 1), ihh1, ihh0 (in the unit),
        ihs_unstd = ln(ihh1 / ihh0), ihs, status [n_loci][2][2] ([direction: left, right]
        [class]; 0 cutoff, 1 edge or break, 2 gap, 3 extent, 4 class below two chromosomes, 5 not
        scanned), steps, kept, c1, n_chrom, work, ids, unit"""
        from ..sim import sweeps as _sw
        who = 'calc_ihs'
        rq = self._sweep_request(who, individs, loci, unit, min_maf, cutoff, max_gap, max_extent,
                                 max_work)
        got = self._sweep_call(who, rq)
        n_chrom = 2 * rq['ids'].size
        c1 = got['c1']
        unstd, h1, h0 = _sw.ihs_unstandardized(got['area'], got['status'], c1, n_chrom,
                                               keep_edge=bool(keep_edge))
        freq = c1 / float(n_chrom)
        return dict(loci=rq['loci'], pos=rq['pos'] / float(rq['scale']), freq=freq,
                    ihh1=h1 / rq['scale'], ihh0=h0 / rq['scale'], ihs_unstd=unstd,
                    ihs=_sw.standardize_by_frequency(unstd, freq, n_freq_bins),
                    status=got['status'], steps=got['steps'],
                    kept=_sw.kept_loci(c1, n_chrom, rq['min_minor']), c1=c1, n_chrom=n_chrom,
                    work=got['work'], ids=rq['ids'], unit=unit)

    def _calc_xpehh(self, groups, unit='morgans', min_maf=0.05, cutoff=0.05, max_gap=None,
                    max_extent=None, individs=None, loci=None, keep_edge=False, max_work=None):
        """the cross-population extended haplotype homozygosity of every locus (Sabeti et al.
        2007) between two groups of individuals (groups as calc_fst takes them; exactly two
        groups; individs restricts both), scanned on the device: around each core locus the
        haplotypes of group a and those of group b are followed outwards, whatever allele they
        carry at the core, and xpehh_unstd = ln(iHH_a / iHH_b); positive where group a carries
        the longer haplotypes.  Loci are kept by their frequency in the two groups pooled.  One
        departure from selscan: each population is scanned to its own cutoff, not until the
        pooled EHH falls below it.  The other arguments as calc_ihs
        -> dict: loci, pos, ihh_a, ihh_b, xpehh_unstd, xpehh (standardised over all defined
        loci), status, steps, kept, c1, names, n_a, n_b, work, ids, unit"""
        from ..sim import fst as _fst
        from ..sim import sweeps as _sw
        who = 'calc_xpehh'
        # (the request checks come first: every living individual, as the groups see them)
        all_ids = self._ld_request(who, None, None, 'loci', min_maf)[0]
        names, order, start = _fst.make_groups(all_ids, groups)
        if len(names) != 2:
            raise ValueError('%s: exactly two groups (got %d)' % (who, len(names)))
        member = np.full(all_ids.size, -1, np.int64)
        member[order[:start[1]]] = 0
        member[order[start[1]:]] = 1
        if individs is not None:
            ids_in = np.asarray(individs, dtype=np.int64).ravel()
            member[~np.isin(all_ids, ids_in)] = -1
        sample = all_ids[member >= 0]
        rq = self._sweep_request(who, sample, loci, unit, min_maf, cutoff, max_gap, max_extent,
                                 max_work)
        grp = member[np.searchsorted(all_ids, rq['ids'])]
        n_a, n_b = int((grp == 0).sum()), int((grp == 1).sum())
        got = self._sweep_call(who, rq, cls=np.repeat(grp, 2).astype(np.uint8))
        ha, hb = _sw.ihh_both(got['area'], got['status'], _sw.class_pairs(2 * n_a),
                              _sw.class_pairs(2 * n_b), keep_edge=bool(keep_edge))
        unstd = _sw.log_ratio(ha, hb)
        n_chrom = 2 * rq['ids'].size
        return dict(loci=rq['loci'], pos=rq['pos'] / float(rq['scale']), ihh_a=ha / rq['scale'],
                    ihh_b=hb / rq['scale'], xpehh_unstd=unstd, xpehh=_sw.standardize(unstd),
                    status=got['status'], steps=got['steps'],
                    kept=_sw.kept_loci(got['c1'], n_chrom, rq['min_minor']), c1=got['c1'],
                    names=names, n_a=n_a, n_b=n_b, work=got['work'], ids=rq['ids'], unit=unit)

    def _calc_ehh(self, locus, unit='morgans', min_maf=0.05, cutoff=0.05, max_gap=None,
                  max_extent=None, individs=None, loci=None, max_work=None):
        """the decay of extended haplotype homozygosity around one core locus (Sabeti et al.
        2002), scanned on the device: per kept locus the scan reached, the share of pairs of
        haplotypes carrying the derived (ehh1) or the ancestral allele (ehh0) at the core that
        are still identical from the core to there; 1 at the core, NaN at loci that are not kept
        and past the scan's end (the first value below the cutoff is included).  The arguments
        as calc_ihs; the core must be a kept locus
        -> dict: locus, loci, pos, ehh1, ehh0, status [2][2], steps [2][2], c1 (of the core),
        n_chrom, ids, unit"""
        from ..sim import sweeps as _sw
        who = 'calc_ehh'
        if isinstance(locus, bool) or int(locus) != locus:
            raise ValueError('%s: locus: one locus number (got %r)' % (who, locus))
        rq = self._sweep_request(who, individs, loci, unit, min_maf, cutoff, max_gap, max_extent,
                                 max_work)
        core = int(np.searchsorted(rq['loci'], int(locus)))
        if core >= rq['loci'].size or rq['loci'][core] != int(locus):
            raise ValueError('%s: locus %d is not among the loci of the request'
                             % (who, int(locus)))
        got = self._sweep_call(who, rq, cores=[core], curve=True)
        n_chrom = 2 * rq['ids'].size
        c1 = got['c1']
        kept = _sw.kept_loci(c1, n_chrom, rq['min_minor'])
        if not kept[core]:
            raise ValueError('%s: locus %d is not kept: %d of %d chromosomes carry allele 1, the '
                             'minor count is below %d (min_maf)'
                             % (who, int(locus), c1[core], n_chrom, rq['min_minor']))
        T = (_sw.class_pairs(n_chrom - c1[core]), _sw.class_pairs(c1[core]))
        e0, e1 = _sw.ehh_curve(got['curve'], kept, core, T, rq['loci'].size)
        return dict(locus=int(locus), loci=rq['loci'], pos=rq['pos'] / float(rq['scale']),
                    ehh1=e1, ehh0=e0, status=got['status'][core], steps=got['steps'][core],
                    c1=int(c1[core]), n_chrom=n_chrom, ids=rq['ids'], unit=unit)

    # -- lineages through the recorded pedigree (structs/pedigree.py; csrc/gnx_lineage.hip) ----
    # The reference simplifies its tables with tskit's default, which drops unary nodes: its
    # lineage at a locus lists only the ancestors that survive simplification for the current
    # sample.  The simplification here (_sort_and_simplify_table_collection) drops only the rows
    # no lineage of the living passes through and keeps unary nodes, so a lineage lists EVERY
    # ancestor.  _check_coalescence is the same either way (two lineages share
    # their oldest in-simulation node exactly when they coalesce inside the simulation); the
    # statistics are taken to the oldest in-simulation ancestor of the full pedigree, and no
    # parity with tskit's simplification is claimed.
    _LINEAGE_DICT_MAX = 2000000          # chain entries _get_lineage_dicts turns into dicts

    def _lineage_request(self, individs, nodes, loci, who):
        """(the TreeTables, sample node ids int64, loci int64) of a lineage request"""
        _need_pedigree(self, who)
        tt = self._tt
        if nodes is None:
            if individs is None:
                ids, order = self._ids_sorted()
                ids = ids[order]
            else:
                ids = np.asarray(individs, dtype=np.int64).ravel()
            rows = np.searchsorted(tt.ids, ids)
            if ids.size and not (tt.ids[np.minimum(rows, tt.ids.size - 1)] == ids).all():
                raise ValueError('%s: individs holds ids the pedigree does not know' % who)
            nodes = (2 * rows[:, None] + np.arange(2)[None, :]).ravel()
        nodes = np.asarray(nodes, dtype=np.int64).ravel()
        if nodes.size == 0:
            raise ValueError('%s: no sample nodes' % who)
        if nodes.min() < 0 or nodes.max() >= 2 * tt.ids.size:
            raise ValueError('%s: nodes are node ids of the pedigree tables, 0..%d'
                             % (who, 2 * tt.ids.size - 1))
        L = self.gen_arch.L
        loci = np.arange(L, dtype=np.int64) if loci is None else \
            np.asarray(loci, dtype=np.int64).ravel()
        if loci.size == 0 or loci.min() < 0 or loci.max() >= L:
            raise ValueError('%s: loci: a non-empty list of loci in 0..%d' % (who, L - 1))
        return tt, nodes, loci

    def _lineage_curr_xy(self, tt, nodes):
        """current x, y [n][2] of the sample nodes' individuals, read from the device columns
        (as _get_coords); NaN rows for individuals that are not alive"""
        ids, order = self._ids_sorted()
        ids = ids[order]
        xy = np.stack([self._field(nat.F_X)[order].astype(np.float64),
                       self._field(nat.F_Y)[order].astype(np.float64)], axis=1)
        want = tt.ids[nodes >> 1]
        pos = np.minimum(np.searchsorted(ids, want), max(ids.size - 1, 0))
        out = np.full((nodes.size, 2), np.nan)
        alive = ids[pos] == want if ids.size else np.zeros(nodes.size, bool)
        out[alive] = xy[pos[alive]]
        return out

    def _get_lineage_dicts(self, loci, nodes=None, drop_before_sim=True,
                           time_before_present=True, use_individs_curr_pos=True,
                           max_time_ago=None, min_time_ago=None):
        """{locus: {sample node: {lineage node: (birth time, array([x, y]))}}}, youngest node
        first (reference structs/species.py:1242-1276, structs/genome.py:1638-1760), the chains
        walked on the device (gnx_lineage_chains).  Node ids are those of this Species'
        pedigree tables (2 * row + homologue); `nodes` defaults to both nodes of every living
        individual in ascending id order.  Times are time + t if time_before_present, and the
        window min_time_ago..max_time_ago applies to the times as returned, as there.
        use_individs_curr_pos puts the individual's current x, y (device columns) in the
        sample node's own entry when that entry is among the kept nodes; the reference raises
        KeyError when it is not, here the dict is left as it is.  The lineages list every
        ancestor: a simplification keeps unary nodes (see the comment above).  Meant for
        plotting-sized requests: above _LINEAGE_DICT_MAX chain entries it raises ValueError - use
        _calc_lineage_stats(as_arrays=True) or _check_coalescence."""
        who = '_get_lineage_dicts'
        tt, nodes, loci = self._lineage_request(None, nodes, loci, who)
        lo, hi = min_time_ago, max_time_ago
        if not time_before_present:           # the window is on the raw table times then
            lo = None if lo is None else lo + self.t
            hi = None if hi is None else hi + self.t
        tab, bt = tt.node_table()
        kw = dict(drop_before_sim=drop_before_sim, min_time_ago=lo, max_time_ago=hi)
        n_kept = self._dev.lineage_trace(tab, bt, nodes, loci, self.t, want=('n_kept',),
                                         locus_range=False, **kw)['n_kept']
        total = int(n_kept.sum(dtype=np.int64))
        if total > self._LINEAGE_DICT_MAX:
            raise ValueError('%s: %d lineage entries (more than %d): nested dicts are for '
                             'plotting-sized requests; use _calc_lineage_stats(as_arrays=True) '
                             'or _check_coalescence' % (who, total, self._LINEAGE_DICT_MAX))
        off, chain = self._dev.lineage_chains(tab, bt, nodes, loci, self.t, n_kept=n_kept, **kw)
        times = bt[chain >> 1].astype(np.float64) + (self.t if time_before_present else 0)
        xy = tt._ind_xy[0][chain >> 1]
        curr = self._lineage_curr_xy(tt, nodes) if use_individs_curr_pos else None
        out = {}
        n = nodes.size
        for i, locus in enumerate(loci.tolist()):
            d_loc = out[locus] = {}
            for j, node in enumerate(nodes.tolist()):
                a, b = off[i * n + j], off[i * n + j + 1]
                d = {int(c): (float(tm), np.array(p)) for c, tm, p in
                     zip(chain[a:b].tolist(), times[a:b], xy[a:b])}
                if curr is not None and node in d:
                    if np.isnan(curr[j, 0]):
                        raise ValueError('%s: use_individs_curr_pos: the individual of node %d '
                                         'is not alive' % (who, node))
                    d[node] = (d[node][0], curr[j].copy())
                d_loc[node] = d
        return out

    def _calc_lineage_stats(self, individs=None, nodes=None, loci=None,
                            stats=['dir', 'dist', 'time', 'speed'], use_individs_curr_pos=True,
                            max_time_ago=None, min_time_ago=None, as_arrays=False):
        """Gene-flow statistics of the lineages of the sample nodes at the loci (reference
        structs/species.py:1309-1343, structs/genome.py:1786-1871): 'dir' the compass
        direction in degrees from the oldest kept node's birth location to the youngest's,
        'dist' and 'time' oldest minus youngest, 'speed' = dist / time.  The youngest and
        oldest kept node of every (locus, node) come from the device (gnx_lineage_trace); the
        floats are computed here in fp64 with the reference's formulas.  -> {stat: {locus:
        [value per node]}} with None where a lineage has fewer than two kept nodes; with
        as_arrays (an extension) {stat: float64 [n_loci][n_nodes] (NaN there), 'nodes', 'loci'}.
        individs are Geonomics ids (default: all living, ascending, two nodes each); nodes are
        node ids of this Species' pedigree tables.  use_individs_curr_pos as in
        _get_lineage_dicts.  The statistics reach back to the oldest in-simulation ancestor of
        the FULL pedigree: the reference's simplified tables list fewer ancestors (see the
        comment above _lineage_request)."""
        from . import pedigree as _ped
        who = '_calc_lineage_stats'
        for st in stats:
            if st not in _ped.LINEAGE_STATS:
                raise ValueError("%s: the only valid statistics are 'dir', 'dist', 'time' and "
                                 "'speed', not %r" % (who, st))
        tt, nodes, loci = self._lineage_request(individs, nodes, loci, who)
        tab, bt = tt.node_table()
        tr = self._dev.lineage_trace(tab, bt, nodes, loci, self.t, drop_before_sim=True,
                                     min_time_ago=min_time_ago, max_time_ago=max_time_ago,
                                     want=('first', 'last', 'n_kept'), locus_range=False)
        curr = self._lineage_curr_xy(tt, nodes) if use_individs_curr_pos else None
        vals = _ped.lineage_stats(tt, nodes, tr['first'], tr['last'], tr['n_kept'], self.t,
                                  stats, curr_xy=curr)
        if as_arrays:
            return dict(vals, nodes=nodes, loci=loci)
        return {st: {locus: [None if v != v else v for v in vals[st][i].tolist()]
                     for i, locus in enumerate(loci.tolist())} for st in stats}

    def _check_coalescence(self, individs=None, loci=None, all_loci=False):
        """whether the lineages of the individuals' nodes (default: all living) have coalesced
        inside the simulation at each locus (default: all) -> {locus: bool}, or one bool for
        all of them if all_loci (reference structs/species.py:1282-1306): the oldest
        in-simulation node is the same for every sample node.  Reduced on the device to a min
        and a max per locus (gnx_lineage_trace): nothing n_loci x n_nodes comes back.  A locus
        at which some sample node has no in-simulation node at all is not coalesced."""
        tt, nodes, loci = self._lineage_request(individs, None, loci, '_check_coalescence')
        tab, bt = tt.node_table()
        tr = self._dev.lineage_trace(tab, bt, nodes, loci, self.t, want=(), locus_range=True)
        co = (tr['locus_lo'] == tr['locus_hi']) & (tr['locus_lo'] >= 0)
        if all_loci:
            return bool(co.all())
        return {locus: bool(c) for locus, c in zip(loci.tolist(), co)}

    # -- pairwise coalescence through the recorded pedigree (sim/coal.py; csrc/gnx_coal.hip) ---
    # look-up chains (pairs of sample nodes x loci) one call may take: 4096 nodes at 10^4 loci
    # are 8.4e10
    _COAL_MAX_WORK = 1 << 37

    def _coal_request(self, who, individs):
        """(the TreeTables, ids ascending, their slots, sample nodes: both of every individual in
        id order) of a coalescence request.  The individuals must be living: a simplified table
        is exact only on the lineages of the living"""
        _need_pedigree(self, who)
        ids, slots = self._geno_sample(individs)
        if ids.size < 1 or ids.size > 2048:
            raise ValueError('%s: 1..2048 individuals (4096 sample nodes) per call (got %d): '
                             'sample them with n=... or individs=...' % (who, ids.size))
        tt, nodes, _ = self._lineage_request(ids, None, None, who)
        return tt, ids, slots, nodes

    @staticmethod
    def _coal_max_ago(who, max_time_ago):
        if max_time_ago is not None and not float(max_time_ago) >= 0:
            raise ValueError('%s: max_time_ago: a number of steps >= 0, or None (got %r)'
                             % (who, max_time_ago))
        return max_time_ago

    def _calc_tmrca(self, individs=None, loci=None, max_time_ago=None, time_edges=None,
                    n_time_bins=20, dist_edges=None, n_classes=10, max_dist=None, groups=None,
                    return_mrca=False, max_work=None):
        """the time to the most recent common ancestor (TMRCA) of every two sample nodes - both
        homologues of the living individuals asked for (all by default, at most 2048) - at every
        locus asked for, from the recorded pedigree, merged on the device (gnx_coal_times).  A
        pair coalesces at a locus when its two lineages meet in one node no older than
        max_time_ago steps (None: anywhere in the tables, the founders included); T is that
        node's age in steps before now.  Means are over the (pair, locus) cells that coalesce,
        and share_coalesced says how many do.  time_edges: integer bounds of the histogram of T
        (default n_time_bins bins over 0 .. max_time_ago, or 0 .. the founders' age).  dist_edges,
        n_classes, max_dist: the distance classes of by_dist, as calc_spatial_structure.  groups
        as calc_fst takes them.  return_mrca: also the MRCA node of every (locus, pair).
        max_work bounds the look-up chains (pairs x loci) of the device call
        -> dict: ids, nodes (2 row + homologue in the pedigree tables, two per individual), loci,
        tmrca float64 [n_nodes][n_nodes] (NaN where the pair never coalesces), n_coalesced int32
        [n_nodes][n_nodes], per_locus (dict: mean, share_coalesced, max), diversity_branch (2 x
        mean T), by_group (dict: names, within, between; or None), by_dist (dict: edges, pairs,
        mean_tmrca, share_coalesced, mean_dist over the pairs of different individuals; None
        with one individual), coal_times (dict: edges, counts, at_risk, ne: the inverse
        coalescence rate 1 / (2 p) per bin, sim/coal.coal_rate), share_coalesced, mrca (int32
        [n_loci][n_pairs], -1 where the pair does not coalesce; or None), work"""
        from ..sim import coal as _co
        from ..sim import fst as _fst
        who = 'calc_tmrca'
        tt, ids, slots, nodes = self._coal_request(who, individs)
        loci = self._lineage_request(ids, None, loci, who)[2]
        max_time_ago = self._coal_max_ago(who, max_time_ago)
        if time_edges is None:
            top = self.t + 1 if max_time_ago is None else min(self.t + 1, int(max_time_ago))
            te = _co.default_time_edges(max(top, 0), n_time_bins)
        else:
            te = np.asarray(time_edges, dtype=np.float64).ravel()
            if not 2 <= te.size <= 64 or (te != np.rint(te)).any() or (np.diff(te) <= 0).any() \
                    or te[0] < 0 or te[-1] >= 2 ** 31:
                raise ValueError('%s: time_edges: 2..64 strictly ascending whole numbers of '
                                 'steps >= 0 (got %r)' % (who, time_edges))
            te = te.astype(np.int64)
        # (no T is negative, so an edge at 0 in front counts the cells that coalesce before te[0])
        dev_te = te if te[0] == 0 else np.r_[0, te]
        member = None
        if groups is not None:
            all_ids = self._geno_sample(None)[0]
            names, order, start = _fst.make_groups(all_ids, groups)
            label = np.full(all_ids.size, -1, np.int64)
            label[order] = np.repeat(np.arange(len(names)), np.diff(start))
            member = label[np.searchsorted(all_ids, ids)]
        if ids.size >= 2:
            dist_edges = _distance_classes(self, who, dist_edges, n_classes, max_dist)
        max_work = _work_limit(who, max_work, self._COAL_MAX_WORK, 'look-up chains')
        tab, bt = tt.node_table()
        want = ('pair_sum', 'pair_cnt', 'locus_sum', 'locus_cnt', 'locus_max') + \
            (('mrca',) if return_mrca else ())
        got = _within_max_work(
            who, lambda: self._dev.coal_times(tab, bt, nodes, loci, self.t, max_time_ago, dev_te,
                                              want, max_work),
            'analyse a sample (n=... or individs=...) or fewer loci (loci=...), or raise '
            'max_work')
        tm, per, share = _co.tmrca_stats(got['pair_sum'], got['pair_cnt'], got['locus_sum'],
                                         got['locus_cnt'], got['locus_max'])
        node_groups = None if member is None else \
            [np.flatnonzero(np.repeat(member, 2) == g) for g in range(len(names))]
        div, by_group = _co.branch_diversity(got['pair_sum'], got['pair_cnt'], node_groups)
        if by_group is not None:
            by_group['names'] = names
        by_dist = None
        if ids.size >= 2:
            by_dist = _co.tmrca_by_distance(self._field(nat.F_X)[slots],
                                            self._field(nat.F_Y)[slots], got['pair_sum'],
                                            got['pair_cnt'], loci.size, dist_edges)
            by_dist['edges'] = dist_edges
        th = got['thist']
        before = 0 if te[0] == 0 else int(th[0])
        rate = _co.coal_rate(th if te[0] == 0 else th[1:], te, got['work'], before)
        return dict(ids=ids, nodes=nodes, loci=loci, tmrca=tm, n_coalesced=got['pair_cnt'],
                    per_locus=per, diversity_branch=div, by_group=by_group, by_dist=by_dist,
                    coal_times=rate, share_coalesced=share, mrca=got.get('mrca'),
                    work=got['work'])

    def _calc_ibd(self, max_time_ago=None, min_len=0.02, min_loci=50, unit='morgans',
                  individs=None, edges=None, n_classes=10, max_dist=None, tract_edges=None,
                  cover=False, max_work=None):
        """the segments shared identical BY DESCENT between the haplotypes of the living
        individuals asked for (all by default, at most 2048), from the recorded pedigree: the
        stretches of loci, no shorter than min_len (in the unit, as calc_ibs_sharing) and
        min_loci loci, over which two haplotypes have one and the same most recent common
        ancestor no older than max_time_ago steps (None: anywhere in the tables), merged on the
        device (gnx_coal_segments).  The truth beside calc_ibs_sharing and calc_roh, which report
        identity by state.  A recombination rate of 0.5 or more is a chromosome boundary no
        segment crosses.  The matrices are folded from haplotypes to individuals as
        calc_ibs_sharing's: off the diagonal the four haplotype pairs of two individuals, on the
        diagonal the individual's own two haplotypes.  hist and cover count every pair of
        haplotypes, an individual's own included
        -> calc_ibs_sharing's dict (ids, n_tracts, shared_len, longest, by_dist, hist, cover,
        work, unit) and f_ibd (per individual: the length its own two haplotypes share over
        genome_len, the realised autozygosity within max_time_ago, which f_roh estimates),
        genome_len"""
        from ..sim import coal as _co
        from ..sim import tracts as _tr
        who = 'calc_ibd'
        _need_pedigree(self, who)
        ids, slots, pos, _, genome_len, ml, mloci = self._tract_request(
            who, individs, unit, min_len, min_loci, 2048,
            ' (4096 sample nodes): sample them with n=... or individs=...')
        tt, ids, slots, nodes = self._coal_request(who, ids)
        max_time_ago = self._coal_max_ago(who, max_time_ago)
        brk = _tr.tract_map(_rec_rates(self), unit)[1]
        edges = _distance_classes(self, who, edges, n_classes, max_dist)
        te = self._tract_edges(who, tract_edges, unit)
        max_work = _work_limit(who, max_work, self._COAL_MAX_WORK, 'look-up chains')
        tab, bt = tt.node_table()
        loci = np.arange(self._dev.L)
        got = _within_max_work(
            who, lambda: self._dev.coal_segments(tab, bt, nodes, loci, pos, self.t, brk,
                                                 max_time_ago, mloci, ml, te, bool(cover),
                                                 max_work),
            'analyse a sample (n=... or individs=...), or raise max_work')
        cnt, tot, longest = _co.fold_to_individuals(got['cnt'], got['len'], got['longest'])
        by = _tr.sharing_stats(self._field(nat.F_X)[slots], self._field(nat.F_Y)[slots], cnt,
                               tot, edges)
        by['mean_len'] = _tr.from_units(by['mean_len'], unit)
        by['edges'] = edges
        hist = None if te is None else _tract_hist(tract_edges, got['hist'], unit)
        own = np.diagonal(tot).astype(np.float64)
        f = own / float(genome_len) if genome_len > 0 else np.full(own.shape, np.nan)
        return dict(ids=ids, n_tracts=cnt, shared_len=_tr.from_units(tot, unit),
                    longest=_tr.from_units(longest, unit), by_dist=by, hist=hist,
                    cover=got['cover'], work=got['work'], unit=unit, f_ibd=f,
                    genome_len=float(_tr.from_units(genome_len, unit)))
