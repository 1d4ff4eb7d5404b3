"""Spatial pedigree as tree-sequence tables (reference: the tskit.TableCollection
kept by structs/species.py:442,692-736,956-1094 when `use_tskit` is True).

The device reports each step's births (gnx_last_births: child and parent ids, the
recombination path and start homologue of both gametes, the birth position); this
module turns them into the rows the reference adds to its tables:

  individuals : one row per individual, location (x, y) at birth, metadata = its id
  nodes       : two per individual (homologue 0, 1), flags 1, time = 1 for the founders
                (the individuals alive at genome assignment) and -t for offspring born
                in main timestep t (the reference's convention: :717-726)
  edges       : per offspring homologue h, one edge per segment of the path of the
                gamete from parent h: [0, bp1 - 0.5), [bp1 - 0.5, bp2 - 0.5), ...,
                [.., L), parent node alternating between the parent's two homologues
                starting at the gamete's start homologue (structs/genome.py:234-281)
  sites, mutations : the founders' genotypes (site per locus with a derived allele in
                at least one founder; one mutation per founder node carrying it)

tskit itself is not needed to build or to write the tables (`write_text` emits
tskit's own text format, `tskit.load_text` reads it; `write_csv` the per-table CSVs of
Model.write_tskit_table_collection, sim/model.py:3449-3486).  Not kept: the coalescent
history msprime simulates for the founders (:956-1094) - founders are roots here.

Periodic simplification (reference structs/species.py:1107-1142, every tskit_simp_interval
main steps) is `simplify`: the rows no lineage of the living passes through are dropped and the
rest renumbered in their old order.  tskit's simplify also removes unary nodes and trims edges
to their ancestral intervals; one parent row and one path per node cannot express that, so
both stay.

Beside the float edge rows the tables keep the integers they are made from (`node_table`:
parent row, path key and start homologue per node, birth time per row).  A lineage at a locus
is a chain of look-ups in them (reference structs/genome.py:1638-1782, there through tskit's
trees): `trace` / `lineages` walk it in numpy, csrc/gnx_lineage.hip on the device, and
`lineage_stat_values` holds the reference's four gene-flow statistics (:1803-1871).  Because
unary nodes are never removed, a lineage lists EVERY ancestor, not only those tskit's
simplification would keep for the current sample.
"""
import numpy as np


LINEAGE_STATS = ('dir', 'dist', 'time', 'speed')


def lineage_stat_values(stats, t_young, xy_young, t_old, xy_old, n_kept):
    """the reference's lineage statistics (structs/genome.py:1803-1871) from the youngest and
    the oldest kept node of each lineage: times [...], locations [..., 2], fp64.  'dir': compass
    degrees of the displacement FROM the oldest TO the youngest node; 'dist' and 'time':
    oldest minus youngest; 'speed' = dist / time.  NaN where n_kept < 2 (the reference's None)"""
    t_young, t_old = np.asarray(t_young, np.float64), np.asarray(t_old, np.float64)
    xy_young, xy_old = np.asarray(xy_young, np.float64), np.asarray(xy_old, np.float64)
    ok = np.asarray(n_kept) >= 2
    out = {}
    with np.errstate(invalid='ignore', divide='ignore'):
        x_diff = xy_old[..., 0] - xy_young[..., 0]
        y_diff = xy_old[..., 1] - xy_young[..., 1]
        dist = np.sqrt(x_diff ** 2 + y_diff ** 2)
        time = t_old - t_young
        for st in stats:
            if st == 'dir':
                ang = np.rad2deg(np.arctan2(xy_young[..., 1] - xy_old[..., 1],
                                            xy_young[..., 0] - xy_old[..., 0]))
                ang = np.where(ang < 0, ang + 360, ang)
                v = (-ang + 90) % 360
            elif st == 'dist':
                v = dist
            elif st == 'time':
                v = time
            elif st == 'speed':
                v = dist / time
            else:
                raise ValueError('unknown lineage statistic %r' % (st,))
            out[st] = np.where(ok, v, np.nan)
    return out


def lineage_stats(tt, nodes, first, last, n_kept, t_curr, stats=LINEAGE_STATS, curr_xy=None):
    """lineage_stat_values of a trace ([n_loci][n_nodes] first / last / n_kept of the sample
    `nodes`) with the birth times and locations of the tables `tt`; curr_xy [n_nodes][2]: the
    sample individuals' current locations, used where the sample node itself is the youngest
    kept node (the reference's use_individs_curr_pos)"""
    _, bt = tt.node_table()
    xy = tt._ind_xy[0]
    nodes = np.asarray(nodes, dtype=np.int64).ravel()
    first, last, n_kept = np.atleast_2d(first), np.atleast_2d(last), np.atleast_2d(n_kept)
    if curr_xy is not None:
        curr_xy = np.asarray(curr_xy, np.float64)
        used = (first == nodes[None, :]).any(axis=0)
        if np.isnan(curr_xy[used]).any():
            raise ValueError('use_individs_curr_pos: a sample node belongs to an individual that '
                             'is not alive')
    out = {st: np.empty(first.shape, np.float64) for st in stats}
    block = max(1, (1 << 22) // max(nodes.size, 1))       # loci per pass: bounded temporaries
    for i in range(0, first.shape[0], block):
        sl = slice(i, i + block)
        f, l = np.maximum(first[sl], 0) >> 1, np.maximum(last[sl], 0) >> 1
        xy_young = xy[f]
        if curr_xy is not None:
            own = first[sl] == nodes[None, :]
            xy_young = np.where(own[..., None], curr_xy[None, :, :], xy_young)
        vals = lineage_stat_values(stats, bt[f].astype(np.float64) + t_curr, xy_young,
                                   bt[l].astype(np.float64) + t_curr, xy[l], n_kept[sl])
        for st in stats:
            out[st][sl] = vals[st]
    return out


class TreeTables:
    def __init__(self, L, bp_off, bp_loci):
        self.L = int(L)
        self._bp_off = np.asarray(bp_off, dtype=np.int64)
        self._bp_loci = np.asarray(bp_loci, dtype=np.int64)
        self._ind_id = [np.zeros(0, np.int64)]       # chunks; ids ascend over the table
        self._ind_xy = [np.zeros((0, 2), np.float64)]
        self._ind_time = [np.zeros(0, np.float64)]
        self._edges = [np.zeros((0, 4), np.float64)]  # left, right, parent node, child node
        # the integers the edges are made from (node_table): per node {parent row, key * 2 +
        # start homologue}, per row the birth time
        self._nt = [np.zeros((0, 2), np.int32)]
        self._bt = [np.zeros(0, np.int32)]
        self._founder_g = None                        # int8 [n_founders, L, 2]
        self.n_founders = 0
        self._new_muts = []                           # (locus, individual id, homologue)

    # -- building ---------------------------------------------------------------------
    def _flush(self):
        for name in ('_ind_id', '_ind_xy', '_ind_time', '_edges', '_nt', '_bt'):
            chunks = getattr(self, name)
            if len(chunks) > 1:
                setattr(self, name, [np.concatenate(chunks)])

    @property
    def ids(self):
        self._flush()
        return self._ind_id[0]

    def _edges_count(self):
        return int(sum(c.shape[0] for c in self._edges))

    def add_founders(self, ids, xy, genotypes=None):
        ids = np.asarray(ids, dtype=np.int64)
        assert self.ids.size == 0, 'founders are added once, first'
        assert (np.diff(ids) > 0).all(), 'founders must come in ascending id order'
        self._ind_id.append(ids)
        self._ind_xy.append(np.asarray(xy, dtype=np.float64))
        self._ind_time.append(np.full(ids.size, 1.0))
        self._nt.append(np.tile(np.array([[-1, 0]], np.int32), (2 * ids.size, 1)))
        self._bt.append(np.full(ids.size, 1, np.int32))
        self.n_founders = ids.size
        self._founder_g = None if genotypes is None else np.asarray(genotypes, dtype=np.int8)

    def add_births(self, t, child, parents, keys, starts, xy):
        """one main timestep's offspring (arrays as gnx_last_births returns them)"""
        child = np.asarray(child, dtype=np.int64)
        if child.size == 0:
            return
        order = np.argsort(child, kind='stable')
        child, parents, keys = child[order], np.asarray(parents)[order], np.asarray(keys)[order]
        starts, xy = np.asarray(starts)[order], np.asarray(xy)[order]
        known = self.ids
        assert known.size == 0 or child[0] > known[-1], 'offspring ids must ascend'
        first_row = known.size
        prow = np.searchsorted(known, parents)              # parents were recorded earlier
        assert (known[np.minimum(prow, known.size - 1)] == parents).all(), (
            'a parent is missing from the individuals table')
        self._ind_id.append(child)
        self._ind_xy.append(xy.astype(np.float64))
        self._ind_time.append(np.full(child.size, -float(t)))
        self._nt.append(np.stack([prow.reshape(-1), 2 * keys.reshape(-1).astype(np.int64)
                                  + starts.reshape(-1).astype(np.int64)], axis=1).astype(np.int32))
        self._bt.append(np.full(child.size, -int(t), np.int32))
        # one gamete per (offspring, homologue): segments from the path's switch points
        B = child.size
        key = keys.reshape(-1).astype(np.int64)             # [2B], (k, h) -> 2k + h
        nbp = self._bp_off[key + 1] - self._bp_off[key]
        nseg = nbp + 1
        g_of = np.repeat(np.arange(2 * B), nseg)             # gamete of each segment
        seg_start = np.concatenate([[0], np.cumsum(nseg)[:-1]])
        j = np.arange(nseg.sum()) - seg_start[g_of]           # segment number inside its gamete
        bp_idx = self._bp_off[key][g_of] + j                 # index of the segment's right switch
        right = np.where(j < nbp[g_of], self._bp_loci[np.minimum(bp_idx, self._bp_loci.size - 1)]
                         - 0.5, float(self.L)) if self._bp_loci.size else np.full(
                             g_of.size, float(self.L))
        left = np.where(j > 0, self._bp_loci[np.maximum(bp_idx - 1, 0)] - 0.5, 0.0) \
            if self._bp_loci.size else np.zeros(g_of.size)
        hom = (j + starts.reshape(-1).astype(np.int64)[g_of]) % 2
        parent_node = 2 * prow.reshape(-1)[g_of] + hom
        child_node = 2 * (first_row + g_of // 2) + (g_of % 2)
        self._edges.append(np.stack([left, right, parent_node.astype(np.float64),
                                     child_node.astype(np.float64)], axis=1))

    def add_mutations(self, ind_ids, loci, homs):
        """new mutations on this step's offspring (ops/mutation.py:62-131)"""
        for i, l, h in zip(ind_ids, loci, homs):
            self._new_muts.append((int(l), int(i), int(h)))

    # -- lineages ------------------------------------------------------------------------
    def node_table(self):
        """(int32 [2 n_rows][2], int32 [n_rows]): for node 2 row + h {row of the parent that
        gave the gamete (-1: a founder node), path key * 2 + start homologue}, and the rows'
        birth times as in the nodes table (founders +1, offspring of main step t: -t)"""
        self._flush()
        return self._nt[0], self._bt[0]

    def parents_of(self, ids):
        """int64 [n][2]: the ids of the two parents of each listed individual, column h the
        parent that gave homologue h; -1 for founders and for ids that are not in the table
        (never recorded, or dropped by simplify)"""
        ids = np.asarray(ids, dtype=np.int64).ravel()
        known = self.ids
        nt, _ = self.node_table()
        out = np.full((ids.size, 2), -1, np.int64)
        if known.size == 0 or ids.size == 0:
            return out
        row = np.minimum(np.searchsorted(known, ids), known.size - 1)
        there = known[row] == ids
        for hom in range(2):
            prow = nt[2 * row + hom, 0].astype(np.int64)
            has = there & (prow >= 0)
            out[has, hom] = known[prow[has]]
        return out

    def _switches_upto(self, key, locus):
        """number of switch points <= locus of path `key` (arrays of one shape)"""
        if self._bp_loci.size == 0:
            return np.zeros(np.shape(key), np.int64)
        g = self.__dict__.get('_bp_global')
        if g is None:                    # switch loci made globally ascending: key * (L + 1) + locus
            owner = np.repeat(np.arange(self._bp_off.size - 1), np.diff(self._bp_off))
            g = self._bp_global = owner * (self.L + 1) + self._bp_loci
        return np.searchsorted(g, key * (self.L + 1) + locus, side='right') - self._bp_off[key]

    @staticmethod
    def _window(min_time_ago, max_time_ago):
        lo = -np.inf if min_time_ago is None else min_time_ago
        hi = np.inf if max_time_ago is None else max_time_ago
        return lo, hi

    def _walk(self, nodes, loci, t_curr, drop_before_sim, min_time_ago, max_time_ago, visit):
        """the lineage of every (locus, node), all at once, one generation back per pass:
        visit(query indices, their current lineage nodes, kept mask) per pass.  -> roots"""
        nt, bt = self.node_table()
        nodes = np.asarray(nodes, dtype=np.int64).ravel()
        loci = np.asarray(loci, dtype=np.int64).ravel()
        if nodes.size and (nodes.min() < 0 or nodes.max() >= nt.shape[0]):
            raise ValueError('nodes: node ids in 0..%d' % (nt.shape[0] - 1))
        if loci.size and (loci.min() < 0 or loci.max() >= self.L):
            raise ValueError('loci: loci in 0..%d' % (self.L - 1))
        lo, hi = self._window(min_time_ago, max_time_ago)
        n = nodes.size
        cur = np.tile(nodes, loci.size)                     # query q = locus index * n + node index
        loc = np.repeat(loci, n)
        root = np.full(cur.size, -1, np.int64)
        act = np.arange(cur.size)
        while act.size:
            c = cur[act]
            t = bt[c >> 1].astype(np.int64)
            kept = (t < 0) if drop_before_sim else np.ones(c.size, bool)
            ago = t + int(t_curr)
            kept &= (lo <= ago) & (ago <= hi)
            visit(act, c, kept)
            prow = nt[c, 0].astype(np.int64)
            done = prow < 0
            root[act[done]] = c[done]
            go = ~done
            act, c, prow = act[go], c[go], prow[go]
            ks = nt[c, 1].astype(np.int64)
            hom = ((ks & 1) + self._switches_upto(ks >> 1, loc[act])) & 1
            cur[act] = 2 * prow + hom
        return root

    def trace(self, nodes, loci, t_curr, drop_before_sim=True, min_time_ago=None,
              max_time_ago=None):
        """Lineages of the sample `nodes` (2 row + h) at `loci` through the recorded pedigree:
        the parent homologue at locus l is (start + #{switch points of the path <= l}) mod 2.
        Kept nodes as the reference keeps them (structs/genome.py:1720-1759): with
        drop_before_sim only table times < 0 (a node born in step 0 has time 0 and is dropped,
        as there), then min_time_ago <= time + t_curr <= max_time_ago.
        -> dict of int32 [n_loci][n_nodes]: root (the founder node reached), first / last (the
        youngest / oldest kept node, -1 if none), n_kept"""
        nodes = np.asarray(nodes, dtype=np.int64).ravel()
        loci = np.asarray(loci, dtype=np.int64).ravel()
        nq = nodes.size * loci.size
        first = np.full(nq, -1, np.int64)
        last = np.full(nq, -1, np.int64)
        n_kept = np.zeros(nq, np.int64)

        def visit(q, c, kept):
            q, c = q[kept], c[kept]
            new = n_kept[q] == 0
            first[q[new]] = c[new]
            last[q] = c
            n_kept[q] += 1

        root = self._walk(nodes, loci, t_curr, drop_before_sim, min_time_ago, max_time_ago,
                          visit)
        shape = (loci.size, nodes.size)
        return dict(root=root.astype(np.int32).reshape(shape),
                    first=first.astype(np.int32).reshape(shape),
                    last=last.astype(np.int32).reshape(shape),
                    n_kept=n_kept.astype(np.int32).reshape(shape))

    def lineages(self, nodes, loci, t_curr, drop_before_sim=True, min_time_ago=None,
                 max_time_ago=None):
        """the kept nodes of every lineage, youngest first, in CSR form: (offsets int64
        [n_loci * n_nodes + 1], nodes int32); query (locus index i, node index j) is
        i * n_nodes + j"""
        nodes = np.asarray(nodes, dtype=np.int64).ravel()
        loci = np.asarray(loci, dtype=np.int64).ravel()
        qs, cs = [], []

        def visit(q, c, kept):
            qs.append(q[kept])
            cs.append(c[kept])

        self._walk(nodes, loci, t_curr, drop_before_sim, min_time_ago, max_time_ago, visit)
        q = np.concatenate(qs) if qs else np.zeros(0, np.int64)
        c = np.concatenate(cs) if cs else np.zeros(0, np.int64)
        order = np.argsort(q, kind='stable')               # passes go back in time: youngest first
        offsets = np.zeros(nodes.size * loci.size + 1, np.int64)
        np.cumsum(np.bincount(q, minlength=nodes.size * loci.size), out=offsets[1:])
        return offsets, c[order].astype(np.int32)

    # -- simplification ------------------------------------------------------------------
    def _sample_rows(self, sample_rows):
        rows = np.unique(np.asarray(sample_rows, dtype=np.int64).ravel())
        n = self.ids.size
        if rows.size == 0 or rows[0] < 0 or rows[-1] >= n:
            raise ValueError('sample_rows: a non-empty list of rows in 0..%d' % (n - 1))
        return rows

    def _path_bits(self, keys):
        """bool [n][L]: bit l of the paths `keys` (the parity of their switch points <= l)"""
        keys = np.asarray(keys, dtype=np.int64)
        flips = np.zeros((keys.size, self.L + 1), np.int8)
        n = self._bp_off[keys + 1] - self._bp_off[keys]
        who = np.repeat(np.arange(keys.size), n)
        idx = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n) + np.repeat(self._bp_off[keys], n)
        if idx.size:
            np.add.at(flips, (who, self._bp_loci[idx]), 1)
        return (np.cumsum(flips[:, :self.L], axis=1) & 1).astype(bool)

    def ancestral_masks(self, sample_rows):
        """bool [2 n_rows][L]: node v is ANCESTRAL at locus l if the lineage at l of some sample
        node passes through v; the sample is both nodes of every row in `sample_rows` (a sample
        node is ancestral at every locus).  The masks follow from the children alone,

            mask[2 prow + 1] |= mask[c] &  (path bits of c ^ start of c)
            mask[2 prow + 0] |= mask[c] & ~(path bits of c ^ start of c)

        for every node c with parent row prow, and a parent is born in an earlier main step than
        its child: one pass over the birth cohorts, youngest first, is exact.  The numpy form of
        csrc/gnx_simplify.hip."""
        nt, bt = self.node_table()
        rows = self._sample_rows(sample_rows)
        mask = np.zeros((nt.shape[0], self.L), bool)
        mask[2 * rows] = True
        mask[2 * rows + 1] = True
        prow_all = nt[:, 0].astype(np.int64)
        has = prow_all >= 0
        assert (bt[prow_all[has]] > bt[np.nonzero(has)[0] >> 1]).all(), (
            'a parent must be born in an earlier step than its child')
        for t in np.unique(bt):                              # ascending: the youngest cohort first
            r = np.nonzero(bt == t)[0]
            c = np.stack([2 * r, 2 * r + 1], 1).ravel()
            c = c[has[c] & mask[c].any(axis=1)]
            if c.size == 0:
                continue
            ks = nt[c, 1].astype(np.int64)
            keys, inv = np.unique(ks >> 1, return_inverse=True)
            x = self._path_bits(keys)[inv] ^ (ks & 1).astype(bool)[:, None]
            m = mask[c]
            np.logical_or.at(mask, 2 * prow_all[c] + 1, m & x)
            np.logical_or.at(mask, 2 * prow_all[c], m & ~x)
        return mask

    def simplify(self, sample_rows, node_loci=None):
        """Drop the rows without an ancestral node (ancestral_masks) for the sample - both nodes
        of every row in `sample_rows`, in the model the living - and renumber the rest in their
        old order.  node_loci int [2 n_rows]: per node the number of loci at which it is
        ancestral, from the device (gnx_pedigree_reach); None: counted here.
        -> int64 [old n_rows]: the new row, or -1.

        Every lineage of every sample node, at every locus, runs through kept rows only, so
        trace / lineages of the sample are what they were up to the renumbering, and
        genotypes_of is exact for the sample.  A node of a kept row that is itself not ancestral
        may lose its parent row: it becomes a root, its edge rows go, and genotypes_of of a kept
        ANCESTOR is exact only on its ancestral loci.  The sites table can lose sites that only
        dropped founders carried; new mutations of dropped individuals go with them.  Unlike
        tskit's simplify, unary nodes stay and edges are not trimmed to ancestral intervals."""
        nt, bt = self.node_table()
        n = bt.size
        rows = self._sample_rows(sample_rows)
        if node_loci is None:
            node_loci = self.ancestral_masks(rows).sum(axis=1)
        anc = np.asarray(node_loci).ravel() > 0
        if anc.size != 2 * n:
            raise ValueError('node_loci: one entry per node (%d), not %d' % (2 * n, anc.size))
        assert anc[2 * rows].all() and anc[2 * rows + 1].all(), 'a sample node is ancestral'
        keep = anc[0::2] | anc[1::2]
        new_row = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
        if keep.all():
            return new_row
        # the node table: parent rows renumbered; a node whose parent row went is a root
        knode = np.repeat(keep, 2)
        nt2 = nt[knode].copy()
        has = nt2[:, 0] >= 0
        newp = np.where(has, new_row[np.maximum(nt2[:, 0], 0)], -1)
        lost = has & (newp < 0)
        assert not (lost & anc[knode]).any(), 'an ancestral node keeps its parent row'
        nt2[:, 0] = newp
        nt2[lost, 1] = 0
        # the edge rows of the kept children whose parent row stays
        e = self._edges[0]
        par, chi = e[:, 2].astype(np.int64), e[:, 3].astype(np.int64)
        ek = (new_row[chi >> 1] >= 0) & (new_row[par >> 1] >= 0)
        e2 = e[ek].copy()
        e2[:, 2] = 2 * new_row[par[ek] >> 1] + (par[ek] & 1)
        e2[:, 3] = 2 * new_row[chi[ek] >> 1] + (chi[ek] & 1)
        old_ids = self._ind_id[0]
        if self._new_muts:
            r = np.searchsorted(old_ids, np.array([m[1] for m in self._new_muts], np.int64))
            self._new_muts = [m for m, k in zip(self._new_muts, keep[r]) if k]
        kf = keep[:self.n_founders]
        if self._founder_g is not None:
            self._founder_g = self._founder_g[kf]
        self.n_founders = int(kf.sum())                   # (kept founders stay the first rows)
        self._nt, self._edges = [nt2], [e2]
        self._bt = [bt[keep]]
        self._ind_id = [old_ids[keep]]
        self._ind_xy = [self._ind_xy[0][keep]]
        self._ind_time = [self._ind_time[0][keep]]
        return new_row

    # -- tables ------------------------------------------------------------------------
    def tables(self):
        self._flush()
        ids, xy, tm = self._ind_id[0], self._ind_xy[0], self._ind_time[0]
        n = ids.size
        nodes = dict(flags=np.ones(2 * n, np.int64), time=np.repeat(tm, 2),
                     population=np.zeros(2 * n, np.int64),
                     individual=np.repeat(np.arange(n), 2))
        e = self._edges[0]
        edges = dict(left=e[:, 0], right=e[:, 1], parent=e[:, 2].astype(np.int64),
                     child=e[:, 3].astype(np.int64))
        individuals = dict(flags=np.zeros(n, np.int64), x=xy[:, 0], y=xy[:, 1], gnx_id=ids)
        sites = dict(position=np.zeros(0), ancestral_state=np.zeros(0, 'U1'))
        muts = dict(site=np.zeros(0, np.int64), node=np.zeros(0, np.int64),
                    derived_state=np.zeros(0, 'U1'))
        m_loc = np.array([m[0] for m in self._new_muts], dtype=np.int64)
        m_node = (2 * np.searchsorted(ids, np.array([m[1] for m in self._new_muts],
                                                     dtype=np.int64))
                  + np.array([m[2] for m in self._new_muts], dtype=np.int64))
        f_loc = f_node = np.zeros(0, np.int64)
        if self._founder_g is not None and self.n_founders:
            f, f_loc, h = np.nonzero(self._founder_g)              # [F, L, 2]
            f_node = 2 * f + h
        loc = np.concatenate([f_loc, m_loc]).astype(np.int64)
        node = np.concatenate([f_node, m_node]).astype(np.int64)
        if loc.size:
            pos, site_idx = np.unique(loc, return_inverse=True)
            sites = dict(position=pos.astype(np.float64), ancestral_state=np.full(pos.size, '0'))
            o = np.lexsort((node, site_idx))
            muts = dict(site=site_idx[o].astype(np.int64), node=node[o],
                        derived_state=np.full(o.size, '1'))
        return dict(nodes=nodes, edges=edges, individuals=individuals, sites=sites,
                    mutations=muts)

    def write_csv(self, file_basename, sep=','):
        """<basename>_{NODES,EDGES,SITES,MUTATIONS,INDIVIDUALS}.csv
        (reference sim/model.py:3449-3486)"""
        for name, tab in self.tables().items():
            cols = [*tab]
            with open('%s_%s.csv' % (file_basename, name.upper()), 'w') as f:
                f.write(sep.join(cols) + '\n')
                for row in zip(*[tab[c] for c in cols]):
                    f.write(sep.join(repr(v.item()) if hasattr(v, 'item') and not isinstance(
                        v, np.str_) else str(v) for v in row) + '\n')

    def write_text(self, file_basename):
        """tskit's text format (tskit.load_text): <basename>.{nodes,edges,sites,mutations,
        individuals}.txt"""
        t = self.tables()
        n, e, i, s, m = t['nodes'], t['edges'], t['individuals'], t['sites'], t['mutations']
        with open(file_basename + '.nodes.txt', 'w') as f:
            f.write('is_sample\ttime\tpopulation\tindividual\n')
            for a, b, c, d in zip(n['flags'], n['time'], n['population'], n['individual']):
                f.write('%i\t%r\t%i\t%i\n' % (a, float(b), c, d))
        with open(file_basename + '.edges.txt', 'w') as f:
            f.write('left\tright\tparent\tchild\n')
            for a, b, c, d in zip(e['left'], e['right'], e['parent'], e['child']):
                f.write('%r\t%r\t%i\t%i\n' % (float(a), float(b), c, d))
        with open(file_basename + '.individuals.txt', 'w') as f:
            f.write('flags\tlocation\tparents\tmetadata\n')
            for a, x, y, g in zip(i['flags'], i['x'], i['y'], i['gnx_id']):
                f.write('%i\t%r,%r\t\t%i\n' % (a, float(x), float(y), g))
        with open(file_basename + '.sites.txt', 'w') as f:
            f.write('position\tancestral_state\n')
            for a, b in zip(s['position'], s['ancestral_state']):
                f.write('%r\t%s\n' % (float(a), b))
        with open(file_basename + '.mutations.txt', 'w') as f:
            f.write('site\tnode\tderived_state\n')
            for a, b, c in zip(m['site'], m['node'], m['derived_state']):
                f.write('%i\t%i\t%s\n' % (a, b, c))

    # -- check -----------------------------------------------------------------------------
    def genotypes_of(self, ids):
        """genotypes [n, L, 2] of the listed individuals, read back through the edges to
        the founders' genotypes - what the tree sequence encodes"""
        assert self._founder_g is not None, 'founder genotypes were not kept'
        t = self.tables()
        e = t['edges']
        n_nodes = t['nodes']['time'].size
        order = np.argsort(e['child'], kind='stable')
        child_sorted = e['child'][order]
        start = np.searchsorted(child_sorted, np.arange(n_nodes + 1))
        cache = {}
        L = self.L
        own = {}
        for l, i, h in self._new_muts:
            own.setdefault(2 * int(np.searchsorted(self.ids, i)) + h, []).append(l)

        def node_geno(node):
            if node in cache:
                return cache[node]
            if node < 2 * self.n_founders:
                g = self._founder_g[node // 2, :, node % 2]
            else:
                g = np.zeros(L, np.int8)
                for k in order[start[node]:start[node + 1]]:
                    lo = int(np.ceil(e['left'][k]))
                    hi = int(np.ceil(e['right'][k])) if e['right'][k] < L else L
                    g[lo:hi] = node_geno(int(e['parent'][k]))[lo:hi]
                for l in own.get(node, ()):
                    g[l] = 1
            cache[node] = g
            return g
        import sys
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 100000))
        rows = np.searchsorted(self.ids, np.asarray(ids, dtype=np.int64))
        return np.stack([np.stack([node_geno(2 * int(r)), node_geno(2 * int(r) + 1)], axis=1)
                         for r in rows])
