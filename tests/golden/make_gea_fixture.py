"""Fixture for Model.run_gea (geonomics_amd/sim/gea.py; reference structs/species.py:2269-2355,
Species._run_cca -> sklearn's CCA(n_components=3) on the table of _make_gea_df, :2218-2266).

Runs only where the reference and sklearn are importable (as make_golden.py, through
_ref_import.py); nothing under tests/ imports it at test time.  A reference model with
N = 400 individuals and L = 96 loci (N > L + 3: the analysis is not degenerate) gets its
genomes assigned, one locus made monomorphic and one pair of loci made identical - the two
ways a column of the genotype table can be exactly dependent - and the reference's own
_run_cca(trt_num=0, plot=False) is called on it.  Stored: the uint8 dosages [N][L], x, y,
e [N][n_layers] (rows in the reference's order of individuals, ids ascending), the Trait's
lyr_num, and the reference's ind_df, loci_df, var_df and trait_loci; only data.

    python tests/golden/make_gea_fixture.py   ->  tests/golden/g18_gea.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG          # noqa: E402  (imports the reference through _ref_import.py)
import scipy                       # noqa: E402
import sklearn                     # noqa: E402

MONOMORPHIC = 17                   # every individual 0|0 here
TWINS = (40, 41)                   # locus 41 is a copy of locus 40


def main():
    mod = MG.make_ref_model(N=400, L=96, seed=18)
    spp = MG.assign_genomes(mod)
    for ind in spp.values():
        ind.g[MONOMORPHIC, :] = 0
        ind.g[TWINS[1], :] = ind.g[TWINS[0], :]
    N, L = len(spp), spp.gen_arch.L
    assert N > L + 3, (N, L)
    res = spp._run_cca(trt_num=0, plot=False)
    trt = spp.gen_arch.traits[0]
    dos = MG.stack_g(spp).sum(axis=2).astype(np.uint8)                 # [N][L], ids ascending
    ids = np.array([*spp])
    assert (np.diff(ids) > 0).all()
    gea_df = res['gea_df']
    # the table the reference analysed is the one stored here
    assert np.array_equal(np.asarray(gea_df.iloc[:, :L]), dos / 2.0)
    x = np.array([ind.x for ind in spp.values()], np.float64)
    y = np.array([ind.y for ind in spp.values()], np.float64)
    e = np.array([ind.e for ind in spp.values()], np.float64)
    assert np.array_equal(np.asarray(gea_df['env']), e[:, trt.lyr_num])
    assert np.array_equal(np.asarray(gea_df['lat']), x)
    assert np.array_equal(np.asarray(gea_df['long']), y)
    meta = dict(MG.META, sklearn=sklearn.__version__, scipy=scipy.__version__,
                numpy=np.__version__, monomorphic=MONOMORPHIC, twins=TWINS,
                call='Species._run_cca(trt_num=0, plot=False)')
    path = os.path.join(HERE, 'g18_gea.npz')
    np.savez_compressed(path, meta=str(meta), dosages=dos, ids=ids, x=x, y=y, e=e,
                        lyr_num=np.int64(trt.lyr_num),
                        ind_df=np.asarray(res['ind_df'], np.float64),
                        loci_df=np.asarray(res['loci_df'], np.float64),
                        var_df=np.asarray(res['var_df'], np.float64),
                        trait_loci=np.asarray(res['trait_loci'], np.int64))
    print('wrote g18_gea.npz %.1f KB (N = %d, L = %d)' % (os.path.getsize(path) / 1e3, N, L))


if __name__ == '__main__':
    main()
