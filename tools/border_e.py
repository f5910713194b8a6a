#!/usr/bin/env python3
"""Cost of the border of lsq_cov_band_bordered (csrc/border.inc) at C1 size, in one process.

On the synthetic C1 system (synthetic.points('c1'): 128² nodes × 9 epochs, below WINDOW_MIN_COLS, all
rows kept) the points get a `cycle` field dealt out at random to k IDs (sigma_corr 0.5), for
k = 64, 512 and 2048: k bias columns behind the grids', the system formed as smooth_fit forms it
for compute_E.  For each k: one warm-up call of cov_band_bordered, then `--repeats` timed calls;
from every call's info the border phase (info[8], steps 2–8) as a fraction of the same call's band
phase (info[4] + info[5], factor + sweeps) and the f64 rate of the two substitutions' flop model
(info[9]) over the WHOLE border phase — a lower bound of the substitution kernels' own rate, since
the phase also holds the assembly, the Schur complement, its factor and the GEMM.  Medians and the
spread (min, max) over the repeats.  For comparison lsq_cov_band of the grid-only system, what the
library could do before the border: the same phases, the same way.

Times are host wall clock around work that ends in a stream synchronise (the library's info).

Usage: python tools/border_e.py OUT.json [--config c1] [--k 64 512 2048] [--repeats 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(v):
    v = [float(x) for x in v]
    return {'median': float(np.median(v)), 'min': min(v), 'max': max(v), 'all': v}


def _system(LS, D, kw, k, rng):
    """(FitSystem, weights, perm, n_border) with k bias IDs (k = 0: the grid-only system)"""
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.errors import band_order, bordered_band_order
    from lssurf_amd.smooth_fit import FitSystem
    extra = {}
    if k:
        D = D.copy()
        D.assign(cycle=(rng.permutation(D.size) % k).astype(float), sigma_corr=np.full(D.size, 0.5))
        extra = dict(bias_params=['cycle'], lsq_bias='columns')
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **dict(kw, **extra))
    keep = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], kw['reference_epoch'])
    fs = FitSystem(S['G_data'], S['Gc'], keep, S['Gc'].col_N)
    w = np.abs(1. / np.concatenate((S['Ed'], S['Ec'])))
    if k:
        perm, nb = bordered_band_order(S['grids'], keep, int(S['grids']['dz'].col_N))
        assert nb == k
    else:
        perm, nb = band_order(S['grids'], keep), 0
    return fs, w, perm, nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--config', default='c1')
    ap.add_argument('--k', type=int, nargs='+', default=[64, 512, 2048])
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()

    import lssurf_amd as LS
    from lssurf_amd import synthetic
    D, kw = synthetic.points(a.config)
    rng = np.random.default_rng(20261020)
    res = {'config': a.config, 'n_points': int(D.size), 'repeats': a.repeats, 'cases': {}}
    for k in [0] + list(a.k):
        fs, w, perm, nb = _system(LS, D, kw, k, rng)
        try:
            fs.solver.set_row_weight(w)
            call = (lambda: fs.solver.cov_band_bordered(perm, nb)) if k else (lambda: fs.solver.cov_band(perm))
            call()   # warm-up: code objects, the full CSR, allocations
            infos, Es = [], []
            for _ in range(a.repeats):
                E, _, info = call()
                infos.append([int(x) for x in info])
                Es.append(E)
        finally:
            fs.close()
        c = {'n_cols': int(perm.size), 'n_border': int(nb), 'info': infos,
             'bitwise_equal_repeats': bool(all(np.array_equal(Es[0], e) for e in Es[1:])),
             'band_phase_s': _stats([1e-6 * (i[4] + i[5]) for i in infos])}
        if k:
            c['border_phase_s'] = _stats([1e-6 * i[8] for i in infos])
            c['border_over_band'] = _stats([i[8] / (i[4] + i[5]) for i in infos])
            c['substitution_flops'] = infos[0][9]
            c['substitution_flops_over_border_phase_per_s'] = _stats([i[9] / (1e-6 * i[8]) for i in infos])
            c['border_bytes'] = infos[0][7]
        res['cases']['grid_only' if not k else f'k{k}'] = c
        print(k, {key: (v['median'] if isinstance(v, dict) else v) for key, v in c.items() if key != 'info'}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
