#!/usr/bin/env python3
"""Cost of the data-bias elimination step (csrc/bias.inc) at C4 size, in one process.

On the synthetic C4 system (synthetic.points('c4'), all rows kept) bias IDs are assigned from the
points' (time, y) bins for 64, 2 048 and 65 536 IDs (c = 1 / 0.5 for every ID), and for each count:

1. lsq_iterate, CGNR + block-Jacobi, without biases and with them: rounds that alternate the two
   on the same handle, each round a warm-up batch and then `--steps` timed iterations (device
   events inside the library, stats['time_s']).  The extra time per step is the difference of the
   two medians of the same run; the budget is the step's byte model (the difference of the
   library's bytes_per_iter) over 0.43 × 8 TB/s, the fraction of peak the existing data-row
   kernels reach.
2. a converged solve (atol = btol = 1e-12) with the multigrid and with the block-Jacobi
   preconditioner, with and without biases: the iteration counts and their ratio.

Usage: python tools/bias_step.py OUT.json [--config c4] [--steps 200] [--rounds 5] [--no-solves]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ID_SHAPES = {64: (8, 8), 2048: (16, 128), 65536: (64, 1024)}   # (time bins, y bins)
TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)


def bias_ids(D, nb):
    nt, ny = ID_SHAPES[nb]
    def bins(v, n):
        v = np.asarray(v, float)
        return np.minimum((n * (v - v.min()) / (v.max() - v.min())).astype(np.int64), n - 1)
    return (bins(D.time, nt) * ny + bins(D.y, ny)).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--config', default='c4')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-solves', action='store_true')
    a = ap.parse_args()

    import lssurf_amd as LS
    from lssurf_amd import synthetic
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.smooth_fit import FitSystem

    D, kw = synthetic.points(a.config)
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    keep = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], kw['reference_epoch'])
    w = np.abs(1. / np.concatenate((S['Ed'], S['Ec'])))
    rhs = np.zeros(w.size)
    rhs[:S['data'].size] = S['data'].z
    fs = FitSystem(S['G_data'], S['Gc'], keep, S['Gc'].col_N, grids=S['grids'])
    sol = fs.solver
    sol.set_row_weight(w)
    sol.set_row_mask(np.ones(w.size, bool))
    res = {'config': a.config, 'n_points': int(fs.n_data), 'n_cols': int(keep.size), 'steps': a.steps,
           'rounds': a.rounds, 'c': 2.0, 'timing': 'device events around the iterations (stats time_s), medians of '
           'alternating rounds in one process', 'budget_rate_bytes_per_s': 0.43 * 8e12, 'ids': {}}

    def step(ids, c):
        sol.set_data_bias(ids, c)                      # drops the captured batch: re-initialised below
        sol.iterate(rhs, 32, precond=3, method=1, b_rows=fs.n_data)       # init + warm-up
        st = sol.iterate(rhs, a.steps, precond=3, method=1, b_rows=fs.n_data)
        return 1e3 * st['time_s'] / a.steps, st['bytes_per_iter']

    try:
        for nb in ID_SHAPES:
            ids, c = bias_ids(S['data'], nb), np.full(nb, 2.0)
            plain, with_b = [], []
            for _ in range(a.rounds):
                t0, b0 = step(None, None)
                t1, b1 = step(ids, c)
                plain.append(t0)
                with_b.append(t1)
            e = {'ids_used': int(np.unique(ids).size), 'step_ms_plain': float(np.median(plain)),
                 'step_ms_bias': float(np.median(with_b)), 'step_ms_plain_all': plain, 'step_ms_bias_all': with_b,
                 'model_bytes': float(b1 - b0)}
            e['extra_us'] = 1e3 * (e['step_ms_bias'] - e['step_ms_plain'])
            e['budget_us'] = 1e6 * e['model_bytes'] / res['budget_rate_bytes_per_s']
            res['ids'][str(nb)] = e
            print(nb, e, flush=True)
        if not a.no_solves:
            for precond, label in ((4, 'multigrid'), (3, 'block_jacobi')):
                if not sol.cg_available(precond)[0]:
                    continue
                iters = {}
                for nb in [0] + list(ID_SHAPES):
                    if nb:
                        sol.set_data_bias(bias_ids(S['data'], nb), np.full(nb, 2.0))
                    else:
                        sol.set_data_bias(None, None)
                    _, st = sol.solve(rhs, precond=precond, method=1, maxit=200000, b_rows=fs.n_data, **TOL)
                    iters[str(nb)] = {'iters': int(st['iters']), 'istop': int(st['istop']), 'time_s': float(st['time_s'])}
                    print(label, nb, iters[str(nb)], flush=True)
                for nb in ID_SHAPES:
                    iters[str(nb)]['ratio'] = iters[str(nb)]['iters'] / max(iters['0']['iters'], 1)
                res['solve_' + label] = iters
    finally:
        fs.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
