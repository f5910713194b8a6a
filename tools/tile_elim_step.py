#!/usr/bin/env python3
"""Tile / chunk mode on matrix-free data rows (lsq_set_cg_tile_dmf, k_cg_dmf_atq_long in
csrc/lsqr_cg.inc) at 28 epochs, in one process.

On a synthetic lattice with 28 epochs (synthetic.points('c4t28') by default, all rows kept) with 144
`rgt × cycle` biases (12 bins along x times 12 bins along time, E_bias 0.5), block-Jacobi throughout:

1. The plain chunk-mode step, no biases: two handles side by side, both with lsq_set_cg_chunks,
     leg `stored`:      the stored Ad / ATd data rows, the step AD -> NORMAL (the parent's path)
     leg `matrix_free`: lsq_set_cg_tile_dmf, the step NORMAL -> AD -> ATQ
   After a warm-up solve on each (32 iterations) the legs alternate `--rounds` times, each visit a
   warm-up batch and `--steps` timed iterations (lsq_iterate, device events inside the library:
   stats['time_s']).  Recorded: ms per iteration of every visit, their median and spread, the byte
   model, and the device bytes held (the drops of free device memory over each leg's creation,
   warm-up and visits).
2. The converged bias solve (atol = btol = 1e-12, cold start):
     `eliminate`: the matrix_free leg with lsq_set_data_bias — what lsq_bias='eliminate' runs with
                  lsq_tile_eliminate and lsq_cg_chunks
     `columns`:   what lsq_bias='auto' does on this problem without the key: the biases as ordinary
                  columns of a triplet-formed system, method 1 falling back to LSQR (--no-columns
                  skips this leg: at c4t28 its host triplets take tens of GB)
   Seconds, iterations, and the distance between the two solutions (grids and biases).  For the
   eliminate leg also profile_cg inside real iterations with and without the biases: the
   elimination's share of the step is the growth of the data rows' stages (AD, E0 … E3, ATQ) over
   the step's total, and the data rows' time stands against their byte model (cg_kernel_bytes) as
   a share of 8 TB/s.

Usage: python tools/tile_elim_step.py OUT.json [--config c4t28] [--steps 200] [--rounds 3] [--no-columns]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)
PEAK = 8e12   # HBM bytes per second
BINS = (12, 12)   # rgt (x) × cycle (time)
E_BIAS = 0.5


def bias_ids(D):
    def bins(v, n):
        v = np.asarray(v, float)
        return np.minimum((n * (v - v.min()) / (v.max() - v.min())).astype(np.int64), n - 1)
    return (bins(D.x, BINS[0]) * BINS[1] + bins(D.time, BINS[1])).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--config', default='c4t28')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--no-columns', action='store_true')
    a = ap.parse_args()

    import torch
    import lssurf_amd as LS
    from lssurf_amd import synthetic
    from lssurf_amd.constraint_functions import node_column_blocks, reference_epoch_keep_cols
    from lssurf_amd.smooth_fit import FitSystem
    from lssurf_amd.solver import LSQSolver

    def free_bytes():
        torch.cuda.synchronize()
        return int(torch.cuda.mem_get_info()[0])

    print(f'forming {a.config} on the host', flush=True)
    D, kw = synthetic.points(a.config)
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    gd = S['grids']['dz']
    keep = reference_epoch_keep_cols(S['G_data'].col_N, gd, kw['reference_epoch'])
    n_full, n_data = int(S['Gc'].col_N), int(S['data'].size)
    w = np.abs(1. / np.concatenate((S['Ed'], S['Ec'])))
    rhs = np.zeros(w.size)
    rhs[:n_data] = S['data'].z
    ids = bias_ids(S['data'])
    nb = BINS[0] * BINS[1]
    c = np.full(nb, 1. / E_BIAS)
    print('formed', flush=True)
    res = {'config': a.config, 'dz_shape': [int(v) for v in gd.shape], 'n_points': n_data, 'n_rows': int(w.size),
           'n_cols': int(keep.size), 'n_bias': nb, 'bias_ids_used': int(np.unique(ids).size), 'E_bias': E_BIAS,
           'steps': a.steps, 'rounds': a.rounds, 'tolerances': TOL,
           'timing': 'device events around the iterations (stats time_s), legs alternating in one process after a '
           'warm-up solve each', 'plain_step': {}, 'bias_solve': {}}
    legs, held = {}, {}
    col = None
    try:
        def tracked(name, fn):
            """fn() with the drop of free device memory over it booked to leg `name`"""
            f0 = free_bytes()
            out = fn()
            held[name] = held.get(name, 0) + f0 - free_bytes()
            return out

        def open_leg(dmf):
            fs = FitSystem(S['G_data'], S['Gc'], keep, n_full, grids=S['grids'], cg_chunks=True, tile_dmf=dmf)
            fs.solver.set_row_weight(w)
            fs.solver.set_row_mask(np.ones(w.size, bool))
            return fs, fs.solver.solve(rhs, precond=3, method=1, maxit=32, b_rows=n_data, **TOL)[1]   # warm-up

        # ---- 1. the plain step ----
        for name, dmf in (('stored', False), ('matrix_free', True)):
            legs[name], st = tracked(name, lambda: open_leg(dmf))
            assert st['method'] == 1, (name, st)
            p = legs[name].solver.profile_cg(reps=1, precond=3)
            res['plain_step'][name] = {'normal_mode': p['normal_mode'], 'data_rows': p['data_rows'], 'step_ms_all': []}
            assert p['data_rows'] == ('matrix-free' if dmf else 'stored'), p
        res['layout'] = legs['matrix_free'].solver.cg_layout_info()
        for rnd in range(a.rounds):
            for name, fs in legs.items():
                def visit(fs=fs):
                    fs.solver.iterate(rhs, 32, precond=3, method=1, b_rows=n_data)
                    return fs.solver.iterate(rhs, a.steps, precond=3, method=1, b_rows=n_data)
                st = tracked(name, visit)
                e = res['plain_step'][name]
                e['step_ms_all'].append(1e3 * st['time_s'] / a.steps)
                e['bytes_per_iter'] = float(st['bytes_per_iter'])
                print(name, rnd, e['step_ms_all'][-1], flush=True)
        for name, e in res['plain_step'].items():
            e['step_ms'] = float(np.median(e['step_ms_all']))
            e['step_ms_min'], e['step_ms_max'] = float(min(e['step_ms_all'])), float(max(e['step_ms_all']))
            e['device_bytes_held'] = int(held[name])
            e['info'] = legs[name].solver.info()
        res['plain_step']['ratio_matrix_free_over_stored'] = \
            res['plain_step']['matrix_free']['step_ms'] / res['plain_step']['stored']['step_ms']

        # ---- 2. the bias solve: eliminate ----
        fs = legs['matrix_free']
        sol = fs.solver
        sol.iterate(rhs, 32, precond=3, method=1, b_rows=n_data)
        prof0 = sol.profile_cg(reps=max(a.steps, 20), precond=3)
        sol.set_data_bias(ids, c)
        ok, why = sol.cg_available(3)
        assert ok, why
        be = res['bias_solve']['eliminate'] = {'step_ms_all': [], 'solves': []}
        for rnd in range(a.rounds):
            sol.set_data_bias(ids, c)                      # drops the live state: re-initialised below
            sol.iterate(rhs, 32, precond=3, method=1, b_rows=n_data)
            st = sol.iterate(rhs, a.steps, precond=3, method=1, b_rows=n_data)
            be['step_ms_all'].append(1e3 * st['time_s'] / a.steps)
            be['bytes_per_iter'] = float(st['bytes_per_iter'])
            x_el, st = sol.solve(rhs, precond=3, method=1, maxit=200000, b_rows=n_data, **TOL)
            b_el = sol.data_bias()
            be['solves'].append({'iters': int(st['iters']), 'istop': int(st['istop']), 'time_s': float(st['time_s']),
                                 'setup_s': float(st.get('setup_s', 0.)), 'method': int(st['method'])})
            print('eliminate', rnd, be['step_ms_all'][-1], be['solves'][-1], flush=True)
        be['step_ms'] = float(np.median(be['step_ms_all']))
        be['solve_s'] = float(np.median([s['time_s'] for s in be['solves']]))
        sol.iterate(rhs, 32, precond=3, method=1, b_rows=n_data)
        prof1 = sol.profile_cg(reps=max(a.steps, 20), precond=3)
        tot = sum(prof1[k] for k in ('cg_data', 'cg_normal', 'cg_update', 'cg_scalars'))
        res['profile_cg_plain'], res['profile_cg_bias'] = prof0, prof1
        res['elimination'] = {'extra_data_ms': prof1['cg_data'] - prof0['cg_data'], 'step_ms_profiled': tot,
                              'share_of_step': (prof1['cg_data'] - prof0['cg_data']) / tot}
        for tag, p in (('plain', prof0), ('bias', prof1)):
            nbytes = p['bytes']['cg_data']
            res['data_rows_' + tag] = {'ms': p['cg_data'], 'model_bytes': nbytes,
                                       'bytes_per_s': nbytes / max(1e-3 * p['cg_data'], 1e-12),
                                       'share_of_peak': nbytes / max(1e-3 * p['cg_data'], 1e-12) / PEAK}

        # ---- 2. the bias solve: columns through LSQR, as lsq_bias='auto' runs it without the key ----
        if not a.no_columns:
            print('forming the columns system from triplets', flush=True)

            def open_columns():
                r1, c1, v1 = S['G_data'].triplets()
                r2, c2, v2 = S['Gc'].triplets()
                m0 = int(w.size)
                rr = np.concatenate([np.ravel(r1), np.ravel(r2) + n_data, np.arange(n_data), m0 + np.arange(nb)])
                cc = np.concatenate([np.ravel(c1), np.ravel(c2), n_full + ids.astype(np.int64), n_full + np.arange(nb)])
                vv = np.concatenate([np.ravel(v1), np.ravel(v2), np.ones(n_data), np.ones(nb)])
                s = LSQSolver(0)
                s.set_col_map(n_full + nb, np.concatenate([keep, n_full + np.arange(nb)]))
                s.set_matrix_coo(m0 + nb, n_full + nb, rr, cc, vv)
                s.set_column_blocks_csr(*node_column_blocks(S['grids'], keep))
                s.set_row_weight(np.concatenate([w, c]))
                s.set_row_mask(np.ones(m0 + nb, bool))
                return s
            col = tracked('columns', open_columns)
            rhs_c = np.concatenate([rhs, np.zeros(nb)])
            bc = res['bias_solve']['columns'] = {'solves': []}

            def solve_columns():
                return col.solve(rhs_c, precond=3, method=1, maxit=400000, **TOL)
            for rnd in range(max(1, a.rounds - 1)):
                x_c, st = tracked('columns', solve_columns)
                bc['solves'].append({'iters': int(st['iters']), 'istop': int(st['istop']), 'time_s': float(st['time_s']),
                                     'method': int(st['method'])})
                print('columns', rnd, bc['solves'][-1], flush=True)
            bc['solve_s'] = float(np.median([s['time_s'] for s in bc['solves']]))
            bc['device_bytes_held'] = int(held['columns'])
            ng = keep.size
            res['bias_solve']['grid_rel_diff'] = float(np.linalg.norm(x_el - x_c[:ng]) / np.linalg.norm(x_c[:ng]))
            res['bias_solve']['bias_rel_diff'] = float(np.linalg.norm(b_el - x_c[ng:]) / np.linalg.norm(x_c[ng:]))
            res['bias_solve']['time_ratio_columns_over_eliminate'] = bc['solve_s'] / be['solve_s']
        res['bias_solve']['bias_norm'] = float(np.linalg.norm(b_el))
    finally:
        for fs in legs.values():
            fs.close()
        if col is not None:
            col.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
