#!/usr/bin/env python3
"""CGNR's chunk mode (lsq_set_cg_chunks, k_cg_normal_chunk in csrc/lsqr_cg.inc) against the LSQR
fallback at 28 epochs, in one process.

On the synthetic C4 lattice with 28 epochs (synthetic.points('c4t28'), all rows kept) two handles
live side by side, one per leg, and method 1 with block-Jacobi (precond 3) runs on both:

  leg A, key off: no CGNR operator (a tile of whole time columns exceeds LDS); the library falls back
         to LSQR on the assembled operator — what every solve at 20 to 64 epochs ran before the key
  leg B, key on:  CGNR in chunk mode

After a warm-up solve on each (32 iterations: the workspaces, the full CSR of leg A, the captured
graphs), the legs alternate `--rounds` times; each visit is `--steps` timed iterations (lsq_iterate,
device events inside the library: stats['time_s']) and one converged solve at smooth_fit's default
tolerances (atol = btol = 1e-12), cold start.  Recorded for both: ms per iteration, iterations and
seconds of the converged solves, device bytes held (the drops of free device memory over the handle's
creation, warm-up and visits, each booked to its own leg) and the relative difference of the two solutions.  For leg B also
the layout (lsq_cg_layout_info), the profile_cg split inside real iterations, the normal kernel's
time against its byte model as a share of 8 TB/s, and the staged-to-owned ratio of the layout the
device reports (grid faces clip the halos) against the derived 2.76 of an unclipped (5, 9) tile.

Usage: python tools/chunk_step.py OUT.json [--config c4t28] [--steps 200] [--rounds 2]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)
PEAK = 8e12   # HBM bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--config', default='c4t28')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=2)
    a = ap.parse_args()

    import torch
    import lssurf_amd as LS
    from lssurf_amd import synthetic
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.smooth_fit import FitSystem

    def free_bytes():
        torch.cuda.synchronize()
        return int(torch.cuda.mem_get_info()[0])

    print(f'forming {a.config} on the host', flush=True)
    D, kw = synthetic.points(a.config)
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    gd = S['grids']['dz']
    keep = reference_epoch_keep_cols(S['G_data'].col_N, gd, kw['reference_epoch'])
    w = np.abs(1. / np.concatenate((S['Ed'], S['Ec'])))
    rhs = np.zeros(w.size)
    rhs[:S['data'].size] = S['data'].z
    print('formed', flush=True)
    res = {'config': a.config, 'dz_shape': [int(v) for v in gd.shape], 'n_points': int(S['data'].size),
           'n_rows': int(w.size), 'n_cols': int(keep.size), 'steps': a.steps, 'rounds': a.rounds,
           'tolerances': TOL, 'timing': 'device events around the iterations (stats time_s), legs alternating in one '
           'process after a warm-up solve each', 'legs': {}}
    legs, held = {}, {}
    try:
        def tracked(name, fn):
            """fn() with the drop of free device memory over it booked to leg `name`"""
            f0 = free_bytes()
            out = fn()
            held[name] = held.get(name, 0) + f0 - free_bytes()
            return out

        def open_leg(chunks):
            fs = FitSystem(S['G_data'], S['Gc'], keep, S['Gc'].col_N, grids=S['grids'], cg_chunks=chunks)
            fs.solver.set_row_weight(w)
            fs.solver.set_row_mask(np.ones(w.size, bool))
            return fs, fs.solver.solve(rhs, precond=3, method=1, maxit=32, b_rows=fs.n_data, **TOL)[1]   # warm-up

        ran = {}
        for name, chunks in (('A_key_off', False), ('B_key_on', True)):
            legs[name], st = tracked(name, lambda: open_leg(chunks))
            ran[name] = st['method']
            res['legs'][name] = {'method_ran': 'cgnr' if st['method'] == 1 else 'lsqr', 'step_ms_all': [], 'solves': []}
        assert ran == {'A_key_off': 0, 'B_key_on': 1}, ran
        res['layout'] = legs['B_key_on'].solver.cg_layout_info()
        assert res['layout']['mode'] == 'chunk', res['layout']
        xs = {}
        for rnd in range(a.rounds):
            for name, fs in legs.items():
                e = res['legs'][name]
                def visit(fs=fs):
                    fs.solver.iterate(rhs, 32, precond=3, method=1, b_rows=fs.n_data)
                    st = fs.solver.iterate(rhs, a.steps, precond=3, method=1, b_rows=fs.n_data)
                    return st, fs.solver.solve(rhs, precond=3, method=1, maxit=200000, b_rows=fs.n_data, **TOL)

                sti, (xs[name], st) = tracked(name, visit)
                e['step_ms_all'].append(1e3 * sti['time_s'] / a.steps)
                e['bytes_per_iter'] = float(sti['bytes_per_iter'])
                e['solves'].append({'iters': int(st['iters']), 'istop': int(st['istop']), 'time_s': float(st['time_s']),
                                    'setup_s': float(st.get('setup_s', 0.)), 'method': int(st['method'])})
                print(name, rnd, e['step_ms_all'][-1], e['solves'][-1], flush=True)
        for name, e in res['legs'].items():
            e['step_ms'] = float(np.median(e['step_ms_all']))
            e['it_per_s'] = 1e3 / e['step_ms']
            e['solve_s'] = float(np.median([s['time_s'] for s in e['solves']]))
            e['info'] = legs[name].solver.info()
            e['device_bytes_held'] = int(held[name])
        A, B = res['legs']['A_key_off'], res['legs']['B_key_on']
        ratios = [sa['time_s'] / sb['time_s'] for sa, sb in zip(A['solves'], B['solves'])]
        res['solve_time_ratio_A_over_B'] = {'per_round': ratios, 'min': float(min(ratios)), 'max': float(max(ratios))}
        res['step_time_ratio_A_over_B'] = A['step_ms'] / B['step_ms']
        xa, xb = xs['A_key_off'], xs['B_key_on']
        res['solution_rel_diff'] = float(np.linalg.norm(xb - xa) / np.linalg.norm(xa))
        # leg B's kernels inside real iterations of a live state
        fs = legs['B_key_on']
        fs.solver.iterate(rhs, 32, precond=3, method=1, b_rows=fs.n_data)
        prof = fs.solver.profile_cg(reps=max(a.steps, 20), precond=3)
        res['profile_cg'] = prof
        nb = prof['bytes']['cg_normal']
        res['normal_kernel'] = {'ms': prof['cg_normal'], 'model_bytes': nb,
                                'bytes_per_s': nb / max(1e-3 * prof['cg_normal'], 1e-12),
                                'share_of_peak': nb / max(1e-3 * prof['cg_normal'], 1e-12) / PEAK}
        # the staged-to-owned ratio of the dz grid's layout as the device reports it, the halos clipped
        # at the grid's faces (cg_chunk_staged's count, restated), against the derived figures of tiles
        # away from the faces: 2.76 for (ty, tc) = (5, 9), and this layout's own
        lay, (S0, S1, S2), h = res['layout'], gd.shape, 2
        ty, nch = lay['ty'], lay['chunks']
        cut = [k * S2 // nch for k in range(nch + 1)]
        ry = sum(min(S0, (i + 1) * ty + h) - max(0, i * ty - h) for i in range(-(-S0 // ty)))
        rx = sum(min(S1, (i + 1) * 64 + h) - max(0, i * 64 - h) for i in range(-(-S1 // 64)))
        rt = sum(min(S2, b + h) - max(0, a_ - h) for a_, b in zip(cut, cut[1:]))
        res['halo'] = {'derived_5x9_unclipped': 2.76,
                       'layout_unclipped': (ty + 2 * h) * (S2 + 2 * h * nch) * (64 + 2 * h) / (ty * S2 * 64.),
                       'layout_clipped': ry * rx * rt / float(S0 * S1 * S2)}
    finally:
        for fs in legs.values():
            fs.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
