#!/usr/bin/env python3
"""Cost of the scaled parts' kernel (k_cg_scaled, csrc/lsqr_cg.inc) and of a masked fit's solve, in one process.

On the synthetic C4 system (synthetic.points('c4'), all rows kept) a disc mask over about 20 % of the dz
nodes (radius 0.252 × the lattice width, centred) is handed to smooth_fit as mask_data: with the default
mask_scale the five grad2_dzdt / grad_dzdt parts take two row scales.  Two handles live side by side: the
unmasked system, and the masked one with lsq_set_cg_scaled.

1. k_cg_scaled inside real iterations (lsq_profile_cg_scaled on the live state): its time per step against
   its byte model — 24 B per column of the grids with scaled parts + 8 B per part and node of field — as a
   fraction of 8 TB/s, with the normal kernel in front of it for scale.
2. The block-Jacobi step of the masked handle against the unmasked one: rounds that alternate the two
   handles, each a warm-up batch and then `--steps` timed iterations (stats['time_s']); medians of the run.
3. Converged solves (atol = btol = 1e-12) of the masked system: CGNR + block-Jacobi with the key, and method
   1 without the key on a third handle — this tree's fallback, LSQR + block-Jacobi, which is what the parent
   commit runs; `--fallback-only` runs that leg alone, for a build of the parent (tools/build_variant.sh),
   whose figures `--parent FILE` merges into the output.  Iterations, seconds and device bytes of each.

Usage: python tools/scaled_step.py OUT.json [--config c4] [--steps 200] [--rounds 5] [--no-solves]
                                   [--fallback-only] [--parent PARENT.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)


def disc_mask(ny, nx, frac=0.2):
    """zeros inside a centred disc that holds `frac` of the nodes"""
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    r2 = frac * ny * nx / np.pi
    return (yy - (ny - 1) / 2.) ** 2 + (xx - (nx - 1) / 2.) ** 2 > r2


def device_bytes():
    import torch
    free, total = torch.cuda.mem_get_info()
    return int(total - free)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--config', default='c4')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-solves', action='store_true')
    ap.add_argument('--fallback-only', action='store_true')
    ap.add_argument('--parent', default=None)
    a = ap.parse_args()

    import lssurf_amd as LS
    from lssurf_amd import synthetic
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.smooth_fit import FitSystem

    D, kw = synthetic.points(a.config)
    n, nt = synthetic.CONFIGS[a.config][:2]
    ny = synthetic.CONFIGS[a.config][3] if len(synthetic.CONFIGS[a.config]) > 3 else n
    mask = disc_mask(ny, n)

    def objects(**extra):
        S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **dict(kw, **extra))
        keep = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], kw['reference_epoch'])
        w = np.abs(1. / np.concatenate((S['Ed'], S['Ec'])))
        rhs = np.zeros(w.size)
        rhs[:S['data'].size] = S['data'].z
        return S, keep, w, rhs

    def handle(S, keep, w, **fkw):
        fs = FitSystem(S['G_data'], S['Gc'], keep, S['Gc'].col_N, grids=S['grids'], **fkw)
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(np.ones(w.size, bool))
        return fs

    res = {'config': a.config, 'steps': a.steps, 'rounds': a.rounds, 'masked_node_fraction': float(1 - mask.mean()),
           'timing': 'device events around the iterations (stats time_s), medians of alternating rounds in one process',
           'peak_bytes_per_s': 8e12}
    Sm, keep_m, wm, rhs_m = objects(mask_data=mask)
    res['n_points_masked'] = int(Sm['data'].size)
    res['n_cols'] = int(keep_m.size)
    open_handles = []
    try:
        if not a.fallback_only:
            Sp, keep_p, wp, rhs_p = objects()
            res['n_points_plain'] = int(Sp['data'].size)
            base = device_bytes()
            plain = handle(Sp, keep_p, wp)
            open_handles.append(plain)
            scaled = handle(Sm, keep_m, wm, cg_scaled=True)
            open_handles.append(scaled)
            ok, why = scaled.solver.cg_available(3)
            if not ok:
                raise RuntimeError(f'no CGNR operator with the key: {why}')
            res['scaled_info'] = scaled.solver.cg_scaled_info()
            cases = {'plain': (plain, rhs_p), 'scaled': (scaled, rhs_m)}

            def step(name):
                fs, b = cases[name]
                fs.solver.iterate(b, 32, precond=3, method=1, b_rows=fs.n_data)       # init + warm-up
                st = fs.solver.iterate(b, a.steps, precond=3, method=1, b_rows=fs.n_data)
                return 1e3 * st['time_s'] / a.steps, st['bytes_per_iter']

            t = {'plain': [], 'scaled': []}
            by = {}
            for _ in range(a.rounds):
                for name in t:
                    ms, by[name] = step(name)
                    t[name].append(ms)
            e = {'step_ms_plain': float(np.median(t['plain'])), 'step_ms_scaled': float(np.median(t['scaled'])),
                 'step_ms_plain_all': t['plain'], 'step_ms_scaled_all': t['scaled'],
                 'bytes_per_iter_plain': float(by['plain']), 'bytes_per_iter_scaled': float(by['scaled'])}
            e['extra_us'] = 1e3 * (e['step_ms_scaled'] - e['step_ms_plain'])
            scaled.solver.iterate(rhs_m, 32, precond=3, method=1, b_rows=scaled.n_data)
            k = scaled.solver.profile_cg_scaled(reps=max(a.steps, 20), precond=3)
            e['k_cg_scaled_us'] = 1e3 * k['k_cg_scaled']
            e['k_cg_scaled_model_bytes'] = k['bytes']
            e['k_cg_scaled_bytes_per_s'] = k['bytes'] / max(1e-3 * k['k_cg_scaled'], 1e-12)
            e['k_cg_scaled_fraction_of_peak'] = e['k_cg_scaled_bytes_per_s'] / res['peak_bytes_per_s']
            e['normal_before_us'] = 1e3 * k['normal_before']
            e['profiled_step_us'] = 1e3 * k['step']
            res['step'] = e
            print(e, flush=True)
            if not a.no_solves:
                x, st = scaled.solver.solve(rhs_m, precond=3, method=1, maxit=200000, b_rows=scaled.n_data, **TOL)
                res['solve_cgnr_scaled'] = {'method': int(st['method']), 'iters': int(st['iters']), 'istop': int(st['istop']),
                                            'time_s': float(st['time_s']), 'setup_s': float(st.get('setup_s', 0.))}
                print('cgnr', res['solve_cgnr_scaled'], flush=True)
            plain.close()
            open_handles.remove(plain)
            res['device_bytes_scaled_handle'] = device_bytes() - base
            scaled.close()
            open_handles.remove(scaled)
        if not a.no_solves:
            base = device_bytes()
            fb = handle(Sm, keep_m, wm)
            open_handles.append(fb)
            ok, why = fb.solver.cg_available(3)
            xf, st = fb.solver.solve(rhs_m, precond=3, method=1, maxit=200000, b_rows=fb.n_data, **TOL)
            res['solve_fallback'] = {'cg_available': bool(ok), 'reason': why, 'method': int(st['method']),
                                     'iters': int(st['iters']), 'istop': int(st['istop']), 'time_s': float(st['time_s']),
                                     'setup_s': float(st.get('setup_s', 0.)), 'device_bytes': device_bytes() - base}
            print('fallback', res['solve_fallback'], flush=True)
            if not a.fallback_only:
                res['solution_rel_diff'] = float(np.linalg.norm(x - xf) / np.linalg.norm(xf))
    finally:
        for fs in open_handles:
            fs.close()
    if a.parent:
        with open(a.parent) as f:
            res['parent'] = json.load(f).get('solve_fallback')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
