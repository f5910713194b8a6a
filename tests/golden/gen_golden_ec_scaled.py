#!/usr/bin/env python3
"""Generate tests/golden/ec_scaled.npz: the `expected` of every constraint operator that the REFERENCE's
constraint_functions.setup_smoothness_constraints builds on masked and mapped grids, with its inputs.  The
reference is imported with the stand-ins of _refstubs.py (a no-op where it is absent); the fixture holds data
only.

Systems: those of tests/scaled_host.py (SYSTEMS): the reference's own fd_grid objects on the same bounds and
spacings, `mask` set to the system's (ny, nx) array on the dz grid (what its setup_mask does with an
ndarray, without the erosion step that needs a pointCollection grid), mask_scale {0: 10, 1: 1}, and
scaling_masks = the system's maps as arrays on the nodes with non-finite entries 1 (smooth_fit.py:467-478
interpolates a map to exactly these nodes).

Per system `<name>`: <name>__shape, <name>__mask (absent: none), <name>__map__<key>, and
<name>__ec__<operator name> = the operator's expected.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import _refstubs
    if not os.path.isdir(_refstubs.REF):
        print('gen_golden_ec_scaled: reference absent; keeping the committed fixture')
        return
    _refstubs.install()
    from LSsurf.constraint_functions import setup_smoothness_constraints
    from LSsurf.fd_grid import fd_grid
    import scaled_host as SH

    out = {}
    for name, ((ny, nx, nt), npts, ref, kind, keys) in SH.SYSTEMS.items():
        _, kw = SH.points(name)
        W, ctr, sp = kw['W'], kw['ctr'], kw['spacing']
        bds = {c: ctr[c] + np.array([-0.5, 0.5]) * W[c] for c in ('x', 'y', 't')}
        z0 = fd_grid([bds['y'], bds['x']], sp['z0'] * np.ones(2), name='z0')
        dz = fd_grid([bds['y'], bds['x'], bds['t']], [sp['dz'], sp['dz'], sp['dt']], name='dz', col_0=z0.N_nodes)
        assert tuple(dz.shape) == (ny, nx, nt) and tuple(z0.shape) == (ny, nx)
        out[f'{name}__shape'] = np.array([ny, nx, nt])
        mask = SH.mask_of(kind, ny, nx)
        if mask is not None:
            dz.mask = mask.astype(bool)
            out[f'{name}__mask'] = mask
        maps = SH.maps_of(keys, name, ny, nx) or {}
        masks = {}
        for key, m in maps.items():
            m = np.array(m, dtype=float)
            m[~np.isfinite(m)] = 1.
            masks[key] = m
            out[f'{name}__map__{key}'] = m
        ops = []
        setup_smoothness_constraints({'z0': z0, 'dz': dz}, ops, dict(kw['E_RMS']), {0: 10, 1: 1},
                                     scaling_masks=masks or None)
        for op in ops:
            out[f'{name}__ec__{op.name}'] = np.asarray(op.expected, dtype=float)
        print(name, [(op.name, op.expected.size, np.unique(op.expected).size) for op in ops])
    np.savez_compressed(os.path.join(HERE, 'ec_scaled.npz'), **out)


if __name__ == '__main__':
    main()
