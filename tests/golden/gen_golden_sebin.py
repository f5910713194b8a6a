#!/usr/bin/env python3
"""Generate tests/golden/sys_sebin.npz: the binned sigma_extra mode of smooth_fit
(sigma_extra_bin_spacing, smooth_fit.py:151-158 -> calc_sigma_extra_on_grid,
calc_sigma_extra.py:46-109) run by the REFERENCE, with the stand-ins of _refstubs.py and the
helpers of gen_golden.py (a no-op where the reference is absent).

Modelled on gen_golden.gen_sekeys: 1 000 points on 1400 × 1200, outliers, 4 outer iterations;
sigma_extra_bin_spacing = 500 gives 9 bin centres, and the extra noise differs between the two
halves of the domain, so the bins — and, through the tent weights, the points — get visibly
different sigma_extra.  The fixture holds inputs and outputs only.

The test allows no edit flip, so the seed must leave no point of any outer iteration within 1e-6
of the editing threshold |r / sigma_aug| = 3: every call of the reference's
calc_sigma_extra_on_grid is recorded and the margin asserted here, on the CPU.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import E_RMS_NB, run_sf, synth_points   # noqa: E402

SEED = 20261022      # editing margin 1.0e-2 (20261019 leaves a point 1.7e-5 from the threshold)
BIN_SPACING = 500.


def gen_sebin(LS, stubs):
    rng = np.random.default_rng(SEED)
    W = {'x': 1400., 'y': 1200., 't': 1.25}
    ctr = {'x': 0., 'y': 0., 't': 0.}
    x, y, t, z = synth_points(rng, W, ctr, 1000)
    # the fit's own misfit is ≈ 0.45 here, so the noisy half needs clearly more than that
    z = z + np.where(x > 0, rng.normal(0, 1.5, x.size), rng.normal(0, 0.05, x.size))
    bad = rng.random(x.size) > 0.93
    z[bad] += (rng.random(bad.sum()) - 0.5) * 40

    # record every binned sigma_extra the reference computes, to measure the editing margin
    sf_mod = sys.modules['LSsurf.smooth_fit']
    ref_on_grid = sf_mod.calc_sigma_extra_on_grid
    calls = []

    def recording(xx, yy, r, sigma, in_TSE, **kw):
        se = ref_on_grid(xx, yy, r, sigma, in_TSE, **kw)
        calls.append((np.array(r), np.array(sigma), np.array(se)))
        return se

    sf_mod.calc_sigma_extra_on_grid = recording
    try:
        run_sf(LS, stubs, 'sebin', {'x': x, 'y': y, 'time': t, 'z': z, 'sigma': np.full(x.size, 0.1)},
               dict(W=W, ctr=ctr, spacing={'z0': 100., 'dz': 100., 'dt': 0.25}, E_RMS=E_RMS_NB,
                    reference_epoch=2, max_iterations=4, VERBOSE=False, dzdt_lags=[1],
                    sigma_extra_bin_spacing=BIN_SPACING))
    finally:
        sf_mod.calc_sigma_extra_on_grid = ref_on_grid
    assert calls, 'the reference never took the binned path'
    margin = min(float(np.min(np.abs(np.abs(r / np.sqrt(s ** 2 + se ** 2)) - 3.0))) for r, s, se in calls)
    centres = np.unique(np.round((x + 1j * y) / BIN_SPACING) * BIN_SPACING)
    distinct = np.unique(calls[-1][2]).size
    print(f'sebin: {len(calls)} binned calls, {centres.size} bin centres, {distinct} distinct sigma_extra, '
          f'editing margin {margin:.3e}')
    assert margin > 1e-6, 'a point sits on the editing threshold: choose another SEED'
    assert distinct > 2


def main():
    import _refstubs
    if not os.path.isdir(_refstubs.REF):
        print('gen_golden_sebin: reference absent; keeping the committed fixture')
        return
    LS = _refstubs.install()
    gen_sebin(LS, _refstubs)


if __name__ == '__main__':
    main()
