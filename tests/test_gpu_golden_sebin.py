"""smooth_fit's binned sigma_extra mode (sigma_extra_bin_spacing -> calc_sigma_extra_on_grid)
pinned to the reference: sys_sebin.npz (tests/golden/gen_golden_sebin.py) — 1 000 points, 9 bin
centres at 500 m spacing, extra noise that differs between the two halves of the domain, outliers,
4 outer iterations.  Tolerances as sys_sekeys (test_gpu_golden_depth.py): no edit flip (the
generator asserts that no point of the reference run sits within 1e-6 of |r/σ_aug| = 3),
sigma_extra ≤ 1e-5, z0 / dz / z_est ≤ 1e-6 relative."""
import numpy as np
import pytest

import lssurf_amd as LS
from conftest import golden, golden_kwargs, golden_points

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    ok = np.isfinite(b)
    return np.linalg.norm(a[ok] - b[ok]) / max(np.linalg.norm(b[ok]), 1e-300)


def test_binned_sigma_extra_matches_reference(gpu_available):
    g = golden('sys_sebin.npz')
    kw = golden_kwargs(g)
    assert kw['sigma_extra_bin_spacing'] == 500.
    S = LS.smooth_fit(data=golden_points(g), **kw)
    tse = S['data'].three_sigma_edit
    flips = int(np.sum(tse != g['data_three_sigma_edit'].astype(bool)))
    assert flips == 0
    se, ref = S['data'].sigma_extra, g['data_sigma_extra']
    assert np.unique(ref).size > 2                      # the bins really differ
    x = g['in_x']                                       # the noisier half carries the larger sigma_extra
    assert np.min(ref[x > 400]) > 1.5 * np.max(ref[x < -400])
    assert _rel(se, ref) < 1e-5
    assert _rel(S['m']['z0'].z0, g['z0']) < 1e-6
    assert _rel(S['m']['dz'].dz, g['dz']) < 1e-6
    assert _rel(S['data'].z_est, g['data_z_est']) < 1e-6
