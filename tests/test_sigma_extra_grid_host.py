"""The batched binned-sigma_extra path on the host (no GPU): the lock-step port of scipy's bounded
scalar search, and calc_sigma_extra_on_grid through the segment builder + lock-step search with
the np.sort evaluator against the per-bin loop (the mirror of the reference), bit for bit."""
import numpy as np
import pytest
import scipy.optimize as scipyo

import importlib

from lssurf_amd.calc_sigma_extra import RDE, calc_sigma_extra, calc_sigma_extra_on_grid

cse = importlib.import_module('lssurf_amd.calc_sigma_extra')   # the package exports the function under this name


def grid_case():
    """20 000 points on [−2e4, 2e4]², spacing 1e4 (25 centres): 50 points with x on exact multiples
    of the spacing and 50 with y so (dx exactly 0 and exactly `half`), two groups one of which has
    fewer than 10 points in most bins, 5 % of the points outside in_TSE.  Shared with the GPU tests."""
    rng = np.random.default_rng(20241)
    n = 20000
    x = rng.uniform(-2e4, 2e4, n)
    y = rng.uniform(-2e4, 2e4, n)
    x[:50] = rng.integers(-2, 3, 50) * 1e4
    y[50:100] = rng.integers(-2, 3, 50) * 1e4
    sigma = rng.uniform(0.05, 0.2, n)
    r = rng.standard_normal(n) * np.sqrt(sigma ** 2 + (0.2 + 0.3 * (x > 0) + 0.2 * (y > 0)) ** 2)
    in_TSE = rng.uniform(size=n) > 0.05
    a = rng.uniform(size=n) < 0.6
    masks = {'a': a, 'b': ~a & (x < -1.2e4)}
    return dict(x=x, y=y, r=r, sigma=sigma, in_TSE=in_TSE, sigma_extra_masks=masks, spacing=1e4,
                sigma_extra_max=0.5)


def _drive(gen_fn, f, lo, hi):
    gen = gen_fn(lo, hi)
    x = next(gen)
    try:
        while True:
            x = gen.send(f(x))
    except StopIteration as stop:
        return stop.value


def _cost_functions():
    rng = np.random.default_rng(7)
    fs = []
    for c in (0.3, 1.0, 2.5, 7.9):                                  # smooth, interior minimum
        fs.append((lambda s, c=c: (s - c) ** 2, 0, 8.0))
        fs.append((lambda s, c=c: np.cosh(s - c) + 0.1 * np.sin(5 * s), 0, 8.0))
        fs.append((lambda s, c=c: np.abs(s - c) ** 0.5, 0.0, np.float64(8.0)))
    for lo, hi in ((0, 3.0), (1.0, 2.0), (-2.0, 5.0)):             # minimum at a bound
        fs.append((lambda s: s, lo, hi))
        fs.append((lambda s: -s, lo, hi))
        fs.append((lambda s: np.exp(-s), lo, hi))
    fs.append((lambda s: 1.0, 0, 1.0))                              # flat
    fs.append((lambda s: (s - 0.5) ** 2, 0, 0.0))                   # empty interval
    for n in (50, 50, 50, 11, 400):                                 # an RDE of few points: piecewise constant
        rr = rng.standard_normal(n) * 0.5
        ss = rng.uniform(0.05, 0.2, n)
        fs.append((lambda s, rr=rr, ss=ss: (RDE(rr / np.sqrt(s ** 2 + ss ** 2)) - 1) ** 2, 0, RDE(rr)))
    for step in (0.1, 0.5, 1.0):                                    # staircases
        fs.append((lambda s, step=step: (np.floor(s / step) * step - 1.3) ** 2, 0, np.float64(4.0)))
    for k in range(8):                                              # rough
        w = rng.uniform(1, 30, 3)
        fs.append((lambda s, w=w: np.sin(w[0] * s) + np.cos(w[1] * s) * 0.5 + (s - 1) ** 2 / w[2], 0, 2.0 + k))
    return fs


def test_lockstep_search_equals_scipy_bounded():
    fs = _cost_functions()
    assert len(fs) >= 36
    for f, lo, hi in fs:
        ref = scipyo.minimize_scalar(f, method='bounded', bounds=[lo, hi])
        x, nfev = _drive(cse._bounded_search, f, lo, hi)
        assert x == ref['x'] and nfev == ref['nfev'], (lo, hi, x, ref['x'], nfev, ref['nfev'])
    for lo, hi in ((1.0, 0.5), (0, np.nan), (0, np.inf)):          # scipy raises; so does the port
        with pytest.raises(ValueError):
            scipyo.minimize_scalar(lambda s: s, method='bounded', bounds=[lo, hi])
        with pytest.raises(ValueError):
            next(cse._bounded_search(lo, hi))


def test_lockstep_searches_advance_together():
    """_search_segments: one evaluator call per step for all unfinished segments; a finished
    segment leaves the active list."""
    rng = np.random.default_rng(3)
    n = 3000
    r, sigma = rng.standard_normal(n) * 0.4, rng.uniform(0.05, 0.2, n)
    segs = [np.sort(rng.choice(n, m, replace=False)) for m in (10, 37, 500, 2999)]
    calls = []

    class Counting(cse.HostSelect):
        def __call__(self, seg, s, raw=False):
            calls.append(len(seg))
            return super().__call__(seg, s, raw)

    val = cse._search_segments(r, sigma, segs, Counting)
    nfev = []
    for idx, v in zip(segs, val):
        rr, ss = r[idx], sigma[idx]
        ref = scipyo.minimize_scalar(lambda s1: (RDE(rr / np.sqrt(s1 ** 2 + ss ** 2)) - 1) ** 2, method='bounded',
                                     bounds=[0, RDE(rr)])
        assert v == ref['x']
        nfev.append(ref['nfev'])
    assert calls[0] == 4                                  # the raw bounds
    assert len(calls) == 1 + max(nfev) and sum(calls[1:]) == sum(nfev)
    assert calls[1:] == sorted(calls[1:], reverse=True)


def test_batched_grid_host_evaluator_equals_loop():
    case = grid_case()
    loop = calc_sigma_extra_on_grid(**case)
    centres = np.unique(np.round((case['x'] + 1j * case['y']) / case['spacing']) * case['spacing'])
    assert centres.size == 25
    assert np.unique(loop).size > 25 and np.max(loop) <= 0.5
    batched = calc_sigma_extra_on_grid(**case, evaluator='host')
    assert np.array_equal(batched, loop)
    # no cap, another averaging length (a point in up to 9 bins), one implicit group
    case2 = dict(case, sigma_extra_masks=None, sigma_extra_max=None, L_avg=2.5e4)
    assert np.array_equal(calc_sigma_extra_on_grid(**case2, evaluator='host'), calc_sigma_extra_on_grid(**case2))


def test_batched_groups_host_evaluator_equals_loop():
    case = grid_case()
    args = (case['r'], case['sigma'], case['in_TSE'], case['sigma_extra_masks'])
    assert np.array_equal(calc_sigma_extra(*args, evaluator='host'), calc_sigma_extra(*args))


def test_batched_path_falls_back_on_non_finite():
    case = grid_case()
    i = int(np.flatnonzero(case['sigma_extra_masks']['a'])[0])
    case['r'] = case['r'].copy()
    case['r'][i] = np.nan
    case['in_TSE'] = case['in_TSE'].copy()
    case['in_TSE'][i] = True
    with pytest.warns(UserWarning, match='host path'):
        got = calc_sigma_extra_on_grid(**case, evaluator='host')
    assert np.array_equal(got, calc_sigma_extra_on_grid(**case), equal_nan=True)
