"""The host V-cycle of tests/mg_host.py, on the CPU: what tests/test_gpu_mg_vcycle.py relies on.

* no factor entry of any level of any case lies where a device R_b⁻¹ that agrees with the host's to
  rounding could round to another bf16 value, and every pivot is clear of the dead-column rule;
* V is symmetric (1e-12) and positive, and its float64 run stays near its extended-precision run
  (e_V; τ = max(1000·e_V, 1e-13) is the GPU tests' tolerance, so e_V must stay far below the
  smallest effect a defect has);
* randvec is the hash k_mg_randvec computes;
* sensitivity: each of eight defects a kernel could have moves V(u) by at least 1e-6 relative, so
  the GPU comparison at τ would see it.

Both precisions run on the same float64 level operators: e_V is the arithmetic's share alone (1e-16 to
2e-14 here; with the operators also formed in extended precision it is 1e-13 on t64, the rounding of
the operator's entries times the conditioning of the coarse levels, which the device shares)."""
import functools

import numpy as np
import pytest

import cgnr_host as CH
import mg_host as M

F64, LD = np.float64, np.longdouble


@functools.lru_cache(maxsize=None)
def _sys(name):
    S = M.case_system(name)
    return S, [float(v) for v in S.all_lambda()]


@pytest.mark.parametrize('name', M.CASES)
def test_factors_clear_of_bf16_boundaries(name):
    S, _ = _sys(name)
    S = getattr(S, 'sub', S)          # z0 refined: the node blocks are the dz-lattice levels'
    exact = M.level_factors(S.lev[F64], S.nt, round=False)      # asserts every pivot > MIN_PIVOT
    for l, f in enumerate(exact[:-1]):
        assert CH.at_risk_entries(CH.factor_entries(f)) == 0, (name, l)


@pytest.mark.parametrize('name', M.CASES)
def test_host_cycle_is_spd_and_precise(name):
    S, lam = _sys(name)
    V64, Vld = S.cycle(lam, F64), S.cycle(lam)
    for l in range(len(S.lev[F64])):
        u, v = M.test_vectors(S.lev[F64][l][1])
        Vu, Vv = V64(u, l), V64(v, l)
        assert abs(v @ Vu - u @ Vv) <= 1e-12 * (abs(v @ Vu) + abs(u @ Vv)), (name, l)
        assert u @ Vu > 0 and v @ Vv > 0
        assert np.all(Vu[~S.lev[F64][l][1]] == 0)
        e = CH.rel(Vu.astype(LD), Vld(u, l))
        print(f'{name} level {l}: e_V {e:.2e}')
        assert e < 1e-11, (name, l, e)


def test_host_lambda_is_below_the_spectrum_edge():
    """the power estimate is a Rayleigh quotient: never above λ_max, and the two precisions agree"""
    for name in ('7x70-8', 't64'):
        S, lam = _sys(name)
        lam_ld = S.host_lambda(LD)
        for l, (a, b) in enumerate(zip(lam, lam_ld)):
            assert abs(a - float(b)) <= 1e-13 * a
            assert a <= M.lambda_max(S.lev[F64][l], S.factors[l]) * (1 + 1e-9)


def test_randvec():
    shape, nt = (64, 64), 12
    keep = np.ones(64 * 64 * 13, bool)
    keep[4096 + 6::12] = False                                      # epoch 6 removed
    v = M.randvec(shape, keep, nt)
    assert v.min() >= -1.0 and v.max() < 1.0 and abs(v.mean()) < 0.02
    assert np.all(v[~keep] == 0.0) and np.count_nonzero(v) == keep.sum()
    # the hash in Python integers, at the first z0 column, the first dz column and the last column
    assert v[0] == -0.7244543728158208 and v[1] == 0.9126583242605983
    assert v[4096] == -0.07696283084394429 and v[53247] == 0.5605847254893881


def test_cheb_is_the_shifted_chebyshev_polynomial():
    """after g steps from x = 0 on the scalar equation a·x = 1, 1 − a·x is T_g((θ − a)/δ) / T_g(σ)"""
    lam = 2.7
    theta, delta = 0.5 * 1.21 * lam, 0.5 * 0.99 * lam
    for a in (0.2 * lam, 0.9 * lam, 1.3 * lam):
        x = d = 0.0
        for g in range(1, 5):
            c1, c2 = M.cheb(lam, g - 1)
            d = c1 * d + c2 * (1 - a * x)
            x += d
            T = np.polynomial.chebyshev.Chebyshev.basis(g)
            assert abs((1 - a * x) - T((theta - a) / delta) / T(theta / delta)) < 1e-13


WRONG = ['coarse_deg2', 'lam1', 'unrounded', 'pre_d0', 'drop_bx', 'prolong_last', 'coarsest_ref', 'post_restart']


@pytest.mark.parametrize('name', ['t64', '7x70-8'])
def test_sensitivity(name):
    S, lam = _sys(name)
    V = S.cycle(lam, F64)
    u = M.test_vectors(S.lev[F64][0][1])[0]
    Vu = V(u)
    for wrong in WRONG:
        if wrong == 'coarse_deg2':
            W = S.cycle(lam, F64, deg=2)
        elif wrong == 'lam1':
            W = S.cycle([lam[0], 1.01 * lam[1]] + lam[2:], F64)
        elif wrong == 'unrounded':
            W = S.cycle(lam, F64, factors=M.level_factors(S.lev[F64], S.nt, round=False))
        else:
            W = S.cycle(lam, F64, wrong=wrong)
        moved = CH.rel(W(u), Vu)
        print(f'{name} {wrong}: {moved:.2e}')
        assert moved >= 1e-6, (name, wrong, moved)
