"""Conditions on the inputs of tests/test_gpu_band_edges.py (host only): each case has the tile
width its table states, is well conditioned, keeps every band tile of R̃ busy, the host's one LSQR
step on A·M reproduces the refined x*, and — the proof that the GPU tests would notice a strided
loop of k_band_bsub / k_band_fsub that did nothing — leaving the strided tiles out of the host's
triangular solves moves x₁ by at least 1e-6.  A case that fails one of these is mended in the
generator (band_host.banded_system), never in the bound."""
import numpy as np
import pytest
import scipy.sparse as sp

import conftest  # noqa: F401
import band_host as H

ALL = list(H.CASES)


@pytest.mark.parametrize('n,reach', ALL)
def test_case_meets_its_conditions(n, reach):
    A, F, _, _ = H.case(n, reach)
    T, w = H.CASES[(n, reach)]
    assert H.tile_width(A) == (T, w) == (F.T, F.w)
    assert F.kappa <= 100.0, F.kappa
    assert np.all(np.diag(F.R) > 0)
    if n <= H.DENSE_EIG_MAX:
        assert np.all(np.tril(F.R, -1) == 0)
    for I in range(T):                                  # no band tile is idle
        for J in range(I, min(I + w, T - 1) + 1):
            t = F.R[I * 64:(I + 1) * 64, J * 64:(J + 1) * 64]
            assert np.abs(t).max() >= 1e-3, (I, J)
    if w + 1 < T:                                       # and R̃ has nothing outside the band
        assert np.all(np.triu(F.R, 64 * (w + 1)) == 0)
    for b in H.edge_rhs(A):
        xs = F.xstar(b)
        assert H.rel_err(H.host_one_step(A, b, F), xs) <= 1e-14
        assert H.rel_err(F.solve_normal(F.Aw.T @ (F.rs * b)), xs) <= 1e-14


@pytest.mark.parametrize('n,reach', [c for c in ALL if H.CASES[c][1] > 8])
def test_a_dead_strided_loop_moves_x1(n, reach):
    """Workgroup p of NW takes the tiles J − K − 1 ≡ p (mod NW): the first in its prefetch, the
    others (J − K − 1 ≥ NW) in the strided loop.  Without them x₁ is off by ≥ 1e-6, eight orders
    above the GPU tests' tolerance."""
    A, F, _, _ = H.case(n, reach)
    b, b_edge = H.edge_rhs(A)
    xs = F.xstar(b)
    tol = H.bound(H.rel_err(H.host_one_step(A, b, F), xs), F.w, F.kappa)
    assert tol < 1e-11
    for nw in H.NW_VALUES:
        if nw >= F.w:
            continue
        x1 = H.host_one_step(A, b, F, drop=lambda K, J: J - K - 1 >= nw)
        assert H.rel_err(x1, xs) >= 1e-6, nw
    x1 = H.host_one_step(A, b_edge, F, drop=lambda K, J: J - K - 1 >= H.NW_DEFAULT)
    assert H.rel_err(x1, F.xstar(b_edge)) >= 1e-6


@pytest.mark.parametrize('n,reach', [(65, 3), (897, 514)])
def test_reweighted_and_warm_references(n, reach):
    """The refactored system's host factor (row weights, 10 % of B's rows masked, the diagonal rows
    kept), the warm start, and the two ways to x* (dense factor, sparse LU) agree."""
    A, F, w_rows, keep = H.case(n, reach, reweight=True)
    assert keep[:n].all() and 0.05 < 1.0 - keep[n:].mean() < 0.2
    assert (F.T, F.w) == H.tile_width(A, keep=keep) and F.kappa <= 100.0
    b = H.edge_rhs(A)[0]
    xs = F.xstar(b)
    Ak = (sp.diags(w_rows * keep) @ A).tocsr()
    assert np.linalg.norm(Ak.T @ (w_rows * keep * b - Ak @ xs.astype(float))) <= 1e-12 * np.linalg.norm(Ak.T @ (w_rows * keep * b))
    assert H.rel_err(H.xstar_lu(A, b, w_rows, keep), xs) <= 4 * H.EPS
    assert H.rel_err(H.host_one_step(A, b, F), xs) <= 1e-14
    x0 = np.random.default_rng(3).standard_normal(n)
    assert H.rel_err(H.host_one_step(A, b, F, x0=x0), xs) <= 1e-14
    assert H.rel_err(H.host_one_step(A, b, F, x0=xs.astype(float)), xs) <= 1e-14


def test_block_order_keeps_the_band():
    for n, reach in [(768, 190), (897, 514)]:
        A, F, _, _ = H.case(n, reach, order='block')
        assert sorted(F.perm) == list(range(n))
        assert (F.T, F.w) == H.CASES[(n, reach)]
        b = H.edge_rhs(A, F.perm)[1]
        assert H.rel_err(H.host_one_step(A, b, F), F.xstar(b)) <= 1e-14


def test_window_sigma_is_the_conditional_sigma():
    A, F, _, _ = H.case(129, 128)
    cols = np.arange(20, 100)
    inner = (np.arange(80) >= 30) & (np.arange(80) < 50)
    ref = np.sqrt(np.diag(np.linalg.inv(F.N[np.ix_(cols, cols)])))
    sig = H.window_sigma(F.N, cols, inner)
    assert np.all(sig[~inner] == 0) and np.max(np.abs(sig[inner] / ref[inner] - 1)) < 1e-13
    op = sp.random(7, 129, density=0.1, random_state=2, format='csr')
    want = np.sqrt(np.diag(op @ np.linalg.inv(F.N) @ op.T))
    assert np.max(np.abs(H.op_sigma(F.N, op) / want - 1)) < 1e-13
