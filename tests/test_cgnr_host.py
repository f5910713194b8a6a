"""tests/cgnr_host.py (TEST INFRASTRUCTURE: the host reference of tests/test_gpu_cgnr_iterates.py)
kept honest on the CPU: its bf16 rounding is torch's, bit for bit; with unrounded factors it runs the
iterates of oracle/cgnr_cpu.c; rounding the factors moves the iterates by far more than any
tolerance the GPU tests grant; and no factor entry of any input of the GPU tests lies where a
last-place difference between host and device R_b⁻¹ could round to another bf16 value."""
import numpy as np
import pytest

import cgnr_host as H
from conftest import golden, golden_csr
from oracle import cpu


def _torch_bf16(x):
    import torch
    return torch.tensor(np.asarray(x, np.float64), dtype=torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def test_bf16_round_is_torch_bf16_on_random_values():
    rng = np.random.default_rng(1)
    x = rng.uniform(1, 2, 100_000) * 2.0 ** rng.integers(-15, 15, 100_000) * rng.choice([-1., 1.], 100_000)
    assert np.unique(np.frexp(x)[1]).size == 30 and (x < 0).any() and (x > 0).any()
    got, want = H.bf16_round(x), _torch_bf16(x)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.count_nonzero(got != x) > 99_000          # the values were not representable to begin with


def test_bf16_round_ties_and_their_neighbours():
    """bf16 keeps 8 significand bits: m/128·2^e, 128 ≤ m < 256.  Exact ties (m + ½) go to the even
    m; one float32 ulp (2^-23 relative to 2^e) either side of a tie goes to the nearer."""
    m = np.arange(128, 256, dtype=np.float64)
    for e in (-9, 0, 7):
        s = 2.0 ** e
        tie = (m + 0.5) / 128 * s
        even = np.where(m % 2 == 0, m, m + 1) / 128 * s
        assert (m % 2 == 0).any() and (m % 2 == 1).any()
        ulp = 2.0 ** -23 * s
        for sign in (1., -1.):
            assert np.array_equal(H.bf16_round(sign * tie), sign * even)
            assert np.array_equal(H.bf16_round(sign * (tie - ulp)), sign * m / 128 * s)
            assert np.array_equal(H.bf16_round(sign * (tie + ulp)), sign * (m + 1) / 128 * s)
            for v in (tie, tie - ulp, tie + ulp):
                assert np.array_equal(H.bf16_round(sign * v).view(np.uint64), _torch_bf16(sign * v).view(np.uint64))
    z = H.bf16_round(np.array([0.0, -0.0]))
    assert np.array_equal(z, [0.0, 0.0]) and np.array_equal(np.signbit(z), [False, True])
    # the double rounding is lf_round's: below the float32 tie 1 + 2^-8 − 2^-30 goes first to the
    # float32 1 + 2^-8, an exact bf16 tie, and from there to the even 1.0
    assert H.bf16_round(1 + 2.0 ** -8 - 2.0 ** -30) == 1.0
    assert H.bf16_round(np.float64(3.0)).shape == ()


def test_block_list_adds_singletons():
    bp, cols = np.array([0, 3, 5, 8]), np.array([7, 1, 4, 9, 0, 2, 3, 8])
    bl = H.block_list(bp, cols, 12)
    assert [C.tolist() for C in bl] == [[[9, 0]], [[7, 1, 4], [2, 3, 8]], [[5], [6], [10], [11]]]
    assert [C.tolist() for C in H.block_list(None, None, 2)] == [[[0], [1]]]
    h = H.synthetic_host('t64z')
    bl = H.block_list(*h.blocks, h.keep_cols.size)
    assert h.keep_cols.size == 61185 and [C.shape for C in bl] == [(4096, 11), (16129, 1)]


def test_stats_at_small_dense_system():
    """stats_at against dense algebra on a random system with M⁻¹ formed as a matrix."""
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    A = sp.random(60, 12, density=0.4, random_state=rng, format='csr') + sp.eye(60, 12, format='csr')
    A, b = sp.csr_matrix(A), rng.standard_normal(60)
    blocks = H.block_list(np.array([0, 4, 8]), rng.permutation(12)[:8], 12)
    f = H.block_factors(A, blocks)
    Ad = A.toarray()
    Rt = np.zeros((12, 12))
    for C, Ri in f:
        for c, r in zip(C, Ri):
            Rt[np.ix_(c, c)] = r
    Re = np.zeros((12, 12))                  # unrounded: M is the block diagonal of AᵀA
    for C, Ri in H.block_factors(A, blocks, round=False):
        for c, r in zip(C, Ri):
            Re[np.ix_(c, c)] = r
            assert np.array_equal(r, np.triu(r))
    inb = Re @ Re.T != 0
    assert np.abs(np.linalg.inv(Re @ Re.T) - Ad.T @ Ad)[inb].max() < 1e-10 * np.abs(Ad.T @ Ad).max()
    assert np.array_equal(Rt, H.bf16_round(Re)) and not np.array_equal(Rt, Re)
    x0 = rng.standard_normal(12)
    out = H.pcg(A, b, f, 4, x0=x0)
    st = H.stats_at(A, b, f, out['x'][4], x0, out['alpha'], out['beta'])
    r = b - Ad @ out['x'][4]
    s = Ad.T @ r
    assert st['r1norm'] == pytest.approx(np.linalg.norm(r), rel=1e-13)
    assert st['arnorm'] == pytest.approx(np.sqrt(s @ Rt @ Rt.T @ s), rel=1e-13)
    assert st['arnorm'] == pytest.approx(np.sqrt(out['rho'][4]), rel=1e-10)
    assert st['xnorm'] == pytest.approx(np.linalg.norm(np.linalg.solve(Rt, out['x'][4] - x0)), rel=1e-12)
    al, be = out['alpha'], out['beta']
    assert st['anorm'] ** 2 == pytest.approx(sum(1 / al[i] + (be[i - 1] / al[i - 1] if i else 0) for i in range(4)))
    # 12 steps solve the 12-column system
    xs = np.linalg.lstsq(Ad, b, rcond=None)[0]
    assert H.rel(H.pcg(A, b, f, 12, x0=x0)['x'][12], xs) < 1e-9


@pytest.mark.parametrize('name', ['sf3d', 't64'])
def test_unrounded_factors_run_the_oracles_iterates(name):
    """round=False: the iterates of oracle.cpu.cgnr_bj(fixed_iters=k), at the bound
    test_oracle_cgnr.py holds between its two restatements."""
    if name == 'sf3d':
        g = golden('sys_sf3d.npz')
        h, A, b = H.golden_host('sf3d'), golden_csr(g), g['b']
    else:
        h, A, b, _ = H.host_case('t64')
    f = H.block_factors(A, H.block_list(*h.blocks, A.shape[1]), round=False)
    out = H.pcg(A, b, f, 20)
    for k in (1, 5, 20):
        xo, st = cpu.cgnr_bj(A, b, *h.blocks, fixed_iters=k, threads=2)
        assert int(st['iters']) == k
        assert np.linalg.norm(out['x'][k] - xo) <= 1e-10 * np.linalg.norm(xo), k


def test_rounded_factors_move_the_iterates():
    """The separation the GPU tests rely on: bf16 factors against exact ones on t64, more than 1e-5
    relative at every k ≤ 13 (measured 3.7e-3 at k = 1 falling to 4.7e-4 at 13), while float64 and
    extended precision agree to 1e-13."""
    h, A, b, blocks = H.host_case('t64')
    fe = H.block_factors(A, blocks, round=False)
    fr = H.block_factors(A, blocks)
    xe, xr = H.pcg(A, b, fe, 13)['x'], H.pcg(A, b, fr, 13)['x']
    xl = H.pcg(A, b, fr, 13, dtype=np.longdouble)['x']
    assert xl.dtype == np.longdouble
    for k in range(1, 14):
        assert H.rel(xe[k], xr[k]) > 1e-5, k
        assert H.rel(xr[k], xl[k]) < 1e-13, k


@pytest.mark.parametrize('name', H.BLOCK_CASES)
def test_no_factor_entry_near_a_rounding_boundary(name):
    """A condition on the inputs, not a tolerance: with an entry at risk the device's M and the
    reference's could differ by one bf16 step without any defect.  Should a new mask, weight or
    extra-row setting leave one, change its seed."""
    h, A, b, blocks = H.host_case(name)
    ent = H.factor_entries(H.block_factors(A, blocks, round=False))     # also asserts the pivots
    assert ent.size == sum(C.shape[0] * C.shape[1] * (C.shape[1] + 1) // 2 for C in blocks)
    assert H.at_risk_entries(ent) == 0
    assert H.at_risk_entries(ent, eps=1e-3) > 0 or ent.size < 1000     # the count does count
