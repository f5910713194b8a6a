"""tests/dense_host.py (TEST INFRASTRUCTURE: the host reference of tests/test_gpu_dense.py) kept
honest on the CPU: the extended-precision factors satisfy their definitions at extended-precision
rounding level; the float64 run's own deviations stay under the cap that keeps every tolerance of the
GPU tests below 1e-11; each defect the GPU tests are there to catch moves its metric by more than
100 tolerances; and one LSQR step preconditioned by R⁻¹ lands on the normal-equations solution, which
is why the GPU tests pin k = 1 and nothing after it."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import lsqr as scipy_lsqr

import dense_host as D
import lsqr_host as L

LD = np.longdouble
EPS = float(np.finfo(LD).eps)


def _fro(a):
    return float(np.sqrt((a * a).sum()))


def test_block_rows_are_the_ones_the_kernels_need():
    assert tuple(-(-n // D.TB) for n in D.SIZES) == D.BLOCK_ROWS
    assert [n for n in D.SIZES if n % D.TB == 1 and n > 1] == [65, 129, 193, 257]
    A, _, _ = D.wide_system()
    assert A.shape == (D.WIDE_BLOCKS * D.WIDE_M, 8200) and A.shape[1] > 2048 * 4
    assert D.WIDE_K % D.TB and D.TB % D.WIDE_K          # the blocks straddle the tile edges
    for n in D.SIZES:
        A, w, keep = D.system(n)
        assert A.shape == (4 * n + 3, n) and w.min() >= 0.5 and w.max() <= 2
        assert 0.8 <= keep.mean() <= (1 if n < 3 else 0.97)


@pytest.mark.parametrize('name', D.ALL)
def test_reference_satisfies_its_definitions(name):
    """R_ldᵀR_ld = N_ld and R_ld·Ri_ld = I within 8·k·eps_ld of their norms, block by block (measured:
    below 1·k·eps_ld); Ri_ld is upper triangular with a positive diagonal."""
    r = D.ref(name)
    assert r.R_ld.dtype == LD and r.Ri_ld.dtype == LD and r.N_ld.dtype == LD and EPS < 1e-18
    k = r.cols.shape[1]
    worst = [0.0, 0.0]
    for N, R, Ri in zip(r.N_ld, r.R_ld, r.Ri_ld):
        worst[0] = max(worst[0], _fro(R.T @ R - N) / _fro(N))
        worst[1] = max(worst[1], _fro(R @ Ri - np.eye(k, dtype=LD)) / (_fro(R) * _fro(Ri)))
        assert not np.tril(Ri, -1).any() and not np.tril(R, -1).any() and (np.diagonal(Ri) > 0).all()
    print(name, [f'{v / (k * EPS):.2f} k eps' for v in worst])
    assert max(worst) <= 8 * k * EPS, worst
    E = np.sqrt(np.array([np.diagonal(np.linalg.inv(N.astype(np.float64))) for N in r.N_ld])).ravel()
    np.testing.assert_allclose(r.E_ld.astype(np.float64), E, rtol=1e-9)       # E is sqrt(diag(N⁻¹))


@pytest.mark.parametrize('name', D.ALL)
def test_float64_spread_stays_under_the_cap(name):
    """A condition on the inputs, not a measurement: e ≤ 1e-14 and e_E ≤ 1e-14, so no tau exceeds
    1e-11.  Should a system miss it, change the system, not the cap.  (Measured: 1.2e-16 … 1.4e-15 on
    the random systems and the wide one, 8.9e-15 / 6.8e-15 on ksweep-9x11-2.)"""
    r = D.ref(name)
    print(name, f'e {r.e:.2e} e_E {r.e_E:.2e} tau {r.tau:.2e} tau_E {r.tau_E:.2e}')
    assert 0 < r.e <= 1e-14 and 0 < r.e_E <= 1e-14
    assert r.tau == max(1000 * r.e, 1e-13) <= 1e-11 and r.tau_E == max(1000 * r.e_E, 1e-13) <= 1e-11


# ---- sensitivity: every defect moves its metric by more than 100 tolerances ----------------------
def _moved(r, Ri, what):
    dev, dE = r.rowdev(Ri) / r.tau, r.edev(r.rowrss(Ri[None])) / r.tau_E
    print(f'{what} on n = {r.n}: rowdev {dev:.1e} tau, E {dE:.1e} tau_E')
    return dev, dE


@pytest.mark.parametrize('name', ['193-plain', '193-graded', '257-plain', '257-graded', D.STRUCTURED])
def test_sensitivity_dropped_kb_term(name):
    r = D.ref(name)
    dev, dE = _moved(r, D.defective(r, 'drop_kb'), 'drop_kb')
    assert dev > 100 and dE > 100


@pytest.mark.parametrize('name', ['129-plain', '193-plain', '193-graded', '257-graded'])
def test_sensitivity_skipped_syrk_tile(name):
    r = D.ref(name)
    dev, dE = _moved(r, D.defective(r, 'skip_syrk_tile'), 'skip_syrk_tile')
    assert dev > 100 and dE > 100


@pytest.mark.parametrize('name', ['65-plain', '65-graded'])
def test_sensitivity_padding_not_identity(name):
    r = D.ref(name)
    dev, dE = _moved(r, D.defective(r, 'pad_not_identity'), 'pad_not_identity')
    assert dev > 100 and dE > 100


@pytest.mark.parametrize('name', ['65-plain', '193-plain', '193-graded', D.STRUCTURED])
def test_sensitivity_masked_row_used(name):
    if name == D.STRUCTURED:                 # that case keeps every row: mask a tenth of them here
        A, w, _ = D.inputs(name)
        r = D.Ref(A, w, D.weights_and_mask(A.shape[0], 5)[1])
    else:
        r = D.ref(name)
    assert not r.keep.all()
    dev, dE = _moved(r, D.defective(r, 'masked_row_in'), 'masked_row_in')
    assert dev > 100 and dE > 100


@pytest.mark.parametrize('name', ['65-plain', '193-graded', D.STRUCTURED])
def test_sensitivity_stale_weights(name):
    A, w, keep = D.inputs(name)
    w2 = D.weights_and_mask(A.shape[0], 7)[0] * (w if name == D.STRUCTURED else 1)
    r = D.Ref(A, w2, keep, w_prev=w)
    dev, dE = _moved(r, D.defective(r, 'stale_weights'), 'stale_weights')
    assert dev > 100 and dE > 100


@pytest.mark.parametrize('name', ['129-plain', '257-plain', D.STRUCTURED])
def test_sensitivity_warm_start_through_the_inverse(name):
    st = D.step(name, True)
    moved = st.dev(1, D.defective(D.ref(name), 'r_for_ri_warm', step=st)) / st.tau[1]
    print(f'r_for_ri_warm on {name}: x_1 {moved:.1e} tau_1')
    assert moved > 100


# ---- the one step ----------------------------------------------------------------------------------
@pytest.mark.parametrize('warm', [False, True], ids=['cold', 'warm'])
@pytest.mark.parametrize('name', D.STEP_CASES)
def test_one_step_is_the_normal_equations_solution(name, warm):
    """x_1^ld = R_ld⁻¹R_ld⁻ᵀ A_wᵀb_w within 1e-15: LSQR on an operator with orthonormal columns is done
    after one step, from any start.  The host float64 arnorm_1 / (anorm_1·r1norm_1) is rounding noise;
    tests/test_gpu_dense.py bounds the device's by 1000 times it (floor 1e-12)."""
    r, st = D.ref(name), D.step(name, warm)
    assert st.kmax == 1 and (st.x0 is not None) == warm
    want = r.solution(D.rhs(name))
    d = st.dev(1, st.ld['x'][1], want)
    ratio = {p: D.arnorm_ratio(getattr(st, p)) for p in ('f64', 'ld')}
    print(f'{name} warm {warm}: x_1^ld from the solution {d:.1e}; arnorm ratio f64 {ratio["f64"]:.1e}, '
          f'extended {ratio["ld"]:.1e}; e_1 {st.e[1]:.1e}; r1norm {float(st.ld["r1norm"][1]):.3g} '
          f'of ‖b_w‖ {float(st.ld["r1norm"][0]):.3g}')
    assert d <= 1e-15
    assert ratio['f64'] <= 1e-13 and ratio['ld'] <= 1e-16            # noise at each precision's level
    assert st.ld['r1norm'][1] > 0.1 * np.sqrt((r.weighted(D.rhs(name))[1] ** 2).sum())   # b has a residual
    assert st.e[1] <= 1e-14 and st.tau[1] <= 1e-11
    for f in ('r1norm', 'anorm', 'acond', 'xnorm'):
        assert st.es[f][1] <= 1e-14, (f, st.es[f][1])
    # scipy's own LSQR on the explicit A·R⁻¹: maxit = 1 stops it (istop 7) unless the noise arnorm_1 is
    # below machine precision as well, when its later rule 1 + test2 ≤ 1 overwrites the 7 with a 5
    A_w, b_w = r.weighted(D.rhs(name))
    out = scipy_lsqr(sp.csr_matrix(A_w @ L.m_explicit(r.factors, r.n)), b_w - (A_w @ st.x0 if warm else 0), atol=0,
                     btol=0, conlim=0, iter_lim=1)
    assert out[2] == 1 and (out[1] == 7 or (out[1] == 5 and 1.0 + out[7] / (out[5] * out[3]) <= 1.0)), out[1:8]
    if warm:                                                           # the start is 10 % off, not the solution
        assert 0.01 <= st.dev(1, st.x0, want) <= 1
