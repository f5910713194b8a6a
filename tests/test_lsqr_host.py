"""tests/lsqr_host.py (TEST INFRASTRUCTURE: the host reference of tests/test_gpu_lsqr_iterates.py)
kept honest on the CPU: in float64 it runs scipy.sparse.linalg.lsqr's iterates and scalars on the
explicit A·M; in extended precision its x_k is the Krylov iterate that cgnr_host.pcg reaches by
another recurrence; each defect the GPU tests are there to catch moves x_k by more than 100·τ_k; no
block-factor entry of any case lies where a last-place difference between host and device R_b⁻¹
could round to another bf16 value; and the cases fall on the side of MF_LDS_MAX the GPU tests say."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import lsqr as scipy_lsqr

import cgnr_host as H
import lsqr_host as L

LD = np.longdouble
# Two float64 restatements of one recurrence differ by association alone; the reference's own
# float64-against-extended spread is ≤ 1.5e-15 for k ≤ 33 on these systems, so 1e-13 is 60 of them.
SCIPY_TOL = 1e-13


@pytest.mark.parametrize('warm', [False, True], ids=['cold', 'warm'])
@pytest.mark.parametrize('precond', [0, 1, 3])
@pytest.mark.parametrize('name', ['t64', 'ksweep-9x11-5'])
def test_float64_runs_scipys_iterates_and_scalars(name, precond, warm):
    c = L.case(name)
    x0 = H.warm_start(c.h) if warm else None
    f = c.factors(precond)
    M = L.m_explicit(f, c.A.shape[1])
    AM = sp.csr_matrix(c.A @ M)
    r0 = c.b if x0 is None else c.b - c.A @ x0
    out = L.lsqr(c.A, c.b, f, 17, x0=x0)
    for k in (1, 2, 5, 17):
        y, istop, itn, r1norm, _, anorm, acond, arnorm, xnorm, _ = scipy_lsqr(AM, r0, atol=0, btol=0, conlim=0,
                                                                             iter_lim=k)
        assert istop == 7 and itn == k
        x = M @ y + (0 if x0 is None else x0)
        assert H.rel(out['x'][k], x) <= SCIPY_TOL, (k, H.rel(out['x'][k], x))
        for fld, want in zip(L.SCALARS, (r1norm, anorm, acond, arnorm, xnorm)):
            assert abs(out[fld][k] - want) <= SCIPY_TOL * abs(want), (k, fld, out[fld][k], want)
        if warm:                                                  # xnorm is the correction's, not ‖M⁻¹x‖
            assert abs(np.linalg.norm(y) - xnorm) <= 1e-10 * xnorm


@pytest.mark.parametrize('name,precond', [('t64', 3), ('t64', 1), ('t64-x0', 3), ('ksweep-7x70-5', 3),
                                          ('ksweep-9x11-5', 3)])
def test_extended_precision_iterate_is_pcgs(name, precond):
    """LSQR on A·M and PCG on AᵀA with M⁻¹ = R̃R̃ᵀ reach the same Krylov iterate in exact arithmetic:
    in extended precision the two recurrences agree within 1e-15 for every k ≤ 33 (measured 1e-17 and
    less).  ksweep-7x70-13 is not among the cases: from k ≈ 20 its Lanczos vectors lose orthogonality as
    Ritz values converge, the two recurrences part by a factor 100 every 8 steps (6e-17 at k = 25, 6e-15
    at 33), and so do float64 and extended precision, which is what e_k and τ_k of that case measure."""
    c = L.case(name)
    f = c.factors(precond)
    ours = L.lsqr(c.A, c.b, f, 33, x0=c.x0, dtype=LD)['x']
    theirs = H.pcg(c.A, c.b, f, 33, x0=c.x0, dtype=LD)['x']
    assert ours.dtype == LD
    worst = max(H.rel(ours[k], theirs[k]) for k in range(1, 34))
    assert worst <= 1e-15, worst


def test_scalars_against_their_definitions():
    """r1norm = ‖b − A x_k‖ and arnorm = ‖MᵀAᵀ(b − A x_k)‖ from the iterate itself, xnorm = ‖y_k‖."""
    c = L.case('ksweep-9x11-5')
    f = c.factors(3)
    x0 = H.warm_start(c.h)
    out = L.lsqr(c.A, c.b, f, 9, x0=x0, dtype=LD)
    A = c.A.astype(LD)
    for k in (1, 4, 9):
        r = c.b - A @ out['x'][k]
        assert abs(np.sqrt(r @ r) - out['r1norm'][k]) <= 1e-14 * out['r1norm'][k]
        s = L.apply_mt(f, A.T @ r)
        assert abs(np.sqrt(s @ s) - out['arnorm'][k]) <= 1e-10 * out['arnorm'][0]
        y = np.zeros_like(r, shape=A.shape[1])
        for C, Ri in f:
            y[C] = np.linalg.solve(Ri, (out['x'][k] - x0)[C].astype(np.float64)[:, :, None])[:, :, 0]
        assert abs(np.sqrt(y @ y) - out['xnorm'][k]) <= 1e-12 * out['xnorm'][k]


# ---- sensitivity: each defect moves x_k by more than 100·τ_k ------------------------------------
SENS = ['t64', 'ksweep-9x11-5']


def _moved(ref, xs, ks):
    """{k: ‖xs[k] − x_k^ld‖ / ‖x_k^ld‖ in units of τ_k}"""
    return {k: ref.dev(k, xs[k]) / ref.tau[k] for k in ks}


def _assert_moved(ref, xs, ks, what):
    moved = _moved(ref, xs, ks)
    print(what, {k: f'{v:.1e}' for k, v in moved.items()})
    assert min(moved.values()) > 100, (what, moved)


def _n_data_rows(c):
    return int(np.count_nonzero(c.mask[:c.h.n_data]))


@pytest.mark.parametrize('name', SENS)
def test_sensitivity_factor_entry_one_bf16_step(name):
    """The largest off-diagonal entry of the first node block's R̃ moved to the next bf16 value."""
    c = L.case(name)
    ref = c.ref(3, 33)
    f = c.factors(3)
    k0 = max(range(len(f)), key=lambda i: f[i][0].shape[1])
    C, Ri = f[k0]
    Ri = Ri.copy()
    off = np.abs(np.triu(Ri[0], 1))
    i, j = np.unravel_index(np.argmax(off), off.shape)
    assert off[i, j] > 0
    v = np.float32(Ri[0, i, j])
    Ri[0, i, j] = float((v.view(np.uint32) + np.uint32(0x10000)).view(np.float32))
    assert Ri[0, i, j] == H.bf16_round(Ri[0, i, j]) and abs(Ri[0, i, j] / float(v) - 1) <= 2.0 ** -7
    bad = f[:k0] + [(C, Ri)] + f[k0 + 1:]
    _assert_moved(ref, L.lsqr(c.A, c.b, bad, 33, dtype=LD)['x'], L.K, 'one bf16 step')


@pytest.mark.parametrize('name', SENS)
def test_sensitivity_factor_for_its_transpose(name):
    """R̃ where R̃ᵀ belongs in the Aᵀ leg (the block epilogue's M for Mᵀ)."""
    c = L.case(name)
    _assert_moved(c.ref(3, 33), L.lsqr(c.A, c.b, c.factors(3), 33, dtype=LD, defect='mt_swap')['x'], L.K, 'mt_swap')


@pytest.mark.parametrize('name,ks', [('t64', L.K[1:]), ('ksweep-9x11-5', L.K), ('ksweep-7x70-13', L.K),
                                     ('sf3d', L.K)])
def test_sensitivity_one_stencil_rows_weight(name, ks):
    """The weight of ONE stencil row (the one with the largest |A x_1|) off by 1e-6, the factors
    unchanged.  t64 from k = 2: its x_1 depends on one of 288 655 rows through β_2 alone and moves by
    57 τ_1 (440 τ_k and more from there on); the small lattices pass at k = 1 as well."""
    c = L.case(name)
    ref = c.ref(3, 33)
    nd = _n_data_rows(c)
    act = np.abs(c.A @ ref.f64['x'][1])
    act[:nd] = 0
    scale = np.ones(c.A.shape[0])
    scale[int(np.argmax(act))] += 1e-6
    xs = L.lsqr(sp.csr_matrix(sp.diags(scale) @ c.A), c.b, c.factors(3), 33, dtype=LD)['x']
    _assert_moved(ref, xs, ks, 'row weight')


@pytest.mark.parametrize('name', SENS)
def test_sensitivity_edge_rows_template_entry_dropped(name):
    """The first stencil row (its centre lies on the grid's corner) without its first entry: what a
    wrong edge-class mask of mf_at_part, or a band of k_mf_fwd one entry short, computes."""
    c = L.case(name)
    A = c.A.copy()
    e = A.indptr[_n_data_rows(c)]
    assert A.indptr[_n_data_rows(c) + 1] - e >= 2 and A.data[e] != 0
    A.data[e] = 0
    _assert_moved(c.ref(3, 33), L.lsqr(A, c.b, c.factors(3), 33, dtype=LD)['x'], L.K, 'entry dropped')


@pytest.mark.parametrize('precond', [1, 3])
@pytest.mark.parametrize('name', SENS)
def test_sensitivity_owed_update_missing(name, precond):
    """x_{k−1} handed out as x_k: the deferred x/w update of the last step never applied."""
    ref = L.case(name).ref(precond, 33)
    xs = {k: ref.ld['x'][k - 1] for k in L.K if k > 1}      # k = 1 would return x0 = 0: no relative distance needed
    assert np.all(ref.ld['x'][0] == 0) and ref.dev(1, ref.ld['x'][0]) == 1.0
    _assert_moved(ref, xs, [k for k in L.K if k > 1], 'owed update')


@pytest.mark.parametrize('precond', [1, 3])
@pytest.mark.parametrize('name', SENS)
def test_sensitivity_stale_v(name, precond):
    """ṽ of step k − 1 read in place of step k's in the w update (the wrong parity buffer): active
    from k = 2, since w_1 = v_1 is set by the set-up."""
    c = L.case(name)
    ref = c.ref(precond, 33)
    xs = L.lsqr(c.A, c.b, c.factors(precond), 33, dtype=LD, defect='stale_v')['x']
    assert ref.dev(1, xs[1]) <= 1e-17
    _assert_moved(ref, xs, [k for k in L.K if k > 1], 'stale v')


@pytest.mark.parametrize('name', SENS)
def test_sensitivity_column_scale_twice(name):
    """cs applied by the kernel to values that already carry it (precond 1)."""
    c = L.case(name)
    _assert_moved(c.ref(1, 33), L.lsqr(c.A, c.b, c.factors(1), 33, dtype=LD, defect='cs_twice')['x'], L.K, 'cs twice')


# ---- conditions on the inputs ---------------------------------------------------------------------
@pytest.mark.parametrize('name', L.BLOCK_CASES)
def test_no_factor_entry_near_a_rounding_boundary(name):
    """A condition on the inputs, not a tolerance (tests/test_cgnr_host.py): with an entry at risk the
    device's M and the reference's could differ by one bf16 step without any defect.  Should a new
    mask or weight setting leave one, change its seed."""
    c = L.case(name)
    ent = H.factor_entries(c.factors(3, round=False))            # also asserts the pivots
    assert ent.size == sum(C.shape[0] * C.shape[1] * (C.shape[1] + 1) // 2 for C in c.blocks)
    assert H.at_risk_entries(ent) == 0


def test_rows_case_leaves_no_part_with_one_row_scale():
    """t64-rows: every stencil part's rows carry at least two different weights (wconst = 0), where
    t64-mask leaves every part with one."""
    from lssurf_amd.assemble import describe
    c, cm = L.case('t64-rows'), L.case('t64-mask')
    stencils = describe(c.h.S['G_data'], c.h.S['Gc'], with_fields=True)[3]
    assert len(stencils) >= 3
    for s in stencils:
        assert np.unique(c.w[s.row0:s.row0 + s.n_eq]).size > 1
        assert np.unique(cm.w[s.row0:s.row0 + s.n_eq]).size == 1
    assert np.array_equal(c.mask, cm.mask) and np.array_equal(c.w[:c.h.n_data], cm.w[:c.h.n_data])


def test_which_side_of_the_lds_limit_each_case_falls_on():
    """The constants are system.hpp's; every case but hbm stages every grid's bands in LDS, hbm's dz
    grid exceeds MF_LDS_MAX and gathers from HBM while its z0 grid stays staged."""
    hpp = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lssurf_amd', 'csrc',
                            'system.hpp')).read()
    npt = int(re.search(r'constexpr int MF_NPT = (\d+);', hpp).group(1))
    assert re.search(r'constexpr int MF_ALIGN = 256 \* MF_NPT;', hpp) and 256 * npt == L.MF_ALIGN
    assert int(re.search(r'constexpr int MF_LDS_MAX = (\d+);', hpp).group(1)) == L.MF_LDS_MAX
    want = {'t64': 1575, 'ta64': 1575, 'sf3d': 1557, 'nb_xt': 1566, 'ksweep-9x11-2': 1545, 'ksweep-9x11-5': 1554,
            'ksweep-7x70-13': 1578, 'hbm': 4119}
    for name in L.CASES:
        got = L.case(name).lds()
        assert got['z0'] == 1542
        if name == 'lin2d':
            assert list(got) == ['z0']
            continue
        assert got['dz'] == want.get(name, want['t64']), (name, got)
        assert (got['dz'] > L.MF_LDS_MAX) == (name == 'hbm')
    nt = L.HBM_NT
    assert want['hbm'] == 3 * (L.MF_ALIGN + nt + 1)      # three y offsets, each spanning ox = ±1 … ot
