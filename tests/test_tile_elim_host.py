"""CPU checks of the inputs of tests/test_gpu_tile_elim.py (tests/tile_elim_host.py) and of smooth_fit's
lsq_tile_eliminate key."""
import numpy as np
import pytest
import scipy.sparse as sp

import conftest  # noqa: F401
import lssurf_amd as LS
import tile_elim_host as T


def test_points_sit_on_the_upper_bounds():
    """the frames hold points whose float subscript is S − 1 exactly in y, x and t, and smooth_fit keeps them"""
    shape, nt = (7, 70), 17
    D, kw = T.points(shape, 2600, nt)
    for v, d, n in ((D.y, 'y', shape[0]), (D.x, 'x', shape[1]), (D.time, 't', nt)):
        hi = 0.5 * kw['W'][d]
        step = kw['spacing']['dt' if d == 't' else 'dz']
        assert v.max() == hi and np.count_nonzero(v == hi) >= 4
        assert (hi - (-hi)) / step == n - 1          # one IEEE division, as the formation computes it
    on_all = (D.y == 0.5 * kw['W']['y']) & (D.x == 0.5 * kw['W']['x']) & (D.time == 0.5 * kw['W']['t'])
    assert on_all.any()
    h = T.host(shape, 2600, nt)
    assert h.n_data == 2600 and tuple(h.S['grids']['dz'].shape) == (shape[0], shape[1], nt)


def test_written_out_system():
    """[A_d B U] with the constraint rows of the eliminated columns: shapes, and the normal equations'
    Schur complement on the grid columns is tests/test_gpu_bias._host_reduced's operator"""
    h = T.host((9, 11), 1200, 16)
    rng = np.random.default_rng(3)
    keep = rng.random(h.n_data) > 0.2
    ids, c = rng.integers(0, 5, h.n_data).astype(np.int32), rng.uniform(1., 30., 5)
    grp = np.where(ids < 2, ids, -1).astype(np.int32)
    slope = (grp, rng.standard_normal((h.n_data, 2)), rng.uniform(1., 5., (2, 2)))
    A, b, ng, nb = T.written_out(h, h.w, keep, ids, c)
    mask = np.concatenate([keep, np.ones(h.w.size - h.n_data, bool)])
    Ag = h.A(h.w, mask)
    assert A.shape == (Ag.shape[0] + 5, ng + 5) and b.size == A.shape[0] and (ng, nb) == (h.keep_cols.size, 5)
    N = (A.T @ A).toarray()
    p = rng.standard_normal(ng)
    red = N[:ng, :ng] @ p - N[:ng, ng:] @ np.linalg.solve(N[ng:, ng:], N[ng:, :ng] @ p)
    Wk, nk = h.w[:h.n_data][keep], int(keep.sum())
    t = Ag[:nk] @ p
    s = np.bincount(ids[keep], weights=Wk * t, minlength=5)
    Dj = np.bincount(ids[keep], weights=Wk ** 2, minlength=5) + c ** 2
    want = Ag.T @ (Ag @ p) - Ag[:nk].T @ (Wk * (s / Dj)[ids[keep]])
    assert np.abs(red - want).max() <= 1e-10 * np.abs(want).max()
    A2, b2, _, _ = T.written_out(h, h.w, keep, ids, c, slope)
    assert A2.shape == (A.shape[0] + 4, A.shape[1] + 4)
    U = sp.csr_matrix(A2)[:nk, ng + 5:].toarray()
    on = grp[keep] >= 0
    assert not U[~on].any() and np.allclose(U[on, 2 * grp[keep][on]], Wk[on] * slope[1][keep][on, 0])


def test_smooth_fit_key_must_be_a_bool():
    D, kw = T.points((9, 11), 1200, 16)
    with pytest.raises(ValueError, match='lsq_tile_eliminate'):
        LS.smooth_fit(data=D, VERBOSE=False, lsq_tile_eliminate=1, **kw)
