"""Host side of tests/test_gpu_tile_elim.py: the frames of cgnr_host.ksweep_points with more points and
a few of them exactly on the upper bounds of y, x and t (dmf_cell's clamped-cell branch), and the
least-squares system with the eliminated columns written out, for the dense oracle.
Test infrastructure only."""
import functools

import numpy as np
import scipy.sparse as sp

import cgnr_host as H

N_EDGE = 12   # points moved onto upper bounds: 4 in y, 4 in x, 4 in t, two of each also on a second bound


def points(shape, npts, nt):
    """cgnr_host.ksweep_points(shape, npts, nt) with the last N_EDGE points on the domain's upper faces:
    y = +W_y/2 (4 points), x = +W_x/2 (4), t = +W_t/2 (4); the first of each four also sits on the next
    dimension's upper bound (an edge of the box), and the very last point on all three (its corner)."""
    D, kw = H.ksweep_points(shape, npts, nt)
    hi = {d: 0.5 * kw['W'][d] for d in ('y', 'x', 't')}
    y, x, t = D.y.copy(), D.x.copy(), D.time.copy()
    n = D.size
    y[n - 12:n - 8] = hi['y']
    x[n - 8:n - 4] = hi['x']
    t[n - 4:] = hi['t']
    x[n - 12], t[n - 8], y[n - 4] = hi['x'], hi['t'], hi['y']
    y[n - 1], x[n - 1] = hi['y'], hi['x']
    D.assign(y=y, x=x, time=t)
    return D, kw


@functools.lru_cache(maxsize=None)
def host(shape, npts, nt):
    """cgnr_host.Host of points(shape, npts, nt)"""
    import lssurf_amd as LS
    D, kw = points(shape, npts, nt)
    h = H.Host(LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw), kw['reference_epoch'])
    assert h.n_data == npts, 'a point on an upper bound fell out of the grids'
    return h


def written_out(h, w, keep, ids, c, slope=None):
    """(A, b, n_grid, n_bias) of the fit with the eliminated columns written out: the kept data rows
    W [A_d  B  U], the grids' constraint rows, then one row c_j per bias and one row per slope column.
    Columns: the grids' kept columns, the biases, the slopes (x, y per group)."""
    mask = np.concatenate([keep, np.ones(h.w.size - h.n_data, bool)])
    Ag = h.A(w, mask)
    nk, n_grid, nb = int(keep.sum()), h.keep_cols.size, c.size
    Wk = w[:h.n_data][keep]
    cols = [sp.csr_matrix((Wk, (np.arange(nk), ids[keep])), shape=(nk, nb))]
    diag = [np.asarray(c, float)]
    if slope is not None:
        grp, u, cs = slope
        on = np.flatnonzero(grp[keep] >= 0)
        g = grp[keep][on]
        U = sp.csr_matrix((np.concatenate([Wk[on] * u[keep][on, 0], Wk[on] * u[keep][on, 1]]),
                           (np.concatenate([on, on]), np.concatenate([2 * g, 2 * g + 1]))), shape=(nk, cs.size))
        cols.append(U)
        diag.append(np.ravel(cs))
    Z = sp.hstack(cols).tocsr()
    nz = Z.shape[1]
    top = sp.hstack([Ag[:nk], Z])
    mid = sp.hstack([Ag[nk:], sp.csr_matrix((Ag.shape[0] - nk, nz))])
    bot = sp.hstack([sp.csr_matrix((nz, n_grid)), sp.diags(np.concatenate(diag))])
    A = sp.vstack([top, mid, bot]).tocsr()
    b = np.concatenate([(w * h.rhs)[mask], np.zeros(nz)])
    return A, b, n_grid, nb
