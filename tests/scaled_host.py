"""Inputs and host references of the tests of per-row constraint scales inside CGNR (lsq_set_cg_scaled,
smooth_fit(lsq_cg_scaled=True); k_cg_scaled in lssurf_amd/csrc/lsqr_cg.inc): smooth_fit systems whose
constraint rows carry one row scale per (y, x) node — a non-uniform mask_data with the default mask_scale,
constraint_scaling_maps, or both — and a numpy restatement of the stencil rows' normal operator from the
part descriptors and the squared-scale fields.  tests/test_scaled_host.py and tests/test_gpu_cg_scaled.py
share them.  Test infrastructure only.

Lattices (ny, nx, nt): non-square, no multiple of any tile (the scaled kernel's 8 or 4 × 16 nodes, the
ring kernel's 64 columns); (17, 66, 12) has two ring tiles and five scaled tiles in x.  reference_epoch
takes 0, nt // 2 and nt − 1.  Masks: one isolated 0 node; zeros along the four edges, 2 / 1 / 1 / 3 nodes
wide; a checkerboard.  Maps: uniform in [0.5, 2] from default_rng, on d3z_dx2dt (which the grad_dzdt rows
take too) and d2z_dt2 — every dz part is then scaled and the dz class table is empty — and on d2z0_dx2
(grad2_z0 and grad_z0: scaled parts on the 2-D grid)."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import cgnr_host as H

MAP_SEED = 20261021
DENSE_MAX = 8000     # columns up to which exact() runs the dense oracle (about 1 s at 7 350)

# name: (ny, nx, nt), points, reference_epoch, mask kind or None, map keys
SYSTEMS = {
    'iso': ((21, 70, 5), 6000, 0, 'iso', ()),
    'edges': ((21, 70, 5), 6000, 2, 'edges', ()),
    'checker': ((21, 70, 5), 6000, 4, 'checker', ()),
    'maps-z0': ((9, 33, 3), 800, 0, None, ('d2z0_dx2',)),
    'maps-dz': ((12, 37, 15), 2500, 7, None, ('d3z_dx2dt', 'd2z_dt2')),
    'mask-maps': ((17, 66, 12), 5000, 11, 'edges', ('d3z_dx2dt', 'd2z0_dx2')),
}
# What lsq_cg_scaled_info must report: the parts whose rows do not share one scale.  The stencil parts are
# grad2_z0 (3: xx, yy, xy) and grad_z0 (2) on z0, grad2_dzdt (3), grad_dzdt (2) and d2z_dt2 (1) on dz.  A
# 2-D mask_data applies to the dz grid alone and d2z_dt2 ignores it: 5.  A map on d2z0_dx2 scales grad2_z0
# and grad_z0 (which falls back on that key): 5.  A map on d3z_dx2dt scales grad2_dzdt and grad_dzdt
# (likewise): 5, with d2z_dt2's own map 6.
SCALED_PARTS = {'iso': 5, 'edges': 5, 'checker': 5, 'maps-z0': 5, 'maps-dz': 6, 'mask-maps': 10}


def mask_of(kind, ny, nx):
    """the (ny, nx) bool mask_data of a kind (None: none)"""
    if kind is None:
        return None
    m = np.ones((ny, nx), bool)
    if kind == 'iso':
        m[ny // 2, nx // 3] = False
    elif kind == 'edges':
        m[:2] = False
        m[-1:] = False
        m[:, :1] = False
        m[:, -3:] = False
    elif kind == 'checker':
        yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
        m = (yy + xx) % 2 == 0
    else:
        raise ValueError(kind)
    return m


def maps_of(keys, name, ny, nx):
    """constraint_scaling_maps of a system: arrays on the (y, x) nodes, one rng stream per (system, key)"""
    out = {}
    for k, key in enumerate(keys):
        rng = np.random.default_rng([MAP_SEED, sorted(SYSTEMS).index(name), k])
        out[key] = rng.uniform(0.5, 2., (ny, nx))
    return out or None


def points(name):
    """(data, smooth_fit keywords) of a system: cgnr_host.ksweep_points' lattice and points with this
    system's reference epoch, mask and maps"""
    (ny, nx, nt), npts, ref, kind, keys = SYSTEMS[name]
    D, kw = H.ksweep_points((ny, nx), npts, nt)
    kw = dict(kw, reference_epoch=ref)
    mask = mask_of(kind, ny, nx)
    if mask is not None:
        kw['mask_data'] = mask
    maps = maps_of(keys, name, ny, nx)
    if maps is not None:
        kw['constraint_scaling_maps'] = maps
    return D, kw


@functools.lru_cache(maxsize=None)
def host(name):
    """cgnr_host.Host of a system (its w = 1 / [Ed; Ec] holds the masked and mapped constraint scales)"""
    import lssurf_amd as LS
    D, kw = points(name)
    return H.Host(LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw), kw['reference_epoch'])


def data_mask(h, seed=5):
    """row mask with 20 % of the data rows dropped"""
    keep = np.random.default_rng(seed).random(h.n_data) > 0.2
    return np.concatenate([keep, np.ones(h.w.size - h.n_data, bool)])


@functools.lru_cache(maxsize=None)
def exact(name):
    """(A, b, x*) with every row kept: x* from the dense oracle, above DENSE_MAX columns from a sparse LU
    of AᵀA with the oracle's corrected semi-normal refinement (the dense factor of 13 464 columns takes
    1.5 GB and tens of seconds)"""
    from oracle.dense import ls_solve_dense
    h = host(name)
    A, b = h.A(), h.w * h.rhs
    if A.shape[1] <= DENSE_MAX:
        return A, b, ls_solve_dense(A, b)
    lu = spla.splu((A.T @ A).tocsc())
    x = lu.solve(A.T @ b)
    for _ in range(4):
        dx = lu.solve(A.T @ (b - A @ x))
        x = x + dx
        if np.max(np.abs(dx)) <= 1e-15 * max(1.0, np.max(np.abs(x))):
            break
    return A, b, x


# ---- the scaled normal, restated from the part descriptors ------------------------------------------
def stencil_parts(h):
    """[(grid shape (3), col0, row0 among the constraint rows, lo, hi, offsets (ntpl, 3), values)] of the
    stencil parts, from the descriptors the device is formed from (assemble.describe)"""
    from lssurf_amd.assemble import describe
    gdesc, interp, coords, stencils, npts, fields = describe(h.S['G_data'], h.S['Gc'], with_fields=True)
    assert not fields
    out = []
    for s in stencils:
        g = gdesc[s.grid]
        nd = int(g.ndim)
        shape = tuple(int(g.shape[k]) for k in range(nd)) + (1,) * (3 - nd)
        lo = tuple(int(s.lo[k]) for k in range(nd)) + (0,) * (3 - nd)
        hi = tuple(int(s.hi[k]) for k in range(nd)) + (1,) * (3 - nd)
        off = np.array([[int(s.off[t][k]) for k in range(nd)] + [0] * (3 - nd) for t in range(s.ntpl)])
        val = np.array([float(s.val[t]) for t in range(s.ntpl)])
        assert int(s.n_eq) == int(np.prod(np.subtract(hi, lo)))
        out.append((shape, int(g.col0), int(s.row0) - npts, lo, hi, off, val))
    return out


def part_fields(h, w):
    """Per stencil part: (W2, uniform) with W2 the (y, x) field of squared row scales read from the rows at
    the first dim-2 position, uniform = every row shares one scale.  Asserts what the device checks: the
    scale is bit-equal along dim 2 at every (y, x)."""
    out = []
    for shape, col0, row0, lo, hi, off, val in stencil_parts(h):
        box = tuple(np.subtract(hi, lo))
        ws = w[h.n_data + row0:h.n_data + row0 + int(np.prod(box))].reshape(box)
        assert np.array_equal(ws, np.broadcast_to(ws[:, :, :1], box)), 'row scales differ along dim 2'
        out.append((ws[:, :, 0] ** 2, bool(np.all(ws == ws.flat[0]))))
    return out


def scaled_normal(h, w, mask, p):
    """AᵀA p over the kept columns, restated: the data rows through the host CSR, every stencil part as
    q += A_qᵀ (W2 ∘ A_q p) on its grid with W2 the part's (y, x) field — t at the part's centre box from
    shifted slices of p, q from the same slices, the removed columns of p zero and their q dropped"""
    nd = h.n_data
    Ad = h.A(w, mask)[:int(np.count_nonzero(mask[:nd]))]
    q = Ad.T @ (Ad @ p)
    assert np.all(mask[nd:]), 'constraint rows are always kept'
    pf = np.zeros(h.n_full)
    pf[h.keep_cols] = p
    qf = np.zeros(h.n_full)
    for (shape, col0, row0, lo, hi, off, val), (W2, _) in zip(stencil_parts(h), part_fields(h, w)):
        P = pf[col0:col0 + int(np.prod(shape))].reshape(shape)
        Q = qf[col0:col0 + int(np.prod(shape))].reshape(shape)
        sl = [tuple(slice(lo[k] + o[k], hi[k] + o[k]) for k in range(3)) for o in off]
        t = sum(v * P[s] for v, s in zip(val, sl)) * W2[:, :, None]
        for v, s in zip(val, sl):
            Q[s] += v * t
    return q + qf[h.keep_cols]
