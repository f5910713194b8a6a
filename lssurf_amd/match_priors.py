"""Prior constraints that tie a fit's dz to saved dz grids (LSsurf/match_priors.py): a saved model
over the fit's own domain (``match_prior_dz``, smooth_fit's ``prior_args``) and the overlapping
edges of neighbouring tiles (``match_tile_edges``, ``prior_edge_args``).

A prior row is interp_dz(y, x, t) − interp_dz(y, x, t_ref) with expected value sigma_scale·sigma_dz
and prior dz: neither an interpolation row nor a stencil row.  ``make_prior_op`` marks its operator
with a part of kind 'extra', so ``assemble.describe(..., extra_rows=True)`` still describes the
other rows and ``FitSystem`` hands these to the device as extra rows (lsq_set_extra_rows).

The grids come in memory (``containers.GridData`` with x, y, t or time, dz, sigma_dz; dz of shape
(y, x, t)); reading h5 files is outside lssurf_amd, as mask files are.

Selections compare floating-point sums with thresholds, so every sum here keeps the operand order
of the reference's expression: a point on a threshold falls on the same side in both.
"""
import re
import warnings

import numpy as np

from . import containers as pc
from .lin_op import lin_op

_AXES = ('x', 'y', 't', 'time')


def _t_of(dz):
    return np.asarray(dz.t if 't' in dz.fields else dz.time)


def grid_as_points(dz, skip_fields=('cell_area', 'mask')):
    """The nodes of a (y, x, t) grid container as points, raveled in (y, x, t) order, with every
    field of the grid's shape."""
    t = _t_of(dz)
    yy, xx, tt = np.meshgrid(np.asarray(dz.y), np.asarray(dz.x), t, indexing='ij')
    out = {'x': xx.ravel(), 'y': yy.ravel(), 't': tt.ravel()}
    for f in dz.fields:
        if f in _AXES or f in skip_fields:
            continue
        a = np.asarray(getattr(dz, f))
        if a.shape == yy.shape:
            out[f] = a.ravel()
    return pc.data().from_dict(out)


def make_prior_op(grids, dz, src_name, ref_time=0, sigma_scale=1):
    """One row per point of dz (x, y, t or time, dz, sigma_dz) that is not at ref_time: the dz
    model at (y, x, t) minus the dz model at (y, x, ref_time), expected sigma_scale·sigma_dz,
    prior dz.  The triplets are the interpolation at t followed by the negated interpolation at
    ref_time, which is the order their duplicates are summed in.  dz itself is left as it is."""
    t = _t_of(dz)
    live = t != ref_time
    y, x, t = (np.asarray(a)[live] for a in (dz.y, dz.x, t))
    g = grids['dz']
    op = lin_op(g, name='prior_dz1_' + src_name).interp_mtx((y, x, t))
    at_ref = lin_op(g, name='prior_dz0_' + src_name).interp_mtx((y, x, np.full(t.shape, ref_time, dtype=float)))
    op.add(at_ref.scale_values(-1.))
    op.expected = sigma_scale * np.asarray(dz.sigma_dz)[live]
    op.prior = np.asarray(dz.dz)[live]
    op.parts = [dict(kind='extra', row0=0, n_eq=int(op.N_eq))]
    return op


def _window(axis, fit_bds, pad, skip):
    """Indices of a saved grid's axis that a prior uses: inside both the fit's bounds and the
    axis's own span (its mean ± half its length, drawn in by pad), then from int(skip / 2) on
    (match_priors.py:85-100; the reference's skip sets the first index only, and so does this)."""
    axis = np.asarray(axis)
    half = (axis[-1] - axis[0]) / 2 - pad
    mid = np.mean(axis)
    lo, hi = np.maximum(fit_bds[0], mid - half), np.minimum(fit_bds[1], mid + half)
    return np.flatnonzero((axis >= lo) & (axis <= hi))[int(skip / 2):]


def match_prior_dz(grids, dzs=None, filenames=None, ref_epoch=0, group='dz', field_mapping=None,
                   skip=None, edge_pad=None, sigma_scale=1, sigma_max=None):
    """One prior operator per saved dz grid in dzs (match_priors.py:46-106).  edge_pad['t'] is
    accepted and not used, as in the reference."""
    if filenames:
        raise NotImplementedError('match_prior_dz: reading h5 files is outside lssurf_amd; pass the grids as dzs=')
    skip = dict({'xy': 1, 't': 1}, **(skip or {}))
    pad_xy = (edge_pad or {}).get('xy', 0)
    fit_bds = grids['dz'].bds
    ops = []
    for saved in (dzs or []):
        if saved is None:
            continue
        t = _t_of(saved)
        iy = _window(saved.y, fit_bds[0], pad_xy, skip['xy'])
        ix = _window(saved.x, fit_bds[1], pad_xy, skip['xy'])
        it = _window(t, fit_bds[2], 0, skip['t'])
        part = {'x': np.asarray(saved.x)[ix], 'y': np.asarray(saved.y)[iy], 't': t[it]}
        for f in saved.fields:
            a = np.asarray(getattr(saved, f))
            if f not in _AXES and a.ndim == 3:
                part[f] = a[np.ix_(iy, ix, it)]
        pts = grid_as_points(pc.grid.data().from_dict(part))
        ops.append(make_prior_op(grids, pts, 'internal_prior', ref_time=t[ref_epoch], sigma_scale=sigma_scale))
    return ops


_TILE_NAME = re.compile(r'E(-?\d+)_N(-?\d+)')


def _tile_centre(name):
    """(x, y) in metres of a tile named E{x_km}_N{y_km} (a trailing .h5 is allowed), or None."""
    found = _TILE_NAME.fullmatch(name[:-3] if name.endswith('.h5') else name)
    return None if found is None else tuple(1000. * int(km) for km in found.groups())


def _edge_strips(x, y, here, there, half, overlap, edge_include):
    """The points of a neighbour (centre there) that constrain the tile centred on here (half-width
    half): inside the tile, within edge_include of one of its edges, and closer than half − overlap
    to the neighbour's centre in x and in y (match_priors.py:197-207; the same sums, so the same
    points)."""
    near_edge = np.zeros(np.shape(x), dtype=bool)
    inside = np.ones(np.shape(x), dtype=bool)
    for c, c0, cn in ((x, here[0], there[0]), (y, here[1], there[1])):
        near_edge |= (c > c0 + half - edge_include) | (c < c0 - half + edge_include)
        inside &= (c >= c0 - half) & (c <= c0 + half) & (np.abs(c - cn) < half - overlap)
    return near_edge & inside


def match_tile_edges(grids, ref_epoch, prior_dir=None, tiles=None, tile_spacing=4.e4, edge_include=3.e3,
                     group='dz', field_mapping=None, sigma_scale=1, sigma_max=None, verbose=False):
    """Operators that match the current tile to its neighbours (match_priors.py:109-224).
    tiles: {'E{x_km}_N{y_km}': grid container}.  Returns the operators and, per tile that gave one,
    the distinct (x, y) of its constraining points, sorted by x and then y."""
    if prior_dir is not None:
        raise NotImplementedError('match_tile_edges: reading tile files (prior_dir) is outside lssurf_amd; '
                                  'pass the tiles as tiles={name: grid}')
    z0, dz_grid = grids['z0'], grids['dz']
    here = (np.mean(z0.bds[1]), np.mean(z0.bds[0]))    # bds are (y, x): the centre as (x, y)
    width = z0.bds[0][1] - z0.bds[0][0]                # the tile is square
    half = width / 2
    overlap = (width - tile_spacing) / 2               # what two adjacent tiles share, per side
    ops, where = [], {}
    for name, tile in (tiles or {}).items():
        there = _tile_centre(name)
        if there is None:
            warnings.warn(f'match_tile_edges: {name!r} is no E{{x_km}}_N{{y_km}} tile name; skipped')
            continue
        apart = max(abs(here[0] - there[0]), abs(here[1] - there[1]))
        if apart == 0 or apart > tile_spacing + edge_include:    # the tile itself, or no neighbour
            continue
        if 'sigma_dz' not in tile.fields:
            warnings.warn(f'match_tile_edges: tile {name!r} has no sigma_dz; skipped')
            continue
        pts = grid_as_points(tile)
        use = _edge_strips(pts.x, pts.y, here, there, half, overlap, edge_include)
        use &= z0.validate_pts((pts.y, pts.x)) & dz_grid.validate_pts((pts.y, pts.x, pts.t))
        if not use.any():
            continue
        ops.append(make_prior_op(grids, pts[use], name, ref_time=_t_of(tile)[ref_epoch], sigma_scale=sigma_scale))
        xy = np.unique(np.c_[pts.x[use], pts.y[use]], axis=0)
        where[name] = (xy[:, 0], xy[:, 1])
        if verbose:
            print(f'match_tile_edges: {name}: {ops[-1].N_eq} rows, sigma_scale={sigma_scale}')
    return ops, where
