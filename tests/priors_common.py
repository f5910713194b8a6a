"""Shared by test_priors_host.py and test_gpu_priors.py: the saved dz grids and smooth_fit keywords
of tests/golden/sys_prior_edge.npz and sys_prior_dz.npz (gen_golden_prior.py)."""
import numpy as np

from conftest import golden_kwargs
from lssurf_amd import containers as pc


def golden_tiles(g):
    """{tile name: grid container} of the fixture's saved dz grids"""
    out = {}
    for name in g['tile_names']:
        name = str(name)
        out[name] = pc.grid.data().from_dict({f: g[f'tile_{name}_{f}'] for f in ('x', 'y', 't', 'dz', 'sigma_dz')})
    return out


def prior_kwargs(g):
    """the fixture's smooth_fit keywords with the in-memory grids put back"""
    kw = golden_kwargs(g)
    if 'prior_edge_args' in kw:
        kw['prior_edge_args'] = dict(kw['prior_edge_args'], tiles=golden_tiles(g))
    if 'prior_args' in kw:
        kw['prior_args'] = dict(kw['prior_args'], dzs=[golden_tiles(g)['prior']])
    return kw


def prior_rows(g):
    """(A_prior, b_prior): the last n_prior rows of the reference's weighted, column-reduced system"""
    from conftest import golden_csr
    n = int(g['n_prior'])
    A = golden_csr(g)
    return A[A.shape[0] - n:], np.asarray(g['b'])[-n:]
