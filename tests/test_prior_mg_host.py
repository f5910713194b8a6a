"""Host side of the priors inside the multigrid preconditioner: the solver key lsq_prior_mg, and the
classification and level-1 transpose of csrc/xr_lump.hpp against tests/mg_host.py's lumping
(tools/xr_lump_check.py: a stand-alone host program around the header, no GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lssurf_amd as LS
from lssurf_amd import synthetic
from lssurf_amd.smooth_fit import DEFAULTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('bad', [1, 0, 'yes', None, [True]])
def test_lsq_prior_mg_must_be_a_bool(bad):
    D, kw = synthetic.points('t15')
    with pytest.raises(ValueError, match='lsq_prior_mg'):
        LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, lsq_prior_mg=bad, **kw)


def test_lsq_prior_mg_defaults_off_and_does_nothing_without_priors():
    assert DEFAULTS['lsq_prior_mg'] is False
    assert DEFAULTS['lsq_precond'] == 'auto' and DEFAULTS['prior_args'] is None and DEFAULTS['prior_edge_args'] is None
    out = []
    for extra in ({}, {'lsq_prior_mg': False}, {'lsq_prior_mg': True}):
        D, kw = synthetic.points('t15')
        out.append(LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **extra, **kw))
    for S in out[1:]:
        assert S.keys() == out[0].keys() and S['prior_ops'] == []
        assert np.array_equal(S['rhs'], out[0]['rhs']) and np.array_equal(S['Ec'], out[0]['Ec'])
        for a, b in zip(S['Gc'].triplets(), out[0]['Gc'].triplets()):
            assert np.array_equal(a, b)


def test_lumping_tables_match_the_host_hierarchy():
    """rows (a), (b), (c) of test_gpu_mg_priors.py on t64 and t15: the blocks summed from the tables
    equal mg_host's lumping of Pᵀ XᵀW²X P to 1e-13 (f64 sums of ≤ 10⁴ terms), and rows over
    non-adjacent epochs are refused by name"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'xr_lump_check.py')], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'xr_lump_check: ok' in r.stdout
