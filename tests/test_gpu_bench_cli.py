"""bench.py's command line on a small config (t64): a plain run times exactly --steps iterations
and reports nothing that needs runs of its own; --dump-outputs writes the statistics the timed
call returned, reproducibly; --full adds the solves and the per-kernel roofline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

STEPS, WARMUP = 7, 3
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--config', 't64',
           '--steps', str(STEPS), '--warmup', str(WARMUP), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines   # one JSON result line
    return json.loads(lines[0])


@pytest.fixture(scope='module')
def plain(gpu_available, tmp_path_factory):
    d = tmp_path_factory.mktemp('dump')
    return _bench('--dump-outputs', str(d)), np.load(d / 'iterate_stats.npy')


def test_plain_run_result_line(plain):
    out, _ = plain
    assert all(k in out for k in HEADLINE)
    assert out['steps'] == STEPS and out['warmup'] == WARMUP and out['full'] is False
    assert out['higher_is_better'] is True and out['dtype'] == 'f64'
    assert out['ms_per_step'] > 0 and out['value'] == pytest.approx(1e3 / out['ms_per_step'], rel=1e-12)
    # nothing that takes a run of its own
    assert out['roofline'] is None and out['cpu_baseline'] is None
    assert not [k for k in out if k.startswith('solve_')]


def test_dump_is_what_the_timed_call_returned(plain, gpu_available):
    """The dump of a child run equals, field by field, the statistics lsq_iterate returns in this
    process after the same warm-up and timed calls on the same seeded system: the iteration count
    exactly, the norms to 1e-9 (the device reductions' summation order is not fixed)."""
    import bench
    _, dump = plain
    assert dump.dtype == np.float64 and dump.shape == (len(bench.DUMP_FIELDS),) and np.all(np.isfinite(dump))
    d = dict(zip(bench.DUMP_FIELDS, dump))
    assert d['iters'] == STEPS + WARMUP   # --steps sets the number of timed steps
    assert d['method'] == 1 and d['xnorm'] > 0 and d['r1norm'] > 0
    fs, rhs, _, _ = bench.build_system('t64', 0)
    try:
        fs.solver.iterate(rhs, WARMUP, precond=3, method=1)
        st = fs.solver.iterate(rhs, STEPS, precond=3, method=1)
    finally:
        fs.close()
    np.testing.assert_allclose(dump, [float(st[k]) for k in bench.DUMP_FIELDS], rtol=1e-9, atol=0)


def test_full_run_adds_solve_and_roofline(plain, tmp_path):
    _, dump = plain
    out = _bench('--full', '--no-pmc', '--no-cpu', '--dump-outputs', str(tmp_path))
    assert out['full'] is True and all(k in out for k in HEADLINE)
    assert out['roofline']['kernel_ms'] and out['roofline']['frac'] > 0
    assert out['solve_istop'] in (1, 2) and out['solve_iters'] > 0 and out['solve_lsqr']['solve_iters'] > 0
    # the extra work runs after the timed steps: the same outputs as the plain run
    np.testing.assert_allclose(np.load(tmp_path / 'iterate_stats.npy'), dump, rtol=1e-9, atol=0)
