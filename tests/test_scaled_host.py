"""Masked and mapped constraint scales on the host (tests/scaled_host.py): the inputs of
tests/test_gpu_cg_scaled.py, pinned without a device.

  1. Ec of every system equals tests/golden/ec_scaled.npz bit for bit: the `expected` of the reference's
     setup_smoothness_constraints on the same masks and maps (tests/golden/gen_golden_ec_scaled.py), so the
     row scales the device tests hand to lsq_set_row_weight are the reference's.
  2. smooth_fit(constraint_scaling_maps=…, return_fit_objects=True) forms a structured system (it raised
     NotImplementedError before), the key 'dz' still raises, and the maps' handling is the reference's:
     a containers.GridData is interpolated to the nodes, non-finite entries become 1, keys with 'z0' go on
     the z0 lattice.
  3. lsq_cg_scaled is validated: anything but a bool raises ValueError.
  4. The restatement of the scaled normal (part descriptors + squared-scale fields) equals Aᵀ(A p) of the
     host-formed A to 1e-13 of max |AᵀA p| (both are exact sums of the same products in another order: the
     error is a few ulp, measured 5e-16), with 20 % of the data rows masked, and the fields are what the
     device builds: one scale per (y, x) node, the expected parts non-uniform.
  5. The exact solutions the GPU solves are compared with satisfy oracle.dense.optimality < 1e-13."""
import numpy as np
import pytest

import conftest  # noqa: F401
import scaled_host as SH
import lssurf_amd as LS
from lssurf_amd import containers as pc
from lssurf_amd.assemble import describe
from oracle.dense import optimality

NAMES = list(SH.SYSTEMS)
OPS = ('grad2_z0', 'grad_z0', 'grad2_dzdt', 'grad_dzdt', 'd2z_dt2')


@pytest.mark.parametrize('name', NAMES)
def test_ec_matches_reference(name):
    g = conftest.golden('ec_scaled.npz')
    (ny, nx, nt), _, _, kind, keys = SH.SYSTEMS[name]
    assert tuple(g[f'{name}__shape']) == (ny, nx, nt)
    mask = SH.mask_of(kind, ny, nx)
    assert (f'{name}__mask' in g.files) == (mask is not None)
    if mask is not None:
        np.testing.assert_array_equal(g[f'{name}__mask'], mask)
    maps = SH.maps_of(keys, name, ny, nx) or {}
    assert sorted(k.split('__map__')[1] for k in g.files if k.startswith(f'{name}__map__')) == sorted(maps)
    for key, m in maps.items():
        np.testing.assert_array_equal(g[f'{name}__map__{key}'], m)
    h = SH.host(name)
    rows = h.S['Gc'].TOC['rows']
    Ec = h.S['Ec']
    assert sorted(k.split('__ec__')[1] for k in g.files if k.startswith(f'{name}__ec__')) == sorted(OPS)
    for op in OPS:
        np.testing.assert_array_equal(Ec[rows[op]], g[f'{name}__ec__{op}'], err_msg=f'{name} {op}')
    # the scales are not uniform where the test needs them not to be
    assert all(np.unique(Ec[rows[op]]).size > 1 for op in ('grad2_dzdt', 'grad_dzdt')) or 'd2z0_dx2' in maps


def test_disc_mask_scales_of_the_issue():
    """t64 with a disc mask: Ec takes two values on the dz constraints, a factor mask_scale[0] = 10 apart"""
    from lssurf_amd import synthetic
    D, kw = synthetic.points('t64')
    yy, xx = np.meshgrid(np.arange(64), np.arange(64), indexing='ij')
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False,
                      mask_data=(yy - 32) ** 2 + (xx - 32) ** 2 > 15 ** 2, **kw)
    rows = S['Gc'].TOC['rows']
    for op in ('grad2_dzdt', 'grad_dzdt'):
        u = np.unique(S['Ec'][rows[op]])
        assert u.size == 2 and u[1] == 10 * u[0], (op, u)
    assert describe(S['G_data'], S['Gc'], with_fields=True) is not None


def test_constraint_scaling_maps_form_a_structured_system():
    name = 'mask-maps'
    D, kw = SH.points(name)
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    d = describe(S['G_data'], S['Gc'], with_fields=True)
    assert d is not None and not d[5] and len(d[3]) == 11   # structured, no field-valued parts
    # the maps reached the constraints: against the same fit without them
    S0 = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False,
                       **{k: v for k, v in kw.items() if k != 'constraint_scaling_maps'})
    rows = S['Gc'].TOC['rows']
    assert not np.array_equal(S['Ec'][rows['grad2_dzdt']], S0['Ec'][rows['grad2_dzdt']])
    assert not np.array_equal(S['Ec'][rows['grad_z0']], S0['Ec'][rows['grad_z0']])
    np.testing.assert_array_equal(S['Ec'][rows['d2z_dt2']], S0['Ec'][rows['d2z_dt2']])


def test_constraint_scaling_maps_handling():
    D, kw = SH.points('maps-dz')
    kw = {k: v for k, v in kw.items() if k != 'constraint_scaling_maps'}
    S0 = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    gz, gd = S0['grids']['z0'], S0['grids']['dz']
    rng = np.random.default_rng(3)
    arr = rng.uniform(0.5, 2., tuple(gd.shape[:2]))
    arr[2, 5] = np.nan
    arr[4, 1] = np.inf
    fixed = np.where(np.isfinite(arr), arr, 1.)
    rows = S0['Gc'].TOC['rows']
    # an array with non-finite entries == the array with 1 there
    Sa = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, constraint_scaling_maps={'d2z_dt2': arr}, **kw)
    Sb = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, constraint_scaling_maps={'d2z_dt2': fixed}, **kw)
    np.testing.assert_array_equal(Sa['Ec'], Sb['Ec'])
    assert np.unique(Sa['Ec'][rows['d2z_dt2']]).size > 1
    np.testing.assert_array_equal(Sa['Ec'][rows['grad_dzdt']], S0['Ec'][rows['grad_dzdt']])
    # a GridData on the nodes themselves interpolates to its own values; a key with 'z0' goes on the z0 lattice
    G = pc.GridData().from_dict({'x': gz.ctrs[1], 'y': gz.ctrs[0], 'z': fixed})
    Sg = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, constraint_scaling_maps={'dz0_dx': G}, **kw)
    Sh = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, constraint_scaling_maps={'dz0_dx': fixed}, **kw)
    np.testing.assert_allclose(Sg['Ec'], Sh['Ec'], rtol=1e-14, atol=0)
    assert np.unique(Sg['Ec'][rows['grad_z0']]).size > 1
    np.testing.assert_array_equal(Sg['Ec'][rows['grad2_z0']], S0['Ec'][rows['grad2_z0']])   # dz0_dx scales grad_z0 alone
    with pytest.raises(NotImplementedError, match='dz_zero'):
        LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, constraint_scaling_maps={'dz': fixed}, **kw)
    with pytest.raises(ValueError, match='shape'):
        LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, constraint_scaling_maps={'d2z_dt2': fixed[1:]},
                      **kw)
    with pytest.raises(ValueError, match='dict'):
        LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, constraint_scaling_maps=[fixed], **kw)


@pytest.mark.parametrize('bad', [1, 0, 'yes', None, 1.0])
def test_key_validation(bad):
    D, kw = SH.points('maps-z0')
    with pytest.raises(ValueError, match='lsq_cg_scaled'):
        LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, lsq_cg_scaled=bad, **kw)


def test_key_default_is_off():
    from lssurf_amd.smooth_fit import DEFAULTS, OUT_OF_SCOPE
    assert DEFAULTS['lsq_cg_scaled'] is False and 'constraint_scaling_maps' not in OUT_OF_SCOPE


@pytest.mark.parametrize('name', NAMES)
def test_restatement_matches_formed_normal(name):
    h = SH.host(name)
    mask = SH.data_mask(h)
    fields = SH.part_fields(h, h.w)
    assert sum(not u for _, u in fields) == SH.SCALED_PARTS[name]
    A = h.A(h.w, mask)
    rng = np.random.default_rng(17)
    for _ in range(2):
        p = rng.standard_normal(h.keep_cols.size)
        q = A.T @ (A @ p)
        err = float(np.max(np.abs(SH.scaled_normal(h, h.w, mask, p) - q)) / np.max(np.abs(q)))
        print(name, 'restatement error', err)
        assert err <= 1e-13


@pytest.mark.parametrize('name', NAMES)
def test_exact_solutions_are_optimal(name):
    A, b, x = SH.exact(name)
    assert A.shape[1] == SH.host(name).keep_cols.size
    opt = optimality(A, b, x)
    print(name, A.shape, 'optimality', opt)
    assert opt < 1e-13


def test_iterate_case_is_clear_of_bf16_rounding_boundaries():
    """tests/test_cgnr_host.py's condition on the input of test_gpu_cg_scaled.py::test_iterates: no entry of
    the node-block factors lies where the device's R_b⁻¹ could round to another bf16 value"""
    import cgnr_host as H
    h = SH.host('edges')
    blocks = H.block_list(*h.blocks, h.keep_cols.size)
    ent = H.factor_entries(H.block_factors(h.A(), blocks, round=False))
    assert H.at_risk_entries(ent) == 0
    assert H.at_risk_entries(ent, eps=1e-3) > 0
