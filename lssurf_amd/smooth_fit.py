"""smooth_fit — the drop-in driver, with the least-squares solve on an MI355X.

Call surface and return value follow LSsurf/smooth_fit.py:354-717 (``smooth_fit(**kwargs)``:
required data, W, ctr, spacing, E_RMS; defaults of :356-401; returns m, E, data, grids,
valid_data, TOC, R, RMS, timing, E_RMS, dzdt_lags; ``return_fit_objects`` early return of
:639-645).  What changes is underneath:

* system formation (smooth_fit.py:588-627) builds the same lin_ops on the host, but the
  weighted, column-reduced matrix ``Ip_r·TCinv·[G_data; Gc]·Ip_c`` is formed ON THE DEVICE
  once (``FitSystem``); outer iterations only re-weight and re-mask rows;
* ``sparseqr.solve`` (:142) becomes device LSQR with a warm start from the previous outer
  iteration; the residual ``G_data·m0`` (:146, :662) is a device SpMV;
* everything else (editing, sigma_extra, convergence tests, parse_model) keeps the reference's
  logic on the host.

Options that add columns/rows outside the fd_grid model (sensor grids, jitter, lagrangian grids)
are outside lssurf_amd's scope and raise NotImplementedError instead of silently changing the fit.
The dz priors (prior_args, prior_edge_args; match_priors.py) take in-memory grids; their rows stay
last in Gc and the device carries them as extra rows inside matrix-free CGNR (lsq_set_extra_rows).
With priors compute_E, n_gpus > 1 and lsq_bias='eliminate' raise NotImplementedError.
lsq_prior_mg=True lets the multigrid preconditioner (precond 4) carry them, lumped into its coarse levels.
Slope biases (data_slope_sensors) go with the data biases: they need bias_params and lsq_bias.
Sensor bias grids (sensor_grid_bias_params; setup_sensor_grid_bias.py) run under the same key lsq_bias:
'eliminate' (one dense block per grid eliminated inside CGNR, lsq_set_sensor_grids; not together with
bias_params, data_slope_sensors or priors), 'columns' or 'auto'.  lsq_sgrid_joint=True lets 'eliminate'
and 'auto' run the grids beside bias_params and data_slope_sensors (lsq_set_sensor_grids_joint: every
bias ID and slope group inside one grid's sensor or outside every grid); priors stay refused.
Data biases (bias_params) run when the solver key lsq_bias says how: 'eliminate' (the device
eliminates them inside CGNR, lsq_set_data_bias), 'columns' (ordinary columns of a generic system)
or 'auto' (with priors: 'columns', with a warning where it would have eliminated).
compute_E with bias_params (and data_slope_sensors) runs when lsq_E_border=True: the bias columns are
the dense border of a bordered band factor (lsq_cov_band_bordered) and E gains sigma_bias /
sigma_slope_bias; without the key it raises NotImplementedError, as do lsq_E_method='window', sensor
bias grids, priors and n_gpus > 1 with it.  lsq_E_border_solve=True (with lsq_E_border=True) lets
lsq_E_method='window', and 'auto' above errors.WINDOW_MIN_COLS columns, run with the biases: tiled
windows on the grid-only system plus one CGNR solve per bias column (lsq_cov_border_solved,
errors.calc_and_parse_errors); 'band' and 'dense' are unchanged, and sensor bias grids, priors and
n_gpus > 1 stay refused.
lsq_tile_eliminate=True lets lsq_bias='eliminate' (and 'auto') run on dz grids of 16 to 19 epochs, and
together with lsq_cg_chunks=True of 20 to 64: tile and chunk mode then take matrix-free data rows
(lsq_set_cg_tile_dmf) and eliminate biases, slopes and sensor grids as below 16 epochs, with block-Jacobi;
timing['tile_eliminate'] says whether the last solve ran so.  Still refused with the key: the multigrid,
priors beside 'eliminate', n_gpus > 1, more than 64 epochs, 20 or more epochs without lsq_cg_chunks; the
compute_E rules above are unchanged.
constraint_scaling_maps (a dict: constraint key -> containers.GridData or an array on the grid's (y, x)
nodes) scales the constraints' expected values as the reference does; the key 'dz' raises
NotImplementedError.  A non-uniform mask or such maps give the constraint rows one row scale per node, and
the device then has no class-table CGNR operator: method 1 falls back to LSQR, and lsq_bias='eliminate',
sensor grids and priors are refused or take the triplet path.  lsq_cg_scaled=True keeps such fits on
matrix-free CGNR with block-Jacobi (lsq_set_cg_scaled; below 16 epochs, one GPU); lsq_precond=4 then raises
with the device's reason and 'auto' takes block-Jacobi; timing['cg_scaled'] says whether the last solve
ran so.
"""
from time import ctime, time

import warnings
import numpy as np

from . import containers as pc
from .data_slope_bias import RESCALE as SLOPE_RESCALE, data_slope_bias, slope_columns
from .bias_functions import assign_bias_ID, bias_expected, edit_by_bias, parse_biases, setup_bias_fit
from .calc_sigma_extra import RDE, calc_sigma_extra, calc_sigma_extra_on_grid
from .constraint_functions import build_reference_epoch_matrix, node_column_blocks, \
    node_column_blocks_affine, reference_epoch_keep_cols, \
    setup_smoothness_constraints
from .grid_functions import setup_averaging_ops, setup_avg_mask_ops, setup_grids, setup_z0_avg, \
    validate_by_dz_mask
from .lin_op import known_range, lin_op, toc_range
from ._native import NativeError
from .assemble import describe, extra_rows_of
from .match_priors import match_prior_dz, match_tile_edges
from .setup_sensor_grid_bias import check_sensor_grid_params, parse_sensor_bias_grids, \
    sensor_grid_device_form, setup_sensor_grid_bias
from .solver import LSQSolver

DEFAULTS = {'reference_epoch': 0, 'W_ctr': 1e4, 'return_fit_objects': False, 'mask_file': None,
            'mask_data': None, 'mask_update_function': None, 'mask_scale': {0: 10, 1: 1}, 'compute_E': False,
            'max_iterations': 10, 'min_iterations': 2, 'sigma_extra_relax': False,
            'sigma_extra_bin_spacing': None, 'sigma_extra_max': None, 'sigma_extra_keys': None,
            'srs_proj4': None, 'N_subset': None, 'bias_params': None, 'bias_filter': None, 'repeat_res': None,
            'converge_tol_dz': 0.05, 'converge_tol_frac_TSE': 0., 'DEM_tol': None, 'repeat_dt': 1,
            'Edit_only': False, 'dzdt_lags': None, 'prior_args': None, 'prior_edge_args': None,
            'avg_scales': [], 'data_slope_sensors': None, 'E_slope_bias': 0.01, 'E_RMS_d2x_PS_bias': None,
            'E_RMS_PS_bias': None, 'constraint_scaling_maps': None, 'error_res_scale': None, 'avg_masks': None,
            'sigma_extra_masks': None, 'bias_nsigma_edit': None, 'bias_nsigma_iteration': 2,
            'bias_edit_vals': None, 'sensor_grid_bias_params': None, 'ancillary_data': None,
            'lagrangian_coords': None, 'z0_average_scale': None, 'erode_source_mask': True, 'VERBOSE': True,
            'DEBUG': False,
            # lssurf_amd solver options (new keys; defaults reproduce the exact LS solution to
            # the tolerance documented in DESIGN.md §Parity)
            'device': 0, 'lsq_atol': 1e-12, 'lsq_btol': 1e-12, 'lsq_conlim': 1e12, 'lsq_maxit': 0,
            'lsq_precond': 'auto', 'lsq_dense_max': 16384, 'lsq_warm_start': True, 'lsq_method': 'auto',
            'lsq_reuse_anorm': True, 'lsq_E_method': 'auto', 'n_gpus': 1, 'devices': None,
            # data biases (bias_params): None refuses them; 'eliminate', 'columns' or 'auto'
            'lsq_bias': None,
            # priors (prior_args / prior_edge_args) inside the multigrid preconditioner: their rows
            # lumped into its coarse levels (opt-in; without priors the key does nothing)
            'lsq_prior_mg': False, 'lsq_E_border': False,
            # compute_E with biases at window scale: the border by CGNR solves (acts with lsq_E_border only)
            'lsq_E_border_solve': False,
            # sensor bias grids beside bias_params / data_slope_sensors eliminated jointly (opt-in; the
            # bias IDs and slope groups must nest in the grids' sensors, as with 'sensor' in bias_params)
            'lsq_sgrid_joint': False,
            # CGNR on dz grids of 20 to 64 epochs: the normal operator's tiles cut along time too (chunk
            # mode) instead of method 1 falling back to LSQR (opt-in; below 20 epochs the key does nothing)
            'lsq_cg_chunks': False,
            # eliminated biases, slopes and sensor grids on dz grids of 16 to 64 epochs: tile and chunk mode
            # on matrix-free data rows (opt-in; 20 and more epochs need lsq_cg_chunks too; below 16 epochs the
            # key does nothing).  Still refused there: multigrid, priors beside 'eliminate', n_gpus > 1, more
            # than 64 epochs; the compute_E rules are unchanged
            'lsq_tile_eliminate': False,
            # masked fits and constraint_scaling_maps inside matrix-free CGNR: constraint rows with one row
            # scale per (y, x) node are applied by their own kernel instead of method 1 falling back to LSQR
            # (opt-in; below 16 epochs, one GPU, block-Jacobi: the multigrid stays refused; without a
            # non-uniform mask or maps the key does nothing)
            'lsq_cg_scaled': False}

OUT_OF_SCOPE = ('lagrangian_coords', 'mask_file', 'bias_edit_vals')


class FitSystem:
    """The device-resident smooth_fit system: G = [G_data; Gc] (unweighted COO -> device CSR),
    Ip_c as a column map; rows re-weighted / re-selected per outer iteration."""

    def __init__(self, G_data, Gc, keep_cols, n_full, device=0, structured=True, grids=None, bias=None,
                 extra_ops=None, extra_csr=None, extra_mg=False, sensor_grids=None, joint=False, iterative=True,
                 cg_chunks=False, tile_dmf=False, cg_scaled=False):
        """cg_scaled: per-row constraint scales inside CGNR (LSQSolver.set_cg_scaled): with row weights that
        give a stencil part one scale per (y, x) node (a mask with mask_scale, constraint_scaling_maps)
        method 1 stays CGNR with block-Jacobi, and eliminated biases, sensor grids and extra rows run as on
        unmasked fits.  Column mode (fewer than 16 epochs) only; precond 4 is refused with the device's reason.
        tile_dmf: tile and chunk mode on matrix-free data rows (LSQSolver.set_cg_tile_dmf), set before the
        formation: with a dz grid of 16 to 19 epochs, or of 20 to 64 beside cg_chunks, bias and sensor_grids
        are then eliminated as below 16 epochs and this constructor's cg_available question passes.
        Multigrid stays refused there, extra rows take the COO path, and 20 or more epochs without
        cg_chunks, or more than 64, still have no CGNR operator.
        cg_chunks: CGNR's chunk mode (LSQSolver.set_cg_chunks), set before the formation: a dz grid of
        20 to 64 epochs then runs method 1 as CGNR instead of falling back to LSQR.  What tile mode
        refuses stays refused: no multigrid, no eliminated bias / sensor_grids (this constructor raises),
        extra rows take the COO path.
        sensor_grids: the dict of setup_sensor_grid_bias.sensor_grid_device_form — eliminated sensor
        bias grids (LSQSolver.set_sensor_grids), together with bias only when joint=True
        (lsq_set_sensor_grids_joint: every bias ID and slope group inside one grid's rows or outside
        every grid; expand() then lays the columns out as the reference does: the biases, the slopes,
        the sensor grids).  G_data and Gc are the
        operators without the grids' columns and constraint rows, the caller's row weights and rhs may
        carry the grids' constraint rows behind them, and the grids take the columns after n_full in
        expand().  A grid's uniform magnitude prior (shift) never reaches the device: the rhs of the
        grid's rows loses it and the returned grid gains it (a row's weights sum to 1 and grad2 of a
        constant is 0, so this is exact).
        bias = (ids, c): eliminated data biases (LSQSolver.set_data_bias) — G_data and Gc are then
        the grid-only operators, the caller's row weights and rhs may carry further (bias
        constraint) rows behind them, and the biases take the columns after n_full in expand().
        bias = (ids, c, (group, u, c_slope)): slope biases too (LSQSolver.set_data_slope): group per
        data row (−1: none), u (rows, 2), c_slope (groups, 2); their values follow the biases in
        expand(), and their constraint rows follow the bias constraint rows on the host.
        extra_ops: the operators behind Gc's last rows that are neither interpolation nor stencil
        rows (the priors of match_priors).  With a structured description of the other rows they
        are staged as the device's extra rows (LSQSolver.set_extra_rows) and matrix-free CGNR
        carries them; if the device refuses, the whole system takes the COO path.
        extra_csr = (indptr, cols_full, vals): extra rows that are not in Gc at all, behind its last
        row (the row weights, mask and rhs of solve() then have n_data + Gc.N_eq + their count
        entries); they need the structured formation.
        extra_mg: ask the device to lump the extra rows into the multigrid's coarse levels
        (LSQSolver.set_extra_rows(lump=True)), so that precond 4 may carry them; where the device
        refuses (e.g. a row over non-adjacent epochs) multigrid_available warns with its reason and
        the system stays on block-Jacobi.
        iterative: False when every solve will be LSQR with precond 2 or 5; extra rows that CGNR cannot
        carry then stay on the stencil-formed system instead of taking the COO path.  With
        iterative=True a system with extra rows, and any system with bias or sensor_grids, asks
        cg_available(1) here: the column norms and the CGNR operator's description are built at
        construction (smooth_fit's timing['device_setup']) and not at the first solve."""
        self.n_data, self.n_con = int(G_data.N_eq), int(Gc.N_eq)
        self.keep_cols = keep_cols
        self.n_full = int(n_full)
        self.solver = LSQSolver(device)
        self.cg_chunks = bool(cg_chunks)
        if self.cg_chunks:
            self.solver.set_cg_chunks(True)
        self.tile_dmf = bool(tile_dmf)
        if self.tile_dmf:
            self.solver.set_cg_tile_dmf(True)
        if not isinstance(cg_scaled, (bool, np.bool_)):
            self.solver.close()
            raise ValueError(f'FitSystem: cg_scaled must be True or False, not {cg_scaled!r}')
        self.cg_scaled = bool(cg_scaled)
        if self.cg_scaled:
            self.solver.set_cg_scaled(True)
        self.solver.set_col_map(self.n_full, keep_cols)
        m = self.n_data + self.n_con
        extra_ops = list(extra_ops or [])
        n_extra = sum(int(op.N_eq) for op in extra_ops)
        if n_extra and extra_rows_of(Gc) != n_extra:
            raise ValueError('FitSystem: extra_ops must be the last rows of Gc')
        if extra_csr is not None:
            if n_extra or not structured:
                raise ValueError('FitSystem: extra_csr goes with the structured formation and without extra_ops')
            n_extra = int(np.size(extra_csr[0])) - 1
            self.n_con += n_extra  # constraint rows as solve() counts them
            m += n_extra
        desc = describe(G_data, Gc, with_fields=True, extra_rows=n_extra > 0) if structured else None
        if extra_csr is not None and desc is None:
            raise ValueError('FitSystem: extra_csr needs a structured description of G_data and Gc')
        self.n_extra = 0           # rows the device holds as extra rows
        if desc is not None:       # rows generated on the device from the grids and stencils
            gdesc, interp, coords, stencils, npts, fields = desc
            # Only a refusal of the extra rows themselves leads to the COO path, and it says so: at staging
            # (e.g. > 32 entries in one row), at formation when the other rows did not come out
            # matrix-free ('extra rows need …'), or behind it when the formed system has no CGNR operator
            # that carries them (16 and more epochs: tile mode, or none at all).  There method 1, and LSQR
            # on the structured operator with precond 1 or 3, raise at every solve; only LSQR with the
            # dense or band preconditioner (2, 5) runs on the stencil-formed system, so a caller that
            # solves that way alone passes iterative=False and keeps it.  Any other formation error stays
            # an error.
            try:
                if n_extra:        # staged first: they become the last rows of the formation
                    self.solver.set_extra_rows(*(extra_csr if extra_csr is not None else _extra_rows_csr(extra_ops)),
                                               lump=bool(extra_mg))
                refusal = None
            except NativeError as e:
                if extra_csr is not None:
                    raise
                refusal = e
            if refusal is None:
                try:
                    self.solver.set_matrix_stencil(m, self.n_full, gdesc, interp, coords, stencils, npts,
                                                   fields=fields)
                    self.n_extra = n_extra
                except NativeError as e:
                    if not n_extra or extra_csr is not None or 'extra rows need' not in str(e):
                        raise
                    refusal = e
            if refusal is None and n_extra and iterative:
                ok, why = self.solver.cg_available(1)
                if not ok:
                    refusal, self.n_extra = why, 0
            if refusal is not None:
                warnings.warn(f'FitSystem: the device refuses the {n_extra} extra rows ({refusal}); the whole '
                              f'system is formed from triplets (COO) and has no matrix-free CGNR',
                              RuntimeWarning, stacklevel=2)
                self.solver.close()   # a fresh handle: nothing staged, nothing half formed
                self.solver = LSQSolver(device)
                if self.cg_chunks:
                    self.solver.set_cg_chunks(True)
                if self.tile_dmf:
                    self.solver.set_cg_tile_dmf(True)
                if self.cg_scaled:
                    self.solver.set_cg_scaled(True)
                self.solver.set_col_map(self.n_full, keep_cols)
                desc = None
        self.desc = desc           # the descriptors (bench.py's structured CPU baseline reads them)
        self.formation = 'stencil' if desc is not None else 'coo'
        if desc is None:           # generic lin_op: host triplets -> device CSR
            r1, c1, v1 = G_data.triplets()
            r2, c2, v2 = Gc.triplets()
            rr, cc, vv = [r1, r2 + self.n_data], [c1, c2], [v1, v2]
            if extra_csr is not None:   # refused above: the rows behind Gc's as triplets
                ip = np.asarray(extra_csr[0], np.int64)
                rr.append(self.n_data + int(Gc.N_eq) + np.repeat(np.arange(ip.size - 1), np.diff(ip)))
                cc.append(np.asarray(extra_csr[1], np.int64))
                vv.append(np.asarray(extra_csr[2], float))
            self.solver.set_matrix_coo(m, self.n_full, np.concatenate(rr), np.concatenate(cc), np.concatenate(vv))
        self.has_blocks = False
        self._grids, self._blocks = grids, None
        if grids is not None:      # per-node column blocks for the block-Jacobi preconditioner
            aff = node_column_blocks_affine(grids, keep_cols)
            if aff is not None:    # formed and checked on the device (no 10⁷-entry host lists)
                try:
                    self.solver.set_column_blocks_affine(*aff)
                    self.has_blocks = True
                except NativeError:
                    pass
            if not self.has_blocks:
                blocks = node_column_blocks(grids, keep_cols)
                if blocks is not None:
                    self.solver.set_column_blocks_csr(*blocks)
                    self.has_blocks = True
                    self._blocks = blocks
        # multigrid (precond 4) availability, probed on first use; with extra rows only when their
        # lumping was requested (extra_mg): otherwise the coarse levels would not carry their term, so
        # 'auto' takes block-Jacobi as with eliminated biases
        self.extra_mg = bool(extra_mg) and self.n_extra > 0
        self._mg = False if (self.n_extra and not self.extra_mg) else None
        self.mg_build_s = 0.0
        self.stats = None
        self.bias_ids, self.bias_vals = None, None
        self.slope_grp, self.slope_u, self.slope_vals = None, None, None
        if bias is not None:
            # only matrix-free CGNR carries the eliminated biases: never the dense preconditioner
            # (LSQR), whatever the size.  'auto' then takes the node-block preconditioner: the multigrid
            # levels are built from the unprojected operator and cost 6–21× the iterations at C4 where
            # block-Jacobi costs 1.6–2× (profiles/bias_c4.json)
            self.dense_ok = False
            try:
                ids, c = bias[:2]
                self.bias_ids = np.asarray(ids).astype(np.int32)
                self.solver.set_data_bias(self.bias_ids, c)
                self.bias_vals = np.zeros(np.size(c))
                if len(bias) > 2 and bias[2] is not None:
                    grp, u, cs = bias[2]
                    self.slope_grp = np.asarray(grp).astype(np.int32)
                    self.slope_u = np.asarray(u, dtype=float).reshape(-1, 2)
                    self.solver.set_data_slope(self.slope_grp, self.slope_u, cs)
                    self.slope_vals = np.zeros((np.size(cs) // 2, 2))
            except Exception:
                self.solver.close()
                raise
        self.sg, self.sg_vals = None, None
        if sensor_grids is not None:
            if bias is not None and not joint:
                self.solver.close()
                raise ValueError('FitSystem: sensor_grids and bias do not go together')
            # matrix-free CGNR only, never the dense preconditioner (LSQR).  Unlike the biases the grids leave
            # the multigrid its iteration count (58 → 64 at C4, profiles/sgrid_c4.json), so 'auto' keeps it
            self.dense_ok = False
            try:
                sg = dict(sensor_grids)
                sg['grid'] = np.asarray(sg['grid']).astype(np.int32)
                self.solver.set_sensor_grids(sg['grid'], sg['node'], sg['wt'], sg['n_nodes'], sg['K'], joint=bool(joint))
            except Exception:
                self.solver.close()
                raise
            self.sg = sg
            self.sg_off = np.concatenate([[0], np.cumsum(sg['n_nodes'])]).astype(np.int64)
            self.sg_vals = np.zeros(int(self.sg_off[-1]))
            on = sg['grid'] >= 0
            self.sg_rows = np.flatnonzero(on)
            self.sg_cols = self.sg_off[sg['grid'][on]][:, None] + np.asarray(sg['node'])[on]
            self.sg_wt = np.asarray(sg['wt'], dtype=float)[on]
            self.sg_row_shift = np.asarray(sg['shift'], dtype=float)[sg['grid'][on]]
        if bias is not None or sensor_grids is not None:
            # The device takes the biases wherever the data rows came out matrix-free, but only the
            # column-mode CGNR step eliminates them: with 16 epochs (dim 2 ≤ CG_MAXT, yet the dz stencil's
            # strip no longer fits the ring) the set calls succeed and every solve would raise.  Ask now,
            # so that 'eliminate' fails here and 'auto' takes 'columns' (found by tests/test_gpu_cgnr_tile.py)
            ok, why = self.solver.cg_available(1)
            if not ok:
                self.solver.close()
                raise NativeError(f'FitSystem: the elimination cannot run on this system: {why}')

    @property
    def blocks(self):
        """(block_ptr, cols) of the node blocks (bench.py's algorithm-matched CPU baseline), made
        on first use when the device took them in affine form."""
        if self._blocks is None and self.has_blocks:
            self._blocks = node_column_blocks(self._grids, self.keep_cols)
        return self._blocks

    def multigrid_available(self, row_weight=None):
        """True when the geometric multigrid preconditioner (lsq precond 4) runs on this system
        (structured single-GPU smooth_fit system with per-node column blocks)."""
        if self._mg is None:
            if not self.has_blocks or self.formation != 'stencil':
                self._mg = False
            else:
                if row_weight is not None and row_weight is not getattr(self, '_w_last', None):
                    self.solver.set_row_weight(row_weight)
                    self._w_last = row_weight
                tic = time()
                ok, why = self.solver.cg_available(4)   # builds the level hierarchy
                self._mg = bool(ok)
                self.mg_build_s = time() - tic
                if not ok and self.extra_mg:
                    warnings.warn(f'FitSystem: multigrid does not carry the {self.n_extra} extra rows ({why}); '
                                  f'the system stays on block-Jacobi', RuntimeWarning, stacklevel=2)
        return self._mg

    def solve(self, row_weight, data_keep, rhs, x0=None, **opts):
        # re-upload only what changed between outer iterations (weights: same array object)
        if row_weight is not getattr(self, '_w_last', None):
            self.solver.set_row_weight(row_weight)
            self._w_last = row_weight
        dk = np.asarray(data_keep, dtype=bool)
        if getattr(self, '_keep_last', None) is None or not np.array_equal(dk, self._keep_last):
            if getattr(self, '_mask', None) is None:   # constraint rows always kept: filled once
                self._mask = np.ones(self.n_data + self.n_con, dtype=bool)
            self._mask[:self.n_data] = dk
            self.solver.set_row_mask(self._mask)
            self._keep_last = dk.copy()
        if self.bias_ids is not None or self.sg is not None:   # the device rows are a prefix of the caller's rows
            rhs = rhs[:self.n_data + self.n_con]
        if self.sg is not None and np.any(self.sg_row_shift):   # a = a' + shift: the device sees zero priors
            rhs = rhs.copy()
            rhs[self.sg_rows] -= self.sg_row_shift
        x, self.stats = self.solver.solve(rhs, x0=x0, b_rows=getattr(self, 'b_rows', 0), **opts)
        if self.bias_ids is not None:
            self.bias_vals = self.solver.data_bias()
        if self.slope_grp is not None:
            self.slope_vals = self.solver.data_slope()
        if self.sg is not None:
            self.sg_vals = self.solver.sensor_grids() + np.repeat(self.sg['shift'], self.sg['n_nodes'])
        return x

    def expand(self, x):
        if self.bias_ids is not None:   # the biases of the last solve, in the columns after the grids
            n_slope = 0 if self.slope_grp is None else self.slope_vals.size
            n_sg = 0 if self.sg is None else self.sg_vals.size
            m0 = np.zeros(self.n_full + self.bias_vals.size + n_slope + n_sg)
            m0[self.n_full:self.n_full + self.bias_vals.size] = self.bias_vals
            if n_slope:   # behind the biases, (x, y) per group
                m0[self.n_full + self.bias_vals.size:m0.size - n_sg] = self.slope_vals.ravel()
            if n_sg:      # joint: the sensor grids behind the slopes
                m0[m0.size - n_sg:] = self.sg_vals
        elif self.sg is not None:      # the grids of the last solve, in the columns after the others
            m0 = np.zeros(self.n_full + self.sg_vals.size)
            m0[self.n_full:] = self.sg_vals
        else:
            m0 = np.zeros(self.n_full)
        m0[self.keep_cols] = x
        return m0

    def data_forward(self, x):
        """G_data · (Ip_c x), bit-identical to scipy's csr matvec of the reference (eliminated
        biases: plus the last solve's bias of each row's ID)."""
        y = self.solver.spmv_rows(x, 0, self.n_data)
        if self.bias_ids is not None:
            y += self.bias_vals[self.bias_ids]
        if self.slope_grp is not None:
            on = self.slope_grp >= 0
            y[on] += np.sum(self.slope_u[on] * self.slope_vals[self.slope_grp[on]], axis=1)
        if self.sg is not None:
            y[self.sg_rows] += np.sum(self.sg_wt * self.sg_vals[self.sg_cols], axis=1)
        return y

    def rows_sumsq(self, x, ranges):
        """Per (first, count) row range of [G_data; Gc]: (Σ (w·G x)², Σ (G x)²), x compact."""
        return self.solver.rows_sumsq(x, ranges)

    def data_colsum(self, f):
        """G_dataᵀ f over the full column space (f per data row)."""
        return self.solver.data_colsum(f)

    def close(self):
        self.solver.close()


def _extra_rows_csr(ops):
    """(indptr, cols, vals) of the stacked operators' triplets, rows in order, a row's entries in
    the order of the triplets (the device sums duplicates in that order)."""
    rr, cc, vv, row0 = [], [], [], 0
    for op in ops:
        r, c, v = op.triplets()
        rr.append(np.ravel(r) + row0)
        cc.append(np.ravel(c))
        vv.append(np.ravel(v))
        row0 += int(op.N_eq)
    r, c, v = np.concatenate(rr), np.concatenate(cc), np.concatenate(vv)
    order = np.argsort(r, kind='stable')
    indptr = np.zeros(row0 + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=row0), out=indptr[1:])
    return indptr, c[order].astype(np.int64), v[order].astype(np.float64)


def check_data_against_DEM(in_TSE, data, m0, G_data, DEM_tol):
    m1 = m0.copy()
    m1[G_data.TOC['cols']['z0']] = 0
    r_DEM = data.z - G_data.toCSR().dot(m1) - data.DEM
    in_TSE[in_TSE] = np.abs(r_DEM[in_TSE]) < DEM_tol
    return in_TSE


def print_TOC(G_data, Gc):
    print(f'G_data : \n\t{len(np.ravel(G_data.v)) / 1000}K values\n\t shape={np.array(G_data.shape) / 1000}K')
    for label, op in (('G_data', G_data), ('Gc', Gc)):
        print(label, 'rows:')
        for name, rr in op.TOC['rows'].items():
            print(f'\t{name}: {len(np.unique(rr)) / 1000}K')


def _solve_opts(args, n, has_blocks=False, multigrid=False, dense_ok=True):
    """LSQR options.  precond 'auto': the exact dense-Cholesky preconditioner (R⁻¹ on the
    device) when n <= lsq_dense_max (one GPU only), else the geometric multigrid V-cycle
    (precond 4, CGNR) when the system supports it, else block-Jacobi per (y, x) node when the
    system has node blocks, else column scaling (maxit 50 n for the iterative ones)."""
    pc_ = args['lsq_precond']
    if pc_ == 'auto':
        pc_ = 2 if dense_ok and n <= args['lsq_dense_max'] else (4 if multigrid else (3 if has_blocks else 1))
    maxit = args['lsq_maxit'] or (0 if pc_ == 2 else 50 * n)
    # method 'auto': CGNR (normal-stencil operator, column-space only) with the iterative
    # preconditioners — the library falls back to LSQR where the structured operator is absent
    meth = {'auto': 1 if pc_ in (1, 3, 4) else 0, 'lsqr': 0, 'cgnr': 1}[args.get('lsq_method', 'auto')]
    return dict(atol=args['lsq_atol'], btol=args['lsq_btol'], conlim=args['lsq_conlim'], maxit=maxit, precond=pc_,
                method=meth)


def _anorm_seed_ok(precond, weight, in_TSE, prev):
    """May this CGNR solve seed its ‖A M^-1/2‖ estimate with the previous solve's (lsq_opts.anorm0)?
    Column scaling and node-block M: always (the preconditioned Frobenius norm is sqrt(n) whatever
    the weights and mask).  Multigrid: only with the previous solve's row weights (not after the
    sigma_extra_relax re-weighting) and at most 1 % of the data rows re-masked by the edits."""
    if precond in (1, 3):
        return True
    if prev is None or prev[0] is not weight or prev[1] is None:
        return False
    m = np.asarray(in_TSE, bool)
    return m.shape == prev[1].shape and int(np.count_nonzero(m != prev[1])) <= 0.01 * max(m.size, 1)


def iterate_fit(data, system, rhs, TCinv, G_data, Gc, in_TSE, timing, args, grids, sigma_extra_masks=None,
                bias_model=None):
    """Outer editing loop (smooth_fit.py:100-210) around the device solve.  TCinv: the diagonal of
    the reference's TCinv (1/σ per row of [G_data; Gc])."""
    if bias_model:   # the IDs edited before the fit keep their data out (smooth_fit.py:106)
        edit_by_bias(data, np.zeros(Gc.col_N), in_TSE, -1, bias_model, args)
    in_TSE_original = np.zeros(data.shape, dtype=bool)
    in_TSE_original[in_TSE] = True
    N_editable = np.sum(data.editable) if 'editable' in data.fields else data.size
    sigma_extra = np.zeros_like(data.z)
    last_iteration = args['max_iterations'] <= 1
    x = None
    rs_data = None
    timing['lsq_iters'] = 0
    # max |Δdz| between iterations (smooth_fit.py:180) on the compact solution: the dz columns are one
    # contiguous run of the ascending keep_cols, and the removed ones are 0 in every m0.  The full
    # m0 is expanded only where it is returned or read (no 10⁷-entry scatter per iteration at C4).
    dsl = _as_slice(Gc.TOC['cols']['dz'])
    kdz = tuple(int(k) for k in np.searchsorted(system.keep_cols, [dsl.start, dsl.stop])) \
        if isinstance(dsl, slice) else None
    # row weights 1/sqrt(E_all²) with E_all = 1/TCinv (smooth_fit.py:103, 129): |TCinv| — the caller's
    # array itself when positive (no pass over, or copy of, the 77 M rows at C4).  sqrt(fl(x²)) = |x|
    # in IEEE arithmetic, so the reference's weight is 1/|fl(1/TCinv)|, which can differ from |TCinv|
    # by one ulp (a relative 1e-16 change of a row weight; DESIGN.md §4 records the deviation).  The
    # weights are a read-only view: nothing may edit them in place, since they alias TCinv.
    weight0 = (TCinv if TCinv.min() > 0 else np.abs(TCinv)).view()
    weight0.flags.writeable = False
    prev_solve = None   # (row weights, data-row mask) of the previous solve: _anorm_seed_ok
    for iteration in range(args['max_iterations']):
        weight = weight0
        if last_iteration and args['sigma_extra_relax']:
            if args['VERBOSE']:
                print('smooth_fit.iterate_fit: relaxing errors by sigma_extra')
            nd = G_data.shape[0]   # E2_plus = E_all² + sigma_extra² on the data rows only
            weight = weight0.copy()
            weight[:nd] = 1. / np.sqrt((1. / TCinv[:nd]) ** 2 + sigma_extra ** 2)
        if args['VERBOSE']:
            print('starting device lsqr solve for iteration %d at %s' % (iteration, ctime()), flush=True)
        tic = time()
        x_last = x
        x0 = x if (args['lsq_warm_start'] and x is not None) else None
        dense_ok = getattr(system, 'dense_ok', True)
        mg = args['lsq_precond'] == 'auto' and (system.keep_cols.size > args['lsq_dense_max'] or not dense_ok) and \
            getattr(system, 'bias_ids', None) is None and system.multigrid_available(weight)
        if mg and 'mg_build' not in timing:
            timing['mg_build'] = system.mg_build_s
        opts = _solve_opts(args, system.keep_cols.size, system.has_blocks, mg, dense_ok)
        last = system.stats
        if args['lsq_reuse_anorm'] and last is not None and last.get('method') == 1 and \
                opts['method'] == 1 and last.get('precond') == opts['precond'] and \
                _anorm_seed_ok(opts['precond'], weight, in_TSE, prev_solve):
            # the CGNR stopping rule starts from the previous solve's ‖A M^-1/2‖ estimate (lsq_opts
            # .anorm0) instead of rebuilding it from zero: with node-block M (or column scaling) the
            # preconditioned Frobenius norm is sqrt(n) whatever the weights, so the estimate stays
            # below it.  The multigrid M has no such invariant: there the seed is taken only when
            # the weights are the previous solve's and at most 1 % of the data rows changed mask
            opts['anorm0'] = float(last['anorm'])
        try:
            x = system.solve(weight, in_TSE, rhs, x0=x0, **opts)
        except NativeError as e:
            if opts['precond'] != 4 or (args['lsq_precond'] == 4 and 'per-row constraint scales' in str(e)):
                raise   # lsq_cg_scaled with an explicit lsq_precond=4: the device's refusal, no silent change
            # the multigrid set-up can fail for these weights (e.g. a coarsest level that is not
            # positive definite): the block-Jacobi solve still reaches the same solution
            print(f'smooth_fit: multigrid preconditioner unavailable ({e}); block-Jacobi for the rest of '
                  f'the fit', flush=True)
            system._mg = False
            opts = _solve_opts(args, system.keep_cols.size, system.has_blocks, False, dense_ok)
            x = system.solve(weight, in_TSE, rhs, x0=x0, **opts)
        if system.stats['istop'] == 7:
            print(f"smooth_fit: LSQR reached its iteration limit ({system.stats['iters']}) before the "
                  f"requested tolerance; raise lsq_maxit or use lsq_precond=2", flush=True)
        system.stats['precond'] = opts['precond']
        # did this solve run the multigrid with the priors' rows lumped into it (lsq_prior_mg)?
        timing['prior_mg'] = bool(opts['precond'] == 4 and getattr(system, 'n_extra', 0) > 0)
        # did this solve run CGNR in chunk mode (lsq_cg_chunks on a dz grid of 20 to 64 epochs)?
        timing['cg_chunks'] = bool(getattr(system, 'cg_chunks', False) and system.stats['method'] == 1 and
                                   system.solver.cg_layout_info()['mode'] == 'chunk')
        # did this solve run CGNR with scaled parts (lsq_cg_scaled on a masked or mapped fit)?
        timing['cg_scaled'] = bool(getattr(system, 'cg_scaled', False) and system.stats['method'] == 1 and
                                   system.solver.cg_scaled_info()['parts'] > 0)
        # did this solve eliminate biases or sensor grids in tile or chunk mode (lsq_tile_eliminate, 16 to 64 epochs)?
        timing['tile_eliminate'] = bool(
            getattr(system, 'tile_dmf', False) and system.stats['method'] == 1 and
            (getattr(system, 'bias_ids', None) is not None or getattr(system, 'sg', None) is not None) and
            system.solver.cg_layout_info()['mode'] in ('tile', 'chunk'))
        prev_solve = (weight, np.asarray(in_TSE, bool).copy() if opts['precond'] == 4 else None)
        system.last_x = x   # compact solution: z_est and the constraint statistics read it, not m0
        timing['sparseqr_solve'] = time() - tic
        timing['lsq_iters'] += int(system.stats['iters'])
        timing.setdefault('lsq_iters_per_solve', []).append(int(system.stats['iters']))
        timing['lsq_setup'] = timing.get('lsq_setup', 0.) + float(system.stats.get('setup_s', 0.))
        timing['lsq_last'] = dict(system.stats)
        tic = time()
        r_data = data.z - system.data_forward(x)
        rs_data = r_data / data.sigma
        timing['residual'] = timing.get('residual', 0.) + time() - tic
        if last_iteration:
            break
        tic_edit = time()
        if args.get('sigma_extra_bin_spacing') is None:
            sigma_extra = calc_sigma_extra(r_data, data.sigma, in_TSE, sigma_extra_masks, device=args['device'])
        else:
            sigma_extra = calc_sigma_extra_on_grid(data.x, data.y, r_data, data.sigma, in_TSE,
                                                   sigma_extra_masks=sigma_extra_masks,
                                                   sigma_extra_max=args['sigma_extra_max'],
                                                   spacing=args['sigma_extra_bin_spacing'],
                                                   device=args['device'])
        sigma_aug = np.sqrt(data.sigma ** 2 + sigma_extra ** 2)
        in_TSE_last = in_TSE
        in_TSE = np.abs(r_data / sigma_aug) < 3.0
        bias_editing_changed = False
        if bias_model:
            bias_editing_changed = edit_by_bias(data, system.expand(x), in_TSE, iteration, bias_model, args)
        if 'editable' in data.fields:
            in_TSE[data.editable == 0] = in_TSE_original[data.editable == 0]
        if args['DEM_tol'] is not None:
            in_TSE = check_data_against_DEM(in_TSE, data, system.expand(x), G_data, args['DEM_tol'])
        if not np.any(in_TSE):
            if args['VERBOSE']:
                print('Edited data empty, returning')
            return system.expand(x), sigma_extra, in_TSE, rs_data
        if kdz is not None:
            xs = x[kdz[0]:kdz[1]]
            ddz = np.abs(xs) if x_last is None else np.subtract(x_last[kdz[0]:kdz[1]], xs)
            dmax = float(np.max(np.abs(ddz, out=ddz))) if ddz.size else 0.0
        else:
            m_last = system.expand(x_last) if x_last is not None else np.zeros(system.n_full)
            dmax = float(np.max(np.abs(m_last[dsl] - system.expand(x)[dsl])))
        if dmax < args['converge_tol_dz'] and iteration > args['min_iterations']:
            if args['VERBOSE']:
                print('Solution identical to previous iteration with tolerance %3.1f, exiting after iteration %d'
                      % (args['converge_tol_dz'], iteration))
            last_iteration = True
        if args['VERBOSE']:
            print('found %d in TSE, dt=%3.0f' % (in_TSE.sum(), timing['sparseqr_solve']), flush=True)
            if sigma_extra_masks is None:
                print(f'\t median(sigma_extra)={np.median(sigma_extra):3.4f}')
            else:
                for key, ii in sigma_extra_masks.items():
                    print(f'\t sigma_extra for {key} : {np.median(sigma_extra[ii]):3.4f}', flush=True)
                for key, ii in sigma_extra_masks.items():
                    print(f'\t sigma_hat for {key} : {RDE(r_data[ii] / sigma_aug[ii]):3.4f}', flush=True)
        if iteration > 0 and iteration > args['bias_nsigma_iteration']:
            frac_TSE_change = len(np.setxor1d(in_TSE_last, in_TSE)) / N_editable
            if frac_TSE_change < args['converge_tol_frac_TSE']:
                if args['VERBOSE']:
                    print('filtering unchanged with tolerance %3.5f, will exit after iteration %d'
                          % (args['converge_tol_frac_TSE'], iteration + 1))
                last_iteration = True
        if iteration >= np.maximum(args['min_iterations'], args['bias_nsigma_iteration'] + 1):
            if np.all(sigma_extra < 0.5 * np.min(data.sigma[in_TSE])) and not bias_editing_changed:
                if args['VERBOSE']:
                    print('sigma_extra is small, performing one additional iteration', flush=True)
                last_iteration = True
        if iteration == args['max_iterations'] - 2:
            last_iteration = True
        timing['edit'] = timing.get('edit', 0.) + time() - tic_edit
    return (system.expand(x) if x is not None else np.zeros(system.n_full)), sigma_extra, in_TSE, rs_data


def _toc_slice(op, name):
    """op.TOC['rows'][name] as a slice when it is one contiguous run (not materialised), else the
    index array"""
    kr = toc_range(op.TOC['rows'], name)
    return slice(kr[0], kr[1] + 1) if kr is not None else _as_slice(op.TOC['rows'][name])


def _as_slice(idx):
    """A contiguous ascending index array as a slice (no fancy-indexing copy of 73 M rows)."""
    kr = known_range(idx)
    if kr is not None:
        return slice(kr[0], kr[1] + 1)
    idx = np.asarray(idx)
    if idx.ndim == 1 and idx.size and idx[-1] - idx[0] == idx.size - 1 and np.all(idx[1:] - idx[:-1] == 1):
        return slice(int(idx[0]), int(idx[-1]) + 1)
    return idx


def _device_constraint_stats(system, m0, Gc, R, RMS):
    """R and RMS of each constraint type (smooth_fit.py:318-331) reduced on the device from the
    formed operator: no host copy of the 10⁷–10⁸ constraint residuals.  False when a type's rows
    are not one contiguous range (then the caller takes the host path)."""
    names, ranges = [], []
    for eq_type in ['d2z_dt2', 'grad2_z0', 'grad2_dzdt', 'grad2_PS']:
        if eq_type in Gc.TOC['rows']:
            rows = _toc_slice(Gc, eq_type)
            if not isinstance(rows, slice):
                return False
            names.append(eq_type)
            ranges.append((system.n_data + rows.start, rows.stop - rows.start))
    if names:
        x = getattr(system, 'last_x', None)   # the compact solution m0 was expanded from (iterate_fit)
        if x is None or x.size != np.size(system.keep_cols):
            x = m0[system.keep_cols]
        sw, su = system.rows_sumsq(x, ranges)
        for name, (first, count), a, b in zip(names, ranges, sw, su):
            R[name] = a
            RMS[name] = np.sqrt(b / count)
    return True


def tcinv_diagonal(Ed, Gc, constraint_op_list):
    """The diagonal of TCinv = diag(1 / [Ed; Ec]) (smooth_fit.py:594-613), written in one pass from
    the ops' expected values (no Ec, no concatenation of the 77 M rows at C4); equal bit for bit to
    1 / np.concatenate((Ed, Ec)).  A constraint row that no op covers has Ec = 0 there: the
    reference's zero check (the ops' own expected values were checked by
    setup_smoothness_constraints)."""
    nd = Ed.size
    out = np.empty(nd + Gc.N_eq)
    np.divide(1., Ed, out=out[:nd])
    Tc = out[nd:]
    covered = 0
    for op in constraint_op_list:
        rows = _toc_slice(Gc, op.name)
        e = np.ravel(op.expected)
        if isinstance(rows, slice):
            np.divide(1., e, out=Tc[rows])
            covered += rows.stop - rows.start
        else:
            Tc[rows] = 1. / e
            covered += np.size(rows)
    if covered != Gc.N_eq:
        raise ValueError('zero value found in constraint sigma')
    return out


def parse_model(m, m0, data, R, RMS, G_data, averaging_ops, Gc, Ec, grids, args, ru=None, system=None):
    """Output grids and fit statistics (smooth_fit.py:276-352).  With the device `system` the
    constraint statistics and the count / misfit maps are reduced on the device."""
    z0g, dzg = grids['z0'], grids['dz']
    # the column ranges as slices (a copy of a slice, not a 12 M-entry gather at C4)
    cols_of = {ff: _as_slice(G_data.TOC['cols'][ff]) for ff in ('z0', 'dz')}
    m['z0'] = pc.grid.data().from_dict({'x': z0g.ctrs[1], 'y': z0g.ctrs[0], 'cell_area': z0g.cell_area,
                                        'mask': z0g.mask, 'z0': np.reshape(np.array(m0[cols_of['z0']]), z0g.shape)})
    m['dz'] = pc.grid.data().from_dict({'x': dzg.ctrs[1], 'y': dzg.ctrs[0], 'time': dzg.ctrs[2],
                                        'dz': np.reshape(np.array(m0[cols_of['dz']]), dzg.shape),
                                        'cell_area': dzg.cell_area, 'mask': dzg.mask})
    for key, op in averaging_ops.items():
        fields = {coord: ctr for coord, ctr in zip(op.dst_grid.coords, op.dst_grid.ctrs)}
        fields.update({'cell_area': op.dst_grid.cell_area, key: op.grid_prod(m0)})
        m[key] = pc.grid.data().from_dict(fields)
    m['all'] = m0
    m['extent'] = np.concatenate((z0g.bds[1], z0g.bds[0]))
    m['sensor_bias_grids'] = parse_sensor_bias_grids(m0, G_data, grids)
    m['jitter_bias_grids'] = {}
    if system is None or not _device_constraint_stats(system, m0, Gc, R, RMS):
        if callable(Ec):         # smooth_fit's on-demand constraint sigma
            Ec = Ec()
        if ru is None:           # unscaled constraint residuals Gc·m0 (device product when available)
            ru = system.solver.spmv(m0[system.keep_cols])[system.n_data:] if hasattr(system, 'solver') \
                else Gc.toCSR().dot(m0)
        for eq_type in ['d2z_dt2', 'grad2_z0', 'grad2_dzdt', 'grad2_PS']:
            if eq_type in Gc.TOC['rows']:
                rows = _toc_slice(Gc, eq_type)
                rc = (1. / Ec[rows]) * ru[rows]   # TCinv_cov.dot(ru), smooth_fit.py:324-326
                R[eq_type] = np.sum(rc ** 2)
                RMS[eq_type] = np.sqrt(np.mean(ru[rows] ** 2))
    tse = data.three_sigma_edit
    r = (data.z - data.z_est)[tse]
    if args['sigma_extra_relax']:
        r_scaled = r / np.sqrt(data.sigma[tse] ** 2 + data.sigma_extra[tse] ** 2)
    else:
        r_scaled = r / data.sigma[tse]
    # Gselᵀ·{1, r_scaled², r²} of smooth_fit.py:341-347: weighted column sums over the kept data rows
    per_point = {'scaled': r_scaled ** 2, 'plain': r ** 2}
    if 'tide' in data.fields:   # smooth_fit.py:346-352: the residual with the tide correction undone
        r_notide = (data.z + data.tide - data.z_est)[tse]
        per_point['notide_plain'] = r_notide ** 2
        per_point['notide_scaled'] = (r_notide / data.sigma[tse]) ** 2
    tse_b = np.asarray(tse).astype(bool).ravel()
    n_cols = G_data.col_N
    sums = None
    if system is not None and getattr(system, 'formation', None) == 'stencil':
        fs = {'count': tse_b.astype(float)}
        for key, vals in per_point.items():
            f = np.zeros(tse_b.size)
            f[tse_b] = vals
            fs[key] = f
        try:   # node gather over the points sorted by cell (no host triplets of the data operator)
            sums = {k: system.data_colsum(f)[:n_cols] for k, f in fs.items()}
        except NativeError:
            sums = None
    if sums is None:   # host: weighted column sums of G_data's triplets
        rr, cc, vv = G_data.triplets()
        rows_tse = np.flatnonzero(tse_b)
        pos = np.full(tse_b.shape, -1)
        pos[rows_tse] = np.arange(rows_tse.size)
        sel = tse_b[rr] & (vv != 0)
        c_sel, v_sel, p_sel = cc[sel], vv[sel], pos[rr[sel]]
        sums = {'count': np.bincount(c_sel, weights=v_sel, minlength=n_cols)}
        for key, vals in per_point.items():
            sums[key] = np.bincount(c_sel, weights=v_sel * vals[p_sel], minlength=n_cols)
    for ff in ['dz', 'z0']:
        cols = cols_of[ff]
        shape = grids[ff].shape
        m[ff].assign({'count': sums['count'][cols].reshape(shape)})
        m[ff].count[m[ff].count == 0] = np.nan
        m[ff].assign({'misfit_scaled_rms': np.sqrt(sums['scaled'][cols].reshape(shape) / m[ff].count)})
        m[ff].assign({'misfit_rms': np.sqrt(sums['plain'][cols].reshape(shape) / m[ff].count)})
        if 'notide_plain' in sums:
            m[ff].assign({'misfit_notide_rms': np.sqrt(sums['notide_plain'][cols].reshape(shape) / m[ff].count)})
            m[ff].assign({'misfit_notide_scaled_rms':
                          np.sqrt(sums['notide_scaled'][cols].reshape(shape) / m[ff].count)})


def _bias_fit_system(G_data, Gc, G_grid, Gc_grid, keep_cols, data, bias_model, mode, grids, device, args,
                     prior_ops=(), sgrid=None):
    """The device system of a fit with data biases.  'eliminate': the grid-only operators on the
    device plus lsq_set_data_bias (the bias constraint rows are the last rows of Gc, so the device
    rows are a prefix of the host rows); 'columns': the biases as ordinary columns of a generic
    (COO-formed) system; 'auto': 'columns' when the grid unknowns (the eliminating system's columns)
    are few enough for the dense preconditioner, when the options ask for what only 'columns' runs
    (LSQR, the dense preconditioner) or when the device cannot eliminate (no matrix-free data rows, or
    slope groups that the bias IDs do not nest in), else 'eliminate'.  Slope biases (slope_bias_dict
    of bias_model) go with the biases either way.
    With prior_ops (the priors behind the bias constraint rows of Gc) only 'columns' runs: the device
    rows of 'eliminate' are a prefix of the host rows, which rows behind the bias constraints would
    break.  smooth_fit refuses 'eliminate' with priors; 'auto' takes 'columns' and warns where it
    would have eliminated, since the generic system costs the memory and speed of matrix-free CGNR.
    sgrid = (sensor_of, constraint_op_list) (lsq_sgrid_joint): sensor bias grids whose columns follow the
    slopes' in G_data, eliminated jointly with the biases (lsq_set_sensor_grids_joint).  Where the device
    refuses (an ID or group that does not nest in the grids, a cap) 'eliminate' raises and 'auto' warns
    and takes 'columns'."""
    n_grid = G_grid.col_N if G_grid is not None else None
    slope_dict = bias_model.get('slope_bias_dict', {})
    if mode == 'auto' and (describe(G_grid, Gc_grid, with_fields=True) is None or
                           np.count_nonzero(keep_cols < n_grid) <= args['lsq_dense_max'] or
                           args['lsq_method'] == 'lsqr' or args['lsq_precond'] == 2):
        mode = 'columns'
    if prior_ops and mode != 'columns':
        warnings.warn("smooth_fit: lsq_bias='auto' with prior_args / prior_edge_args takes 'columns': biases and "
                      "priors together run as a generic (COO-formed) system, not matrix-free CGNR",
                      RuntimeWarning, stacklevel=3)
        mode = 'columns'
    if mode != 'columns':
        sg = sensor_grid_device_form(data, grids, *sgrid) if sgrid is not None else None
        n_sg = int(np.sum(sg['n_nodes'])) if sg is not None else 0
        n_bias = int(G_data.col_N) - int(n_grid) - 2 * len(slope_dict) - n_sg
        ids = np.asarray(data.bias_ID).astype(np.int32)
        c = 1. / bias_expected(bias_model, n_bias)
        bias = (ids, c)
        if slope_dict:   # the groups in the order of their columns
            _, group, u = slope_columns(data, np.array(list(slope_dict.keys())))
            bias += ((group, u, np.full((len(slope_dict), 2), 1. / (bias_model['E_slope_bias'] * SLOPE_RESCALE))),)
        try:
            return FitSystem(G_grid, Gc_grid, keep_cols[keep_cols < n_grid], n_grid, device=device, grids=grids,
                             bias=bias, sensor_grids=sg, joint=sg is not None, cg_chunks=args['lsq_cg_chunks'],
                             tile_dmf=args['lsq_tile_eliminate'], cg_scaled=args['lsq_cg_scaled'])
        except NativeError as e:
            if mode == 'eliminate':
                raise
            if sg is not None:
                warnings.warn(f"smooth_fit: lsq_bias='auto' with lsq_sgrid_joint takes 'columns': the device refuses "
                              f"the joint elimination ({e})", RuntimeWarning, stacklevel=3)
    return FitSystem(G_data, Gc, keep_cols, Gc.col_N, device=device, grids=grids, cg_chunks=args['lsq_cg_chunks'],
                     tile_dmf=args['lsq_tile_eliminate'], cg_scaled=args['lsq_cg_scaled'])


def _sgrid_fit_system(G_data, Gc, G_grid, Gc_grid, keep_cols, data, sgrid_sensor, constraint_op_list, mode, grids,
                      device, args):
    """The device system of a fit with sensor bias grids (and no biases, slopes or priors).
    'eliminate': the operators without the grids on the device plus lsq_set_sensor_grids (the grids'
    constraint rows are the last rows of Gc, so the device rows are a prefix of the host rows);
    'columns': the grids as ordinary columns of a generic (COO-formed) system; 'auto': 'columns' when
    the other unknowns are few enough for the dense preconditioner, when the options ask for what only
    'columns' runs (LSQR, the dense preconditioner) or when the device refuses (no matrix-free data
    rows, a grid over the size cap), else 'eliminate'."""
    n_grid = G_grid.col_N if G_grid is not None else None
    if mode == 'auto' and (describe(G_grid, Gc_grid, with_fields=True) is None or
                           np.count_nonzero(keep_cols < n_grid) <= args['lsq_dense_max'] or
                           args['lsq_method'] == 'lsqr' or args['lsq_precond'] == 2):
        mode = 'columns'
    if mode != 'columns':
        sg = sensor_grid_device_form(data, grids, sgrid_sensor, constraint_op_list)
        try:
            return FitSystem(G_grid, Gc_grid, keep_cols[keep_cols < n_grid], n_grid, device=device, grids=grids,
                             sensor_grids=sg, cg_chunks=args['lsq_cg_chunks'],
                             tile_dmf=args['lsq_tile_eliminate'], cg_scaled=args['lsq_cg_scaled'])
        except NativeError:
            if mode == 'eliminate':
                raise
    return FitSystem(G_data, Gc, keep_cols, Gc.col_N, device=device, grids=grids, cg_chunks=args['lsq_cg_chunks'],
                     tile_dmf=args['lsq_tile_eliminate'], cg_scaled=args['lsq_cg_scaled'])


def _constraint_scaling_masks(maps, grids):
    """constraint_scaling_maps on the grids' (y, x) nodes (smooth_fit.py:467-485): keys with 'z0' on the z0
    lattice, the rest on the dz lattice, non-finite entries 1.  A map is a containers.GridData (interpolated
    to the nodes) or an array already on them.  The key 'dz' (the dz_zero rows) stays outside lssurf_amd."""
    if maps is None:
        return None
    if not isinstance(maps, dict):
        raise ValueError('smooth_fit: constraint_scaling_maps must be a dict of maps by constraint key')
    masks = {}
    for key, this_map in maps.items():
        if key == 'dz':
            raise NotImplementedError("smooth_fit: constraint_scaling_maps['dz'] (the dz_zero rows) is outside "
                                      "lssurf_amd (SURVEY.md §2)")
        grid = grids['z0'] if 'z0' in key else grids['dz']
        if hasattr(this_map, 'interp'):
            mask = np.array(this_map.interp(grid.ctrs[1], grid.ctrs[0], gridded=True), dtype=float)
        else:
            mask = np.array(this_map, dtype=float)
        if mask.shape != tuple(grid.shape[:2]):
            raise ValueError(f'smooth_fit: constraint_scaling_maps[{key!r}] has shape {mask.shape}, the grid\'s '
                             f'(y, x) nodes are {tuple(grid.shape[:2])}')
        mask[~np.isfinite(mask)] = 1.
        masks[key] = mask
    return masks


def smooth_fit(**kwargs):
    required = ('data', 'W', 'ctr', 'spacing', 'E_RMS')
    args = dict(DEFAULTS)
    args.update(kwargs)
    for field in required:
        if field not in kwargs:
            raise ValueError('%s must be defined' % field)
    for key in OUT_OF_SCOPE:
        if args.get(key) is not None:
            raise NotImplementedError(f'smooth_fit: {key!r} is outside lssurf_amd (SURVEY.md §2)')
    has_slopes = args.get('data_slope_sensors') is not None and len(args['data_slope_sensors']) > 0
    if has_slopes:
        # slope biases are eliminated (or carried as columns) with the data biases: the same key says how,
        # and every refusal of bias_params below holds for them
        if args['lsq_bias'] is None:
            raise NotImplementedError("smooth_fit: 'data_slope_sensors' needs the solver key lsq_bias ('eliminate', "
                                      "'columns' or 'auto'); without it slope biases are outside lssurf_amd")
        if args['bias_params'] is None:
            raise ValueError("smooth_fit: 'data_slope_sensors' needs 'bias_params' (the model's biases are read "
                             "back through them)")
    if not isinstance(args['lsq_prior_mg'], (bool, np.bool_)):
        raise ValueError(f"smooth_fit: lsq_prior_mg must be True or False, not {args['lsq_prior_mg']!r}")
    if not isinstance(args['lsq_E_border'], (bool, np.bool_)):
        raise ValueError(f"smooth_fit: lsq_E_border must be True or False, not {args['lsq_E_border']!r}")
    if not isinstance(args['lsq_E_border_solve'], (bool, np.bool_)):
        raise ValueError(f"smooth_fit: lsq_E_border_solve must be True or False, not {args['lsq_E_border_solve']!r}")
    if not isinstance(args['lsq_sgrid_joint'], (bool, np.bool_)):
        raise ValueError(f"smooth_fit: lsq_sgrid_joint must be True or False, not {args['lsq_sgrid_joint']!r}")
    if not isinstance(args['lsq_cg_chunks'], (bool, np.bool_)):
        raise ValueError(f"smooth_fit: lsq_cg_chunks must be True or False, not {args['lsq_cg_chunks']!r}")
    if not isinstance(args['lsq_cg_scaled'], (bool, np.bool_)):
        raise ValueError(f"smooth_fit: lsq_cg_scaled must be True or False, not {args['lsq_cg_scaled']!r}")
    if not isinstance(args['lsq_tile_eliminate'], (bool, np.bool_)):
        raise ValueError(f"smooth_fit: lsq_tile_eliminate must be True or False, not {args['lsq_tile_eliminate']!r}")
    bias_mode = args['lsq_bias']
    if args['bias_params'] is not None:
        if bias_mode is None:
            raise NotImplementedError("smooth_fit: 'bias_params' needs the solver key lsq_bias ('eliminate', "
                                      "'columns' or 'auto'); without it data biases are outside lssurf_amd")
        if bias_mode not in ('eliminate', 'columns', 'auto'):
            raise ValueError(f"smooth_fit: lsq_bias must be 'eliminate', 'columns' or 'auto', not {bias_mode!r}")
        if args['compute_E'] and not args['lsq_E_border']:
            raise NotImplementedError("smooth_fit: compute_E with bias_params (sigma_bias) is outside lssurf_amd")
        if args['compute_E'] and args['lsq_E_method'] == 'window' and not args['lsq_E_border_solve']:
            from .errors import WINDOW_BORDER_REFUSAL
            raise NotImplementedError('smooth_fit: ' + WINDOW_BORDER_REFUSAL)
        if int(args['n_gpus']) > 1 or (args['devices'] is not None and len(args['devices']) > 1):
            raise NotImplementedError("smooth_fit: bias_params runs on one GPU")
        if bias_mode == 'eliminate' and args['lsq_method'] == 'lsqr':
            raise NotImplementedError("smooth_fit: lsq_bias='eliminate' runs CGNR; lsq_method='lsqr' needs "
                                      "lsq_bias='columns'")
        if bias_mode == 'eliminate' and args['lsq_precond'] not in ('auto', 1, 3, 4):
            raise NotImplementedError("smooth_fit: lsq_bias='eliminate' runs CGNR with lsq_precond 'auto', 1, 3 or "
                                      "4; the dense preconditioner needs lsq_bias='columns'")

    has_priors = args.get('prior_args') is not None or args.get('prior_edge_args') is not None
    has_sgrids = args.get('sensor_grid_bias_params') is not None and len(args['sensor_grid_bias_params']) > 0
    sgrid_mode, sgrid_joint = None, False
    if has_sgrids:
        # sensor bias grids: the same key says how they run, and the refusals of bias_params hold
        sgrid_mode = bias_mode
        if sgrid_mode is None:
            raise NotImplementedError("smooth_fit: 'sensor_grid_bias_params' needs the solver key lsq_bias ('eliminate', "
                                      "'columns' or 'auto'); without it sensor bias grids are outside lssurf_amd")
        if sgrid_mode not in ('eliminate', 'columns', 'auto'):
            raise ValueError(f"smooth_fit: lsq_bias must be 'eliminate', 'columns' or 'auto', not {sgrid_mode!r}")
        check_sensor_grid_params(args['sensor_grid_bias_params'])
        if args['compute_E']:
            raise NotImplementedError("smooth_fit: compute_E with sensor_grid_bias_params is outside lssurf_amd")
        if int(args['n_gpus']) > 1 or (args['devices'] is not None and len(args['devices']) > 1):
            raise NotImplementedError("smooth_fit: sensor_grid_bias_params runs on one GPU")
        if sgrid_mode == 'eliminate' and args['lsq_method'] == 'lsqr':
            raise NotImplementedError("smooth_fit: lsq_bias='eliminate' runs CGNR; lsq_method='lsqr' needs "
                                      "lsq_bias='columns'")
        if sgrid_mode == 'eliminate' and args['lsq_precond'] not in ('auto', 1, 3, 4):
            raise NotImplementedError("smooth_fit: lsq_bias='eliminate' runs CGNR with lsq_precond 'auto', 1, 3 or "
                                      "4; the dense preconditioner needs lsq_bias='columns'")
        # lsq_sgrid_joint: the biases and slopes that nest in the grids' sensors join their grid's block
        sgrid_joint = bool(args['lsq_sgrid_joint']) and args['bias_params'] is not None and not has_priors and \
            sgrid_mode != 'columns'
        if (args['bias_params'] is not None or has_slopes or has_priors) and not sgrid_joint:
            # the joint eliminated block is no longer one dense block per grid
            if sgrid_mode == 'eliminate':
                raise NotImplementedError("smooth_fit: sensor_grid_bias_params with lsq_bias='eliminate' does not go "
                                          "together with bias_params, data_slope_sensors or priors; "
                                          "lsq_bias='columns' (or 'auto') carries them all")
            if sgrid_mode == 'auto':
                warnings.warn("smooth_fit: lsq_bias='auto' with sensor_grid_bias_params beside bias_params, "
                              "data_slope_sensors or priors takes 'columns': a generic (COO-formed) system, not "
                              "matrix-free CGNR", RuntimeWarning, stacklevel=2)
                sgrid_mode = bias_mode = 'columns'
    if has_priors:
        # priors (match_priors): rows behind the constraints that the device carries as extra rows
        if args['compute_E']:
            raise NotImplementedError("smooth_fit: compute_E with prior_args / prior_edge_args is outside lssurf_amd")
        if int(args['n_gpus']) > 1 or (args['devices'] is not None and len(args['devices']) > 1):
            raise NotImplementedError("smooth_fit: prior_args / prior_edge_args run on one GPU")
        if args['bias_params'] is not None and bias_mode == 'eliminate':
            raise NotImplementedError("smooth_fit: priors with lsq_bias='eliminate' are outside lssurf_amd; "
                                      "lsq_bias='columns' (or 'auto') carries both")

    valid_data = np.isfinite(args['data'].z)
    if 'sensor' not in args['data'].fields:
        args['data'].assign(sensor=np.zeros(args['data'].shape))
    timing = {}
    m, E, R, RMS = {}, {}, {}, {}
    tic = time()
    grids, bds = setup_grids(args)
    valid_data = valid_data & grids['dz'].validate_pts(args['data'].coords()) & \
        grids['z0'].validate_pts(args['data'].coords()[0:2])
    if not np.any(valid_data):
        if args['VERBOSE']:
            print('smooth_fit: no valid data')
        return {'m': m, 'E': E, 'data': None, 'grids': grids, 'valid_data': valid_data, 'TOC': {}, 'R': {},
                'RMS': {}, 'timing': timing, 'E_RMS': args['E_RMS']}
    data = args['data'].copy_subset(valid_data)
    validate_by_dz_mask(data, grids, valid_data)
    if args['sigma_extra_keys'] is not None:
        # one sigma_extra group per key: the data whose field takes any of the listed values
        # (smooth_fit.py:442-447; the masks are over the valid subset already)
        args['sigma_extra_masks'] = {}
        for key, field_vals in args['sigma_extra_keys'].items():
            mask = np.zeros_like(data.sensor, dtype=bool)
            for field, vals in field_vals.items():
                mask |= np.isin(getattr(data, field), vals)
            args['sigma_extra_masks'][key] = mask
    elif args['sigma_extra_masks'] is not None:
        for key in args['sigma_extra_masks']:
            args['sigma_extra_masks'][key] = args['sigma_extra_masks'][key][valid_data == 1]
    if data.size == 0:
        print('\tsmooth_fit.py: after masking, no data found')
        return {'m': m, 'E': E, 'data': data, 'grids': grids, 'valid_data': valid_data, 'TOC': {}, 'R': {},
                'RMS': {}, 'timing': timing, 'E_RMS': args['E_RMS']}

    def interp_ops():
        G = lin_op(grids['z0'], name='interp_z').interp_mtx(data.coords()[0:2])
        return G.add(lin_op(grids['dz'], name='interp_dz').interp_mtx(data.coords()))
    G_data = interp_ops()
    constraint_op_list = []
    if args['VERBOSE']:
        print(f"smooth_fit: E_RMS={args['E_RMS']}")
    setup_smoothness_constraints(grids, constraint_op_list, args['E_RMS'], args['mask_scale'],
                                 scaling_masks=_constraint_scaling_masks(args['constraint_scaling_maps'], grids))
    zero_prior = set()   # priors created here are zeros: rhs is already zero on their rows
    for op in constraint_op_list:
        if op.prior is None:
            op.prior = np.zeros(np.shape(op.expected))   # calloc: untouched pages (73 M rows at C4)
            zero_prior.add(op.name)
    # data biases: one column per unique combination of the bias parameters behind the grids'
    # columns, and their constraint rows last (smooth_fit.py:492-498).  G_grid / Gc_grid: the
    # operators without them, which the device holds when it eliminates the biases itself
    bias_model, G_grid, Gc_grid = {}, None, None
    if args['bias_params'] is not None:
        data, bias_model = assign_bias_ID(data, args['bias_params'], bias_filter=args['bias_filter'])
        # (also what compute_E's border solves run on: errors.split_border)
        if bias_mode != 'columns' or (args['compute_E'] and args['lsq_E_border_solve']):
            G_grid = interp_ops()
            Gc_grid = lin_op(None, name='constraints').vstack(list(constraint_op_list))
        setup_bias_fit(data, bias_model, G_data, constraint_op_list, bias_param_name='bias_ID')
        constraint_op_list[-1].prior = np.zeros(np.shape(constraint_op_list[-1].expected))
        zero_prior.add(constraint_op_list[-1].name)
        if args['bias_nsigma_edit']:
            bias_model['bias_param_dict']['edited'] = np.zeros_like(bias_model['bias_param_dict']['ID'], dtype=bool)
    # slope biases: two columns per listed sensor that the valid data hold, behind the bias columns, and
    # their constraint rows behind the bias constraint rows (smooth_fit.py:515-525)
    if has_slopes:
        sensors = np.asarray(args['data_slope_sensors'])
        args['data_slope_sensors'] = sensors[np.isin(sensors, data.sensor)]
        if len(args['data_slope_sensors']) > 0:
            bias_model['E_slope_bias'] = args['E_slope_bias']
            G_slope, Gc_slope, bias_model = data_slope_bias(data, bias_model, sensors=args['data_slope_sensors'],
                                                            col_0=G_data.col_N, E_rms_bias=args['E_slope_bias'])
            if G_slope is not None:
                G_data.add(G_slope)
                constraint_op_list.append(Gc_slope)
                zero_prior.add(Gc_slope.name)
    # sensor bias grids: a grid's columns behind everything so far and its constraint rows behind the
    # constraints so far, grid by grid (smooth_fit.py:570-572).  G_grid / Gc_grid: the operators
    # without them, which the device holds when it eliminates the grids itself
    sgrid_sensor = {}
    if has_sgrids:
        if sgrid_mode != 'columns' and not sgrid_joint:   # joint: the operators without the biases, made above
            G_grid = interp_ops()
            Gc_grid = lin_op(None, name='constraints').vstack(list(constraint_op_list))
        for params in args['sensor_grid_bias_params']:
            n_before = len(constraint_op_list)
            name = setup_sensor_grid_bias(data, grids, G_data, constraint_op_list, **params)
            if name is not None:
                sgrid_sensor[name] = params['sensor']
            for op in constraint_op_list[n_before:]:
                if op.prior is None:
                    op.prior = np.zeros(np.shape(op.expected))
                    zero_prior.add(op.name)
        if not sgrid_sensor:
            has_sgrids, sgrid_mode, sgrid_joint = False, None, False
    sgrid_ops = {'grad2_' + name for name in sgrid_sensor} | {'mag_' + name for name in sgrid_sensor}
    # priors, in the reference's order (smooth_fit.py:575-582), behind every other constraint
    prior_ops = []
    if args.get('prior_args') is not None:
        prior_ops += match_prior_dz(grids, **args['prior_args'])
    if args.get('prior_edge_args') is not None:
        edge_ops, _ = match_tile_edges(grids, args['reference_epoch'], **args['prior_edge_args'])
        prior_ops += edge_ops
        if args['VERBOSE']:
            print(f'smooth_fit: found prior constraints in {len(edge_ops)} tiles')
    constraint_op_list += prior_ops
    prior_names = {op.name for op in prior_ops}
    Gc = lin_op(None, name='constraints').vstack(constraint_op_list)
    N_eq = G_data.N_eq + Gc.N_eq
    Ed = data.sigma.ravel()
    if not np.all(Ed):     # no boolean temporary
        raise ValueError('zero value found in data sigma')
    TCinv_diag = tcinv_diagonal(Ed, Gc, constraint_op_list)

    def Ec():   # the reference reads Ec only as 1/Ec: made on demand (73 M rows at C4)
        out = np.zeros(Gc.N_eq)
        for op in constraint_op_list:
            out[_toc_slice(Gc, op.name)] = op.expected
        return out
    if args['DEBUG']:
        print_TOC(G_data, Gc)
    rhs = np.zeros([N_eq])
    rhs[0:data.size] = data.z.ravel()
    b_rows = data.size   # rhs[b_rows:] == 0: only the data rows (and non-zero priors) cross PCIe
    b_rows_all = None    # the same with the prior ops counted (systems that hold them as ordinary rows)
    b_rows_sg = None     # and with the sensor grids' magnitude priors (systems that hold them as ordinary rows)
    for op in constraint_op_list:   # rhs[data.size:] = the concatenated priors
        if op.name not in zero_prior:
            rows = _toc_slice(Gc, op.name)
            prior = np.ravel(op.prior)
            if isinstance(rows, slice):
                rhs[data.size + rows.start:data.size + rows.stop] = prior
                end = rows.stop
            else:
                rhs[data.size + rows] = prior
                end = int(np.max(rows)) + 1 if np.size(rows) else 0
            if np.any(prior != 0):
                if op.name in prior_names:   # the device uploads its extra rows' b itself
                    b_rows_all = max(b_rows_all or 0, data.size + end)
                elif op.name in sgrid_ops:   # eliminated grids: the device never sees their prior
                    b_rows_sg = max(b_rows_sg or 0, data.size + end)
                else:
                    b_rows = max(b_rows, data.size + end)
    keep_cols = reference_epoch_keep_cols(G_data.col_N, grids['dz'], args['reference_epoch'])
    timing['setup'] = time() - tic
    in_TSE = data.three_sigma_edit > 0.01 if 'three_sigma_edit' in data.fields else np.ones(G_data.N_eq, dtype=bool)
    if args['VERBOSE']:
        print('initial: %d:' % np.max(G_data.r), flush=True)
    if args['return_fit_objects']:
        out = {'data': data, 'G_data': G_data, 'Gc': Gc, 'grids': grids, 'Ed': Ed, 'Ec': Ec(),
               'prior_ops': prior_ops, 'rhs': rhs}
        if sgrid_sensor:   # what FitSystem(sensor_grids=) takes
            out['sensor_grids'] = sensor_grid_device_form(data, grids, sgrid_sensor, constraint_op_list)
        return out

    system = None
    try:
        if args['max_iterations'] > 0:
            tic = time()
            devices = args['devices'] if args['devices'] is not None else \
                [args['device'] + k for k in range(int(args['n_gpus']))]
            if len(devices) > 1:   # y-slab ranks on several devices of this process (lssurf_amd.dist)
                from .dist import MultiDeviceFitSystem
                if len(set(devices)) > 1:
                    warnings.warn('smooth_fit(n_gpus > 1) on distinct devices: the threaded device-group '
                                  'path (one RCCL communicator per device) has been tested only as ranks '
                                  'sharing one device; see INTEGRATION.md §5', RuntimeWarning, stacklevel=2)
                system = MultiDeviceFitSystem(G_data, Gc, keep_cols, Gc.col_N, devices)
            elif bias_model:
                system = _bias_fit_system(G_data, Gc, G_grid, Gc_grid, keep_cols, data, bias_model,
                                          bias_mode, grids, devices[0], args, prior_ops=prior_ops,
                                          sgrid=(sgrid_sensor, constraint_op_list) if sgrid_joint else None)
            elif has_sgrids and not prior_ops:
                system = _sgrid_fit_system(G_data, Gc, G_grid, Gc_grid, keep_cols, data, sgrid_sensor,
                                           constraint_op_list, sgrid_mode, grids, devices[0], args)
            else:
                # the dense (2) or band (5) preconditioner: LSQR on the stencil-formed system carries extra rows
                dense = args['lsq_precond'] in (2, 5) or (args['lsq_precond'] == 'auto' and
                                                          keep_cols.size <= args['lsq_dense_max'])
                system = FitSystem(G_data, Gc, keep_cols, Gc.col_N, device=devices[0], grids=grids,
                                   extra_ops=prior_ops, extra_mg=bool(args['lsq_prior_mg']) and bool(prior_ops),
                                   iterative=not dense, cg_chunks=args['lsq_cg_chunks'],
                                   tile_dmf=args['lsq_tile_eliminate'], cg_scaled=args['lsq_cg_scaled'])
            if b_rows_all is not None and not getattr(system, 'n_extra', 0):
                b_rows = max(b_rows, b_rows_all)
            if b_rows_sg is not None and getattr(system, 'sg', None) is None:
                b_rows = max(b_rows, b_rows_sg)
            system.b_rows = b_rows
            if has_sgrids:   # how the sensor bias grids ran
                timing['sensor_grids'] = 'eliminate' if getattr(system, 'sg', None) is not None else 'columns'
                timing['sgrid_joint'] = timing['sensor_grids'] == 'eliminate' and \
                    getattr(system, 'bias_ids', None) is not None
            timing['formation'] = getattr(system, 'formation', None)   # 'stencil' or 'coo'
            timing['extra_rows'] = int(getattr(system, 'n_extra', 0))  # prior rows the device holds as extra rows
            timing['device_setup'] = time() - tic
            tic_iteration = time()
            m0, sigma_extra, in_TSE, rs_data = iterate_fit(data, system, rhs, TCinv_diag, G_data, Gc, in_TSE,
                                                           timing, args, grids,
                                                           sigma_extra_masks=args['sigma_extra_masks'],
                                                           bias_model=bias_model)
            timing['iteration'] = time() - tic_iteration
            valid_data[valid_data] = in_TSE
            data.assign({'three_sigma_edit': in_TSE})
            data.assign({'sigma_extra': sigma_extra})
            x_c = getattr(system, 'last_x', None)   # m0[keep_cols], without the 10⁷-entry gather
            data.assign({'z_est': np.reshape(system.data_forward(x_c if x_c is not None else m0[keep_cols]),
                                             data.shape)})
            if args['mask_update_function'] is not None:
                averaging_ops = {}
                parse_model(m, m0, data, R, RMS, G_data, averaging_ops, Gc, Ec(), grids, args)
                args['mask_update_function'](grids, m, args)
            averaging_ops = setup_averaging_ops(grids['dz'], grids['dz'].col_N, args, grids['dz'].cell_area)
            averaging_ops.update(setup_z0_avg(grids, grids['dz'].col_N, args))
            averaging_ops.update(setup_avg_mask_ops(grids['dz'], G_data.col_N, args['avg_masks'], args['dzdt_lags']))
            parse_model(m, m0, data, R, RMS, G_data, averaging_ops, Gc, Ec, grids, args, system=system)
            if bias_model:   # the biases, in the order of the bias IDs (smooth_fit.py:309-310)
                m['bias'], m['slope_bias'] = parse_biases(m0, bias_model, args['bias_params'], data=data)
            tse = data.three_sigma_edit == 1
            r_data = data.z_est[tse] - data.z[tse]
            R['data'] = np.sum((r_data / data.sigma[tse]) ** 2)
            RMS['data'] = np.sqrt(np.mean(r_data ** 2))
        else:
            averaging_ops = setup_averaging_ops(grids['dz'], grids['dz'].col_N, args, grids['dz'].cell_area)
            averaging_ops.update(setup_z0_avg(grids, grids['dz'].col_N, args))
            averaging_ops.update(setup_avg_mask_ops(grids['dz'], G_data.col_N, args['avg_masks'], args['dzdt_lags']))
        if args['compute_E']:
            from .errors import calc_and_parse_errors
            if 'sigma_extra' not in data.fields:
                data.assign({'sigma_extra': np.zeros_like(data.sigma)})
                tse = data.three_sigma_edit == 1
                r_data = data.z_est[tse] - data.z[tse]
                data.sigma_extra[tse] = calc_sigma_extra(r_data, data.sigma[tse], np.ones(tse.sum(), dtype=bool))
            if args['VERBOSE']:
                print('Starting uncertainty calculation', flush=True)
                tic_error = time()
            calc_and_parse_errors(E, G_data, Gc, Ed, Ec(), data, in_TSE, keep_cols, grids, averaging_ops,
                                  device=args['device'], timing=timing, method=args['lsq_E_method'],
                                  bias_model=bias_model, bias_params=args['bias_params'],
                                  border_solve=bool(args['lsq_E_border_solve']) and bool(bias_model),
                                  grid_ops=(G_grid, Gc_grid) if bias_model and not has_sgrids else None,
                                  fit_args=args)
            if args['VERBOSE']:
                print('\tUncertainty propagation took %3.2f seconds' % (time() - tic_error), flush=True)
    finally:
        if system is not None:
            system.close()
    out = {'m': m, 'E': E, 'data': data, 'grids': grids, 'valid_data': valid_data, 'TOC': Gc.TOC, 'R': R,
           'RMS': RMS, 'timing': timing, 'E_RMS': args['E_RMS'], 'dzdt_lags': args['dzdt_lags']}
    if bias_model:   # beyond the reference's keys: the bias model, with the IDs edit_by_bias removed
        out['bias_model'] = bias_model
    return out


# re-exported for callers that build Ip_c explicitly (smooth_fit.py:624)
__all__ = ['smooth_fit', 'iterate_fit', 'parse_model', 'FitSystem', 'build_reference_epoch_matrix',
           'check_data_against_DEM']
