"""Host (numpy / scipy) block-Jacobi CGNR for the iterate tests of lsq method 1
(lssurf_amd/csrc/lsqr_cg.inc, block.hip): textbook PCG on AᵀA x = Aᵀb with M⁻¹ = R̃R̃ᵀ per column
block, R̃ = the upper R_b⁻¹ of (AᵀA)_bb = R_bᵀR_b rounded to bf16 as the device keeps it, written
from the definitions and run in float64 or in extended precision.  With the factors rounded alike,
the device's iterates differ from these by summation order alone.  Also the inputs (systems, masks,
weights, extra rows) that tests/test_cgnr_host.py and tests/test_gpu_cgnr_iterates.py share.
Test infrastructure only."""
import functools

import numpy as np
import scipy.sparse as sp


# ---- the reference ---------------------------------------------------------------------------
def bf16_round(a):
    """double -> float32 -> bf16 (round to nearest even on the 16 dropped bits), as float64."""
    f = np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))
    u = f.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(a))


def block_list(block_ptr, cols, n):
    """The blocks given plus one singleton per unlisted column (what lsq_set_column_blocks
    documents), grouped by size: a list of (n_blocks, k) arrays of column ids, each block's columns
    in the order given."""
    out = []
    listed = np.zeros(n, bool)
    if block_ptr is not None and len(block_ptr) > 1:
        bp, cols = np.asarray(block_ptr, np.int64), np.asarray(cols, np.int64)
        lens = np.diff(bp)
        assert np.unique(cols).size == cols.size, 'a column in two blocks'
        listed[cols] = True
        for k in np.unique(lens):
            b = np.flatnonzero(lens == k)
            out.append(cols[bp[b][:, None] + np.arange(k)[None, :]])
    single = np.flatnonzero(~listed)
    if single.size:
        out.append(single[:, None])
    assert sum(C.size for C in out) == n
    return out


MIN_PIVOT = 1e-8   # k_block_factor calls a column dead at d ≤ 1e-12·d0: no input may come near that


def block_factors(A, blocks, round=True):
    """[(C, R̃)] per block size: R̃ (n_blocks, k, k) the upper R_b⁻¹ of N_b = (AᵀA)_bb = R_bᵀR_b,
    rounded to bf16 when `round`."""
    return normal_factors((A.T @ A).tocsr(), blocks, round)


def normal_factors(N, blocks, round=True):
    """block_factors of a normal matrix N given as such (tests/mg_host.py: a multigrid level's)."""
    out = []
    for C in blocks:
        nb, k = C.shape
        if k == 1:
            Nb = N.diagonal()[C[:, 0]].reshape(nb, 1, 1)
        else:
            Nb = np.asarray(N[np.repeat(C, k, axis=1).ravel(), np.tile(C, (1, k)).ravel()]).reshape(nb, k, k)
        R = np.swapaxes(np.linalg.cholesky(Nb), 1, 2)                 # upper, N_b = RᵀR
        piv = np.einsum('bii->bi', R) ** 2 / np.einsum('bii->bi', Nb)
        assert piv.min() > MIN_PIVOT, f'pivot {piv.min():.3e}: too near the dead-column rule'
        Ri = np.triu(np.linalg.solve(R, np.broadcast_to(np.eye(k), (nb, k, k))))
        out.append((C, bf16_round(Ri) if round else Ri))
    return out


def jacobi_factors(A):
    """1×1 factors 1/‖A_j‖, unrounded (precond 1)."""
    nrm = np.sqrt(np.asarray(A.multiply(A).sum(axis=0)).ravel())
    assert nrm.min() > 0
    return [(np.arange(A.shape[1])[:, None], (1.0 / nrm).reshape(-1, 1, 1))]


def apply_minv(factors, s):
    """z = M⁻¹s = R̃(R̃ᵀs) block by block, in s's precision."""
    z = np.zeros_like(s)
    for C, Ri in factors:
        Ri = Ri.astype(s.dtype)
        y = (Ri * s[C][:, :, None]).sum(axis=1)        # R̃ᵀ s
        z[C] = (Ri * y[:, None, :]).sum(axis=2)        # R̃ y
    return z


def pcg(A, b, factors, iters, x0=None, dtype=np.float64):
    """PCG on AᵀA x = Aᵀb from x0 (0), x updated at every step.  Returns a dict: x (iters + 1, n)
    with x[k] the iterate after k steps, p (iters, n) the directions, alpha, beta (iters) and rho
    (iters + 1) = sᵀM⁻¹s."""
    A = sp.csr_matrix(A).astype(dtype)
    AT = A.T.tocsr()
    b = np.asarray(b).astype(dtype)
    x = np.zeros(A.shape[1], dtype) if x0 is None else np.asarray(x0).astype(dtype)
    s = AT @ (b - A @ x)
    z = apply_minv(factors, s)
    p = z.copy()
    rho = s @ z
    xs, ps, al, be, rh = [x.copy()], [], [], [], [rho]
    for _ in range(iters):
        t = A @ p
        alpha = rho / (t @ t)
        x = x + alpha * p
        s = s - alpha * (AT @ t)
        z = apply_minv(factors, s)
        rho_new = s @ z
        beta = rho_new / rho
        ps.append(p)
        p = z + beta * p
        rho = rho_new
        xs.append(x)
        al.append(alpha)
        be.append(beta)
        rh.append(rho)
    return dict(x=np.array(xs), p=np.array(ps), alpha=np.array(al), beta=np.array(be), rho=np.array(rh))


def stats_at(A, b, factors, x_k, x0, alphas, betas):
    """What the device estimates by recurrence, from the definitions, after k = len(alphas) steps:
    r1norm = ‖b − A x_k‖, arnorm = sqrt(sᵀM⁻¹s) with s = Aᵀ(b − A x_k), xnorm = ‖R̃⁻¹(x_k − x0)‖ (the
    correction in the preconditioned coordinates x = R̃y), anorm = sqrt(Σ_i 1/α_i + β_{i−1}/α_{i−1})."""
    r = b - A @ x_k
    s = A.T @ r
    d = x_k - (0 if x0 is None else x0)
    y2 = 0.0
    for C, Ri in factors:
        y = np.linalg.solve(Ri.astype(np.float64), d[C].astype(np.float64)[:, :, None])
        y2 += float((y ** 2).sum())
    al, be = np.asarray(alphas, np.float64), np.asarray(betas, np.float64)
    tr = (1.0 / al).sum() + (be[:-1] / al[:-1]).sum()
    return dict(r1norm=float(np.sqrt(r @ r)), arnorm=float(np.sqrt(s @ apply_minv(factors, s))),
                xnorm=float(np.sqrt(y2)), anorm=float(np.sqrt(tr)))


def at_risk_entries(Rinv_entries, eps=1e-11):
    """Entries whose bf16 rounding changes when the double moves by a relative eps: there a device
    R_b⁻¹ that agrees with the host's to rounding could round the other way."""
    v = np.asarray(Rinv_entries, np.float64).ravel()
    r = bf16_round(v)
    return int(np.count_nonzero((bf16_round(v * (1 + eps)) != r) | (bf16_round(v * (1 - eps)) != r)))


def factor_entries(factors):
    """The upper-triangle entries of every block of (unrounded) factors, one flat array."""
    return np.concatenate([Ri[:, np.triu_indices(Ri.shape[1])[0], np.triu_indices(Ri.shape[1])[1]].ravel()
                           for _, Ri in factors])


# ---- the inputs the CPU and GPU tests share ----------------------------------------------------
KS = (1, 2, 3, 4, 5, 7, 8, 9, 13)         # stops with 1, 2, 3 and no owed α p, in the first x cycle and later
KS9 = tuple(k for k in KS if k <= 9)
KSWEEP = [((9, 11), 300), ((7, 70), 600)]  # (ny, nx) nodes, points
KSWEEP_NT = (2, 3, 5, 8, 13)
MASK_SEED, X0_SEED, KSWEEP_SEED = 11, 13, 20260101
# tests/test_gpu_cgnr_tile.py: 16 and more epochs, where the CGNR operator leaves column mode.  (7, 70):
# two x tiles, rows no multiple of the tile's; (5, 200): x tiles clear of both edges; (9, 11): small
# enough for the dense oracle (15: the last column-mode size, 20: no CGNR operator at all)
TILE_SWEEP = [((7, 70), 600), ((5, 200), 900)]
TILE_NT = (16, 17, 19)
TILE_DENSE = ((9, 11), 300)
TILE_DENSE_NT = (16, 19, 20)
TILE_MASKED = [((5, 200), 19), ((7, 70), 16)]


class Host:
    """One smooth_fit system on the host: fit objects S, kept columns, row weights w, rhs, the node
    blocks (block_ptr, cols), and the weighted A with every row kept."""

    def __init__(self, S, reference_epoch):
        from lssurf_amd.constraint_functions import node_column_blocks, reference_epoch_keep_cols
        self.S = S
        self.keep_cols = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], reference_epoch)
        self.n_full = int(S['Gc'].col_N)
        self.n_data = int(S['data'].size)
        self.w = 1. / np.concatenate((S['Ed'], S['Ec']))
        self.rhs = np.zeros(self.w.size)
        self.rhs[:self.n_data] = S['data'].z
        self.blocks = node_column_blocks(S['grids'], self.keep_cols)

    @property
    def G(self):
        """unweighted [G_data; Gc] over the kept columns"""
        if getattr(self, '_G', None) is None:
            self._G = sp.vstack([self.S['G_data'].toCSR(), self.S['Gc'].toCSR()]).tocsc()[:, self.keep_cols].tocsr()
        return self._G

    def A(self, w=None, mask=None):
        """diag(w)·G, the rows of `mask` only: what get_csr() returns, up to rounding"""
        w = self.w if w is None else w
        A = sp.csr_matrix(sp.diags(w) @ self.G)
        return A if mask is None else A[np.flatnonzero(mask)]

    def fit_system(self, **kw):
        from lssurf_amd.smooth_fit import FitSystem
        S = self.S
        return FitSystem(S['G_data'], S['Gc'], self.keep_cols, self.n_full, grids=S['grids'], **kw)


@functools.lru_cache(maxsize=None)
def synthetic_host(name):
    import lssurf_amd as LS
    from lssurf_amd import synthetic
    D, kw = synthetic.points(name)
    return Host(LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw), kw['reference_epoch'])


@functools.lru_cache(maxsize=None)
def golden_host(name='sf3d'):
    import lssurf_amd as LS
    from conftest import golden, golden_kwargs, golden_points
    g = golden(f'sys_{name}.npz')
    kw = golden_kwargs(g)
    return Host(LS.smooth_fit(data=golden_points(g), return_fit_objects=True, **kw), kw['reference_epoch'])


def ksweep_points(shape, npts, nt):
    """(data, smooth_fit keywords) of a (ny, nx) lattice with nt epochs (node blocks of nt columns) and
    npts points, built as lssurf_amd.synthetic does (config_kwargs / points) with a seed of its own."""
    from lssurf_amd import containers as pc
    from lssurf_amd.synthetic import E_RMS_NOTEBOOK
    ny, nx = shape
    W = {'x': (nx - 1) * 100., 'y': (ny - 1) * 100., 't': (nt - 1) * 0.25}
    kw = dict(W=W, ctr={'x': 0., 'y': 0., 't': 0.}, spacing={'z0': 100., 'dz': 100., 'dt': 0.25},
              E_RMS=dict(E_RMS_NOTEBOOK), reference_epoch=nt // 2)
    rng = np.random.default_rng(KSWEEP_SEED + 1000 * ny + nt)
    x, y, t = ((rng.random(npts) - 0.5) * W[d] for d in ('x', 'y', 't'))
    z = 10 * np.sin(4 * np.pi * x / max(W['x'], 1.)) * np.cos(6 * np.pi * y / max(W['y'], 1.)) + 0.5 * t \
        + rng.normal(0, 0.1, npts)
    return pc.data().from_dict({'x': x, 'y': y, 'time': t, 'z': z, 'sigma': np.full(npts, 0.1)}), kw


@functools.lru_cache(maxsize=None)
def ksweep_host(shape, npts, nt):
    """The system of ksweep_points on the host."""
    import lssurf_amd as LS
    D, kw = ksweep_points(shape, npts, nt)
    return Host(LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw), kw['reference_epoch'])


def mask_and_weights(h):
    """The `t64-mask` case: data-row mask rng.random > 0.2, data weights × U(0.5, 2).
    Returns (row weights, row mask over every row)."""
    rng = np.random.default_rng(MASK_SEED)
    keep = rng.random(h.n_data) > 0.2
    w = h.w.copy()
    w[:h.n_data] *= rng.uniform(0.5, 2, h.n_data)
    return w, np.concatenate([keep, np.ones(h.w.size - h.n_data, bool)])


def warm_start(h):
    return 1e-2 * np.random.default_rng(X0_SEED).standard_normal(h.keep_cols.size)


def frame_priors(h, reference_epoch, sigma=1e-4):
    """The rows of tests/test_gpu_priors._frame_priors on h (t64): ((indptr, cols, vals), weights,
    priors) — one row per dz node of a 3-node edge frame and non-reference epoch, 1 at the node and
    −1 at its (removed) reference-epoch column."""
    gd = h.S['grids']['dz']
    ny, nx, nt = gd.shape
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    frame = (yy < 3) | (yy >= ny - 3) | (xx < 3) | (xx >= nx - 3)
    cols = []
    for y, x in zip(yy[frame], xx[frame]):
        for t in range(nt):
            if t != reference_epoch:
                cols += [gd.col_0 + np.ravel_multi_index((y, x, t), gd.shape),
                         gd.col_0 + np.ravel_multi_index((y, x, reference_epoch), gd.shape)]
    n = len(cols) // 2
    csr = (2 * np.arange(n + 1, dtype=np.int64), np.asarray(cols, np.int64), np.tile([1., -1.], n))
    return csr, np.full(n, 1. / sigma), 0.1 * np.random.default_rng(37).standard_normal(n)


def extra_rows_host(h, csr, wx):
    """diag(wx)·X over the kept columns (zeros dropped), as the device appends it behind A."""
    ip, cols, vals = csr
    X = sp.csr_matrix((vals, cols, ip), shape=(ip.size - 1, h.n_full))[:, h.keep_cols]
    Xw = sp.csr_matrix(sp.diags(wx) @ X)
    Xw.eliminate_zeros()
    return Xw


def rel(a, b):
    """‖a − b‖ / ‖b‖ in the operands' precision"""
    return float(np.sqrt(((a - b) ** 2).sum()) / np.sqrt((b ** 2).sum()))


BLOCK_CASES = ['t64', 't64-mask', 'sf3d', 't15', 't64z', 'priors'] + \
    [f'ksweep-{ny}x{nx}-{nt}' for (ny, nx), _ in KSWEEP for nt in KSWEEP_NT] + \
    [f'tile-{ny}x{nx}-{nt}' for (ny, nx), _ in TILE_SWEEP for nt in TILE_NT] + \
    [f'tile-{TILE_DENSE[0][0]}x{TILE_DENSE[0][1]}-{nt}' for nt in TILE_DENSE_NT] + \
    [f'tile-{ny}x{nx}-{nt}-mask' for (ny, nx), nt in TILE_MASKED]


def host_case(name):
    """(host, A, b, blocks) of a GPU case's system formed on the host: A weighted and row-selected,
    b = the weighted, selected rhs, blocks = block_list of the node blocks.  t64-mf, t64-csr, t64-x0
    and jacobi run on t64's system; a name that ends in -mask has mask_and_weights applied."""
    if name.startswith(('ksweep', 'tile')):
        shape, nt = name.split('-')[1:3]
        shape = tuple(int(v) for v in shape.split('x'))
        h = ksweep_host(shape, dict(KSWEEP + TILE_SWEEP + [TILE_DENSE])[shape], int(nt))
    elif name == 'sf3d':
        h = golden_host('sf3d')
    else:
        h = synthetic_host(name if name in ('t15', 't64z') else 't64')
    w, mask = mask_and_weights(h) if name.endswith('-mask') else (h.w, np.ones(h.w.size, bool))
    A, b = h.A(w, mask), (w * h.rhs)[mask]
    if name == 'priors':
        csr, wx, prior = frame_priors(h, h.S['grids']['dz'].shape[2] // 2)
        A, b = sp.vstack([A, extra_rows_host(h, csr, wx)]).tocsr(), np.r_[b, wx * prior]
    return h, A, b, block_list(*h.blocks, h.keep_cols.size)
