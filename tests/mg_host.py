"""Host (scipy) multigrid hierarchy for the GPU tests of precond 4 (lssurf_amd/csrc/mg.inc): the
same prolongation (bilinear in (y, x), coarse node a on fine node 2a, identity in t), Galerkin
stencil operators PᵀN_sP and (y, x)-lumped data operators, built from the formed A the device
returns.

On those levels, the V-cycle itself (VCycle), written from the definitions in mg.inc's header and
run in float64 or in extended precision: Chebyshev smoothing on M̃⁻¹N_ℓ with M̃⁻¹ = R̃R̃ᵀ per node block
and R̃ the upper R_b⁻¹ rounded to bf16 as the device keeps it (tests/cgnr_host.py), the unscaled
restriction Pᵀ(r − N x), x += P x_c, a dense solve over the kept columns of the coarsest level.  The
set-up's λ estimate (randvec, power_lambda), the true λ_max(M̃⁻¹N_ℓ) (lambda_max) and textbook PCG
with z = V(s) (pcg_v).  Test infrastructure only."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import cgnr_host as CH


def prolong1(nf, last_odd=0.5):
    """1-D prolongation fine (nf) <- coarse (nf // 2 + 1).  last_odd: the weights of a last row that
    is odd (0.5; the sensitivity tests put a wrong one there)."""
    nc = nf // 2 + 1
    r, c, v = [], [], []
    for i in range(nf):
        if i % 2 == 0:
            r.append(i)
            c.append(i // 2)
            v.append(1.0)
        else:
            r += [i, i]
            c += [(i - 1) // 2, (i + 1) // 2]
            v += [0.5, 0.5] if i < nf - 1 else [last_odd, last_odd]
    return sp.csr_matrix((v, (r, c)), shape=(nf, nc))


def prolong_full(ny, nx, nt, last_odd=0.5):
    """Full-space prolongation of the [z0 (ny·nx); dz (ny·nx·nt)] column layout."""
    Py, Px = prolong1(ny, last_odd), prolong1(nx, last_odd)
    P2 = sp.kron(Py, Px).tocsr()
    P3 = sp.kron(P2, sp.identity(nt)).tocsr()
    return sp.block_diag([P2, P3]).tocsr(), Py.shape[1], Px.shape[1]


def node_of(ny, nx, nt):
    nodes = np.arange(ny * nx)
    return np.concatenate([nodes, np.repeat(nodes, nt)])


def slot_of(ny, nx, nt):
    return np.concatenate([np.zeros(ny * nx, int), 1 + np.tile(np.arange(nt), ny * nx)])


def lump_by_node(D, node, slot):
    """Move entry (i, j) to (i, j') with j' = the column of node(i) holding slot(j)."""
    Dc = D.tocoo()
    n = D.shape[0]
    table = np.full((node.max() + 1, slot.max() + 1), -1)
    table[node, slot] = np.arange(n)
    jn = table[node[Dc.row], slot[Dc.col]]
    ok = jn >= 0
    return sp.csr_matrix((Dc.data[ok], (Dc.row[ok], jn[ok])), shape=D.shape)


def hierarchy(A, n_data_rows, keep_cols, ny, nx, nt, coarse=5, coarse_cols=1024,   # mg.inc MG_COARSE, MG_COARSE_COLS
              parts=False):
    """Levels [(shape, keep_mask_full, N_operator_full)] with N over each level's FULL column
    space (rows / columns of removed epochs zero).  Level 0: AᵀA; coarse: Galerkin stencil part +
    lumped data part.  parts: a fourth entry per level, the lumped data part B alone (level 0: None)."""
    n_full = ny * nx * (1 + nt)
    keep = np.zeros(n_full, bool)
    keep[keep_cols] = True
    E = sp.csr_matrix((np.ones(keep_cols.size), (keep_cols, np.arange(keep_cols.size))),
                      shape=(n_full, keep_cols.size))       # compact -> full
    Ad, As = A[:n_data_rows], A[n_data_rows:]
    Ns = (E @ (As.T @ As) @ E.T).tocsr()
    Nd = (E @ (Ad.T @ Ad) @ E.T).tocsr()
    levels = [((ny, nx), keep, (Ns + Nd).tocsr()) + ((None,) if parts else ())]
    while max(ny, nx) > coarse and not (len(levels) > 1 and ny * nx * (1 + nt) <= coarse_cols):
        P, nyc, nxc = prolong_full(ny, nx, nt)
        Ns = (P.T @ Ns @ P).tocsr()
        Nd = lump_by_node((P.T @ Nd @ P).tocsr(), node_of(nyc, nxc, nt), slot_of(nyc, nxc, nt))
        kc = np.concatenate([np.ones(nyc * nxc, bool), np.tile(keep[ny * nx:ny * nx + nt], nyc * nxc)])
        Dk = sp.diags(kc.astype(float))
        ny, nx, keep = nyc, nxc, kc
        levels.append(((ny, nx), keep, (Dk @ (Ns + Nd) @ Dk).tocsr()) + (((Dk @ Nd @ Dk).tocsr(),) if parts else ()))
    return levels


# ---- the V-cycle -----------------------------------------------------------------------------
def level_blocks(shape, keep, nt):
    """(nodes, k) full column ids of a level's node blocks: z0, then the kept epochs ascending."""
    nn = shape[0] * shape[1]
    kt = np.flatnonzero(keep[nn:nn + nt])
    nodes = np.arange(nn)[:, None]
    return np.concatenate([nodes, nn + nodes * nt + kt[None, :]], axis=1)


def level_factors(levels, nt, round=True):
    """Per smoothing level [(C, R̃)] (cgnr_host.normal_factors of the level's node blocks, from the
    float64 operator), None for the coarsest."""
    return [CH.normal_factors(sp.csr_matrix(N).astype(np.float64), [level_blocks(shape, keep, nt)], round)
            for shape, keep, N, *_ in levels[:-1]] + [None]


def cheb(lam, step):
    """(c1, c2) of Chebyshev step `step` on [0.11 λ, 1.1 λ] (Saad, Alg. 12.1; mg_smooth_body)."""
    lmax = 1.1 * lam
    lmin = 0.1 * lmax
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    c1, c2 = 0.0, 1.0 / theta
    for _ in range(step):
        rn = 1.0 / (2.0 * sigma - rho)
        c1, c2 = rn * rho, 2.0 * rn / delta
        rho = rn
    return c1, c2


def refined_solve(M, b, passes=4):
    """M⁻¹b in b's precision: a float64 Cholesky factor, refined with residuals in b's precision
    (np.linalg has no extended precision)."""
    cf = scipy.linalg.cho_factor(np.asarray(M, np.float64))
    x = np.zeros_like(b)
    for _ in range(passes):
        x = x + scipy.linalg.cho_solve(cf, np.asarray(b - M @ x, np.float64)).astype(b.dtype)
    return x


class VCycle:
    """x = V_l(r) on the levels of hierarchy(..., parts=True), in the precision of their operators.
    lam: λ per smoothing level; deg0 / deg: the Chebyshev degree on level 0 / below.  `wrong` names one
    deliberate defect (tests/test_mg_host.py: each must move V(u)):
      pre_d0        pre-smoothing step 1 takes d = 0 for the previous direction, not d = x₁
      post_restart  post-smoothing step 1 takes step 0's coefficients
      drop_bx       B x missing from the residual a coarse level restricts
      prolong_last  the prolongation's weights at a last odd row 1 instead of 0.5
      coarsest_ref  the coarsest solve carries the removed epoch's column as a copy of its neighbour
                    epoch's instead of leaving it out"""

    def __init__(self, levels, factors, nt, lam, deg0=2, deg=1, wrong=None):
        self.levels, self.factors, self.nt, self.lam = levels, factors, nt, list(lam)
        self.deg0, self.deg, self.wrong = deg0, deg, wrong
        self.dtype = levels[0][2].dtype
        self.P = []
        for (ny, nx), *_ in levels[:-1]:
            self.P.append(prolong_full(ny, nx, nt)[0].astype(self.dtype))
        self.Pup = self.P if wrong != 'prolong_last' else \
            [prolong_full(ny, nx, nt, last_odd=1.0)[0].astype(self.dtype) for (ny, nx), *_ in levels[:-1]]
        shape, keep, N = levels[-1][:3]
        self.kc = np.flatnonzero(keep)
        if wrong == 'coarsest_ref':
            nn = shape[0] * shape[1]
            tref = int(np.flatnonzero(~keep[nn:nn + nt])[0])
            jr = nn + np.arange(nn) * nt + tref
            jn = jr + (1 if tref + 1 < nt else -1)
            T = sp.csr_matrix((np.ones(nn), (jn, jr)), shape=N.shape).astype(self.dtype)
            IT = sp.identity(N.shape[0], dtype=self.dtype, format='csr') + T
            D = sp.csr_matrix((N.diagonal()[jn], (jr, jr)), shape=N.shape)
            self.Nc = (IT.T @ N @ IT + D).toarray()
            self.kc = np.arange(N.shape[0])
        else:
            self.Nc = N[self.kc][:, self.kc].toarray()

    def minv(self, l, s):
        return CH.apply_minv(self.factors[l], s)

    def __call__(self, r, l=0):
        r = np.asarray(r).astype(self.dtype)
        shape, keep, N = self.levels[l][:3]
        if l == len(self.levels) - 1:
            x = np.zeros_like(r)
            x[self.kc] = refined_solve(self.Nc, r[self.kc])
            return np.where(keep, x, 0)
        lam, deg = self.lam[l], (self.deg if l else self.deg0)
        c1, c2 = cheb(lam, 0)
        x = d = c2 * self.minv(l, r)                    # step 0 from x = 0: d₀ = x₁
        for k in range(1, deg):
            c1, c2 = cheb(lam, k)
            if k == 1 and self.wrong == 'pre_d0':
                d = np.zeros_like(x)
            d = c1 * d + c2 * self.minv(l, r - N @ x)
            x = x + d
        Nres = N - self.levels[l][3] if (l and self.wrong == 'drop_bx') else N
        rc = np.where(self.levels[l + 1][1], self.P[l].T @ (r - Nres @ x), 0)
        x = x + self.Pup[l] @ self(rc, l + 1)
        d = np.zeros_like(x)
        for k in range(deg):
            c1, c2 = cheb(lam, 0 if (k == 1 and self.wrong == 'post_restart') else k)
            d = c1 * d + c2 * self.minv(l, r - N @ x)
            x = x + d
        return x


# ---- the set-up's λ ----------------------------------------------------------------------------
def randvec(shape, keep, nt):
    """k_mg_randvec: the splitmix-style hash of each column's id in the level's own full layout,
    mapped to [−1, 1); 0 on the removed epoch."""
    n = shape[0] * shape[1] * (1 + nt)
    with np.errstate(over='ignore'):
        h = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x632BE59BD9B4E019)
        h ^= h >> np.uint64(31)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(29)
    v = (h >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0
    return np.where(keep, v, 0.0)


MG_POW = 20   # mg.inc


def power_lambda(level, factors, nt, steps=MG_POW, dtype=np.float64):
    """The set-up's estimate of λ_max(M̃⁻¹N) (mg_setup_rest, k_mg_power_scalar): from w = randvec, per
    step x = (1 + scal)·w, w = M̃⁻¹N x, s1 = x·N x, s2 = w·N x, scal = 1/√s2 − 1 (x is M-normalised
    from the second step on); λ = the largest s1 of the steps ≥ 1."""
    shape, keep, N = level[:3]
    N = N.astype(dtype)
    w = randvec(shape, keep, nt).astype(dtype)
    scal, lam = dtype(0.0), dtype(0.0)
    for k in range(steps):
        x = w + scal * w
        q = N @ x
        w = CH.apply_minv(factors, q)
        s1, s2 = x @ q, w @ q
        lam = dtype(0.0) if k == 0 else max(lam, s1)
        scal = 1.0 / np.sqrt(s2) - 1.0
    return lam


def lambda_max(level, factors, tol=1e-7):
    """The largest eigenvalue of R̃ᵀ N R̃ (= λ_max(M̃⁻¹N)), by Lanczos."""
    shape, keep, N = level[:3]
    (C, Ri), = factors
    n = N.shape[0]

    def op(v):
        z = np.zeros(n)
        z[C] = (Ri * v.reshape(C.shape)[:, None, :]).sum(axis=2)      # R̃ v
        q = N @ z
        return (Ri * q[C][:, :, None]).sum(axis=1).ravel()           # R̃ᵀ q

    A = spla.LinearOperator((C.size, C.size), matvec=op, dtype=np.float64)
    return float(spla.eigsh(A, k=1, which='LA', tol=tol, v0=np.ones(C.size))[0][0])


def pcg_v(A, b, V, iters, x0=None, dtype=np.float64):
    """Textbook PCG on AᵀA x = Aᵀb with z = V(s) (V: on the system's columns); x (iters + 1, n)."""
    A = sp.csr_matrix(A).astype(dtype)
    AT = A.T.tocsr()
    b = np.asarray(b).astype(dtype)
    x = np.zeros(A.shape[1], dtype) if x0 is None else np.asarray(x0).astype(dtype)
    s = AT @ (b - A @ x)
    z = V(s)
    p = z.copy()
    rho = s @ z
    xs = [x.copy()]
    for _ in range(iters):
        t = A @ p
        alpha = rho / (t @ t)
        x = x + alpha * p
        s = s - alpha * (AT @ t)
        z = V(s)
        rho_new = s @ z
        p = z + (rho_new / rho) * p
        rho = rho_new
        xs.append(x)
    return np.array(xs)


class System:
    """One case on the host: its levels in float64 and the same operators held in extended precision
    (the two runs of the cycle differ by their arithmetic alone), the rounded factors, cycles on demand."""

    def __init__(self, A, n_data_rows, keep_cols, shape3):
        ny, nx, nt = shape3
        self.nt, self.keep_cols = nt, np.asarray(keep_cols)
        lev = hierarchy(A, n_data_rows, keep_cols, ny, nx, nt, parts=True)
        self.lev = {np.float64: lev,
                    np.longdouble: [(s, k, N.astype(np.longdouble), None if B is None else B.astype(np.longdouble))
                                    for s, k, N, B in lev]}
        self.factors = level_factors(self.lev[np.float64], nt)
        self.n_full = ny * nx * (1 + nt)

    def cycle(self, lam, dtype=np.longdouble, factors=None, **kw):
        return VCycle(self.lev[dtype], self.factors if factors is None else factors, self.nt, lam, **kw)

    def host_lambda(self, dtype=np.float64):
        """the mirror's λ of every smoothing level"""
        return [power_lambda(lv, f, self.nt, dtype=dtype) for lv, f in zip(self.lev[np.float64][:-1], self.factors)]

    all_lambda = host_lambda

    def level_lambda_max(self, l, tol=1e-7):
        return lambda_max(self.lev[np.float64][l], self.factors[l], tol)

    def compact(self, V):
        """V on the system's (kept) columns"""
        def Vc(s):
            u = np.zeros(self.n_full, s.dtype)
            u[self.keep_cols] = s
            return V(u)[self.keep_cols]
        return Vc


class MixedSystem:
    """z0 on a 2× refinement of the dz lattice (mgx_vcycle; columns: z0 (fy·fx), then dz): the fine
    level is the system itself, smoothed on its z0 columns only by Chebyshev-Jacobi with
    D = diag(AᵀA), unrounded; the coarse correction x += P₀V_X(P₀ᵀ(r − N x)) comes from the system
    Galerkin-projected onto the dz lattice by P₀ = (bilinear on z0, the identity on dz), an ordinary
    System.  Level 0 here is the fine level, level l ≥ 1 is level l − 1 of `sub`."""

    def __init__(self, A, n_data_rows, keep_cols, zshape, shape3):
        (fy, fx), (ny, nx, nt) = zshape, shape3
        self.nz, nn = fy * fx, ny * nx
        self.n_full, self.nt, self.keep_cols = self.nz + nn * nt, nt, np.asarray(keep_cols)
        self.keep = np.zeros(self.n_full, bool)
        self.keep[keep_cols] = True
        assert self.keep[:self.nz].all()
        E = sp.csr_matrix((np.ones(keep_cols.size), (keep_cols, np.arange(keep_cols.size))),
                          shape=(self.n_full, keep_cols.size))
        A = sp.csr_matrix(A)
        Py, Px = prolong1(fy), prolong1(fx)
        assert (Py.shape[1], Px.shape[1]) == (ny, nx)
        self.P0 = sp.block_diag([sp.kron(Py, Px), sp.identity(nn * nt)]).tocsr()       # full <- dz lattice
        self.keep_sub = np.concatenate([np.ones(nn, bool), self.keep[self.nz:]])
        ksub = np.flatnonzero(self.keep_sub)
        self.sub = System((A @ E.T @ self.P0).tocsc()[:, ksub].tocsr(), n_data_rows, ksub, shape3)
        N = (E @ (A.T @ A) @ E.T).tocsr()
        self.N = {np.float64: N, np.longdouble: N.astype(np.longdouble)}
        self.dinv = 1.0 / N.diagonal()[:self.nz]
        self.lev = {dt: [((fy, fx), self.keep, self.N[dt], None)] + self.sub.lev[dt] for dt in self.N}

    def host_lambda(self, dtype=np.float64, steps=MG_POW):
        """[λ of the fine level], all the device exposes (mg_setup_mixed: the hash of the z0 column's
        index, x scaled as (scal + 1)·w)"""
        N = self.N[np.float64][:self.nz, :self.nz].astype(dtype)
        dinv = self.dinv.astype(dtype)
        x = randvec((1, self.nz), np.ones(self.nz, bool), 0).astype(dtype)
        lam = dtype(0.0)
        for k in range(steps):
            q = N @ x
            w = dinv * q
            s1, s2 = x @ q, w @ q
            lam = dtype(0.0) if k == 0 else max(lam, s1)
            x = (1.0 / np.sqrt(s2) - 1.0 + 1.0) * w
        return [lam]

    def all_lambda(self, dtype=np.float64):
        """the fine level's λ, then the dz-lattice levels''"""
        return self.host_lambda(dtype) + self.sub.host_lambda(dtype)

    def level_lambda_max(self, l, tol=1e-7):
        if l:
            return self.sub.level_lambda_max(l - 1, tol)
        s = np.sqrt(self.dinv)
        N = self.N[np.float64][:self.nz, :self.nz]
        A = spla.LinearOperator((self.nz, self.nz), matvec=lambda v: s * (N @ (s * v)), dtype=np.float64)
        return float(spla.eigsh(A, k=1, which='LA', tol=tol, v0=np.ones(self.nz))[0][0])

    def cycle(self, lam, dtype=np.longdouble, deg0=2, deg=1):
        """lam: the fine level's λ, then the dz-lattice levels'"""
        Vsub = self.sub.cycle(lam[1:], dtype, deg0=deg0, deg=deg)
        N, P0, dinv, nz = self.N[dtype], self.P0.astype(dtype), self.dinv.astype(dtype), self.nz

        def V(r, l=0):
            if l:
                return Vsub(r, l - 1)
            r = np.asarray(r).astype(dtype)
            x = np.zeros_like(r)
            d = np.zeros(nz, dtype)
            for k in range(deg0):
                c1, c2 = cheb(lam[0], k)
                d = c1 * d + c2 * dinv * (r - N @ x)[:nz]
                x[:nz] += d
            x = x + P0 @ Vsub(np.where(self.keep_sub, P0.T @ (r - N @ x), 0))
            d = np.zeros(nz, dtype)
            for k in range(deg0):
                c1, c2 = cheb(lam[0], k)
                d = c1 * d + c2 * dinv * (r - N @ x)[:nz]
                x[:nz] += d
            return x
        return V

    compact = System.compact


# ---- the cases tests/test_mg_host.py and tests/test_gpu_mg_vcycle.py share ------------------------
LATTICES = {'7x70-8': ((7, 70), 600, 8),        # three levels, 70 → 36 → 19: elongated, even and odd sizes
            '5x200-13': ((5, 200), 900, 13),    # 13 slots: the unfused restriction, the BJ_LANES smoother
            '23x38-3': ((23, 38), 900, 3),      # level 1 (960 columns) is the coarsest by MG_COARSE_COLS
            '33x33-5': ((33, 33), 1200, 5)}     # odd sizes down to 5
CASES = list(LATTICES) + ['t64', 't64-mask', 't64z']
U_SEED = 41


def case_host(name):
    """(cgnr_host.Host, row weights, row mask over every row, (ny, nx, nt)) of a case"""
    h = CH.ksweep_host(*LATTICES[name]) if name in LATTICES else CH.synthetic_host('t64z' if name == 't64z' else 't64')
    w, mask = CH.mask_and_weights(h) if name.endswith('-mask') else (h.w, np.ones(h.w.size, bool))
    return h, w, mask, tuple(int(v) for v in h.S['grids']['dz'].shape)


def case_system(name, A=None):
    """System of a case from A (None: the host-formed one)"""
    h, w, mask, shape3 = case_host(name)
    A = h.A(w, mask) if A is None else A
    if name == 't64z':
        return MixedSystem(A, h.n_data, h.keep_cols, tuple(int(v) for v in h.S['grids']['z0'].shape), shape3)
    return System(A, int(mask[:h.n_data].sum()), h.keep_cols, shape3)


def test_vectors(keep, count=2, seed=U_SEED):
    """`count` standard normal vectors on the kept columns of a level (0 elsewhere)"""
    rng = np.random.default_rng(seed + keep.size)
    return [np.where(keep, rng.standard_normal(keep.size), 0.0) for _ in range(count)]
