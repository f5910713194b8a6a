// mg.inc — precond 4: a geometric multigrid V-cycle as the CGNR preconditioner (method 1).
// Included at the end of lsqr_cg.inc's anonymous namespace (namespace lsq).
//
// Why: block-Jacobi PCG needs ~600 iterations at C4 and the count grows with the grid (349 at
// 512², 621 at 1024²): the smoothness constraints make AᵀA a high-order elliptic operator whose
// smooth error modes a node-local preconditioner cannot reach.  A V-cycle over the (y, x) node
// lattice removes them on coarse grids; the CPU prototype (tools/mg_proto.py) needs 36 PCG
// iterations at 64² and at 256² (block-Jacobi: 480 / 583).
//
// Levels ℓ = 0 (the system) … L−1 halve the (y, x) lattice of smooth_fit's z0 and dz grids
// (S → S/2 + 1, coarse node a sits on fine node 2a), keeping t.  The prolongation P_ℓ is
// bilinear in (y, x), the identity in t and per grid, so it maps kept columns onto kept columns
// (the reference epoch's dz columns stay removed on every level).  Coarse operators:
//   stencil rows — Galerkin N_{ℓ+1} = P_ℓᵀ N_ℓ P_ℓ of the normal-stencil class table, computed
//                  exactly on the host (ns_galerkin): again a class table, applied by the same
//                  ring kernel (k_cg_normal_col + k_cg_xedge) as the fine level;
//   data rows    — lumped over (y, x) neighbours: per node the (z0, dz(t)) block
//                  B_ℓ[m] = Σ_points rs² w_m^ℓ(p) τ τᵀ, τ = (1, …, 1−f_t, f_t, …) the point's z0 and
//                  epoch weights, w_m^ℓ its bilinear weight at node m of level ℓ (Ad·P is exactly
//                  the level-ℓ interpolation, so B_ℓ is the row-sum lumping of its Galerkin data
//                  term; prototype: 36 vs 32 iterations with the exact term).  B_ℓ is an arrow +
//                  tridiagonal (t) block: 3·nt doubles per node.
//   extra rows   — (lsq_set_extra_rows_lumping) exact on level 0 (k_xr_fwd / k_xr_atq); below, each
//                  row is a (y, x) weight times a τ with a z0 entry and two adjacent epochs, lumped
//                  into B_1 like a data row (k_mg_lump_xr) and restricted with it.
// Smoother: Chebyshev of degree MG_DEG0 (level 0) / MG_DEG (coarse levels) on M_ℓ⁻¹N_ℓ, M_ℓ = the per-node blocks of N_ℓ (level 0:
// the block-Jacobi factors of precond 3, fp32 R_b⁻¹), interval [λ/10, 1.1 λ] with λ the Rayleigh
// quotient of MG_POW power steps in the M inner product.  Coarsest level (≤ MG_COARSE nodes per
// side): dense Cholesky inverse.  The same polynomial before and after the coarse correction
// makes the V-cycle symmetric positive definite, so it is a valid PCG preconditioner.
//
// Vectors live in each level's FULL column space (grids in the system's column order), so the
// restriction / prolongation kernels index grids directly; removed columns stay 0.

}  // namespace  (lsqr_cg.inc's; the hierarchy types live in lsq: System holds an MgHier*)

struct MgGeom {   // one level's column layout
    int32_t S0, S1, nt, tref;    // node lattice, dz epochs (0: no dz grid), removed epoch (−1: none)
    int32_t has_z, pad;
    int64_t colz, cold, nodes, n_full;
    FastDiv fd_s1, fd_nt;        // 32-bit divisions by S1 and nt (an int64 division is ~100 instructions)
};
struct MgSlots {  // node block slots (every level): t of slot s (−1: z0), slots of t−1 / t+1
    int32_t t[16], lo[16], hi[16];
    int32_t zs, nt;              // z0 slot (−1: none), epochs
};
struct MgTab {    // one grid's class table on the device (tile layout)
    int32_t on, S0, S1, S2, K0, K1, K2, n0, n1, n2, noff, coef0;
    int32_t od[5];               // index of offset (0, 0, dt), dt = −2..2 (−1: absent)
    int32_t hy, hx, ht;          // stencil half-widths
};

struct MgMix {    // z0 on a 2× refinement of the dz lattice (mg_build_mixed): the system's layout
    int32_t z0col, dzcol, Sf0, Sf1, Sc0, Sc1, nt, tref;
    int64_t nz, nsz;             // z0 columns (fine nodes); dz-lattice nodes
};

struct MgTk {     // k_mg_tile_kt: per grid, its compressed interior-class row in MgLevel::tkc
    int32_t c0[MF_MAX_GRIDS];    // first coefficient (grid order of the level's CgDesc)
};

struct MgLevel {
    MgGeom geo{};
    BlkAffine aff{};
    std::vector<NsTable> ns;     // per system grid (same indices)
    MgTab tz{}, td{};            // z0 / dz tables (device view)
    CgDesc cgh{};
    DBuf<CgDesc> cgd;
    DBuf<double> coef, coefc;    // tile table (all grids) / column-mode table
    DBuf<int32_t> offs;          // coarsest: offsets [grid z0: noff×3][grid dz: noff×3]
    int gN = 0, gB = 0;          // normal-kernel / block-kernel grids
    DBuf<double> B;              // ℓ ≥ 1: lumped data per node
    DBuf<double> vz;             // ℓ ≥ 1, field-valued z0 parts: Galerkin 5×5 (dy, dx) row per z0 node
    DBuf<double> Ri;             // ℓ ≥ 1: packed (AᵀA)_bb -> R_b⁻¹ (fp64 scratch)
    DBuf<lf_t> Lf;               // ℓ ≥ 1: R_b⁻¹ (lf_t)
    DBuf<int64_t> ptr;           // ℓ ≥ 1: block pointers b·kslot
    DBuf<double> x, r, q, d, res, part;
    bool coarsest = false;
    bool direct = false;         // small level: k_mg_direct instead of the ring kernel + x-edge pass
    bool tile = false;           // ℓ ≥ 1: k_mg_tile (MG_T² node tiles) instead of both
    int tile_grid = 0;           // k_mg_tile: workgroups (the tiles of every grid), LDS bytes
    size_t tile_lds = 0;
    // k_mg_tile_kt (round 5): the interior class row with the taps of each (dy, dx) group stored once
    // per dim-2 boundary class (5 rows for 12 epochs, K2 = 2) instead of once per t; 0 = k_mg_tile
    int tile_kt = 0;             // 1: coefficients by scalar loads, 2: staged in LDS
    MgTk tk{};
    DBuf<double> tkc;
    size_t tk_lds = 0;
    int64_t npad = 0;
    DBuf<double> dN, dRi, tmp;
    // a rank's partitioned coarse level (1 ≤ ℓ ≤ MgHier::lp): the vectors stay global (every rank
    // holds the whole level), the rank computes its owned node rows [oa, ob) only and exchanges
    // boundary rows with its neighbours (hb: pack / receive buffers of both sides)
    int32_t oa = 0, ob = 0;
    DBuf<double> hb;
};

struct MgHier {
    ~MgHier() {
        if (rg) (void)hipGraphExecDestroy(rg);
    }
    // a rank's replicated coarse levels (below the partitioned ones, no exchange inside): their
    // V-cycle captured once as a hipGraph and replayed (mg_vcycle_graph); level rg_l
    hipGraphExec_t rg = nullptr;
    int rg_l = -1;
    bool rg_failed = false;
    std::vector<MgLevel> lev;
    MgSlots sl{};
    int kslot = 0, nt = 0, tref = -1, nbB = 2, withz = 0, gz = -1, gd = -1;
    int deg0 = 2, deg = 1;       // Chebyshev degree on level 0 / on coarse levels (MG_DEG0, MG_DEG; env overrides)
    int deg0_pre = 2;            // level 0's pre-smoothing degree (LSQ_MG_DEG0_PRE, development: ≠ deg0
                                 // makes the V-cycle non-symmetric)
    int fuse = 5;                // bit 0: the first smoothing step in the CG update; bit 2: the
                                 // restriction inside the next level's first smoothing step
                                 // (k_mg_restrict_smooth, round 6: C4 solve 0.1158 → 0.1143 s, c4y8
                                 // 0.0421 → 0.0417 s, bitwise equal; `profiles/r06_mg_rsfuse_ab.txt`)
                                 // (LSQ_MG_FUSE, masked with 5)
    DBuf<double> lam;            // λ estimate per level
    DBuf<double> scal;           // op-kernel β (power steps: scale − 1; V-cycle: 0)
    DBuf<CgState> mst;           // stop = 0: the set-up ops run regardless of the solve's state
    DBuf<double> part1, part2, part_t;
    DBuf<double> part_x;         // level 0 with lumped extra rows: k_xr_fwd's partials (scratch)
    DBuf<double> d0, res0;       // level-0 Chebyshev direction and residual
    bool var = false;            // field-valued z0 parts (k_cg_var2d on level 0, MgLevel::vz below)
    DBuf<double> part_v;         // their level-0 partials (scratch)
    // a rank of a distributed solve (mg_build_dist): level 0 is the rank's window (owned node rows
    // ± halo rows; its operator partial, completed by the halos), levels ≥ 1 are the GLOBAL coarse
    // levels, replicated on every rank (identical tables, lumped data all-reduced once per solve)
    bool dist = false;
    int32_t wa = 0, oa = 0, ob = 0;   // global node rows: window start, owned [oa, ob)
    int lp = 0;                  // levels 1 … lp partitioned over the ranks (MgLevel::oa / ob), the rest replicated
    MgGeom g0g{};                // the global level-0 geometry (column layout for hashing)
    DBuf<int> err;
    DBuf<unsigned long long> ndead;
    // z0 on a 2× refinement of the dz lattice (mg_build_mixed): no levels here — this level is the
    // system itself (its exact operator: stencil rows + stored data rows), smoothed on its z0
    // columns by Chebyshev-Jacobi; the coarse correction is the shared-lattice hierarchy of S.mx
    // (z0 restricted bilinearly, dz unchanged: every dz component is corrected there)
    bool mixed = false;
    MgMix mix{};
    DBuf<double> xdinv, xpart;   // 1 / diag(N) of the z0 columns; operator partial scratch
    MgTab xtz{}, xtd{};          // S.mx level 0's class tables (tile layout) for its exact node blocks
    DBuf<double> xcoef, xB, xRi;
    DBuf<int64_t> xptr;
};

void mg_free(MgHier* h) { delete h; }
void mg_graph_drop(MgHier* H) {
    if (H && H->rg) {
        (void)hipGraphExecDestroy(H->rg);
        H->rg = nullptr;
        H->rg_l = -1;
    }
}

namespace {

// Chebyshev degree of each pre- and post-smoothing: level 0 (LSQ_MG_DEG0) and the coarse levels
// (LSQ_MG_DEG).  C4 (iterations / solve): 2/2 45 / 0.182 s, 2/1 47 / 0.152 s, 1/1 65 / 0.153 s,
// 3/1 42 / 0.177 s, 3/2 41 / 0.206 s — degree 1 halves the coarse levels' latency-bound launches
// for two more iterations.
constexpr int MG_DEG0 = 2, MG_DEG = 1;
// Power steps per level for λ_max(M⁻¹N).  A Chebyshev smoother on [0.11 λ, 1.1 λ] contracts only
// below 2θ = 1.21 λ, so the estimate must reach λ_max / 1.21.  λ_max / λ after 10, 16, 20 steps (host
// Lanczos against the device's λ, tests/test_gpu_mg_vcycle.py): t256 level 2 1.42, 1.17, 1.12; t64 with
// edited rows level 0 1.24, 1.13, 1.05; a 5 × 200 lattice level 0 1.23, 1.20, 1.18 (the worst at 20).
// 10 → 20: C4 set-up 11.5 → 18.0 ms per solve (solve 117 ms, 47 iterations either way), t64 52 → 53
// and t256 55 → 56 iterations (the wider interval).
constexpr int MG_POW = 20;
constexpr int MG_COARSE = 5;     // coarsest level: at most this many nodes per side
// … or at most this many columns (LSQ_MG_COARSE_COLS; round 6): an elongated lattice — a rank's
// y-slab window, the notebooks' x-t strips — reaches ≤ 5 rows long before ≤ 5 columns, and each
// level between costs ~7 latency-bound launches for a few hundred columns; a dense inverse of ≤ 1 k
// columns is one GEMV.  Square lattices (C4: 9² × 13 = 1 053 columns) keep the ≤ 5-per-side rule.
constexpr int64_t MG_COARSE_COLS = 1024;
constexpr int64_t MG_DIRECT = 1 << 18;   // levels with at most this many columns: k_mg_direct (LSQ_MG_DIRECT)
constexpr int64_t MG_TILE_MIN = 1 << 16; // levels with more columns: k_mg_tile + k_mg_edge (LSQ_MG_TILE)
constexpr int MG_NB_MAX = 48;    // lumped data doubles per node (3·nt, nt ≤ 16)
constexpr int MG_XZERO = 1, MG_RES = 2, MG_POWER = 4, MG_RHO = 8;   // k_mg_smooth modes
constexpr int MG_DX = 16;        // step 1 after a zero start: the previous direction is x itself
constexpr int MG_NOD = 32;       // last step: the direction is not stored
constexpr int MG_NEEDD = 64;     // the step reads the previous direction d (set by mg_launch_smooth)

// ---- device helpers --------------------------------------------------------------------------

__device__ __forceinline__ void mg_decode(const MgGeom& G, int64_t c, int64_t& node, int& t) {
    if (G.has_z && c >= G.colz && c < G.colz + G.nodes) {
        node = c - G.colz;
        t = -1;
        return;
    }
    const int64_t e = c - G.cold;
    node = fdiv((uint32_t)e, G.fd_nt);
    t = (int)(e - node * G.nt);
}
__device__ __forceinline__ int64_t mg_col(const MgGeom& G, int64_t node, int t) {
    return t < 0 ? G.colz + node : G.cold + node * G.nt + t;
}

// r_c = P_ℓᵀ res_f: each coarse column gathers the ≤ 3×3 fine nodes of its prolongation support.
// qf non-null (level 0, whose operator has no lumped block): res_f = rf − qf; qf null (coarse
// levels): rf is the residual of the smoother's MG_RES pass.
// MG_RU columns per thread and loop trip, their gathers issued together (one column per trip left
// the level-0 restriction and prolongation latency-bound at ~2.8 TB/s)
#ifndef MG_RU_DEF
#define MG_RU_DEF 4
#endif
constexpr int MG_RU = MG_RU_DEF;   // -DMG_RU_DEF=…: A/B builds
__global__ __launch_bounds__(BLOCK) void k_mg_restrict(const CgState* __restrict__ st, MgGeom F, MgGeom C,
                                                       const double* __restrict__ rf, const double* __restrict__ qf,
                                                       double* __restrict__ rc) {
    if (st->stop) return;
    const int bid = blockIdx.x, nblk = gridDim.x;
    const int64_t stride = (int64_t)nblk * BLOCK;
    for (int64_t c0 = (int64_t)bid * BLOCK + threadIdx.x; c0 < C.n_full; c0 += MG_RU * stride) {
        double acc[MG_RU];
#pragma unroll
        for (int u = 0; u < MG_RU; ++u) {
            const int64_t c = c0 + u * stride;
            acc[u] = 0.0;
            if (c >= C.n_full) continue;
            int64_t node;
            int t;
            mg_decode(C, c, node, t);
            if (t >= 0 && t == C.tref) continue;
            const int y = (int)fdiv((uint32_t)node, C.fd_s1), x = (int)(node - (int64_t)y * C.S1);
            for (int dy = -1; dy <= 1; ++dy) {
                const int fy = 2 * y + dy;
                if (fy < 0 || fy >= F.S0) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int fx = 2 * x + dx;
                    if (fx < 0 || fx >= F.S1) continue;
                    const int64_t fc = mg_col(F, (int64_t)fy * F.S1 + fx, t);
                    acc[u] += ((dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0)) * (qf ? rf[fc] - qf[fc] : rf[fc]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < MG_RU; ++u)
            if (c0 + u * stride < C.n_full) rc[c0 + u * stride] = acc[u];
    }
}

// x_f += P_ℓ x_c: each fine column gathers its ≤ 2×2 coarse parents
__global__ __launch_bounds__(BLOCK) void k_mg_prolong(const CgState* __restrict__ st, MgGeom F, MgGeom C,
                                                      const double* __restrict__ xc, double* __restrict__ xf) {
    if (st->stop) return;
    const int bid = blockIdx.x, nblk = gridDim.x;
    const int64_t stride = (int64_t)nblk * BLOCK;
    for (int64_t c0 = (int64_t)bid * BLOCK + threadIdx.x; c0 < F.n_full; c0 += MG_RU * stride) {
        double acc[MG_RU], xo[MG_RU];
        bool on[MG_RU];
#pragma unroll
        for (int u = 0; u < MG_RU; ++u) {
            const int64_t c = c0 + u * stride;
            acc[u] = xo[u] = 0.0;
            on[u] = false;
            if (c >= F.n_full) continue;
            int64_t node;
            int t;
            mg_decode(F, c, node, t);
            if (t >= 0 && t == F.tref) continue;
            on[u] = true;
            xo[u] = xf[c];
            const int y = (int)fdiv((uint32_t)node, F.fd_s1), x = (int)(node - (int64_t)y * F.S1);
            const int ya = y >> 1, xa = x >> 1, ny = (y & 1) ? 2 : 1, nx = (x & 1) ? 2 : 1;
            const double wy = (y & 1) ? 0.5 : 1.0, wx = (x & 1) ? 0.5 : 1.0;
            for (int a = 0; a < ny; ++a)
                for (int b = 0; b < nx; ++b) acc[u] += (wy * wx) * xc[mg_col(C, (int64_t)(ya + a) * C.S1 + xa + b, t)];
        }
#pragma unroll
        for (int u = 0; u < MG_RU; ++u)
            if (on[u]) xf[c0 + u * stride] = xo[u] + acc[u];
    }
}

// Ranks (mg_build_dist): level 0 is the window F (global node rows wa + local), level 1 the global
// coarse level C.  Restriction of the OWNED fine rows [oa, ob) into the global coarse vector rows
// [ca, cb) (the whole vector: every rank writes all of it, the other rows 0, and the ranks' vectors
// are summed; a partitioned coarse level: the rows the owned fine rows reach, [oa_c − 1, ob_c + 1),
// whose ghost rows go to their owners by a reverse halo).  A partitioned fine level F (global
// storage) passes wa = 0 and its residual as rf (qf null).
__global__ __launch_bounds__(BLOCK) void k_mg_restrict_win(const CgState* __restrict__ st, MgGeom F, MgGeom C, int wa,
                                                           int oa, int ob, const double* __restrict__ rf,
                                                           const double* __restrict__ qf, double* __restrict__ rc,
                                                           int ca, int cb) {
    if (st->stop) return;
    const int64_t n_rows = C.has_z ? (int64_t)(cb - ca) * C.S1 * (1 + C.nt) : (int64_t)(cb - ca) * C.S1 * C.nt;
    for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < n_rows; k += (int64_t)gridDim.x * BLOCK) {
        // k → a column of rows [ca, cb): the z0 block's rows first, then the dz block's
        const int64_t nzr = C.has_z ? (int64_t)(cb - ca) * C.S1 : 0;
        const int64_t c = k < nzr ? C.colz + (int64_t)ca * C.S1 + k : C.cold + (int64_t)ca * C.S1 * C.nt + (k - nzr);
        int64_t node;
        int t;
        mg_decode(C, c, node, t);
        double acc = 0.0;
        if (!(t >= 0 && t == C.tref)) {
            const int y = (int)fdiv((uint32_t)node, C.fd_s1), x = (int)(node - (int64_t)y * C.S1);
            for (int dy = -1; dy <= 1; ++dy) {
                const int gy = 2 * y + dy;
                if (gy < oa || gy >= ob) continue;
                const int fy = gy - wa;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int fx = 2 * x + dx;
                    if (fx < 0 || fx >= F.S1) continue;
                    const int64_t fc = mg_col(F, (int64_t)fy * F.S1 + fx, t);
                    acc += ((dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0)) * (qf ? rf[fc] - qf[fc] : rf[fc]);
                }
            }
        }
        rc[c] = acc;
    }
}

// x_f += P x_c on the window columns of global rows [fa, fb) (replicated coarse level: every window
// row, the coarse x being the same on every rank; partitioned: the owned rows, the coarse rows they
// reach refreshed by a forward halo first).  A partitioned fine level passes wa = 0.
__global__ __launch_bounds__(BLOCK) void k_mg_prolong_win(const CgState* __restrict__ st, MgGeom F, MgGeom C, int wa,
                                                          const double* __restrict__ xc, double* __restrict__ xf, int fa,
                                                          int fb) {
    if (st->stop) return;
    for (int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x; c < F.n_full; c += (int64_t)gridDim.x * BLOCK) {
        int64_t node;
        int t;
        mg_decode(F, c, node, t);
        if (t >= 0 && t == F.tref) continue;
        const int ly = (int)fdiv((uint32_t)node, F.fd_s1), x = (int)(node - (int64_t)ly * F.S1), y = ly + wa;
        if (y < fa || y >= fb) continue;
        const int ya = y >> 1, xa = x >> 1, ny = (y & 1) ? 2 : 1, nx = (x & 1) ? 2 : 1;
        const double wy = (y & 1) ? 0.5 : 1.0, wx = (x & 1) ? 0.5 : 1.0;
        double acc = 0.0;
        for (int a = 0; a < ny; ++a)
            for (int b = 0; b < nx; ++b) acc += (wy * wx) * xc[mg_col(C, (int64_t)(ya + a) * C.S1 + xa + b, t)];
        xf[c] += acc;
    }
}

// Field-valued z0 rows: a rank's partial level-0 rows (its window, its own centres) → their
// Galerkin rows on the GLOBAL level 1 (partial; the ranks' are summed)
__global__ __launch_bounds__(BLOCK) void k_mg_var_galerkin_win(int S0w, int S1f, int wa, int S0c, int S1c,
                                                               const double* __restrict__ Nf, double* __restrict__ Nc) {
    const int64_t nodes = (int64_t)S0c * S1c;
    for (int64_t a = (int64_t)blockIdx.x * BLOCK + threadIdx.x; a < nodes; a += (int64_t)gridDim.x * BLOCK) {
        const int ay = (int)(a / S1c), ax = (int)(a - (int64_t)ay * S1c);
        double acc[25];
#pragma unroll
        for (int k = 0; k < 25; ++k) acc[k] = 0.0;
        for (int dy = -1; dy <= 1; ++dy) {
            const int iy = 2 * ay + dy, ly = iy - wa;   // global fine row, window row
            if (ly < 0 || ly >= S0w) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int ix = 2 * ax + dx;
                if (ix < 0 || ix >= S1f) continue;
                const double wi = (dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0);
                const double* Ni = Nf + ((int64_t)ly * S1f + ix) * 25;
                for (int d = 0; d < 25; ++d) {
                    const double v = Ni[d];
                    if (v == 0.0) continue;
                    const int jy = iy + d / 5 - 2, jx = ix + d % 5 - 2;
                    if (jy < 0 || jx < 0 || jx >= S1f) continue;
                    const int nby = (jy & 1) ? 2 : 1, nbx = (jx & 1) ? 2 : 1;
                    const double py = (jy & 1) ? 0.5 : 1.0, px = (jx & 1) ? 0.5 : 1.0;
                    for (int u = 0; u < nby; ++u)
                        for (int w = 0; w < nbx; ++w) {
                            const int ey = (jy >> 1) + u - ay, ex = (jx >> 1) + w - ax;
                            acc[(ey + 2) * 5 + ex + 2] += (wi * v) * (py * px);
                        }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 25; ++k) Nc[a * 25 + k] = acc[k];
    }
}

// Level-1 lumped data blocks from the level-0 points (sorted by fine cell): one lane per coarse
// node of a row strip; the points of the node's ≤ 4×4 fine cells are four runs of the sorted
// order; accumulators in LDS [entry][lane] (the epoch index varies per point).
// B[m] = [Σc, Σc τ_t (t < nt), Σc τ_t² (t < nt), Σc τ_t τ_{t+1} (t < nt−1)], c = rs² w_m(p).
// wa > 0 (a rank): the points are the rank's window (fine rows wa + local), the coarse level global
__global__ __launch_bounds__(64) void k_mg_lump1(DmfDesc D, const int32_t* __restrict__ cell,
                                                 const double4* __restrict__ pt, int S0c, int S1c, int nt, int nbB,
                                                 int withz, double* __restrict__ B, int wa) {
    __shared__ double LA[MG_NB_MAX * 64];
    const int lane = threadIdx.x;
    const int nsx = (S1c + 63) / 64;
    const int a = blockIdx.x / nsx, b = (blockIdx.x - a * nsx) * 64 + lane;
    const bool mine = a < S0c && b < S1c;
    for (int k = 0; k < nbB; ++k) LA[k * 64 + lane] = 0.0;
    if (mine) {
        const int C0 = D.S0 - 1, C1 = D.S1 - 1;   // fine cells per dim
        const int xlo = max(2 * b - 2, 0), xhi = min(2 * b + 1, C1 - 1);
        for (int ry = max(2 * a - 2 - wa, 0); ry <= min(2 * a + 1 - wa, C0 - 1) && xlo <= xhi; ++ry) {
            const int p0 = cell[ry * C1 + xlo], p1 = cell[ry * C1 + xhi + 1];
            for (int i = p0; i < p1; ++i) {
                const double4 P = pt[i];
                double fy, fx;
                const int cy = dmf_cell(0.5 * (P.x + (double)wa), S0c, fy), cx = dmf_cell(0.5 * P.y, S1c, fx);
                const double wy = cy == a ? 1.0 - fy : (cy + 1 == a ? fy : 0.0);
                const double wx = cx == b ? 1.0 - fx : (cx + 1 == b ? fx : 0.0);
                const double cc = (P.w * P.w) * (wy * wx);
                if (cc == 0.0) continue;
                if (withz) LA[lane] += cc;
                if (nt) {
                    double ft;
                    const int ct = dmf_cell(P.z, D.S2, ft);
                    const double at = 1.0 - ft;
                    if (withz) {
                        LA[(1 + ct) * 64 + lane] += cc * at;
                        LA[(2 + ct) * 64 + lane] += cc * ft;
                    }
                    LA[(1 + nt + ct) * 64 + lane] += cc * (at * at);
                    LA[(2 + nt + ct) * 64 + lane] += cc * (ft * ft);
                    LA[(1 + 2 * nt + ct) * 64 + lane] += cc * (at * ft);
                }
            }
        }
        for (int k = 0; k < nbB; ++k) B[((int64_t)a * S1c + b) * nbB + k] = LA[k * 64 + lane];
    }
}

// The extra rows' share of the level-1 blocks (lsq_set_extra_rows_lumping; xr_lump.hpp): a row is a
// (y, x) weight times an epoch vector τ with a z0 entry and at most two adjacent epochs (t, t + 1),
// i.e. a data row with its own τ_z, so it lumps into the same layout:
//   B[m] += Σ_r rs_r² w¹_{m,r} · [τ_z², τ_z τ_t, τ_t², τ_t τ_{t+1}]
// over the transpose of the touched level-1 nodes (rows ascending inside a node).  Launched after
// k_mg_lump1 wrote B; k_mg_restrict_b then carries the sum to the levels below.  One row's share of
// node accumulators acc[entry · 64 + lane] in LDS (the epoch varies per row):
__device__ __forceinline__ void mg_lump_xr_row(double* __restrict__ acc, int lane, double c, const double4 T, int nt,
                                               int has_z) {
    const int t = (int)T.w;
    if (has_z) acc[lane] += c * (T.x * T.x);
    if (nt) {
        const bool two = t + 1 < nt;
        if (has_z) {
            acc[(1 + t) * 64 + lane] += c * (T.x * T.y);
            if (two) acc[(2 + t) * 64 + lane] += c * (T.x * T.z);
        }
        acc[(1 + nt + t) * 64 + lane] += c * (T.y * T.y);
        if (two) {
            acc[(2 + nt + t) * 64 + lane] += c * (T.z * T.z);
            acc[(1 + 2 * nt + t) * 64 + lane] += c * (T.y * T.z);
        }
    }
}

// one lane per touched node (the nodes over XR_LONG rows are left to k_mg_lump_xr_long); the 64
// nodes of a workgroup are then added to B node by node, entry k by lane k
__global__ __launch_bounds__(64) void k_mg_lump_xr(int64_t nln, const int32_t* __restrict__ ln,
                                                   const int64_t* __restrict__ lp, const int32_t* __restrict__ lr,
                                                   const double* __restrict__ lw, const double4* __restrict__ lt,
                                                   const double* __restrict__ rs, int nt, int nbB, int has_z,
                                                   double* __restrict__ B) {
    __shared__ double LA[MG_NB_MAX * 64];
    __shared__ int32_t LN[64];
    const int lane = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    for (int k = 0; k < nbB; ++k) LA[k * 64 + lane] = 0.0;
    int32_t node = -1;
    if (j < nln) {
        const int64_t a = lp[j], e = lp[j + 1];
        if (e - a <= XR_LONG) {
            node = ln[j];
            for (int64_t k = a; k < e; ++k) {
                const int32_t r = lr[k];
                const double s = rs[r];
                mg_lump_xr_row(LA, lane, (s * s) * lw[k], lt[r], nt, has_z);
            }
        }
    }
    LN[lane] = node;
    __syncthreads();
    if (lane < nbB)
        for (int i = 0; i < 64; ++i) {
            const int32_t m = LN[i];
            if (m >= 0) B[(int64_t)m * nbB + lane] += LA[lane * 64 + i];
        }
}

// a wave per long node: lane l adds entries l, l + 64, … in row order, then the fixed shuffle tree
// per block entry
__global__ __launch_bounds__(64) void k_mg_lump_xr_long(int64_t nlong, const int32_t* __restrict__ longn,
                                                        const int32_t* __restrict__ ln, const int64_t* __restrict__ lp,
                                                        const int32_t* __restrict__ lr, const double* __restrict__ lw,
                                                        const double4* __restrict__ lt, const double* __restrict__ rs,
                                                        int nt, int nbB, int has_z, double* __restrict__ B) {
    __shared__ double LA[MG_NB_MAX * 64];
    const int lane = threadIdx.x;
    if ((int64_t)blockIdx.x >= nlong) return;
    const int32_t j = longn[blockIdx.x];
    for (int k = 0; k < nbB; ++k) LA[k * 64 + lane] = 0.0;
    const int64_t e = lp[j + 1];
    for (int64_t k = lp[j] + lane; k < e; k += 64) {
        const int32_t r = lr[k];
        const double s = rs[r];
        mg_lump_xr_row(LA, lane, (s * s) * lw[k], lt[r], nt, has_z);
    }
    double mine = 0.0;
    for (int k = 0; k < nbB; ++k) {
        const double s = wave_sum(LA[k * 64 + lane]);
        if (lane == k) mine = s;
    }
    if (lane < nbB) B[(int64_t)ln[j] * nbB + lane] += mine;
}

// B_{ℓ+1}[m] = Σ_n P_nm B_ℓ[n] (lumping of a lumped block field: exact restriction)
__global__ __launch_bounds__(BLOCK) void k_mg_restrict_b(int S0f, int S1f, int S0c, int S1c, int nbB,
                                                         const double* __restrict__ Bf, double* __restrict__ Bc) {
    const int64_t total = (int64_t)S0c * S1c * nbB;
    for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < total; q += (int64_t)gridDim.x * BLOCK) {
        const int64_t node = q / nbB;
        const int k = (int)(q - node * nbB);
        const int y = (int)(node / S1c), x = (int)(node - (int64_t)y * S1c);
        double acc = 0.0;
        for (int dy = -1; dy <= 1; ++dy) {
            const int fy = 2 * y + dy;
            if (fy < 0 || fy >= S0f) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int fx = 2 * x + dx;
                if (fx < 0 || fx >= S1f) continue;
                acc += ((dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0)) * Bf[((int64_t)fy * S1f + fx) * nbB + k];
            }
        }
        Bc[q] = acc;
    }
}

// Field-valued z0 parts on the multigrid levels: N_v = A_vᵀW²A_v is a per-node 5×5 (dy, dx)
// stencil on the z0 lattice (templates within ±1), stored row-wise (25 doubles per node, offset
// (dy + 2)·5 + dx + 2).  Level 0 (k_mg_var_n0, scratch) from the fields; level ℓ+1 = PᵀN_ℓP
// (k_mg_var_galerkin, exact, closed on ±2); applied on the coarse levels by k_mg_var_apply.
constexpr int MG_VN = 25;
__global__ __launch_bounds__(BLOCK) void k_mg_var_n0(CgVar V, double* __restrict__ N) {
    const int64_t nodes = (int64_t)V.S0 * V.S1;
    const int W1 = V.hi1 - V.lo1;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < nodes; i += (int64_t)gridDim.x * BLOCK) {
        const int y = (int)(i / V.S1), x = (int)(i - (int64_t)y * V.S1);
        double* Ni = N + i * MG_VN;
        for (int e1 = 0; e1 < V.ntpl; ++e1) {
            const int cy = y - V.oy[e1], cx = x - V.ox[e1];
            if (cy < V.lo0 || cy >= V.hi0 || cx < V.lo1 || cx >= V.hi1) continue;
            const int64_t k = (int64_t)(cy - V.lo0) * W1 + (cx - V.lo1);
            const double a1 = V.w * (V.val[e1] * V.F[V.fsel[e1] * V.n_eq + k]);
            for (int e2 = 0; e2 < V.ntpl; ++e2) {
                const double a2 = V.w * (V.val[e2] * V.F[V.fsel[e2] * V.n_eq + k]);
                Ni[(V.oy[e2] - V.oy[e1] + 2) * 5 + (V.ox[e2] - V.ox[e1] + 2)] += a1 * a2;
            }
        }
    }
}

// Nc = PᵀNf P per coarse node (P: coarse a on fine 2a, ½ on the odd neighbours — mg_parents)
__global__ __launch_bounds__(BLOCK) void k_mg_var_galerkin(int S0f, int S1f, int S0c, int S1c,
                                                           const double* __restrict__ Nf, double* __restrict__ Nc) {
    const int64_t nodes = (int64_t)S0c * S1c;
    for (int64_t a = (int64_t)blockIdx.x * BLOCK + threadIdx.x; a < nodes; a += (int64_t)gridDim.x * BLOCK) {
        const int ay = (int)(a / S1c), ax = (int)(a - (int64_t)ay * S1c);
        double acc[MG_VN];
#pragma unroll
        for (int k = 0; k < MG_VN; ++k) acc[k] = 0.0;
        for (int dy = -1; dy <= 1; ++dy) {
            const int iy = 2 * ay + dy;
            if (iy < 0 || iy >= S0f) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int ix = 2 * ax + dx;
                if (ix < 0 || ix >= S1f) continue;
                const double wi = (dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0);
                const double* Ni = Nf + ((int64_t)iy * S1f + ix) * MG_VN;
                for (int d = 0; d < MG_VN; ++d) {
                    const double v = Ni[d];
                    if (v == 0.0) continue;
                    const int jy = iy + d / 5 - 2, jx = ix + d % 5 - 2;
                    if (jy < 0 || jy >= S0f || jx < 0 || jx >= S1f) continue;
                    const int by0 = jy >> 1, bx0 = jx >> 1;
                    const int nby = (jy & 1) ? 2 : 1, nbx = (jx & 1) ? 2 : 1;
                    const double py = (jy & 1) ? 0.5 : 1.0, px = (jx & 1) ? 0.5 : 1.0;
                    for (int u = 0; u < nby; ++u)
                        for (int w = 0; w < nbx; ++w) {
                            const int ey = by0 + u - ay, ex = bx0 + w - ax;   // |e| ≤ 2 (closed)
                            acc[(ey + 2) * 5 + ex + 2] += (wi * v) * (py * px);
                        }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < MG_VN; ++k) Nc[a * MG_VN + k] = acc[k];
    }
}

// q[z0 node] += Σ_e N[node][e] p[node + e], p = z + β p_old (p_old may be null)
__global__ __launch_bounds__(BLOCK) void k_mg_var_apply(const CgState* __restrict__ st, MgGeom G,
                                                        const double* __restrict__ N, const double* __restrict__ z,
                                                        const double* __restrict__ pold,
                                                        const double* __restrict__ betap, double* __restrict__ q) {
    if (st->stop) return;
    const double beta = betap ? *betap : st->beta;
    for (int64_t a = (int64_t)blockIdx.x * BLOCK + threadIdx.x; a < G.nodes; a += (int64_t)gridDim.x * BLOCK) {
        const int y = (int)fdiv((uint32_t)a, G.fd_s1), x = (int)(a - (int64_t)y * G.S1);
        const double* Na = N + a * MG_VN;
        double acc = 0.0;
        for (int d = 0; d < MG_VN; ++d) {
            const int yy = y + d / 5 - 2, xx = x + d % 5 - 2;
            if (yy < 0 || yy >= G.S0 || xx < 0 || xx >= G.S1) continue;
            const int64_t j = G.colz + (int64_t)yy * G.S1 + xx;
            acc += Na[d] * (pold ? z[j] + beta * pold[j] : z[j]);
        }
        q[G.colz + a] += acc;
    }
}

__device__ __forceinline__ const double* mg_row(const MgTab& T, const double* coef, int y, int x, int t) {
    const int cy = cg_cls(y, T.S0, T.K0, T.n0), cx = cg_cls(x, T.S1, T.K1, T.n1), ct = cg_cls(t, T.S2, T.K2, T.n2);
    return coef + T.coef0 + ((int64_t)(cy * T.n1 + cx) * T.n2 + ct) * T.noff;
}

// (AᵀA)_bb of coarse node blocks (packed upper by columns, e = j(j+1)/2 + i): the node's
// stencil diagonal block from the class tables plus its lumped data block
__global__ __launch_bounds__(BLOCK) void k_mg_block_build(int64_t nodes, int S1, int kslot, MgSlots sl, int nbB,
                                                          MgTab tz, MgTab td, const double* __restrict__ coef,
                                                          const double* __restrict__ B, const double* __restrict__ vz,
                                                          double* __restrict__ Ri) {
    const int npk = kslot * (kslot + 1) / 2, nt = sl.nt;
    for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < nodes * npk; q += (int64_t)gridDim.x * BLOCK) {
        const int64_t node = q / npk;
        const int e = (int)(q - node * npk);
        int j = 0;
        while ((j + 1) * (j + 2) / 2 <= e) ++j;
        const int i = e - j * (j + 1) / 2;
        const int y = (int)(node / S1), x = (int)(node - (int64_t)y * S1);
        int si = -1, sj = -1;
        for (int s = 0; s < 16; ++s) {
            if (s == i) si = sl.t[s];
            if (s == j) sj = sl.t[s];
        }
        const double* Bn = B + node * nbB;
        double v = 0.0;
        if (si < 0 && sj < 0) {
            if (tz.on) v += mg_row(tz, coef, y, x, 0)[tz.od[2]];
            if (vz) v += vz[node * MG_VN + 12];
            v += Bn[0];
        } else if (si < 0 || sj < 0) {
            v += Bn[1 + (si < 0 ? sj : si)];
        } else {
            const int dt = sj - si;
            if (td.on && dt >= -2 && dt <= 2 && td.od[dt + 2] >= 0) v += mg_row(td, coef, y, x, si)[td.od[dt + 2]];
            if (dt == 0) v += Bn[1 + nt + si];
            else if (dt == 1 || dt == -1) v += Bn[1 + 2 * nt + min(si, sj)];
        }
        Ri[q] = v;
    }
}

// Coarsest level: the dense N over its full column space (identity on removed columns and on the
// padding), one thread per row
__global__ __launch_bounds__(BLOCK) void k_mg_dense_build(int64_t npad, MgGeom G, MgTab tz, MgTab td,
                                                          const int32_t* __restrict__ offz,
                                                          const int32_t* __restrict__ offd,
                                                          const double* __restrict__ coef,
                                                          const double* __restrict__ B, int nbB,
                                                          const double* __restrict__ vz,
                                                          double* __restrict__ N) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < npad; i += (int64_t)gridDim.x * BLOCK) {
        double* row = N + i * npad;
        if (i >= G.n_full) {
            row[i] = 1.0;
            continue;
        }
        int64_t node;
        int t;
        mg_decode(G, i, node, t);
        if (t >= 0 && t == G.tref) {
            row[i] = 1.0;
            continue;
        }
        const int y = (int)fdiv((uint32_t)node, G.fd_s1), x = (int)(node - (int64_t)y * G.S1), tt = t < 0 ? 0 : t;
        const MgTab& T = t < 0 ? tz : td;
        const int32_t* off = t < 0 ? offz : offd;
        if (T.on) {
            const double* cr = mg_row(T, coef, y, x, tt);
            for (int o = 0; o < T.noff; ++o) {
                const int yy = y + off[3 * o], xx = x + off[3 * o + 1], t2 = tt + off[3 * o + 2];
                if (yy < 0 || yy >= G.S0 || xx < 0 || xx >= G.S1 || t2 < 0 || t2 >= T.S2) continue;
                if (t >= 0 && t2 == G.tref) continue;
                row[mg_col(G, (int64_t)yy * G.S1 + xx, t < 0 ? -1 : t2)] += cr[o];
            }
        }
        if (t < 0 && vz)
            for (int d = 0; d < MG_VN; ++d) {
                const int yy = y + d / 5 - 2, xx = x + d % 5 - 2;
                if (yy >= 0 && yy < G.S0 && xx >= 0 && xx < G.S1) row[mg_col(G, (int64_t)yy * G.S1 + xx, -1)] += vz[node * MG_VN + d];
            }
        const double* Bn = B + node * nbB;
        const int nt = G.nt;
        if (t < 0) {
            row[i] += Bn[0];
            for (int t2 = 0; t2 < nt; ++t2)
                if (t2 != G.tref) row[mg_col(G, node, t2)] += Bn[1 + t2];
        } else {
            if (G.has_z) row[mg_col(G, node, -1)] += Bn[1 + t];
            row[i] += Bn[1 + nt + t];
            if (t + 1 < nt && t + 1 != G.tref) row[mg_col(G, node, t + 1)] += Bn[1 + 2 * nt + t];
            if (t - 1 >= 0 && t - 1 != G.tref) row[mg_col(G, node, t - 1)] += Bn[1 + 2 * nt + t - 1];
        }
    }
}

// Smoother / residual / power step over the node blocks of one level (lane layout of k_cg_block:
// kslot lanes per block, 64 / kslot blocks per wave, the wave's fp32 factors and lumped data rows
// staged in LDS, block values exchanged through the wave's LDS row).  For column c of a block:
//   resid = r − q − (B x)  (q = N_s x from the ring kernel; B only on coarse levels; XZERO: r)
//   RES:   res = resid
//   POWER: resid = q + B x (= N x); d = M⁻¹ resid; partials x·resid, d·resid
//   else:  z = M⁻¹ resid; d = c1 d + c2 z (Chebyshev step `step`); x += d; RHO: partial r·x
// CM ≥ 0: the mode as a compile-time constant (the hot V-cycle modes: every load of a block step
// issues together; runtime mode flags left the r/q, x/d and factor loads in three dependent
// rounds behind branch joins — 200 µs per level-0 pass against 170 for the larger CG update)
template <bool HB>
struct MgSmoothLds {   // k_mg_smooth's wave slices: factors, lumped blocks, block exchange row
    double LR[BLOCK / 64][2 * BJ_NPK_MAX];
    double LB[HB ? BLOCK / 64 : 1][HB ? 4 * 64 : 1];
    double SX[BLOCK / 64][64 + BJ_LANES];
};
// RS (XZERO only): the block's right-hand side is formed here, r_c = P_ℓᵀ res_f from the finer level
// RF (res_f = rf − qf; qf null: rf) by mg_restrict_col, and stored to rw — the restriction and the
// level's first smoothing step in one launch (MgHier::fuse bit 2)
__device__ __forceinline__ double mg_restrict_col(const MgGeom& F, const MgGeom& C, int64_t c,
                                                  const double* __restrict__ rf, const double* __restrict__ qf) {
    int64_t node;
    int t;
    mg_decode(C, c, node, t);
    double acc = 0.0;
    if (t >= 0 && t == C.tref) return acc;
    const int y = (int)fdiv((uint32_t)node, C.fd_s1), x = (int)(node - (int64_t)y * C.S1);
    for (int dy = -1; dy <= 1; ++dy) {   // the order and weights of k_mg_restrict
        const int fy = 2 * y + dy;
        if (fy < 0 || fy >= F.S0) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int fx = 2 * x + dx;
            if (fx < 0 || fx >= F.S1) continue;
            const int64_t fc = mg_col(F, (int64_t)fy * F.S1 + fx, t);
            const double res = qf ? rf[fc] - qf[fc] : rf[fc];
            acc += ((dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0)) * res;
        }
    }
    return acc;
}
struct MgRestrictSrc {
    MgGeom F, C;
    const double *rf, *qf;
    double* rw;
};
template <int K, bool HB, int CM, bool RS = false>   // K: loop length ≥ kslot (12 or BJ_LANES); HB: lumped data blocks (levels ≥ 1)
__device__ __forceinline__ void mg_smooth_body(int64_t nb, int npks, const BlkAffine& aff, int kslot, const MgSlots& sl,
                                               int nbB, const lf_t* __restrict__ Lf, const double* __restrict__ B,
                                               const double* __restrict__ r, const double* __restrict__ q,
                                               double* __restrict__ x, double* __restrict__ d,
                                               double* __restrict__ res, const double* __restrict__ lam, int mode,
                                               int step, double* __restrict__ part, double* __restrict__ part2,
                                               const uint8_t* __restrict__ live, MgSmoothLds<HB>& sm,
                                               const MgRestrictSrc* rs = nullptr) {
    auto& LR = sm.LR;
    auto& LB = sm.LB;
    auto& SX = sm.SX;
    const int bid = blockIdx.x, nblk = gridDim.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int L = kslot, W = 64 / L;
    const int grp = lane / L, j = lane - grp * L, gbase = grp * L;
    if (lane < BJ_LANES) SX[wv][64 + lane] = 0.0;
    int64_t abase = 0, astride = 0;
    int tj = -1, lo = -1, hi = -1;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i == j) {
            abase = aff.base[i];
            astride = aff.stride[i];
            tj = sl.t[i];
            lo = sl.lo[i];
            hi = sl.hi[i];
        }
    const int md = CM >= 0 ? CM : mode;
    const bool xz = md & MG_XZERO, power = md & MG_POWER, resonly = md & MG_RES;
    double c1 = 0.0, c2 = 0.0;   // Chebyshev step `step` on [λ/10, 1.1 λ] (Saad, Alg. 12.1)
    if (!power && !resonly) {
        const double lmax = 1.1 * lam[0], lmin = 0.1 * lmax;
        const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
        double rho = 1.0 / sigma;
        c2 = 1.0 / theta;
        for (int k = 1; k <= step; ++k) {
            const double rn = 1.0 / (2.0 * sigma - rho);
            c1 = rn * rho;
            c2 = 2.0 * rn / delta;
            rho = rn;
        }
    }
    const int nt = sl.nt;
    double s1 = 0.0, s2 = 0.0;
    const int64_t wstride = (int64_t)nblk * (BLOCK / 64) * W;
    for (int64_t b0 = ((int64_t)bid * (BLOCK / 64) + wv) * W; b0 < nb; b0 += wstride) {
        const int64_t b = b0 + grp;
        const bool mine = grp < W && b < nb && j < kslot;
        const int nbw = (int)min<int64_t>(W, nb - b0);
        const int64_t c = mine ? abase + b * astride : 0;
        double rj;
        if constexpr (RS) {
            rj = mine ? mg_restrict_col(rs->F, rs->C, c, rs->rf, rs->qf) : 0.0;
            if (mine) rs->rw[c] = rj;
        } else {
            rj = (mine && !power) ? r[c] : 0.0;
        }
        const double qj = (mine && !xz) ? q[c] : 0.0;
        const double xj = (mine && !xz) ? x[c] : 0.0;
        const double dj = (mine && (md & MG_NEEDD)) ? d[c] : 0.0;
        double* X = SX[wv];
        const double* Xb = X + gbase;
        double bx = 0.0;
        if (HB && !xz) {
            const double* src = B + b0 * nbB;
            const int cnt = nbw * nbB;
            double v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = lane + 64 * i < cnt ? src[lane + 64 * i] : 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (lane + 64 * i < cnt) LB[wv][lane + 64 * i] = v[i];
            X[lane] = xj;
            const double* Bn = LB[wv] + grp * nbB;
            if (mine) {
                if (tj < 0) {
                    bx = Bn[0] * xj;
#pragma unroll
                    for (int i = 0; i < K; ++i)
                        if (i < kslot && sl.t[i] >= 0) bx += Bn[1 + sl.t[i]] * Xb[i];
                } else {
                    bx = (sl.zs >= 0 ? Bn[1 + tj] * Xb[sl.zs] : 0.0) + Bn[1 + nt + tj] * xj;
                    if (hi >= 0) bx += Bn[1 + 2 * nt + tj] * Xb[hi];
                    if (lo >= 0) bx += Bn[1 + 2 * nt + tj - 1] * Xb[lo];
                }
            }
        }
        const double resid = xz ? rj : (power ? qj + bx : (rj - qj) - bx);
        if (resonly) {
            if (mine && (!live || live[c])) res[c] = resid;
            continue;
        }
        {
            const int cnt = nbw * npks / LF_PER8;   // 8-byte words
            const double* __restrict__ src = reinterpret_cast<const double*>(Lf + b0 * npks);
            constexpr int NV = bj_words(K);
            double v[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i)   // the factor stream: non-temporal (k_cg_block)
                v[i] = lane + 64 * i < cnt ? __builtin_nontemporal_load(src + lane + 64 * i) : 0.0;
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (lane + 64 * i < cnt) LR[wv][lane + 64 * i] = v[i];
        }
        const lf_t* M = reinterpret_cast<const lf_t*>(LR[wv]) + grp * npks;
        float fv[K];
        lf_rowcol<K>(M, j, kslot, mine, fv);
        X[lane] = resid;
        double w = 0.0;   // w = R_b⁻ᵀ resid
#pragma unroll
        for (int i = 0; i < K; ++i) w += (i <= j ? (double)fv[i] : 0.0) * Xb[i];
        X[lane] = w;
        double zz = 0.0;  // z = R_b⁻¹ w
#pragma unroll
        for (int i = 0; i < K; ++i) zz += (i >= j ? (double)fv[i] : 0.0) * Xb[i];
        if (!mine || (live && !live[c])) continue;   // ranks: ghost nodes are the owners' business
        if (power) {
            d[c] = zz;
            s1 += xj * resid;
            s2 += zz * resid;
            continue;
        }
        const double dn = c1 * ((md & MG_DX) ? xj : dj) + c2 * zz;
        const double xn = xj + dn;
        x[c] = xn;
        if (!(md & MG_NOD)) d[c] = dn;
        if (md & MG_RHO) s1 += rj * xn;
    }
    if (part) store_partial(s1, part, bid);
    if (part2) store_partial(s2, part2, bid);
}
template <int K, bool HB, int CM>
__global__ __launch_bounds__(BLOCK) void k_mg_smooth(const CgState* __restrict__ st, int64_t nb, int npks, BlkAffine aff,
                                                     int kslot, MgSlots sl, int nbB, const lf_t* __restrict__ Lf,
                                                     const double* __restrict__ B, const double* __restrict__ r,
                                                     const double* __restrict__ q, double* __restrict__ x,
                                                     double* __restrict__ d, double* __restrict__ res,
                                                     const double* __restrict__ lam, int mode, int step,
                                                     double* __restrict__ part, double* __restrict__ part2,
                                                     const uint8_t* __restrict__ live) {
    if (st->stop) return;
    __shared__ MgSmoothLds<HB> sm;
    mg_smooth_body<K, HB, CM>(nb, npks, aff, kslot, sl, nbB, Lf, B, r, q, x, d, res, lam, mode, step, part, part2, live,
                              sm);
}
// the restriction into level ℓ+1 and that level's first pre-smoothing step (from x = 0, the
// direction not stored: degree ≤ 2) in one launch; r of level ℓ+1 is written for the later passes
template <int K>
__global__ __launch_bounds__(BLOCK) void k_mg_restrict_smooth(const CgState* __restrict__ st, int64_t nb, int npks,
                                                              BlkAffine aff, int kslot, MgSlots sl,
                                                              const lf_t* __restrict__ Lf, double* __restrict__ x,
                                                              const double* __restrict__ lam, MgRestrictSrc rs) {
    if (st->stop) return;
    __shared__ MgSmoothLds<false> sm;
    mg_smooth_body<K, false, MG_XZERO | MG_NOD, true>(nb, npks, aff, kslot, sl, 0, Lf, nullptr, nullptr, nullptr, x,
                                                      nullptr, nullptr, lam, MG_XZERO | MG_NOD, 0, nullptr, nullptr,
                                                      nullptr, sm, &rs);
}

// Small coarse levels (n_full ≤ MG_DIRECT): q = N_s p gathered per column straight from the class
// table (every class exact, no x-edge pass); p = z + β p_old formed on the fly (pnew: written).
// LPC lanes share a column (offsets strided over the lanes, then a shuffle reduction), so a level
// with few columns still spreads over the chip and each lane's gather chain stays short — one
// lane per column left a 125-long dependent load chain (~30 µs whatever the level size).
template <int LPC>
__global__ __launch_bounds__(BLOCK) void k_mg_direct(const CgState* __restrict__ st, MgGeom G, MgTab tz, MgTab td,
                                                     const int32_t* __restrict__ offz,
                                                     const int32_t* __restrict__ offd,
                                                     const int32_t* __restrict__ djz, const int32_t* __restrict__ djd,
                                                     const double* __restrict__ coef, const double* __restrict__ z,
                                                     const double* __restrict__ pold,
                                                     const double* __restrict__ betap, double* __restrict__ pnew,
                                                     double* __restrict__ q, int ra, int rb) {
    if (st->stop) return;
    const double beta = betap ? *betap : st->beta;
    const int bid = blockIdx.x, nblk = gridDim.x;
    const int sub = threadIdx.x % LPC;
    const int64_t per = (int64_t)nblk * (BLOCK / LPC);
    // every lane of a column group runs the same trip count (shuffles need the whole group)
    for (int64_t c0 = (int64_t)bid * (BLOCK / LPC); c0 < G.n_full; c0 += per) {
        const int64_t c = c0 + threadIdx.x / LPC;
        bool live = c < G.n_full;
        int64_t node = 0;
        int t = 0;
        if (live) mg_decode(G, c, node, t);
        const int y = (int)fdiv((uint32_t)node, G.fd_s1), x = (int)(node - (int64_t)y * G.S1), tt = t < 0 ? 0 : t;
        live = live && y >= ra && y < rb;   // a rank's partitioned level: its owned node rows
        const MgTab& T = t < 0 ? tz : td;
        const int32_t* off = t < 0 ? offz : offd;
        const int32_t* dj = t < 0 ? djz : djd;
        double acc = 0.0;
        if (live && T.on) {
            const double* cr = mg_row(T, coef, y, x, tt);
            const bool inner = y >= T.hy && y < G.S0 - T.hy && x >= T.hx && x < G.S1 - T.hx && tt >= T.ht &&
                               tt < T.S2 - T.ht;
#pragma unroll 4
            for (int o = sub; o < T.noff; o += LPC) {
                int64_t j = c + dj[o];
                double cf = cr[o];
                if (!inner) {
                    const int yy = y + off[3 * o], xx = x + off[3 * o + 1], t2 = tt + off[3 * o + 2];
                    const bool ok = yy >= 0 && yy < G.S0 && xx >= 0 && xx < G.S1 && t2 >= 0 && t2 < T.S2;
                    j = ok ? j : c;
                    cf = ok ? cf : 0.0;
                }
                acc += cf * (pold ? z[j] + beta * pold[j] : z[j]);
            }
        }
#pragma unroll
        for (int m = LPC / 2; m >= 1; m /= 2) acc += __shfl_xor(acc, m, LPC);
        if (live && sub == 0) {
            q[c] = acc;
            if (pnew) pnew[c] = pold ? z[c] + beta * pold[c] : z[c];
        }
    }
}

// Coarse levels (ℓ ≥ 1): q = N_s p in two kernels on two streams, each writing its own nodes.
// The levels are too small to hide the latency of the ring kernel's long strips (level 1 at C4:
// 392 strips of 3 ring steps, 70–85 µs for 3.4 M columns + 15 µs of x-edge pass) or of per-column
// gathers (k_mg_direct, 50 µs at level 3).
//  k_mg_tile — nodes of the interior (y, x) class, MG_T × MG_T node tiles, one workgroup per
//    tile: p = z + β p_old over the tile and its halo staged once into LDS (dim 2 padded by 2
//    zeros on each side); lane = node (wave w: tile rows 4w..4w+3), a thread owns the node's
//    whole dim-2 column and walks the (dy, dx) groups: one LDS column read per group, ≤ 5 dt
//    taps per t from registers, the interior class row's coefficients by scalar loads.
//  k_mg_edge — nodes of the boundary classes (the K0-row and K1-column bands), exact tile-layout
//    rows, LPC lanes per (node, t) item over the offsets (k_mg_direct's gather).
constexpr int MG_T = 16;
// LDS doubles per node column: dim 2 plus 2 zero pads on each side, odd so that the lanes' column
// reads (stride TP) fall in different banks (a stride of 16 doubles serialised every read)
__host__ __device__ constexpr int mg_tile_tp(int mt) { return mt == 1 ? 1 : ((mt + 4) | 1); }

template <int MT, int DT>
__device__ __forceinline__ void mg_tile_groups(const CgGrid& C, const double* __restrict__ cf0,
                                               const double* __restrict__ L, int ib, int wxt, int g0, int ng,
                                               double (&acc)[MT]) {
    constexpr int W = 2 * DT + 1, TP = mg_tile_tp(MT), TPAD = MT == 1 ? 0 : 2;
    for (int g = g0; g < g0 + ng; ++g) {
        const int lo = ib + (C.gdy[g] * wxt + C.gdx[g]) * TP + TPAD - DT;
        const double* cf = cf0 + C.gc[g];
        double cv[MT + 2 * DT];
#pragma unroll
        for (int j = 0; j < MT + 2 * DT; ++j) cv[j] = L[lo + j];
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int d = 0; d < W; ++d) acc[t] += cf[t * W + d] * cv[t + d];
    }
}

// one grid's share of a tile: MT = 1 (2-D grid) or the level's column length (dim 2 ≤ MT)
template <int MT>
__device__ __forceinline__ void mg_tile_grid(const CgGrid& C, const double* __restrict__ coefc, int y0, int x0,
                                             double beta, const double* __restrict__ z,
                                             const double* __restrict__ pold, double* __restrict__ pnew,
                                             double* __restrict__ q, double* L, int dbg) {
    constexpr int TP = mg_tile_tp(MT), TPAD = MT == 1 ? 0 : 2;
    const int S0 = C.shape[0], S1 = C.shape[1], S2 = MT == 1 ? 1 : C.shape[2];
    const int hy = C.hy, hx = C.hx, wxt = MG_T + 2 * hx, ncell = (MG_T + 2 * hy) * wxt;
    const uint32_t mdiv = 0xFFFFFFFFu / (uint32_t)wxt + 1u;   // cell / wxt by a multiply-high (cell < 2^16)
    const int64_t col0 = C.col0;
    const int K0 = C.K[0], K1 = C.K[1];
    // 1. stage p over the tile and its halo (zeros outside the grid and in the dim-2 pads; the
    //    tile's own nodes go to pnew)
    //    MG_SU elements in flight per thread (one dependent load per loop trip left the staging
    //    latency-bound: ~50 µs per tile)
    constexpr int MG_SU = 8;
    const int nimg = ncell * TP;
    for (int j0 = threadIdx.x; j0 < nimg; j0 += MG_SU * BLOCK) {
        int64_t gi[MG_SU];
        bool ld[MG_SU], own[MG_SU];
#pragma unroll
        for (int k = 0; k < MG_SU; ++k) {
            const int j = j0 + k * BLOCK;
            const int cell = MT == 1 ? j : j / TP, tt = MT == 1 ? 0 : j - cell * TP;
            const int r = (int)__umulhi((uint32_t)cell, mdiv), c = cell - r * wxt;
            const int y = y0 - hy + r, x = x0 - hx + c, t = tt - TPAD;
            ld[k] = j < nimg && y >= 0 && y < S0 && x >= 0 && x < S1 && t >= 0 && t < S2;
            own[k] = r >= hy && r < hy + MG_T && c >= hx && c < hx + MG_T;
            gi[k] = ld[k] ? col0 + ((int64_t)y * S1 + x) * S2 + t : 0;
        }
        double v[MG_SU];
#pragma unroll
        for (int k = 0; k < MG_SU; ++k) v[k] = ld[k] && !(dbg & 2) ? z[gi[k]] : 0.0;
        if (pold) {
#pragma unroll
            for (int k = 0; k < MG_SU; ++k) v[k] += ld[k] ? beta * pold[gi[k]] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < MG_SU; ++k) {
            if (j0 + k * BLOCK < nimg) L[j0 + k * BLOCK] = v[k];
            if (pnew && ld[k] && own[k]) pnew[gi[k]] = v[k];
        }
    }
    __syncthreads();
    // 2. q for the thread's node when it is of the interior class (the rest: k_mg_edge)
    const int lane = threadIdx.x & 63, ly = 4 * (int)(threadIdx.x >> 6) + (lane >> 4), lx = lane & 15;
    const int y = y0 + ly, x = x0 + lx;
    double acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = 0.0;
    const int ib = ((ly + hy) * wxt + lx + hx) * TP;
    const int n0 = C.ngrp[0], n1 = C.ngrp[1], n2 = C.ngrp[2];
    // the interior class row: wave-uniform scalar loads (coefficients through LDS broadcasts made
    // the kernel LDS-bound: 42 reads per group and lane against 16 for the p column)
    const int rb = __builtin_amdgcn_readfirstlane(C.coefc0 + (K0 * C.ncls[1] + K1) * C.rowlen);
    const double* __restrict__ cf0 = coefc + rb;
    if (n0 && !(dbg & 1)) mg_tile_groups<MT, 0>(C, cf0, L, ib, wxt, 0, n0, acc);
    if (MT > 1 && n1 && !(dbg & 1)) mg_tile_groups<MT, 1>(C, cf0, L, ib, wxt, n0, n1, acc);
    if (MT > 1 && n2 && !(dbg & 1)) mg_tile_groups<MT, 2>(C, cf0, L, ib, wxt, n0 + n1, n2, acc);
    if (y >= K0 && y < S0 - K0 && x >= K1 && x < S1 - K1) {
        double* __restrict__ qn = q + col0 + ((int64_t)y * S1 + x) * S2;
#pragma unroll
        for (int t = 0; t < MT; ++t)
            if (t < S2) qn[t] = acc[t];
    }
}

// boundary node k of a grid (0 ≤ k < mg_edge_count): the K0 bands of rows, then the K1 bands of
// columns of the rows between
__host__ __device__ __forceinline__ int64_t mg_edge_count(int S0, int S1, int K0, int K1) {
    return 2 * (int64_t)K0 * S1 + (int64_t)(S0 - 2 * K0) * 2 * K1;
}
__device__ __forceinline__ void mg_edge_node(uint32_t k, int S0, int S1, int K0, int K1, int& y, int& x) {
    const uint32_t band = (uint32_t)K0 * (uint32_t)S1;
    if (k < 2 * band) {
        const uint32_t kk = k < band ? k : k - band;
        y = (int)(kk / (uint32_t)S1);
        x = (int)(kk - (uint32_t)y * (uint32_t)S1);
        if (k >= band) y += S0 - K0;
        return;
    }
    const uint32_t kk = k - 2 * band;
    const int r = (int)(kk / (uint32_t)(2 * K1)), j = (int)(kk - (uint32_t)r * (uint32_t)(2 * K1));
    y = K0 + r;
    x = j < K1 ? j : S1 - 2 * K1 + j;
}

// the boundary-class items of a level (grid-stride over the items)
template <int LPC>
__global__ __launch_bounds__(BLOCK) void k_mg_edge(const CgState* __restrict__ st, MgGeom G, MgTab tz, MgTab td,
                                                   const int32_t* __restrict__ offz, const int32_t* __restrict__ offd,
                                                   const double* __restrict__ coef, const double* __restrict__ z,
                                                   const double* __restrict__ pold,
                                                   const double* __restrict__ betap, double* __restrict__ q, int ra,
                                                   int rb) {
    if (st->stop) return;
    const double beta = betap ? *betap : st->beta;
    const int bid = blockIdx.x, nblk = gridDim.x;
    const int sub = threadIdx.x % LPC;
    const int64_t nz = tz.on ? mg_edge_count(G.S0, G.S1, tz.K0, tz.K1) : 0;
    const int64_t nd = td.on ? mg_edge_count(G.S0, G.S1, td.K0, td.K1) * td.S2 : 0;
    const int64_t per = (int64_t)nblk * (BLOCK / LPC);
    for (int64_t e0 = (int64_t)bid * (BLOCK / LPC); e0 < nz + nd; e0 += per) {
        const int64_t e = e0 + threadIdx.x / LPC;
        bool live = e < nz + nd;
        const bool isz = e < nz;
        const MgTab& T = isz ? tz : td;
        const int32_t* off = isz ? offz : offd;
        int y = 0, x = 0, t = 0;
        if (live) {
            uint32_t k = (uint32_t)(isz ? e : e - nz);
            if (!isz) {
                const uint32_t kn = k / (uint32_t)T.S2;
                t = (int)(k - kn * (uint32_t)T.S2);
                k = kn;
            }
            mg_edge_node(k, G.S0, G.S1, T.K0, T.K1, y, x);
            live = y >= ra && y < rb;
        }
        const int64_t node = (int64_t)y * G.S1 + x;
        const int64_t c = isz ? G.colz + node : G.cold + node * G.nt + t;
        double acc = 0.0;
        if (live) {
            const double* cr = mg_row(T, coef, y, x, t);
            for (int o = sub; o < T.noff; o += LPC) {
                const int yy = y + off[3 * o], xx = x + off[3 * o + 1], t2 = t + off[3 * o + 2];
                const bool ok = yy >= 0 && yy < G.S0 && xx >= 0 && xx < G.S1 && t2 >= 0 && t2 < T.S2;
                const int64_t nn = (int64_t)yy * G.S1 + xx;
                const int64_t j = ok ? (isz ? G.colz + nn : G.cold + nn * G.nt + t2) : c;
                acc += (ok ? cr[o] : 0.0) * (pold ? z[j] + beta * pold[j] : z[j]);
            }
        }
#pragma unroll
        for (int m = LPC / 2; m >= 1; m /= 2) acc += __shfl_xor(acc, m, LPC);
        if (live && sub == 0) q[c] = acc;
    }
}

// the interior tiles (k_mg_edge: the boundary-class items, on the side stream — run after the
// tiles inside this launch instead, C4 levels 1–3 took 30 µs more per V-cycle than the ~11 µs
// join gaps they saved)
template <int MAXT>
__global__ __launch_bounds__(BLOCK) void k_mg_tile(const CgState* __restrict__ st, const CgDesc* __restrict__ cd,
                                                   const double* __restrict__ coefc, const double* __restrict__ z,
                                                   const double* __restrict__ pold, const double* __restrict__ betap,
                                                   double* __restrict__ pnew, double* __restrict__ q, int dbg, int ra,
                                                   int rb) {
    if (st->stop) return;
    const double beta = betap ? *betap : st->beta;
    int b = blockIdx.x;   // workgroups: the tiles of grid 0, then those of grid 1, …
    for (int g = 0; g < cd->n_grids; ++g) {
        const CgGrid& C = cd->g[g];
        if (!C.noff) continue;
        const int ntx = (C.shape[1] + MG_T - 1) / MG_T, nty = (C.shape[0] + MG_T - 1) / MG_T;
        if (b >= nty * ntx) {
            b -= nty * ntx;
            continue;
        }
        if ((dbg & 4) && C.shape[2] == 1) return;
        const int ty = b / ntx, y0 = ty * MG_T, x0 = (b - ty * ntx) * MG_T;
        if (y0 + MG_T <= ra || y0 >= rb) return;   // a rank's partitioned level: tiles of its owned rows
        if (C.shape[2] == 1) mg_tile_grid<1>(C, coefc, y0, x0, beta, z, pold, pnew, q, mf_zl, dbg);
        else mg_tile_grid<MAXT>(C, coefc, y0, x0, beta, z, pold, pnew, q, mf_zl, dbg);
        return;
    }
}

// k_mg_tile with a class-compressed coefficient row (round 5; VERDICT r4 #2a: k_mg_tile waited 54 %
// of its wave cycles on 60 scalar coefficients per (dy, dx) group, loaded 8–16 doubles at a time
// behind lgkmcnt(0)).  The taps of a group depend on t only through t's dim-2 boundary class (as the
// level-0 wave-strip table, rw_tc), so a group holds NC·W coefficients (12 epochs, K2 = 2: 5 class
// rows of W = 2·DT + 1 taps — 25 instead of 60 for DT = 2); taps that reach outside the column
// (t + d − DT ∉ [0, S2)) are skipped at compile time, so a group reads only its neighbour column's
// own S2 values and the image needs no dim-2 pads (stride MG_TKP = 13, odd: conflict-free column
// reads; 41.6 KB of LDS for a 16×16 tile with a 2-node halo instead of 54.4 KB: three workgroups
// per CU instead of two).  CFL: the row staged once per workgroup in LDS (broadcast reads) instead
// of scalar loads.
constexpr int MG_TKP = 13;
template <int MT, int NC, int DT, bool CFL>
__device__ __forceinline__ void mg_tk_groups(const CgGrid& C, const double* __restrict__ cf, const double* L, int ib,
                                             int wxt, int g0, int ng, double (&acc)[MT]) {
    constexpr int W = 2 * DT + 1, TP = MT == 1 ? 1 : MG_TKP, KT = (NC - 1) / 2;
    for (int g = g0; g < g0 + ng; ++g, cf += NC * W) {
        const double* col = L + ib + (C.gdy[g] * wxt + C.gdx[g]) * TP;
        double cv[MT];
#pragma unroll
        for (int j = 0; j < MT; ++j) cv[j] = col[j];
        double c[NC * W];
#pragma unroll
        for (int j = 0; j < NC * W; ++j) c[j] = cf[j];
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int d = 0; d < W; ++d) {
                const int tt = t + d - DT;
                if (tt >= 0 && tt < MT) acc[t] += c[rw_tc(t, MT, KT) * W + d] * cv[tt];
            }
    }
}

template <int MT, int NC, bool CFL>
__device__ __forceinline__ void mg_tk_grid(const CgGrid& C, const double* __restrict__ tkc, int c0, int ncoef, int y0,
                                           int x0, double beta, const double* __restrict__ z,
                                           const double* __restrict__ pold, double* __restrict__ pnew,
                                           double* __restrict__ q, double* L) {
    constexpr int TP = MT == 1 ? 1 : MG_TKP;
    const int S0 = C.shape[0], S1 = C.shape[1], S2 = MT;
    const int hy = C.hy, hx = C.hx, wxt = MG_T + 2 * hx, ncell = (MG_T + 2 * hy) * wxt;
    const uint32_t mdiv = 0xFFFFFFFFu / (uint32_t)wxt + 1u;   // cell / wxt by a multiply-high (cell < 2^16)
    const int64_t col0 = C.col0;
    const int K0 = C.K[0], K1 = C.K[1];
    const int nimg = ncell * TP;
    double* Lc = L + nimg;   // CFL: the compressed row after the image
    if (CFL)
        for (int j = threadIdx.x; j < ncoef; j += BLOCK) Lc[j] = tkc[c0 + j];
    // 1. stage p over the tile and its halo (zeros outside the grid and in the column pad)
    constexpr int MG_SU = 8;
    for (int j0 = threadIdx.x; j0 < nimg; j0 += MG_SU * BLOCK) {
        int64_t gi[MG_SU];
        bool ld[MG_SU], own[MG_SU];
#pragma unroll
        for (int k = 0; k < MG_SU; ++k) {
            const int j = j0 + k * BLOCK;
            const int cell = MT == 1 ? j : j / TP, t = MT == 1 ? 0 : j - cell * TP;
            const int r = (int)__umulhi((uint32_t)cell, mdiv), c = cell - r * wxt;
            const int y = y0 - hy + r, x = x0 - hx + c;
            ld[k] = j < nimg && y >= 0 && y < S0 && x >= 0 && x < S1 && t < S2;
            own[k] = r >= hy && r < hy + MG_T && c >= hx && c < hx + MG_T;
            gi[k] = ld[k] ? col0 + ((int64_t)y * S1 + x) * S2 + t : 0;
        }
        double v[MG_SU];
#pragma unroll
        for (int k = 0; k < MG_SU; ++k) v[k] = ld[k] ? z[gi[k]] : 0.0;
        if (pold) {
#pragma unroll
            for (int k = 0; k < MG_SU; ++k) v[k] += ld[k] ? beta * pold[gi[k]] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < MG_SU; ++k) {
            if (j0 + k * BLOCK < nimg) L[j0 + k * BLOCK] = v[k];
            if (pnew && ld[k] && own[k]) pnew[gi[k]] = v[k];
        }
    }
    __syncthreads();
    // 2. q for the thread's node when it is of the interior class (the rest: k_mg_edge)
    const int lane = threadIdx.x & 63, ly = 4 * (int)(threadIdx.x >> 6) + (lane >> 4), lx = lane & 15;
    const int y = y0 + ly, x = x0 + lx;
    double acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = 0.0;
    const int ib = ((ly + hy) * wxt + lx + hx) * TP;
    const int n0 = C.ngrp[0], n1 = C.ngrp[1], n2 = C.ngrp[2];
    const double* __restrict__ cf = CFL ? Lc : tkc + __builtin_amdgcn_readfirstlane(c0);
    if (n0) mg_tk_groups<MT, NC, 0, CFL>(C, cf, L, ib, wxt, 0, n0, acc);
    if (MT > 1 && n1) mg_tk_groups<MT, NC, 1, CFL>(C, cf + NC * n0, L, ib, wxt, n0, n1, acc);
    if (MT > 1 && n2) mg_tk_groups<MT, NC, 2, CFL>(C, cf + NC * (n0 + 3 * n1), L, ib, wxt, n0 + n1, n2, acc);
    if (y >= K0 && y < S0 - K0 && x >= K1 && x < S1 - K1) {
        double* __restrict__ qn = q + col0 + ((int64_t)y * S1 + x) * S2;
#pragma unroll
        for (int t = 0; t < MT; ++t) qn[t] = acc[t];
    }
}

template <bool CFL>
__global__ __launch_bounds__(BLOCK) void k_mg_tile_kt(const CgState* __restrict__ st, const CgDesc* __restrict__ cd,
                                                      const double* __restrict__ tkc, MgTk tk,
                                                      const double* __restrict__ z, const double* __restrict__ pold,
                                                      const double* __restrict__ betap, double* __restrict__ pnew,
                                                      double* __restrict__ q, int ra, int rb) {
    if (st->stop) return;
    const double beta = betap ? *betap : st->beta;
    int b = blockIdx.x;   // workgroups: the tiles of grid 0, then those of grid 1, …
    for (int g = 0; g < cd->n_grids; ++g) {
        const CgGrid& C = cd->g[g];
        if (!C.noff) continue;
        const int ntx = (C.shape[1] + MG_T - 1) / MG_T, nty = (C.shape[0] + MG_T - 1) / MG_T;
        if (b >= nty * ntx) {
            b -= nty * ntx;
            continue;
        }
        const int ty = b / ntx, y0 = ty * MG_T, x0 = (b - ty * ntx) * MG_T;
        if (y0 + MG_T <= ra || y0 >= rb) return;   // a rank's partitioned level: tiles of its owned rows
        const int ncoef = C.ngrp[0] + 3 * C.ngrp[1] + 5 * C.ngrp[2];
        if (C.shape[2] == 1) mg_tk_grid<1, 1, CFL>(C, tkc, tk.c0[g], ncoef, y0, x0, beta, z, pold, pnew, q, mf_zl);
        else mg_tk_grid<12, 5, CFL>(C, tkc, tk.c0[g], 5 * ncoef, y0, x0, beta, z, pold, pnew, q, mf_zl);
        return;
    }
}

// coarsest level: Ninv = Ri·Riᵀ (Ri = R⁻¹ upper, npad × npad row-major), 64×64 tiles per workgroup
__global__ __launch_bounds__(BLOCK) void k_mg_gram(const double* __restrict__ Ri, int64_t npad,
                                                   double* __restrict__ C) {
    __shared__ double Ta[64][65];
    __shared__ double Tb[64][65];
    const int nb = (int)(npad / 64);
    const int ib = blockIdx.x % nb, jb = blockIdx.x / nb;
    const int tr = threadIdx.x / 16, tc = threadIdx.x % 16;
    double acc[4][4] = {};
    for (int kb = max(ib, jb); kb < nb; ++kb) {   // Ri[i][k] = 0 for k < i
        __syncthreads();
        for (int idx = threadIdx.x; idx < 64 * 64; idx += BLOCK) {
            const int r = idx / 64, cc = idx % 64;
            Ta[r][cc] = Ri[(int64_t)(ib * 64 + r) * npad + kb * 64 + cc];
            Tb[r][cc] = Ri[(int64_t)(jb * 64 + r) * npad + kb * 64 + cc];
        }
        __syncthreads();
        for (int k = 0; k < 64; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = Ta[tr * 4 + u][k];
                b[u] = Tb[tc * 4 + u][k];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] += a[u] * b[v];
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) C[(int64_t)(ib * 64 + tr * 4 + u) * npad + jb * 64 + tc * 4 + v] = acc[u][v];
}

// y = M x, one wave per row (coalesced row reads)
__global__ __launch_bounds__(BLOCK) void k_mg_gemv(const CgState* __restrict__ st, const double* __restrict__ M,
                                                   int64_t n, int64_t ld, const double* __restrict__ x,
                                                   double* __restrict__ y) {
    if (st->stop) return;
    const int bid = blockIdx.x, nblk = gridDim.x;
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)bid * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)nblk * 4) {
        double s = 0.0;
        for (int64_t j = lane; j < n; j += 64) s += M[i * ld + j] * x[j];
        s = wave_sum(s);
        if (lane == 0) y[i] = s;
    }
}

// power step scalars: λ = max(λ, x·Nx) (x is M-normalised from the second step on), next scale
// 1/sqrt(d·Nx) as the op kernel's β − 1 (p = z + β p_old with p_old = z)
__global__ __launch_bounds__(BLOCK) void k_mg_power_scalar(const double* part1, const double* part2, int np, int k,
                                                           double* lam, double* scal) {
    const double s1 = reduce_parts(part1, np);
    const double s2 = reduce_parts(part2, np);
    if (threadIdx.x) return;
    lam[0] = k == 0 ? 0.0 : fmax(lam[0], s1);
    scal[0] = s2 > 0.0 ? 1.0 / sqrt(s2) - 1.0 : 0.0;
}

// deterministic pseudo-random start vector on the kept columns, hashed from the column's id in
// the global layout Gg (node_off: the global node of local node 0 — a rank's window), so a ghost
// column gets its owner's value
__global__ __launch_bounds__(BLOCK) void k_mg_randvec(MgGeom G, MgGeom Gg, int64_t node_off, double* __restrict__ v) {
    for (int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x; c < G.n_full; c += (int64_t)gridDim.x * BLOCK) {
        int64_t node;
        int t;
        mg_decode(G, c, node, t);
        const int64_t cg = mg_col(Gg, node + node_off, t);
        uint64_t h = (uint64_t)cg * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
        h ^= h >> 31;
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 29;
        v[c] = (t >= 0 && t == G.tref) ? 0.0 : (double)(h >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
}

// ---- z0 on a 2× refinement of the dz lattice (mg_build_mixed) ----------------------------------

// Chebyshev step `step` on [λ/10, 1.1 λ] (as k_mg_smooth)
__device__ __forceinline__ void mg_cheb(const double* lam, int step, double& c1, double& c2) {
    const double lmax = 1.1 * lam[0], lmin = 0.1 * lmax;
    const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
    double rho = 1.0 / sigma;
    c1 = 0.0;
    c2 = 1.0 / theta;
    for (int k = 1; k <= step; ++k) {
        const double rn = 1.0 / (2.0 * sigma - rho);
        c1 = rn * rho;
        c2 = 2.0 * rn / delta;
        rho = rn;
    }
}

// Chebyshev-Jacobi on the z0 columns of the fine level (modes of k_mg_smooth): resid = r − q
// (XZERO: r; POWER: q = N x), z = D⁻¹ resid; POWER: d = z, partials x·resid, z·resid; else
// d = c1 d_prev + c2 z (DX: d_prev = x), x += d (d stored unless NOD)
__global__ __launch_bounds__(BLOCK) void k_mgx_smooth(const CgState* __restrict__ st, MgMix X,
                                                      const double* __restrict__ dinv, const double* __restrict__ r,
                                                      const double* __restrict__ q, double* __restrict__ x,
                                                      double* __restrict__ d, const double* __restrict__ lam, int mode,
                                                      int step, double* __restrict__ part, double* __restrict__ part2) {
    if (st->stop) return;
    const bool xz = mode & MG_XZERO, power = mode & MG_POWER;
    double c1 = 0.0, c2 = 0.0;
    if (!power) mg_cheb(lam, step, c1, c2);
    const bool needd = !power && step > 0 && !(mode & MG_DX);
    double s1 = 0.0, s2 = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < X.nz; j += (int64_t)gridDim.x * BLOCK) {
        const int64_t c = X.z0col + j;
        const double xj = xz ? 0.0 : x[c];
        const double resid = xz ? r[c] : (power ? q[c] : r[c] - q[c]);
        const double zz = dinv[j] * resid;
        if (power) {
            d[c] = zz;
            s1 += xj * resid;
            s2 += zz * resid;
            continue;
        }
        const double dn = c1 * ((mode & MG_DX) ? xj : (needd ? d[c] : 0.0)) + c2 * zz;
        x[c] = xj + dn;
        if (!(mode & MG_NOD)) d[c] = dn;
    }
    if (part) store_partial(s1, part, blockIdx.x);
    if (part2) store_partial(s2, part2, blockIdx.x);
}

// power steps: v = (scal + 1)·d on the z0 columns (M-normalised iterate)
__global__ __launch_bounds__(BLOCK) void k_mgx_scale(MgMix X, const double* __restrict__ scal, const double* __restrict__ d,
                                                     double* __restrict__ v) {
    const double f = scal[0] + 1.0;
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < X.nz; j += (int64_t)gridDim.x * BLOCK)
        v[X.z0col + j] = f * d[X.z0col + j];
}

// r_sub = P₀ᵀ(r − q): z0 bilinear restriction from the fine lattice (coarse node a on fine 2a, ½ on
// the odd neighbours), dz unchanged (the reference epoch 0).  Sub layout: z0 (nsz), then dz.
__global__ __launch_bounds__(BLOCK) void k_mgx_restrict(const CgState* __restrict__ st, MgMix X,
                                                        const double* __restrict__ r, const double* __restrict__ q,
                                                        double* __restrict__ rs) {
    if (st->stop) return;
    const int64_t n = X.nsz * (1 + X.nt);
    for (int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x; c < n; c += (int64_t)gridDim.x * BLOCK) {
        double acc = 0.0;
        if (c < X.nsz) {
            const int y = (int)(c / X.Sc1), x = (int)(c - (int64_t)y * X.Sc1);
            for (int dy = -1; dy <= 1; ++dy) {
                const int fy = 2 * y + dy;
                if (fy < 0 || fy >= X.Sf0) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int fx = 2 * x + dx;
                    if (fx < 0 || fx >= X.Sf1) continue;
                    const int64_t f = X.z0col + (int64_t)fy * X.Sf1 + fx;
                    acc += ((dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0)) * (r[f] - q[f]);
                }
            }
        } else {
            const int64_t e = c - X.nsz;
            const int t = (int)(e % X.nt);
            acc = t == X.tref ? 0.0 : r[X.dzcol + e] - q[X.dzcol + e];
        }
        rs[c] = acc;
    }
}

// x += P₀ x_sub (z0: bilinear from the dz lattice; dz: the same columns)
__global__ __launch_bounds__(BLOCK) void k_mgx_prolong(const CgState* __restrict__ st, MgMix X,
                                                       const double* __restrict__ xs, double* __restrict__ x) {
    if (st->stop) return;
    const int64_t n = X.nz + X.nsz * X.nt;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        if (i < X.nz) {
            const int y = (int)(i / X.Sf1), xx = (int)(i - (int64_t)y * X.Sf1);
            const int ya = y >> 1, xa = xx >> 1, ny = (y & 1) ? 2 : 1, nx = (xx & 1) ? 2 : 1;
            const double wy = (y & 1) ? 0.5 : 1.0, wx = (xx & 1) ? 0.5 : 1.0;
            double acc = 0.0;
            for (int a = 0; a < ny; ++a)
                for (int b = 0; b < nx; ++b) acc += (wy * wx) * xs[(int64_t)(ya + a) * X.Sc1 + xa + b];
            x[X.z0col + i] += acc;
        } else {
            const int64_t e = i - X.nz;
            if ((int)(e % X.nt) != X.tref) x[X.dzcol + e] += xs[X.nsz + e];
        }
    }
}

// partials of Σ s·z over the full column space (ρ of the CG step)
__global__ __launch_bounds__(BLOCK) void k_mgx_dot(const CgState* __restrict__ st, int64_t n, const double* __restrict__ s,
                                                   const double* __restrict__ z, double* __restrict__ part) {
    if (st->stop) return;
    double a = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x; c < n; c += (int64_t)gridDim.x * BLOCK) a += s[c] * z[c];
    store_partial(a, part, blockIdx.x);
}

// 1 / diag(AᵀA) of the z0 columns: Σ_rows (rs·G)² over Gᵀ's row of the compact column
__global__ __launch_bounds__(BLOCK) void k_mgx_diag(MgMix X, const int32_t* __restrict__ colmap,
                                                    const int64_t* __restrict__ trp, const int32_t* __restrict__ tci,
                                                    const double* __restrict__ tval, const double* __restrict__ rs,
                                                    double* __restrict__ dinv) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < X.nz; j += (int64_t)gridDim.x * BLOCK) {
        const int32_t k = colmap[X.z0col + j];
        double a = 0.0;
        if (k >= 0)
            for (int64_t e = trp[k]; e < trp[k + 1]; ++e) {
                const double v = rs[tci[e]] * tval[e];
                a += v * v;
            }
        dinv[j] = a > 0.0 ? 1.0 / a : 0.0;
    }
}

// deterministic start vector of the power steps on the z0 columns (the dz columns stay 0)
__global__ __launch_bounds__(BLOCK) void k_mgx_randvec(MgMix X, double* __restrict__ v) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < X.nz; j += (int64_t)gridDim.x * BLOCK) {
        uint64_t h = (uint64_t)j * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
        h ^= h >> 31;
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 29;
        v[X.z0col + j] = (double)(h >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
}

// The exact node blocks of a shared-lattice level with matrix-free data rows: per node the data
// term Σ_points rs² w(p)² τ τᵀ (w: the point's bilinear weight at the node; τ as k_mg_lump1) in
// the lumped-block layout, to which k_mg_block_build adds the stencil block — the diagonal blocks
// of AᵀA without a formed matrix (S.mx level 0's block-Jacobi factors).
__global__ __launch_bounds__(64) void k_mg_lump0(DmfDesc D, const int32_t* __restrict__ cell,
                                                 const double4* __restrict__ pt, int nt, int nbB, int withz,
                                                 double* __restrict__ B) {
    __shared__ double LA[MG_NB_MAX * 64];
    const int lane = threadIdx.x;
    const int nsx = (D.S1 + 63) / 64;
    const int a = blockIdx.x / nsx, b = (blockIdx.x - a * nsx) * 64 + lane;
    const bool mine = a < D.S0 && b < D.S1;
    for (int k = 0; k < nbB; ++k) LA[k * 64 + lane] = 0.0;
    if (mine) {
        const int C0 = D.S0 - 1, C1 = D.S1 - 1;
        const int xlo = max(b - 1, 0), xhi = min(b, C1 - 1);
        for (int ry = max(a - 1, 0); ry <= min(a, C0 - 1); ++ry) {
            const int p0 = cell[ry * C1 + xlo], p1 = cell[ry * C1 + xhi + 1];
            for (int i = p0; i < p1; ++i) {
                const double4 P = pt[i];
                double fy, fx;
                const int cy = dmf_cell(P.x, D.S0, fy), cx = dmf_cell(P.y, D.S1, fx);
                const double wy = cy == a ? 1.0 - fy : (cy + 1 == a ? fy : 0.0);
                const double wx = cx == b ? 1.0 - fx : (cx + 1 == b ? fx : 0.0);
                const double w = wy * wx;
                const double cc = (P.w * P.w) * (w * w);
                if (cc == 0.0) continue;
                if (withz) LA[lane] += cc;
                if (nt) {
                    double ft;
                    const int ct = dmf_cell(P.z, D.S2, ft);
                    const double at = 1.0 - ft;
                    if (withz) {
                        LA[(1 + ct) * 64 + lane] += cc * at;
                        LA[(2 + ct) * 64 + lane] += cc * ft;
                    }
                    LA[(1 + nt + ct) * 64 + lane] += cc * (at * at);
                    LA[(2 + nt + ct) * 64 + lane] += cc * (ft * ft);
                    LA[(1 + 2 * nt + ct) * 64 + lane] += cc * (at * ft);
                }
            }
        }
        for (int k = 0; k < nbB; ++k) B[((int64_t)a * D.S1 + b) * nbB + k] = LA[k * 64 + lane];
    }
}

// ---- host: Galerkin class tables ---------------------------------------------------------------

// coarse parents of fine index j (P_ℓ: coarse a at fine 2a, weight ½ on the odd neighbours)
int mg_parents(int j, int* a, double* w) {
    if (!(j & 1)) {
        a[0] = j / 2;
        w[0] = 1.0;
        return 1;
    }
    a[0] = (j - 1) / 2;
    a[1] = (j + 1) / 2;
    w[0] = w[1] = 0.5;
    return 2;
}

// C = PᵀF P for one grid (P bilinear in dims 0, 1; identity in dim 2): the row of each coarse
// class representative, computed from the fine table; the class boundary K_c is conservative
// (a coarse row at ≥ K_c from both ends only sees interior fine rows) and checked.
bool ns_galerkin(const NsTable& F, NsTable& C, std::string& why) {
    C = NsTable{};
    if (!F.on) {
        for (int e = 0; e < 2; ++e) C.shape[e] = F.shape[e] / 2 + 1;
        C.shape[2] = F.shape[2];
        return true;
    }
    C.on = true;
    for (int e = 0; e < 2; ++e) C.shape[e] = F.shape[e] / 2 + 1;
    C.shape[2] = F.shape[2];
    int h[2] = {0, 0};
    for (const auto& o : F.offs)
        for (int e = 0; e < 2; ++e) h[e] = std::max(h[e], std::abs(o[e]));
    for (int e = 0; e < 2; ++e) {
        C.K[e] = (std::max(F.K[e], h[e]) + 3) / 2 + 1;
        C.ncls[e] = C.shape[e] <= 2 * C.K[e] + 1 ? C.shape[e] : 2 * C.K[e] + 1;
        // every node its own class: K only names the row the ring kernel applies to a whole
        // dim-1 strip (k_cg_xedge corrects the others), so it must be a valid position
        if (C.ncls[e] == C.shape[e]) C.K[e] = std::min(C.K[e], C.shape[e] - 1);
    }
    C.K[2] = F.K[2];
    C.ncls[2] = F.ncls[2];
    // a coarse row: dense over the 5×5×5 offset box (|dy|, |dx| ≤ 2 by the Galerkin radius, |dt| ≤ 2
    // in column mode), touched marks the offsets some term reached
    struct Row {
        std::array<double, 125> v;
        std::array<bool, 125> on;
    };
    auto box = [](int ey, int ex, int et) { return (ey + 2) * 25 + (ex + 2) * 5 + (et + 2); };
    bool wide = false;
    auto row_at = [&](int ay, int ax, int at, Row& row) {
        row.v.fill(0.0);
        row.on.fill(false);
        for (int dy = -1; dy <= 1; ++dy) {
            const int iy = 2 * ay + dy;
            if (iy < 0 || iy >= F.shape[0]) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int ix = 2 * ax + dx;
                if (ix < 0 || ix >= F.shape[1]) continue;
                const double wi = (dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0);
                const double* fr = F.row(cls_of(iy, F.shape[0], F.K[0], F.ncls[0]), cls_of(ix, F.shape[1], F.K[1], F.ncls[1]),
                                         cls_of(at, F.shape[2], F.K[2], F.ncls[2]));
                for (size_t o = 0; o < F.offs.size(); ++o) {
                    const double v = fr[o];
                    if (v == 0.0) continue;
                    const int jy = iy + F.offs[o][0], jx = ix + F.offs[o][1], jt = at + F.offs[o][2];
                    if (jy < 0 || jy >= F.shape[0] || jx < 0 || jx >= F.shape[1] || jt < 0 || jt >= F.shape[2]) continue;
                    const int et = F.offs[o][2];
                    int by[2], bx[2];
                    double py[2], px[2];
                    const int ny = mg_parents(jy, by, py), nx = mg_parents(jx, bx, px);
                    for (int u = 0; u < ny; ++u)
                        for (int w = 0; w < nx; ++w) {
                            const int ey = by[u] - ay, ex = bx[w] - ax;
                            if (std::abs(ey) > 2 || std::abs(ex) > 2 || std::abs(et) > 2) {
                                wide = true;
                                continue;
                            }
                            const int k = box(ey, ex, et);
                            row.v[k] += (wi * v) * (py[u] * px[w]);
                            row.on[k] = true;
                        }
                }
            }
        }
    };
    // the class table for the current K / ncls
    auto fill = [&]() -> bool {
        const int nrow = C.ncls[0] * C.ncls[1] * C.ncls[2];
        std::vector<Row> rows(nrow);
        std::array<bool, 125> any;
        any.fill(false);
        for (int cy = 0; cy < C.ncls[0]; ++cy)
            for (int cx = 0; cx < C.ncls[1]; ++cx)
                for (int ct = 0; ct < C.ncls[2]; ++ct) {
                    Row& r = rows[(cy * C.ncls[1] + cx) * C.ncls[2] + ct];
                    row_at(cls_rep(cy, C.shape[0], C.K[0], C.ncls[0]), cls_rep(cx, C.shape[1], C.K[1], C.ncls[1]),
                           cls_rep(ct, C.shape[2], C.K[2], C.ncls[2]), r);
                    for (int k = 0; k < 125; ++k) any[k] = any[k] || (r.on[k] && r.v[k] != 0.0);
                }
        if (wide) { why = "multigrid: a Galerkin coarse stencil wider than ±2"; return false; }
        std::vector<std::array<int, 3>> offs;   // ascending (dy, dx, dt) = ascending box index
        std::vector<int> kof;
        for (int k = 0; k < 125; ++k)
            if (any[k]) {
                offs.push_back({k / 25 - 2, (k / 5) % 5 - 2, k % 5 - 2});
                kof.push_back(k);
            }
        if (offs.empty()) {   // an all-zero table (a grid whose parts are all field-valued)
            offs.push_back({0, 0, 0});
            kof.push_back(box(0, 0, 0));
        }
        if ((int)offs.size() > CG_MAX_OFF) { why = "multigrid: Galerkin coarse stencil wider than CG_MAX_OFF"; return false; }
        C.offs = offs;
        const size_t noff = offs.size();
        C.coef.assign((size_t)nrow * noff, 0.0);
        for (int r = 0; r < nrow; ++r)
            for (size_t o = 0; o < noff; ++o) C.coef[(size_t)r * noff + o] = rows[r].v[kof[o]];
        return true;
    };
    // does the row at position `pos` of dim e (dims e' ≠ e at their interior representative) equal
    // the INTERIOR class row of the current table, for every t class?
    auto matches = [&](int e, int pos) -> bool {
        for (int ct = 0; ct < C.ncls[2]; ++ct) {
            int p[3] = {cls_rep(C.ncls[0] == C.shape[0] ? 0 : C.K[0], C.shape[0], C.K[0], C.ncls[0]),
                        cls_rep(C.ncls[1] == C.shape[1] ? 0 : C.K[1], C.shape[1], C.K[1], C.ncls[1]),
                        cls_rep(ct, C.shape[2], C.K[2], C.ncls[2])};
            p[e] = pos;
            Row r;
            row_at(p[0], p[1], p[2], r);
            int cl[2] = {cls_of(p[0], C.shape[0], C.K[0], C.ncls[0]), cls_of(p[1], C.shape[1], C.K[1], C.ncls[1])};
            cl[e] = C.K[e];
            const double* ref = C.row(cl[0], cl[1], ct);
            const size_t noff = C.offs.size();
            double scale = 0.0;
            for (size_t o = 0; o < noff; ++o) scale = std::max(scale, std::fabs(ref[o]));
            std::array<double, 125> want;
            want.fill(0.0);
            for (size_t o = 0; o < noff; ++o) want[box(C.offs[o][0], C.offs[o][1], C.offs[o][2])] = ref[o];
            for (int k = 0; k < 125; ++k)
                if (std::fabs(want[k] - r.v[k]) > 1e-12 * scale) return false;
        }
        return true;
    };
    if (!fill()) return false;
    // class structure check: the interior representative equals the middle and the last interior node
    for (int e = 0; e < 2; ++e) {
        if (C.ncls[e] == C.shape[e]) continue;
        if (!matches(e, C.shape[e] / 2) || !matches(e, C.shape[e] - 1 - C.K[e])) {
            why = "multigrid: Galerkin class structure check failed";
            return false;
        }
    }
    // tighten K (fewer x-edge items): the smallest K' whose positions K'..K−1 at both ends already
    // carry the interior row
    bool changed = false;
    for (int e = 0; e < 2; ++e) {
        if (C.ncls[e] == C.shape[e]) continue;
        int Kt = C.K[e];
        while (Kt > 0 && matches(e, Kt - 1) && matches(e, C.shape[e] - Kt)) --Kt;
        if (Kt < C.K[e]) {
            C.K[e] = Kt;
            C.ncls[e] = 2 * Kt + 1;
            changed = true;
        }
    }
    if (changed && !fill()) return false;
    return true;
}

MgTab mg_tab(const NsTable& T, int coef0) {
    MgTab m{};
    m.on = T.on ? 1 : 0;
    m.S0 = T.shape[0];
    m.S1 = T.shape[1];
    m.S2 = T.shape[2];
    m.K0 = T.K[0];
    m.K1 = T.K[1];
    m.K2 = T.K[2];
    m.n0 = T.ncls[0];
    m.n1 = T.ncls[1];
    m.n2 = T.ncls[2];
    m.noff = (int)T.offs.size();
    m.coef0 = coef0;
    for (const auto& o : T.offs) {
        m.hy = std::max(m.hy, std::abs(o[0]));
        m.hx = std::max(m.hx, std::abs(o[1]));
        m.ht = std::max(m.ht, std::abs(o[2]));
    }
    for (int k = 0; k < 5; ++k) {
        m.od[k] = -1;
        const std::array<int, 3> o = {0, 0, k - 2};
        const auto it = std::find(T.offs.begin(), T.offs.end(), o);
        if (it != T.offs.end()) m.od[k] = (int)(it - T.offs.begin());
    }
    return m;
}

BlkAffine mg_affine(const MgGeom& G, const MgSlots& sl, int kslot) {
    BlkAffine a{};
    for (int s = 0; s < kslot; ++s) {
        a.base[s] = sl.t[s] < 0 ? G.colz : G.cold + sl.t[s];
        a.stride[s] = sl.t[s] < 0 ? 1 : G.nt;
    }
    return a;
}

int mg_grid_blocks(int64_t nb) { return grid_for(std::max<int64_t>(nb, 1) * BJ_LANES, BLOCK, bj_grid_cap()); }

// Build the level hierarchy (host tables, device descriptions, buffers) for a system whose
// normal-stencil tables exist.  False (+ reason) when the system lacks smooth_fit's structure.
// levels ≥ 2 of the field-valued z0 rows from level 1 (local Galerkin; a rank's level 1 is already
// the global sum)
void mg_var_coarse(System& S) {
    MgHier& H = *S.mg;
    if (!H.var) return;
    for (size_t l = 2; l < H.lev.size(); ++l) {
        const MgGeom &F = H.lev[l - 1].geo, &C = H.lev[l].geo;
        hipLaunchKernelGGL(k_mg_var_galerkin, dim3(grid_for(C.nodes)), dim3(BLOCK), 0, S.stream, F.S0, F.S1, C.S0, C.S1,
                           H.lev[l - 1].vz.p, H.lev[l].vz.p);
        KERNEL_CHECK();
    }
    HIP_CHECK(hipStreamSynchronize(S.stream));
}

// Lumping requested for the extra rows (lsq_set_extra_rows_lumping): classify the formed rows and
// build the transpose over the touched level-1 nodes for this hierarchy's geometry (xr_lump.hpp).
// Kept across rebuilds of the hierarchy with the same geometry.  A refusal leaves lump_ok false
// with its reason; xr_refusal reports it.
void xr_lump_prepare(System& S) {
    XrData& X = S.xr;
    if (!X.m_x || !X.lump_req || !S.mg || S.mg->mixed || S.mg->dist) return;
    const MgHier& H = *S.mg;
    const MgGeom &g0 = H.lev[0].geo, &g1 = H.lev[1].geo;
    XrLumpGeom G;
    G.S0 = g0.S0, G.S1 = g0.S1, G.nt = g0.nt, G.has_z = g0.has_z;
    G.colz = g0.colz, G.cold = g0.cold;
    G.S0c = g1.S0, G.S1c = g1.S1;
    if (X.lump_built && X.lump_geo == G) return;
    X.lump_built = true;
    X.lump_ok = false;
    X.lump_geo = G;
    const XrLumpHost L = xr_lump_build(G, X.m_x, X.st_rp.data(), X.st_ci.data(), X.st_val.data(), XR_LONG);
    if (!L.ok) {
        X.lump_why = L.why;
        return;
    }
    hipStream_t st = S.stream;
    auto up = [&](auto& buf, const auto& v) {
        buf.alloc(std::max<int64_t>((int64_t)v.size(), 1));
        if (!v.empty()) buf.upload(v.data(), (int64_t)v.size(), st);
    };
    up(X.l_tau, L.tau);
    up(X.l_node, L.node);
    up(X.l_ptr, L.ptr);
    up(X.l_row, L.row);
    up(X.l_w, L.w);
    up(X.l_longn, L.long_node);
    HIP_CHECK(hipStreamSynchronize(st));
    X.l_rows = L.nrows;
    X.l_nodes = (int64_t)L.node.size();
    X.l_ent = L.ptr.back();
    X.l_long = (int64_t)L.long_node.size();
    X.l_dev_bytes = (int64_t)(X.l_tau.bytes() + X.l_node.bytes() + X.l_ptr.bytes() + X.l_row.bytes() + X.l_w.bytes() +
                              X.l_longn.bytes());
    X.lump_why.clear();
    X.lump_ok = true;
}

// the extra rows ride this hierarchy: lumped on the coarse levels, exact on level 0
inline bool xr_lumped(const System& S) { return xr_active(S) && S.xr.lump_req && S.xr.lump_ok; }

// B_1 += the extra rows' lumped blocks for the current row scales (after mg_setup_lump1)
void mg_setup_lump_xr(System& S) {
    if (!xr_lumped(S)) return;
    const XrData& X = S.xr;
    const MgHier& H = *S.mg;
    const double4* T = reinterpret_cast<const double4*>(X.l_tau.p);
    const double* rs = S.rs.p + X.row0;
    const int has_z = H.lev[0].geo.has_z;
    if (X.l_nodes)
        hipLaunchKernelGGL(k_mg_lump_xr, dim3((unsigned)((X.l_nodes + 63) / 64)), dim3(64), 0, S.stream, X.l_nodes,
                           X.l_node.p, X.l_ptr.p, X.l_row.p, X.l_w.p, T, rs, H.nt, H.nbB, has_z, H.lev[1].B.p);
    if (X.l_long)
        hipLaunchKernelGGL(k_mg_lump_xr_long, dim3((unsigned)X.l_long), dim3(64), 0, S.stream, X.l_long, X.l_longn.p,
                           X.l_node.p, X.l_ptr.p, X.l_row.p, X.l_w.p, T, rs, H.nt, H.nbB, has_z, H.lev[1].B.p);
    KERNEL_CHECK();
}

// algorithmic bytes of one lumping pass: per entry its row id and w¹ (12 B) with the row's rs and τ
// gathers (40 B); per touched node its id, pointer and block read and written
double xr_lump_bytes(const System& S) {
    const XrData& X = S.xr;
    return 52.0 * (double)X.l_ent + (12.0 + 16.0 * (double)S.mg->nbB) * (double)X.l_nodes;
}

// A rank of a distributed solve (lsqr_cg_dist.inc group_mg_build): the global level-0 class tables
// (from the global stencil description, lsq_dist_set_global), the global level-0 geometry, and the
// rank's window rows (global node rows: window start wa, owned [oa, ob)).
struct MgDistInfo {
    std::vector<NsTable> T0;
    int S0g;
    int wa, oa, ob;
};

bool mg_build_mixed(System& S, std::string& why);

// k_mg_tile_kt's compressed interior-class rows (MgLevel::tkc) from a tiled level's column-mode
// table, when they hold it exactly: every 3-D grid has 12 epochs with the 5-class dim-2 layout
// (K2 = 2), every t of a class has the class row's taps, and every tap that reaches outside the
// column is zero.  Otherwise tile_kt stays 0 (k_mg_tile).  LSQ_MG_TILE_KT: 0 off, 1 scalar
// coefficient loads, 2 (default) coefficients staged in LDS.
void mg_tile_kt_table(MgLevel& V, const std::vector<double>& coefc, hipStream_t stream) {
    const int mode = getenv("LSQ_MG_TILE_KT") ? atoi(getenv("LSQ_MG_TILE_KT")) : 2;   // per build (tests toggle it)
    V.tile_kt = 0;
    if (mode <= 0) return;
    std::vector<double> tk;
    size_t lds = 0, ncmax = 0;
    for (int g = 0; g < V.cgh.n_grids; ++g) {
        const CgGrid& C = V.cgh.g[g];
        V.tk.c0[g] = (int32_t)tk.size();
        if (!C.noff) continue;
        const int S2 = C.shape[2];
        if (S2 != 1 && (S2 != 12 || C.K[2] != 2)) return;
        const int NC = S2 == 1 ? 1 : 5, KT = (NC - 1) / 2;
        const double* row = coefc.data() + C.coefc0 + (size_t)(C.K[0] * C.ncls[1] + C.K[1]) * C.rowlen;
        size_t nc = 0;
        for (int gi = 0; gi < C.ngrp[0] + C.ngrp[1] + C.ngrp[2]; ++gi) {
            const int DT = gi < C.ngrp[0] ? 0 : gi < C.ngrp[0] + C.ngrp[1] ? 1 : 2, W = 2 * DT + 1;
            if (S2 == 1 && DT) return;
            const double* cg = row + C.gc[gi];
            for (int c = 0; c < NC; ++c) {
                const int rep = c < KT ? c : (c > KT ? S2 - NC + c : KT);   // a t of class c
                for (int d = 0; d < W; ++d) tk.push_back(cg[rep * W + d]);
            }
            for (int t = 0; t < S2; ++t)
                for (int d = 0; d < W; ++d) {
                    const double v = cg[t * W + d], vc = tk[tk.size() - (size_t)NC * W + rw_tc(t, S2, KT) * W + d];
                    const int tt = t + d - DT;
                    if ((tt < 0 || tt >= S2) ? v != 0.0 : v != vc) return;   // not class-compressible
                }
            nc += (size_t)NC * W;
        }
        ncmax = std::max(ncmax, nc);
        const int tp = S2 == 1 ? 1 : MG_TKP;
        lds = std::max(lds, sizeof(double) * (size_t)(MG_T + 2 * C.hy) * (MG_T + 2 * C.hx) * tp);
    }
    if (mode >= 2) lds += sizeof(double) * ncmax;
    if (lds > 64 * 1024) return;
    V.tkc.alloc(std::max<int64_t>((int64_t)tk.size(), 1));
    V.tkc.upload(tk.data(), (int64_t)tk.size(), stream);
    HIP_CHECK(hipStreamSynchronize(stream));   // tk is released here
    V.tk_lds = lds;
    V.tile_kt = mode >= 2 ? 2 : 1;
}

bool mg_build(System& S, std::string& why, const MgDistInfo* di) {
    if (S.dist && !di) { why = "multigrid: a rank builds its levels through the group (lsq_dist_set_global)"; return false; }
    // lsq_set_cg_scaled: the Galerkin coarse tables of such parts are not class tables any more
    if (!S.cg_sc.empty()) { why = "multigrid: per-row constraint scales"; return false; }
    if (S.mx && !di && !(S.cgh.colmode && S.dmf.ok)) return mg_build_mixed(S, why);
    if (!S.cg_ok || !S.cgh.colmode) { why = "multigrid: needs the column-mode normal-stencil operator"; return false; }
    if (!cg_use_dmf(S)) { why = "multigrid: needs matrix-free data rows (one shared (y, x) lattice)"; return false; }
    ensure_blocks(S);
    if (!S.blk_affine || S.blk_kmax > BJ_LANES) { why = "multigrid: needs affine per-node column blocks"; return false; }
    auto H = new MgHier();
    std::unique_ptr<MgHier> guard(H);
    const int ng = (int)S.cg_ns.size();
    for (int g = 0; g < ng; ++g) {
        const NsTable& T = S.cg_ns[g];
        if (!T.on) continue;
        if (T.shape[2] == 1 && H->gz < 0) H->gz = g;
        else if (T.shape[2] > 1 && H->gd < 0) H->gd = g;
        else { why = "multigrid: more than one z0-like or dz-like grid"; return false; }
    }
    if (H->gz < 0 && H->gd < 0) { why = "multigrid: no stencil grid"; return false; }
    const NsTable* Tz = H->gz >= 0 ? &S.cg_ns[H->gz] : nullptr;
    const NsTable* Td = H->gd >= 0 ? &S.cg_ns[H->gd] : nullptr;
    const int S0 = Tz ? Tz->shape[0] : Td->shape[0], S1 = Tz ? Tz->shape[1] : Td->shape[1];
    if (Tz && Td && (Td->shape[0] != S0 || Td->shape[1] != S1)) { why = "multigrid: z0 and dz lattices differ"; return false; }
    if (S.dmf.S0 != S0 || S.dmf.S1 != S1) { why = "multigrid: point lattice differs from the grids"; return false; }
    const int nt = Td ? Td->shape[2] : 0;
    const int64_t nodes = (int64_t)S0 * S1;
    MgGeom g0{};
    g0.S0 = S0;
    g0.S1 = S1;
    g0.nt = nt;
    g0.has_z = Tz ? 1 : 0;
    g0.colz = Tz ? Tz->col0 : 0;
    g0.cold = Td ? Td->col0 : 0;
    g0.nodes = nodes;
    g0.n_full = nodes * ((Tz ? 1 : 0) + nt);
    g0.fd_s1 = make_fastdiv((uint32_t)S1);
    g0.fd_nt = make_fastdiv((uint32_t)std::max(nt, 1));
    if (g0.n_full >= (int64_t)1 << 31) { why = "multigrid: more than 2^31 columns"; return false; }
    if (g0.n_full != S.n_full) { why = "multigrid: the column space holds more than the z0 / dz grids"; return false; }
    if (Tz && Td && !((g0.colz == 0 && g0.cold == nodes) || (g0.cold == 0 && g0.colz == nodes * nt))) {
        why = "multigrid: grids are not contiguous in the column space";
        return false;
    }
    if (S.dmf.n2 > 1 || S.dmf.n3 > 1 || (S.dmf.n2 && (!Tz || S.dmf.col2[0] != g0.colz)) ||
        (S.dmf.n3 && (!Td || S.dmf.col3 != g0.cold))) {
        why = "multigrid: data rows do not interpolate the stencil grids";
        return false;
    }
    if (nt > 16 || 3 * nt > MG_NB_MAX) { why = "multigrid: more than 16 epochs"; return false; }
    H->withz = S.dmf.n2 ? 1 : 0;
    // slots from the level-0 affine blocks: z0 first (if any), then the kept epochs ascending
    const int k = S.blk_kmax;
    if (S.nblk != nodes) { why = "multigrid: one column block per node required"; return false; }
    MgSlots sl{};
    sl.zs = -1;
    sl.nt = nt;
    std::vector<int> kept(nt, 0);
    for (int s = 0; s < k; ++s) {
        const int64_t base = S.blk_aff.base[s], stride = S.blk_aff.stride[s];
        if (Tz && base == g0.colz && stride == 1) {
            if (s != 0) { why = "multigrid: z0 must be the first column of a node block"; return false; }
            sl.t[s] = -1;
            sl.zs = s;
        } else if (Td && stride == nt && base >= g0.cold && base < g0.cold + nt) {
            sl.t[s] = (int)(base - g0.cold);
            if (s > 0 && sl.t[s - 1] >= sl.t[s]) { why = "multigrid: node block epochs not ascending"; return false; }
            kept[sl.t[s]] = 1;
        } else {
            why = "multigrid: node blocks do not match the grid layout";
            return false;
        }
    }
    int nrem = 0;
    for (int t = 0; t < nt; ++t)
        if (!kept[t]) {
            ++nrem;
            H->tref = t;
        }
    if (nrem > 1 || (Tz && sl.zs < 0)) { why = "multigrid: unsupported column removal"; return false; }
    for (int s = 0; s < k; ++s) {
        sl.lo[s] = sl.hi[s] = -1;
        for (int s2 = 0; s2 < k; ++s2) {
            if (sl.t[s] >= 0 && sl.t[s2] >= 0 && sl.t[s2] == sl.t[s] - 1) sl.lo[s] = s2;
            if (sl.t[s] >= 0 && sl.t[s2] >= 0 && sl.t[s2] == sl.t[s] + 1) sl.hi[s] = s2;
        }
    }
    H->sl = sl;
    H->kslot = k;
    H->deg = MG_DEG;
    H->deg0 = MG_DEG0;
    if (const char* e = getenv("LSQ_MG_DEG")) H->deg = std::max(1, atoi(e));
    if (const char* e = getenv("LSQ_MG_DEG0")) H->deg0 = std::max(1, atoi(e));
    H->deg0_pre = getenv("LSQ_MG_DEG0_PRE") ? std::max(1, atoi(getenv("LSQ_MG_DEG0_PRE"))) : H->deg0;
    if (const char* e = getenv("LSQ_MG_FUSE")) H->fuse = atoi(e) & 5;
    H->nt = nt;
    g0.tref = H->tref;
    H->nbB = std::max(2, (3 * nt + 1) & ~1);
    // levels
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, S.device);
    H->lev.resize(1);
    {
        MgLevel& V = H->lev[0];
        V.geo = g0;
        V.aff = mg_affine(g0, sl, k);
        for (int s = 0; s < k; ++s)
            if (V.aff.base[s] != S.blk_aff.base[s] || V.aff.stride[s] != S.blk_aff.stride[s]) {
                why = "multigrid: node block layout mismatch";
                return false;
            }
        V.ns = S.cg_ns;
        V.gB = mg_grid_blocks(nodes);
        // level 0's smoothing writes the CG step's ρ partials (MG_RHO) that k_cg_beta sums over the CG
        // update's grid, and the update's fused first smoothing step feeds level 0: one grid for both
        // (round 6: capping either alone broke the solve — 1 or 21 764 iterations)
        if (V.gB != cg_grids(S, 4).gB) {
            why = "multigrid: level-0 smoothing grid differs from the CG update grid";
            return false;
        }
        V.gN = cg_grid_normal(S);
        V.part.alloc(V.gN + S.cgh.pad[0]);
    }
    // coarse levels: Galerkin of the level-0 tables — a rank's are its window's partial ones, so
    // its coarse levels start from the GLOBAL level-0 tables and geometry (replicated levels)
    const std::vector<NsTable>* prev_ns = &H->lev[0].ns;
    MgGeom prev_geo = g0;
    if (di) {
        if ((int)di->T0.size() != ng) { why = "multigrid: the global description has other grids"; return false; }
        H->dist = true;
        H->wa = di->wa;
        H->oa = di->oa;
        H->ob = di->ob;
        prev_ns = &di->T0;
        prev_geo.S0 = di->S0g;
        prev_geo.nodes = (int64_t)prev_geo.S0 * prev_geo.S1;
        prev_geo.n_full = prev_geo.nodes * ((Tz ? 1 : 0) + nt);
        prev_geo.colz = (Tz && Td && g0.colz != 0) ? prev_geo.nodes * nt : 0;
        prev_geo.cold = (Tz && Td && g0.cold != 0) ? prev_geo.nodes : 0;
        H->g0g = prev_geo;
    } else {
        H->g0g = g0;
    }
    static const int coarse = getenv("LSQ_MG_COARSE") ? std::max(3, atoi(getenv("LSQ_MG_COARSE"))) : MG_COARSE;
    static const int64_t coarse_cols = getenv("LSQ_MG_COARSE_COLS") ? atoll(getenv("LSQ_MG_COARSE_COLS")) : MG_COARSE_COLS;
    while (std::max(prev_geo.S0, prev_geo.S1) > coarse && !(H->lev.size() > 1 && H->lev.back().coarsest)) {
        MgLevel V;
        V.ns.resize(ng);
        for (int g = 0; g < ng; ++g)
            if (!ns_galerkin((*prev_ns)[g], V.ns[g], why)) return false;
        MgGeom G = prev_geo;
        G.S0 = G.S0 / 2 + 1;
        G.S1 = G.S1 / 2 + 1;
        G.nodes = (int64_t)G.S0 * G.S1;
        G.n_full = G.nodes * ((Tz ? 1 : 0) + nt);
        G.fd_s1 = make_fastdiv((uint32_t)G.S1);
        G.colz = (Tz && Td && g0.colz != 0) ? G.nodes * nt : 0;
        G.cold = (Tz && Td && g0.cold != 0) ? G.nodes : 0;
        for (int g = 0; g < ng; ++g) {
            V.ns[g].col0 = (g == H->gz) ? G.colz : (g == H->gd ? G.cold : 0);
            V.ns[g].node0 = 0;
        }
        V.geo = G;
        V.aff = mg_affine(G, sl, k);
        V.coarsest = std::max(G.S0, G.S1) <= coarse || G.n_full <= coarse_cols;
        static const int64_t direct_max = getenv("LSQ_MG_DIRECT") ? atoll(getenv("LSQ_MG_DIRECT")) : MG_DIRECT;
        // k_mg_tile + k_mg_edge on coarse levels with more than LSQ_MG_TILE columns (default
        // MG_TILE_MIN; 0: off — ring / direct kernels) whose grids have interior classes
        static const int64_t tile_min = getenv("LSQ_MG_TILE") ? atoll(getenv("LSQ_MG_TILE")) : MG_TILE_MIN;
        V.direct = !V.coarsest && G.n_full <= direct_max;
        V.gB = mg_grid_blocks(G.nodes);
        std::vector<double> coef, coefc;
        if (!V.coarsest && tile_min > 0 && G.n_full > tile_min) {   // column-mode tables, dim 2 ≤ 12
            std::vector<double> cf, cc;
            CgDesc d{};
            std::string w2;
            if (cg_layout(V.ns, cus, d, cf, cc, w2) && d.colmode && d.maxt3 <= 12) {
                size_t lds = 0;
                int nt = 0;
                bool ok = true;
                for (int g = 0; g < d.n_grids; ++g) {
                    const CgGrid& C = d.g[g];
                    if (!C.noff) continue;
                    ok = ok && C.ncls[0] == 2 * C.K[0] + 1 && C.ncls[1] == 2 * C.K[1] + 1 && C.shape[0] > 2 * C.K[0] &&
                         C.shape[1] > 2 * C.K[1];
                    const int tp = mg_tile_tp(C.shape[2] == 1 ? 1 : 12);
                    lds = std::max(lds, sizeof(double) * (size_t)(MG_T + 2 * C.hy) * (MG_T + 2 * C.hx) * tp);
                    nt += ((C.shape[0] + MG_T - 1) / MG_T) * ((C.shape[1] + MG_T - 1) / MG_T);   // one workgroup per grid tile
                }
                if (ok && lds <= 64 * 1024) {
                    V.tile = true;
                    V.direct = false;
                    V.tile_lds = lds;
                    V.tile_grid = nt;
                }
            }
        }
        if (!V.coarsest && !V.direct) {
            if (!cg_layout(V.ns, cus, V.cgh, coef, coefc, why)) return false;
            if (!V.cgh.colmode) { why = "multigrid: a coarse level is not column-mode"; return false; }
            if (V.tile) mg_tile_kt_table(V, coefc, S.stream);
            V.cgd.alloc(1);
            V.cgd.upload(&V.cgh, 1, S.stream);
            V.gN = cg_ns_grid(V.cgh);
            V.part.alloc(V.gN + V.cgh.pad[0]);
        } else {
            for (int g = 0; g < ng; ++g) coef.insert(coef.end(), V.ns[g].coef.begin(), V.ns[g].coef.end());
            V.gN = 0;
        }
        // device table views (tile-layout offsets into `coef`, grid order)
        int off0 = 0;
        std::vector<int32_t> offs;
        for (int g = 0; g < ng; ++g) {
            const int c0 = (V.coarsest || V.direct) ? off0 : V.cgh.g[g].coef0;
            if (g == H->gz) V.tz = mg_tab(V.ns[g], c0);
            if (g == H->gd) V.td = mg_tab(V.ns[g], c0);
            off0 += (int)V.ns[g].coef.size();
        }
        for (const MgTab* T : {&V.tz, &V.td}) {
            const NsTable* N = (T == &V.tz) ? (H->gz >= 0 ? &V.ns[H->gz] : nullptr) : (H->gd >= 0 ? &V.ns[H->gd] : nullptr);
            if (N)
                for (const auto& o : N->offs) offs.insert(offs.end(), {o[0], o[1], o[2]});
        }
        for (const MgTab* T : {&V.tz, &V.td}) {   // column deltas of the offsets (k_mg_direct)
            const NsTable* N = (T == &V.tz) ? (H->gz >= 0 ? &V.ns[H->gz] : nullptr) : (H->gd >= 0 ? &V.ns[H->gd] : nullptr);
            if (N)
                for (const auto& o : N->offs) offs.push_back((o[0] * G.S1 + o[1]) * N->shape[2] + o[2]);
        }
        V.coef.alloc(std::max<int64_t>((int64_t)coef.size(), 1));
        V.coef.upload(coef.data(), (int64_t)coef.size(), S.stream);
        if (!V.coarsest && !V.direct) {
            V.coefc.alloc(std::max<int64_t>((int64_t)coefc.size(), 1));
            V.coefc.upload(coefc.data(), (int64_t)coefc.size(), S.stream);
        }
        V.offs.alloc(std::max<int64_t>((int64_t)offs.size(), 1));
        V.offs.upload(offs.data(), (int64_t)offs.size(), S.stream);
        const int64_t nf = G.n_full;
        for (DBuf<double>* b : {&V.x, &V.r, &V.q, &V.d, &V.res}) {
            b->alloc(nf);
            b->zero(S.stream);
        }
        V.B.alloc(G.nodes * H->nbB);
        if (!V.coarsest) {
            const int npk = k * (k + 1) / 2, npks = lf_stride(npk);
            V.Ri.alloc(G.nodes * npk);
            V.Lf.alloc(G.nodes * npks);
            std::vector<int64_t> ptr(G.nodes + 1);
            for (int64_t b = 0; b <= G.nodes; ++b) ptr[b] = b * k;
            V.ptr.alloc(G.nodes + 1);
            V.ptr.upload(ptr.data(), G.nodes + 1, S.stream);
        } else {
            V.npad = (nf + 63) / 64 * 64;
            V.dN.alloc(V.npad * V.npad);
            V.dRi.alloc(V.npad * V.npad);
            V.tmp.alloc(V.npad);
            V.tmp.zero(S.stream);
        }
        H->lev.push_back(std::move(V));
        prev_ns = &H->lev.back().ns;
        prev_geo = H->lev.back().geo;
    }
    if (H->lev.size() < 2) { why = "multigrid: grid too small for a coarse level"; return false; }
    // field-valued parts (on the z0 grid, templates within ±1): their exact Galerkin rows per
    // coarse z0 node, from the level-0 rows (scratch)
    if (!S.cg_var.empty()) {
        for (const CgVar& V : S.cg_var)
            if (H->gz < 0 || V.col0 != g0.colz || V.S0 != S0 || V.S1 != S1 || V.R != 1) {
                why = "multigrid: field-valued parts must be ±1 templates on the z0 grid";
                return false;
            }
        H->var = true;
        H->part_v.alloc(std::max(S.cg_nvb, 1));
        DBuf<double> N0(nodes * MG_VN);
        N0.zero(S.stream);
        for (const CgVar& V : S.cg_var)
            hipLaunchKernelGGL(k_mg_var_n0, dim3(grid_for(nodes)), dim3(BLOCK), 0, S.stream, V, N0.p);
        KERNEL_CHECK();
        for (size_t l = 1; l < H->lev.size(); ++l) H->lev[l].vz.alloc(H->lev[l].geo.nodes * MG_VN);
        const MgGeom& C1 = H->lev[1].geo;
        if (di)   // the rank's partial level-1 rows; the group sums them, then mg_var_coarse
            hipLaunchKernelGGL(k_mg_var_galerkin_win, dim3(grid_for(C1.nodes)), dim3(BLOCK), 0, S.stream, g0.S0, g0.S1,
                               di->wa, C1.S0, C1.S1, N0.p, H->lev[1].vz.p);
        else
            hipLaunchKernelGGL(k_mg_var_galerkin, dim3(grid_for(C1.nodes)), dim3(BLOCK), 0, S.stream, g0.S0, g0.S1,
                               C1.S0, C1.S1, N0.p, H->lev[1].vz.p);
        KERNEL_CHECK();
        HIP_CHECK(hipStreamSynchronize(S.stream));
    }
    H->lam.alloc(2 * H->lev.size());
    H->lam.zero(S.stream);
    H->scal.alloc(4);   // [0, 2): level 0 / the V-cycle; [2, 4): the coarse levels' concurrent power steps
    H->scal.zero(S.stream);
    H->mst.alloc(1);
    CgState z{};
    H->mst.upload(&z, 1, S.stream);
    H->part1.alloc(2 * NPART);
    H->part2.alloc(2 * NPART);
    H->part_t.alloc(NPART);
    H->part_x.alloc(XR_NPART);
    H->d0.alloc(S.n_full);
    H->d0.zero(S.stream);
    H->res0.alloc(S.n_full);
    H->res0.zero(S.stream);
    H->err.alloc(1);
    H->ndead.alloc(1);
    HIP_CHECK(hipStreamSynchronize(S.stream));
    S.mg = guard.release();
    if (!di) mg_var_coarse(S);
    if (!di) xr_lump_prepare(S);
    return true;
}

// z0 on a 2× refinement of the dz lattice: the level-1 system S.mx (shared dz lattice: z0 class
// table Galerkin-restricted, dz table unchanged, matrix-free data rows on the dz lattice, node
// blocks z0 + kept epochs) and its ordinary hierarchy; this level smooths the z0 columns only.
bool mg_build_mixed(System& S, std::string& why) {
    System& X = *S.mx;
    if (!S.cg_ok || !S.cgh.colmode) { why = "multigrid: needs the column-mode normal-stencil operator"; return false; }
    if (!S.cg_var.empty()) { why = "multigrid: field-valued parts with z0 on a finer lattice"; return false; }
    MgMix m{};
    m.z0col = S.mx_z0col;
    m.dzcol = S.mx_dzcol;
    m.Sf0 = S.mx_Sf0;
    m.Sf1 = S.mx_Sf1;
    m.Sc0 = S.mx_Sc0;
    m.Sc1 = S.mx_Sc1;
    m.nt = S.mx_nt;
    m.nz = (int64_t)m.Sf0 * m.Sf1;
    m.nsz = (int64_t)m.Sc0 * m.Sc1;
    const NsTable *Tz = nullptr, *Td = nullptr;
    for (const NsTable& T : S.cg_ns) {
        if (!T.on) continue;
        if (T.shape[2] == 1 && T.shape[0] == m.Sf0 && T.shape[1] == m.Sf1 && T.col0 == m.z0col && !Tz) Tz = &T;
        else if (T.shape[2] == m.nt && T.shape[0] == m.Sc0 && T.shape[1] == m.Sc1 && T.col0 == m.dzcol && !Td) Td = &T;
        else { why = "multigrid: grids other than z0 (fine lattice) and dz"; return false; }
    }
    if (!Tz || !Td) { why = "multigrid: needs stencil rows on both the z0 and the dz grid"; return false; }
    if (S.n_full != m.nz + m.nsz * m.nt) { why = "multigrid: the column space holds more than the z0 / dz grids"; return false; }
    // the removed columns: at most one epoch of every dz node, no z0 column
    std::vector<int32_t> cm(S.n_full);
    S.colmap.download(cm.data(), S.n_full, S.stream);
    HIP_CHECK(hipStreamSynchronize(S.stream));
    for (int64_t j = 0; j < m.nz; ++j)
        if (cm[m.z0col + j] < 0) { why = "multigrid: removed z0 columns"; return false; }
    m.tref = -1;
    for (int t = 0; t < m.nt; ++t)
        if (cm[m.dzcol + t] < 0) {
            if (m.tref >= 0) { why = "multigrid: unsupported column removal"; return false; }
            m.tref = t;
        }
    for (int64_t e = 0; e < m.nsz * m.nt; ++e)
        if ((cm[m.dzcol + e] < 0) != ((int)(e % m.nt) == m.tref)) { why = "multigrid: unsupported column removal"; return false; }
    // level 1: the tables on the dz lattice, z0 first
    NsTable Tz1, Td1 = *Td;
    if (!ns_galerkin(*Tz, Tz1, why)) return false;
    if (Tz1.shape[0] != m.Sc0 || Tz1.shape[1] != m.Sc1) { why = "multigrid: z0 lattice is not a 2x refinement"; return false; }
    Tz1.col0 = 0;
    Tz1.node0 = 0;
    Td1.col0 = m.nsz;
    Td1.node0 = 0;
    X.cg_ns = {Tz1, Td1};
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, S.device);
    std::vector<double> coef, coefc;
    CgDesc c{};
    if (!cg_layout(X.cg_ns, cus, c, coef, coefc, why)) return false;
    if (!c.colmode) { why = "multigrid: the dz-lattice level is not column-mode"; return false; }
    X.cgh = c;
    X.cgd.alloc(1);
    X.cgd.upload(&X.cgh, 1, S.stream);
    X.cg_coef.alloc(std::max<int64_t>((int64_t)coef.size(), 1));
    X.cg_coef.upload(coef.data(), (int64_t)coef.size(), S.stream);
    X.cg_coefc.alloc(std::max<int64_t>((int64_t)coefc.size(), 1));
    X.cg_coefc.upload(coefc.data(), (int64_t)coefc.size(), S.stream);
    X.cg_var.clear();
    X.cg_nvb = 0;
    X.cg_ok = true;
    X.n_full = m.nsz * (1 + m.nt);
    X.G.n = m.nsz * (1 + m.nt - (m.tref >= 0 ? 1 : 0));
    // node blocks: z0, then the kept epochs
    const int k = 1 + m.nt - (m.tref >= 0 ? 1 : 0);
    if (k > BJ_LANES) { why = "multigrid: more than 16 columns per node"; return false; }
    X.nblk = m.nsz;
    X.blk_kmax = k;
    X.blk_affine = true;
    X.blk_aff = BlkAffine{};
    X.blk_aff.base[0] = 0;
    X.blk_aff.stride[0] = 1;
    for (int t = 0, s2 = 1; t < m.nt; ++t)
        if (t != m.tref) {
            X.blk_aff.base[s2] = m.nsz + t;
            X.blk_aff.stride[s2] = m.nt;
            ++s2;
        }
    std::vector<int64_t> ptr(m.nsz + 1);
    for (int64_t b = 0; b <= m.nsz; ++b) ptr[b] = b * k;
    X.blk_ptr.alloc(m.nsz + 1);
    X.blk_ptr.upload(ptr.data(), m.nsz + 1, S.stream);
    const int npk = k * (k + 1) / 2, npks = lf_stride(npk);
    X.blk_Lf.alloc(m.nsz * npks);
    X.blk_valid = true;
    cg_workspace(X);
    for (DBuf<double>* b : {&X.cg_x, &X.cg_s, &X.cg_z, &X.cg_q}) b->zero(S.stream);   // removed columns stay 0
    for (auto& b : X.cg_pb) b.zero(S.stream);
    mg_free(X.mg);
    X.mg = nullptr;
    if (!mg_build(X, why)) return false;
    auto H = new MgHier();
    std::unique_ptr<MgHier> guard(H);
    H->mixed = true;
    H->mix = m;
    H->deg0 = MG_DEG0;
    if (const char* e = getenv("LSQ_MG_DEG0")) H->deg0 = std::max(1, atoi(e));
    H->deg0_pre = getenv("LSQ_MG_DEG0_PRE") ? std::max(1, atoi(getenv("LSQ_MG_DEG0_PRE"))) : H->deg0;
    H->xdinv.alloc(m.nz);
    H->xpart.alloc(cg_grid_normal(S) + S.cgh.pad[0] + 1);
    H->xtz = mg_tab(Tz1, 0);
    H->xtd = mg_tab(Td1, (int)Tz1.coef.size());
    std::vector<double> xc(Tz1.coef);
    xc.insert(xc.end(), Td1.coef.begin(), Td1.coef.end());
    H->xcoef.alloc((int64_t)xc.size());
    H->xcoef.upload(xc.data(), (int64_t)xc.size(), S.stream);
    H->xB.alloc(m.nsz * X.mg->nbB);
    H->xRi.alloc(m.nsz * npk);
    H->xptr.alloc(m.nsz + 1);
    H->xptr.upload(ptr.data(), m.nsz + 1, S.stream);
    H->lam.alloc(2);
    H->lam.zero(S.stream);
    H->scal.alloc(4);   // [0, 2): level 0 / the V-cycle; [2, 4): the coarse levels' concurrent power steps
    H->scal.zero(S.stream);
    H->mst.alloc(1);
    CgState z{};
    H->mst.upload(&z, 1, S.stream);
    H->part1.alloc(2 * NPART);
    H->part2.alloc(2 * NPART);
    H->part_t.alloc(NPART);
    H->d0.alloc(S.n_full);
    H->d0.zero(S.stream);
    H->err.alloc(1);
    H->ndead.alloc(1);
    HIP_CHECK(hipStreamSynchronize(S.stream));
    S.mg = guard.release();
    return true;
}

// ---- host: launches ------------------------------------------------------------------------------

// coarse levels: q += the Galerkin rows of the field-valued z0 parts (after the level's stencil
// kernels wrote q)
void mg_launch_var(System& S, MgHier& H, int l, const CgState* st, const double* z, const double* pold,
                   const double* betap, double* q) {
    if (!H.var || l == 0) return;
    const MgLevel& V = H.lev[l];
    hipLaunchKernelGGL(k_mg_var_apply, dim3(grid_for(V.geo.nodes)), dim3(BLOCK), 0, S.stream, st, V.geo, V.vz.p, z, pold,
                       betap, q);
}

// level 0 with lumped extra rows (xr_lumped): q += XᵀW_x²X p, exact as in the CG step, between the
// data rows' Ad·p and the node gather.  k_xr_fwd's partials go to the hierarchy's own scratch
// (nothing reads them here).
void mg_launch_xr(System& S, MgHier& H, const CgState* st, const double* p, double* q) {
    if (!xr_lumped(S)) return;
    xr_launch_fwd(S, st, nullptr, p, 1.0, H.part_x.p);
    xr_launch_atq(S, st, q);
}

// q = N_s x (+ the exact data rows on level 0) with p = z + β p_old formed by the ring kernel
// (β from betap; p_old may be null; p written to pnew when non-null).  The operand the x-edge
// correction and the data rows read is pnew, or z.
// ra, rb: node rows computed (a rank's partitioned coarse level: its owned rows; tile / direct only)
void mg_launch_op(System& S, MgHier& H, int l, const CgState* st, const double* z, const double* pold,
                  const double* betap, double* pnew, double* q, int ra = 0, int rb = 1 << 30) {
    MgLevel& V = H.lev[l];
    if (V.tile) {   // boundary-class nodes beside the interior tiles (disjoint writes of q)
        // LSQ_MG_TILE_DBG (development phase switches; results wrong when set): 1 skip the
        // compute, 2 skip the staging loads, 4 skip the 2-D grids
        static const int tile_dbg = getenv("LSQ_MG_TILE_DBG") ? atoi(getenv("LSQ_MG_TILE_DBG")) : 0;
        const int64_t ne = (V.tz.on ? mg_edge_count(V.geo.S0, V.geo.S1, V.tz.K0, V.tz.K1) : 0) +
                           (V.td.on ? mg_edge_count(V.geo.S0, V.geo.S1, V.td.K0, V.td.K1) * V.td.S2 : 0);
        const int nz = H.gz >= 0 ? V.tz.noff : 0;
        HIP_CHECK(hipEventRecord(S.ev_fork, S.stream));
        HIP_CHECK(hipStreamWaitEvent(S.side, S.ev_fork, 0));
        hipLaunchKernelGGL(k_mg_edge<8>, dim3((unsigned)std::max<int64_t>(1, (ne * 8 + BLOCK - 1) / BLOCK)), dim3(BLOCK),
                           0, S.side, st, V.geo, V.tz, V.td, V.offs.p, V.offs.p + 3 * nz, V.coef.p, z, pold, betap, q,
                           ra, rb);
        HIP_CHECK(hipEventRecord(S.ev_join, S.side));
        if (V.tile_kt == 2)
            hipLaunchKernelGGL(k_mg_tile_kt<true>, dim3(V.tile_grid), dim3(BLOCK), V.tk_lds, S.stream, st, V.cgd.p,
                               V.tkc.p, V.tk, z, pold, betap, pnew, q, ra, rb);
        else if (V.tile_kt == 1)
            hipLaunchKernelGGL(k_mg_tile_kt<false>, dim3(V.tile_grid), dim3(BLOCK), V.tk_lds, S.stream, st, V.cgd.p,
                               V.tkc.p, V.tk, z, pold, betap, pnew, q, ra, rb);
        else
            hipLaunchKernelGGL(k_mg_tile<12>, dim3(V.tile_grid), dim3(BLOCK), V.tile_lds, S.stream, st, V.cgd.p,
                               V.coefc.p, z, pold, betap, pnew, q, tile_dbg, ra, rb);
        HIP_CHECK(hipStreamWaitEvent(S.stream, S.ev_join, 0));
        mg_launch_var(S, H, l, st, z, pold, betap, q);
        return;
    }
    if (V.direct) {
        const int nz = H.gz >= 0 ? V.tz.noff : 0, nd = H.gd >= 0 ? V.td.noff : 0;
        const int32_t *oz = V.offs.p, *od = oz + 3 * nz, *dz = od + 3 * nd, *dd = dz + nz;
        // lanes per column: about 2 M lanes in flight, 4..64
        const int64_t nf = V.geo.n_full;
        const int lpc = nf <= (1 << 15) ? 64 : nf <= (1 << 18) ? 16 : 4;
        const int cpb = BLOCK / lpc;
        const dim3 grid((unsigned)std::min<int64_t>((nf + cpb - 1) / cpb, 8 * MAX_GRID));
        if (lpc == 64)
            hipLaunchKernelGGL(k_mg_direct<64>, grid, dim3(BLOCK), 0, S.stream, st, V.geo, V.tz, V.td, oz, od, dz, dd,
                               V.coef.p, z, pold, betap, pnew, q, ra, rb);
        else if (lpc == 16)
            hipLaunchKernelGGL(k_mg_direct<16>, grid, dim3(BLOCK), 0, S.stream, st, V.geo, V.tz, V.td, oz, od, dz, dd,
                               V.coef.p, z, pold, betap, pnew, q, ra, rb);
        else
            hipLaunchKernelGGL(k_mg_direct<4>, grid, dim3(BLOCK), 0, S.stream, st, V.geo, V.tz, V.td, oz, od, dz, dd,
                               V.coef.p, z, pold, betap, pnew, q, ra, rb);
        mg_launch_var(S, H, l, st, z, pold, betap, q);
        return;
    }
    const CgDesc& ch = l ? V.cgh : S.cgh;
    const CgDesc* cd = l ? V.cgd.p : S.cgd.p;
    const double* coefc = l ? V.coefc.p : S.cg_coefc.p;
    const double* coef = l ? V.coef.p : S.cg_coef.p;
    cg_launch_ns(ch, cd, coefc, S.stream, st, z, pold, pnew, q, V.part.p, betap);
    const double* p = pnew ? pnew : z;
    if (l) {
        hipLaunchKernelGGL(k_cg_xedge<8>, dim3(ch.pad[0]), dim3(BLOCK), 0, S.stream, st, cd, coef, p, q, V.part.p + V.gN);
        mg_launch_var(S, H, l, st, z, pold, betap, q);
    } else if (!H.var) {   // exact data rows: t = Ad·p and the x-edge correction in one launch, then q += Adᵀt
        const CgGrids g = cg_grids(S, 3);
        const double4* P = reinterpret_cast<const double4*>(S.dmf_pt.p);
        hipLaunchKernelGGL(k_cg_ad_xedge<8>, dim3(g.gD + ch.pad[0]), dim3(BLOCK), 0, S.stream, st, S.dmf, P, p, S.cg_t.p,
                           H.part_t.p, g.gD, cd, coef, q, V.part.p + V.gN);
        mg_launch_xr(S, H, st, p, q);
        cg_launch_dmf_atq(S, st, S.cg_t.p, q);
    } else {   // field-valued parts: the x-edge correction and their rows beside t = Ad·p (side stream)
        HIP_CHECK(hipEventRecord(S.ev_fork, S.stream));
        HIP_CHECK(hipStreamWaitEvent(S.side, S.ev_fork, 0));
        hipLaunchKernelGGL(k_cg_xedge<8>, dim3(ch.pad[0]), dim3(BLOCK), 0, S.side, st, cd, coef, p, q, V.part.p + V.gN);
        if (H.var) cg_launch_var(S, p, q, H.part_v.p, S.side, st);   // field-valued parts: exact, as in the CG step
        HIP_CHECK(hipEventRecord(S.ev_join, S.side));
        const CgGrids g = cg_grids(S, 3);
        const double4* P = reinterpret_cast<const double4*>(S.dmf_pt.p);
        hipLaunchKernelGGL(k_cg_dmf_ad, dim3(g.gD), dim3(BLOCK), 0, S.stream, st, S.dmf, P, p, S.cg_t.p, H.part_t.p);
        HIP_CHECK(hipStreamWaitEvent(S.stream, S.ev_join, 0));
        mg_launch_xr(S, H, st, p, q);   // after the join: the x-edge pass on S.side also updates q
        cg_launch_dmf_atq(S, st, S.cg_t.p, q);
    }
}

struct MgVec {
    const double* r;
    double *x, *q, *d, *res;
};
MgVec mg_vecs(System& S, MgHier& H, int l) {
    if (l == 0) return {S.cg_s.p, S.cg_z.p, S.cg_q.p, H.d0.p, H.res0.p};
    MgLevel& V = H.lev[l];
    return {V.r.p, V.x.p, V.q.p, V.d.p, V.res.p};
}

// nodes [n0, n1) (n1 < 0: all): a rank's partitioned coarse level smooths its owned node rows — the
// block ids shift by n0 (columns through the affine map, factors and lumped blocks by offset)
void mg_launch_smooth(System& S, MgHier& H, int l, const CgState* st, const MgVec& v, int mode, int step,
                      double* part, double* part2, int64_t n0 = 0, int64_t n1 = -1) {
    MgLevel& V = H.lev[l];
    const int npk = H.kslot * (H.kslot + 1) / 2, npks = lf_stride(npk);
    const lf_t* Lf = l ? V.Lf.p : S.blk_Lf.p;
    const double* B = l ? V.B.p : nullptr;
    BlkAffine aff = V.aff;
    int64_t nb = V.geo.nodes;
    int gB = V.gB;
    if (n1 >= 0) {
        for (int s = 0; s < H.kslot; ++s) aff.base[s] += n0 * aff.stride[s];
        Lf += n0 * npks;
        if (B) B += n0 * H.nbB;
        nb = n1 - n0;
        gB = mg_grid_blocks(nb);
    }
    const double* lam = H.lam.p + l;
    if (!(mode & (MG_POWER | MG_RES | MG_DX)) && step > 0) mode |= MG_NEEDD;
    using KernT = void (*)(const CgState*, int64_t, int, BlkAffine, int, MgSlots, int, const lf_t*, const double*,
                           const double*, const double*, double*, double*, double*, const double*, int, int, double*,
                           double*, const uint8_t*);
    KernT kern = nullptr;
    if (H.kslot <= 12) {   // the V-cycle's modes at Chebyshev degrees ≤ 2 as compile-time constants
        switch (mode) {
#define MG_SMODE(M) \
    case (M): kern = B ? k_mg_smooth<12, true, (M)> : k_mg_smooth<12, false, (M)>; break;
            MG_SMODE(MG_DX | MG_NOD)
            MG_SMODE(0)
            MG_SMODE(MG_NOD | MG_NEEDD)
            MG_SMODE(MG_NOD | MG_NEEDD | MG_RHO)
            MG_SMODE(MG_NOD)
            MG_SMODE(MG_NOD | MG_RHO)
            MG_SMODE(MG_XZERO | MG_NOD)
            MG_SMODE(MG_XZERO)
            MG_SMODE(MG_RES)
            MG_SMODE(MG_POWER)
#undef MG_SMODE
            default: kern = B ? k_mg_smooth<12, true, -1> : k_mg_smooth<12, false, -1>;
        }
    } else {
        kern = B ? k_mg_smooth<BJ_LANES, true, -1> : k_mg_smooth<BJ_LANES, false, -1>;
    }
    const uint8_t* live = (H.dist && l == 0) ? S.live.p : nullptr;   // a rank's level 0: owned columns only
    hipLaunchKernelGGL(kern, dim3(gB), dim3(BLOCK), 0, S.stream, st, nb, npks, aff, H.kslot, H.sl, H.nbB, Lf, B, v.r, v.q,
                       v.x, v.d, v.res, lam, mode, step, part, part2, live);
}

// one V-cycle from level l: x_l = V(r_l).  Level 0 reads r = S.cg_s and writes x = S.cg_z; its
// last smoothing step also leaves the partials of rᵀx in S.cg_part_r (ρ of the CG step).
void mg_vcycle(System& S, MgHier& H, int l, const CgState* st, bool x1_ready = false) {
    MgLevel& V = H.lev[l];
    const MgVec v = mg_vecs(S, H, l);
    const double* zero = H.scal.p + 1;   // β = 0
    if (V.coarsest) {   // x = N⁻¹ r with the explicit inverse (dN holds Ri·Riᵀ after set-up)
        const int64_t n = V.geo.n_full;
        hipLaunchKernelGGL(k_mg_gemv, dim3((unsigned)std::min<int64_t>((n + 3) / 4, MAX_GRID)), dim3(BLOCK), 0, S.stream,
                           st, V.dN.p, n, V.npad, v.r, v.x);
        return;
    }
    // pre-smoothing from x = 0: d_0 = x_1, so step 1 reads x for it and d is stored only when a
    // later step needs it
    const int deg = l ? H.deg : H.deg0, dpre = l ? H.deg : H.deg0_pre;
    if (!x1_ready) mg_launch_smooth(S, H, l, st, v, MG_XZERO | (dpre <= 2 ? MG_NOD : 0), 0, nullptr, nullptr);
    for (int k = 1; k < dpre; ++k) {
        mg_launch_op(S, H, l, st, v.x, nullptr, zero, nullptr, v.q);
        mg_launch_smooth(S, H, l, st, v, (k == 1 ? MG_DX : 0) | (k == dpre - 1 ? MG_NOD : 0), k, nullptr, nullptr);
    }
    MgLevel& C = H.lev[l + 1];
    // restriction of the residual: level 0's r − q formed on the fly, a coarse level's res = r − q − B x
    // by an MG_RES pass of the smoother.  fuse bit 2: the restriction inside level ℓ+1's first
    // smoothing step (a smoothing level below, not the coarsest)
    const int lc = l + 1;
    const bool rsf = (H.fuse & 4) && H.kslot <= 12 && H.deg <= 2 && !C.coarsest;
    mg_launch_op(S, H, l, st, v.x, nullptr, zero, nullptr, v.q);
    if (l) mg_launch_smooth(S, H, l, st, v, MG_RES, 0, nullptr, nullptr);
    if (rsf) {
        const int npk = H.kslot * (H.kslot + 1) / 2, npks = lf_stride(npk);
        const MgRestrictSrc rs{V.geo, C.geo, l ? v.res : v.r, l ? nullptr : v.q, C.r.p};
        hipLaunchKernelGGL(k_mg_restrict_smooth<12>, dim3(C.gB), dim3(BLOCK), 0, S.stream, st, C.geo.nodes, npks, C.aff,
                           H.kslot, H.sl, (const lf_t*)C.Lf.p, C.x.p, H.lam.p + lc, rs);
    } else {
        hipLaunchKernelGGL(k_mg_restrict, dim3(grid_for(C.geo.n_full)), dim3(BLOCK), 0, S.stream, st, V.geo, C.geo,
                           l ? v.res : v.r, l ? nullptr : v.q, C.r.p);
    }
    mg_vcycle(S, H, lc, st, rsf);
    hipLaunchKernelGGL(k_mg_prolong, dim3(grid_for(V.geo.n_full)), dim3(BLOCK), 0, S.stream, st, V.geo, C.geo, C.x.p,
                       v.x);
    for (int k = 0; k < deg; ++k) {
        mg_launch_op(S, H, l, st, v.x, nullptr, zero, nullptr, v.q);
        const bool last = l == 0 && k == deg - 1;
        mg_launch_smooth(S, H, l, st, v, (last ? MG_RHO : 0) | (k == deg - 1 ? MG_NOD : 0), k,
                         last ? S.cg_part_r.p : nullptr, nullptr);
    }
}

// A rank's replicated coarse levels [l, L): their V-cycle replayed from a hipGraph captured at the
// first call (LSQ_MG_RGRAPH=0: eager).  The eager path launches each of the ~30 small kernels of
// those levels from the host, and the host's launch rate left 4–6 µs gaps between kernels of 4–8
// µs (one rank's window at N = 8, `gpurun_out/r5y`).  The hierarchy's buffers are allocated at its
// build only, so the captured pointers stay valid until it is rebuilt (or graph_cache_drop).  A
// capture HIP refuses leaves the rank on the eager path.
// The rank's own device is made current around the capture and the launch (a device group's
// host thread may have another rank's device current), and a stream that is already being
// captured (the group iteration's own graph, LSQ_DIST_GRAPH=1) takes the eager launches into that
// capture instead of a nested capture or a graph launched into a capturing stream.
struct MgDeviceScope {
    int prev = -1;
    explicit MgDeviceScope(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) HIP_CHECK(hipSetDevice(dev));
        else prev = -1;
    }
    ~MgDeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
void mg_vcycle_graph(System& S, MgHier& H, int l) {
    static const int on = getenv("LSQ_MG_RGRAPH") ? atoi(getenv("LSQ_MG_RGRAPH")) : 1;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(S.stream, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
    if (!on || H.rg_failed || cap != hipStreamCaptureStatusNone) {
        mg_vcycle(S, H, l, S.cst.p);
        return;
    }
    MgDeviceScope dev(S.device);
    if (!H.rg || H.rg_l != l) {
        if (H.rg) (void)hipGraphExecDestroy(H.rg);
        H.rg = nullptr;
        bool ok = hipStreamBeginCapture(S.stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            try {
                mg_vcycle(S, H, l, S.cst.p);
            } catch (...) {
                ok = false;
            }
            hipGraph_t graph = nullptr;
            const hipError_t e = hipStreamEndCapture(S.stream, &graph);
            ok = ok && e == hipSuccess && graph && hipGraphInstantiate(&H.rg, graph, nullptr, nullptr, 0) == hipSuccess;
            if (graph) (void)hipGraphDestroy(graph);
        }
        if (!ok) {
            (void)hipGetLastError();
            if (H.rg) (void)hipGraphExecDestroy(H.rg);
            H.rg = nullptr;
            H.rg_failed = true;
            mg_vcycle(S, H, l, S.cst.p);
            return;
        }
        H.rg_l = l;
    }
    HIP_CHECK(hipGraphLaunch(H.rg, S.stream));
}

// Per-solve set-up for the current row weights / mask (after cg_dmf_prepare refreshed the points'
// row scales): lumped data blocks, coarse block factors, the coarsest dense inverse, λ per level.
// level-1 lumped data blocks from this system's points (a rank: its partial sums over the global
// level 1 — the group adds them)
void mg_setup_lump1(System& S) {
    MgHier& H = *S.mg;
    const double4* P = reinterpret_cast<const double4*>(S.dmf_pt.p);
    const MgGeom& G1 = H.lev[1].geo;
    const int nsx = (G1.S1 + 63) / 64;
    hipLaunchKernelGGL(k_mg_lump1, dim3((unsigned)(G1.S0 * nsx)), dim3(64), 0, S.stream, S.dmf, S.dmf_cell.p, P, G1.S0,
                       G1.S1, H.nt, H.nbB, H.withz, H.lev[1].B.p, H.dist ? H.wa : 0);
    KERNEL_CHECK();
}

void mg_setup_rest(System& S, int l_pow0);
void mg_setup_mixed(System& S);
void mg_setup(System& S) {
    if (S.mg->mixed) {
        mg_setup_mixed(S);
        return;
    }
    mg_setup_lump1(S);
    mg_setup_lump_xr(S);
    mg_setup_rest(S, 0);
}

// coarse lumped data (ℓ ≥ 2), coarse block factors, the coarsest inverse, and λ of the levels
// l_pow0.. (a rank: 1.., its level 0's λ comes from the group's power steps)
void mg_setup_rest(System& S, int l_pow0) {
    MgHier& H = *S.mg;
    hipStream_t st = S.stream;
    const int L = (int)H.lev.size();
    SetupTrace tr;
    tr.mark(st, "  mg lump1");
    for (int l = 2; l < L; ++l) {
        const MgGeom &F = H.lev[l - 1].geo, &C = H.lev[l].geo;
        hipLaunchKernelGGL(k_mg_restrict_b, dim3(grid_for(C.nodes * H.nbB)), dim3(BLOCK), 0, st, F.S0, F.S1, C.S0, C.S1,
                           H.nbB, H.lev[l - 1].B.p, H.lev[l].B.p);
    }
    H.ndead.zero(st);
    H.err.zero(st);
    for (int l = 1; l < L; ++l) {
        MgLevel& V = H.lev[l];
        if (V.coarsest) {
            V.dN.zero(st);
            hipLaunchKernelGGL(k_mg_dense_build, dim3(grid_for(V.npad)), dim3(BLOCK), 0, st, V.npad, V.geo, V.tz, V.td,
                               V.offs.p, V.offs.p + 3 * (H.gz >= 0 ? V.tz.noff : 0), V.coef.p, V.B.p, H.nbB,
                               H.var ? V.vz.p : nullptr, V.dN.p);
            KERNEL_CHECK();
            tr.mark(st, "  mg dense build");
            dense_spd_factor(V.dN.p, V.dRi.p, V.npad, H.err.p, st);
            tr.mark(st, "  mg dense factor");
            const int nb = (int)(V.npad / 64);
            hipLaunchKernelGGL(k_mg_gram, dim3(nb * nb), dim3(BLOCK), 0, st, V.dRi.p, V.npad, V.dN.p);   // dN = N⁻¹
            KERNEL_CHECK();
            tr.mark(st, "  mg dense gram");
        } else {
            const int npk = H.kslot * (H.kslot + 1) / 2;
            hipLaunchKernelGGL(k_mg_block_build, dim3(grid_for(V.geo.nodes * npk)), dim3(BLOCK), 0, st, V.geo.nodes,
                               V.geo.S1, H.kslot, H.sl, H.nbB, V.tz, V.td, V.coef.p, V.B.p, H.var ? V.vz.p : nullptr,
                               V.Ri.p);
            KERNEL_CHECK();
            block_factor_packed(V.geo.nodes, V.ptr.p, H.kslot, V.Ri.p, V.Lf.p, H.ndead.p, st);
            tr.mark(st, "  mg block factor");
        }
    }
    // λ_max(M⁻¹N) per smoothing level: power steps in the M inner product on private vectors
    const CgState* ms = H.mst.p;
    static const int npow = getenv("LSQ_MG_POW") ? std::max(2, atoi(getenv("LSQ_MG_POW"))) : MG_POW;
    // (issued on S.stream, whichever stream pair that is: see the concurrent branch below)
    auto power = [&](int l, double* scal, double* p1, double* p2) {
        MgLevel& V = H.lev[l];
        const MgVec v0 = mg_vecs(S, H, l);
        // scratch: d holds the unnormalised iterate, x its scaled copy; r / res untouched
        double* w = l ? V.d.p : H.d0.p;
        double* xv = l ? V.x.p : H.res0.p;   // level 0: res0 (cg_z belongs to the solve)
        double* q = l ? V.q.p : S.cg_q.p;
        hipLaunchKernelGGL(k_mg_randvec, dim3(grid_for(V.geo.n_full)), dim3(BLOCK), 0, S.stream, V.geo, V.geo, (int64_t)0,
                           w);
        HIP_CHECK(hipMemsetAsync(scal, 0, 2 * sizeof(double), S.stream));
        const MgVec vp = {v0.r, xv, q, w, v0.res};
        for (int k = 0; k < npow; ++k) {
            mg_launch_op(S, H, l, ms, w, w, scal, xv, q);
            mg_launch_smooth(S, H, l, ms, vp, MG_POWER, 0, p1, p2);
            hipLaunchKernelGGL(k_mg_power_scalar, dim3(1), dim3(BLOCK), 0, S.stream, p1, p2, V.gB, k, H.lam.p + l, scal);
        }
        KERNEL_CHECK();
        // level vectors back to zero (the V-cycle relies on zero removed columns only, but keep
        // the scratch clean for the test hooks)
        if (l) {
            V.x.zero(S.stream);
            V.d.zero(S.stream);
        }
        tr.mark(S.stream, "  mg power");
    };
    // One GPU: the coarse levels' steps (each reads only its own level's operator, factors and
    // vectors; their own scalars and partials) run on a second stream pair beside level 0's, whose
    // full-chip kernels leave room for their small latency-bound ones.  LSQ_MG_POW_CONC=0: in turn.
    static const bool conc_env = !getenv("LSQ_MG_POW_CONC") || atoi(getenv("LSQ_MG_POW_CONC")) != 0;
    if (conc_env && l_pow0 == 0 && !H.dist && L > 2) {
        if (!S.aux) {
            HIP_CHECK(hipStreamCreateWithFlags(&S.aux, hipStreamNonBlocking));
            HIP_CHECK(hipStreamCreateWithFlags(&S.aux_side, hipStreamNonBlocking));
            HIP_CHECK(hipEventCreateWithFlags(&S.ev_aux, hipEventDisableTiming));
        }
        if (!S.side) {
            HIP_CHECK(hipStreamCreateWithFlags(&S.side, hipStreamNonBlocking));
            HIP_CHECK(hipEventCreateWithFlags(&S.ev_fork, hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(&S.ev_join, hipEventDisableTiming));
        }
        HIP_CHECK(hipEventRecord(S.ev_aux, st));   // the coarse factors above are done
        HIP_CHECK(hipStreamWaitEvent(S.aux, S.ev_aux, 0));
        {
            struct Swap {   // S.stream / S.side → the aux pair for the coarse levels' launches
                System& S;
                explicit Swap(System& s) : S(s) { std::swap(S.stream, S.aux), std::swap(S.side, S.aux_side); }
                ~Swap() { std::swap(S.stream, S.aux), std::swap(S.side, S.aux_side); }
            } swap(S);
            for (int l = 1; l + 1 < L; ++l) power(l, H.scal.p + 2, H.part1.p + NPART, H.part2.p + NPART);
            HIP_CHECK(hipEventRecord(S.ev_aux, S.stream));
        }
        power(0, H.scal.p, H.part1.p, H.part2.p);
        HIP_CHECK(hipStreamWaitEvent(st, S.ev_aux, 0));
    } else {
        for (int l = l_pow0; l + 1 < L; ++l) power(l, H.scal.p, H.part1.p, H.part2.p);
    }
    HIP_CHECK(hipMemsetAsync(H.scal.p, 0, 4 * sizeof(double), st));
    H.res0.zero(st);
    int herr = 0;
    HIP_CHECK(hipMemcpyAsync(&herr, H.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (herr) throw std::runtime_error("multigrid: the coarsest-level operator is not positive definite");
}

// CG step with the multigrid preconditioner, part 1: x every CG_XK-th step (as k_cg_block) and
// s −= αq, as a plain stream over the full column space (removed columns: p = 0, so x stays 0
// there; s picks up −αq at them, which no kernel reads: every consumer of s reads kept columns)
__global__ __launch_bounds__(BLOCK) void k_cg_sx_stream(const CgState* __restrict__ st, int64_t nf, CgP P,
                                                        const double* __restrict__ q, double* __restrict__ x,
                                                        double* __restrict__ s) {
    if (st->stop) return;
    const bool xupd = st->pend == CG_XK - 1;
    const double a0 = st->pend_a[0], a1 = st->pend_a[1], a2 = st->pend_a[2], alpha = st->alpha;
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < nf; j += (int64_t)gridDim.x * BLOCK) {
        const double qj = q[j], sj = s[j];
        if (xupd) x[j] = (((x[j] + a0 * P.p[0][j]) + a1 * P.p[1][j]) + a2 * P.p[2][j]) + alpha * P.p[3][j];
        s[j] = sj - alpha * qj;
    }
}

// the multigrid preconditioner inside a CG step: s −= αq (x every CG_XK-th step), z = V(s), ρ
// partials of sᵀz into S.cg_part_r (from the last smoothing kernel of level 0)
void mgx_vcycle(System& S, MgHier& H, const CgState* st);
void mg_precond(System& S, const CgGrids& g, const CgP& P) {
    MgHier& H = *S.mg;
    if (H.mixed) {
        hipLaunchKernelGGL(k_cg_sx_stream, dim3(grid_for(S.n_full, BLOCK * 4)), dim3(BLOCK), 0, S.stream, S.cst.p,
                           S.n_full, P, S.cg_q.p, S.cg_x.p, S.cg_s.p);
        mgx_vcycle(S, H, S.cst.p);
        return;
    }
    if (H.deg0_pre <= 2 && (H.fuse & 1)) {   // the update kernel also takes the first smoothing step (z = c₂ M⁻¹ s)
        cg_launch_block(S, g, P, S.cg_z.p, H.lam.p);
        mg_vcycle(S, H, 0, S.cst.p, true);
        return;
    }
    hipLaunchKernelGGL(k_cg_sx_stream, dim3(grid_for(S.n_full, BLOCK * 4)), dim3(BLOCK), 0, S.stream, S.cst.p, S.n_full,
                       P, S.cg_q.p, S.cg_x.p, S.cg_s.p);
    mg_vcycle(S, H, 0, S.cst.p);
}

// the fine level's operator: q = N x (stencil rows through the ring kernel + x-edge pass, stored
// data rows t = Ad x, q += ATd t), as the CG step applies it
void mgx_op(System& S, MgHier& H, const CgState* st, const double* x, double* q) {
    const int gN = cg_grid_normal(S);
    const double* zero = H.scal.p + 1;
    cg_launch_ns(S.cgh, S.cgd.p, S.cg_coefc.p, S.stream, st, x, nullptr, nullptr, q, H.xpart.p, zero);
    hipLaunchKernelGGL(k_cg_xedge<8>, dim3(S.cgh.pad[0]), dim3(BLOCK), 0, S.stream, st, S.cgd.p, S.cg_coef.p, x, q,
                       H.xpart.p + gN);
    const CgGrids g = cg_grids(S, 4);
    hipLaunchKernelGGL(k_cg_data, dim3(g.gD), dim3(BLOCK), 0, S.stream, st, S.mfh.npts, S.Ad.nslices, S.Ad.sp.p,
                       S.Ad.ci.p, S.Ad.val.p, x, nullptr, S.cg_t.p, H.part_t.p);
    hipLaunchKernelGGL(k_cg_atdq, dim3((unsigned)((S.mfh.nodes + CG_AR * BLOCK - 1) / (CG_AR * BLOCK))), dim3(BLOCK), 0,
                       S.stream, st, S.mfd.p, S.ATd.rp.p, S.ATd.ci.p, S.ATd.val.p, S.cg_t.p, q);
}

int mgx_grid(const MgMix& m) { return grid_for(std::max<int64_t>(m.nz, 1), BLOCK, NPART); }

// one V-cycle from the fine level: x = S.cg_z = V(r = S.cg_s); ρ partials Σ s·z into S.cg_part_r
void mgx_vcycle(System& S, MgHier& H, const CgState* st) {
    const MgMix& m = H.mix;
    System& X = *S.mx;
    const int gx = mgx_grid(m), deg = H.deg0;
    double *r = S.cg_s.p, *x = S.cg_z.p, *q = S.cg_q.p, *d = H.d0.p;
    HIP_CHECK(hipMemsetAsync(x + m.dzcol, 0, sizeof(double) * m.nsz * m.nt, S.stream));   // dz: from the coarse correction
    hipLaunchKernelGGL(k_mgx_smooth, dim3(gx), dim3(BLOCK), 0, S.stream, st, m, H.xdinv.p, r, q, x, d, H.lam.p,
                       MG_XZERO | (deg <= 2 ? MG_NOD : 0), 0, nullptr, nullptr);
    for (int k = 1; k < deg; ++k) {
        mgx_op(S, H, st, x, q);
        hipLaunchKernelGGL(k_mgx_smooth, dim3(gx), dim3(BLOCK), 0, S.stream, st, m, H.xdinv.p, r, q, x, d, H.lam.p,
                           (k == 1 ? MG_DX : 0) | (k == deg - 1 ? MG_NOD : 0), k, nullptr, nullptr);
    }
    mgx_op(S, H, st, x, q);
    const int64_t nsub = m.nsz * (1 + m.nt);
    hipLaunchKernelGGL(k_mgx_restrict, dim3(grid_for(nsub)), dim3(BLOCK), 0, S.stream, st, m, r, q, X.cg_s.p);
    mg_vcycle(X, *X.mg, 0, st);
    hipLaunchKernelGGL(k_mgx_prolong, dim3(grid_for(m.nz + m.nsz * m.nt)), dim3(BLOCK), 0, S.stream, st, m, X.cg_z.p, x);
    for (int k = 0; k < deg; ++k) {
        mgx_op(S, H, st, x, q);
        hipLaunchKernelGGL(k_mgx_smooth, dim3(gx), dim3(BLOCK), 0, S.stream, st, m, H.xdinv.p, r, q, x, d, H.lam.p,
                           k == deg - 1 ? MG_NOD : 0, k, nullptr, nullptr);
    }
    hipLaunchKernelGGL(k_mgx_dot, dim3(cg_grids(S, 4).gB), dim3(BLOCK), 0, S.stream, st, S.n_full, r, x, S.cg_part_r.p);
}

// per solve: S.mx's points take this system's row scales, its exact node blocks are factored, its
// hierarchy set up; this level's z0 Jacobi diagonal and λ_max(D⁻¹N) on the z0 columns
void mg_setup_mixed(System& S) {
    MgHier& H = *S.mg;
    const MgMix& m = H.mix;
    System& X = *S.mx;
    MgHier& HX = *X.mg;
    hipStream_t st = S.stream;
    hipLaunchKernelGGL(k_dmf_rs, dim3(grid_for(X.dmf.npts)), dim3(BLOCK), 0, st, X.dmf.npts, X.dmf_perm.p, S.rs.p,
                       reinterpret_cast<double4*>(X.dmf_pt.p));
    const int nsx = (X.dmf.S1 + 63) / 64;
    hipLaunchKernelGGL(k_mg_lump0, dim3((unsigned)(X.dmf.S0 * nsx)), dim3(64), 0, st, X.dmf, X.dmf_cell.p,
                       reinterpret_cast<const double4*>(X.dmf_pt.p), HX.nt, HX.nbB, HX.withz, H.xB.p);
    const int npk = HX.kslot * (HX.kslot + 1) / 2;
    hipLaunchKernelGGL(k_mg_block_build, dim3(grid_for(m.nsz * npk)), dim3(BLOCK), 0, st, m.nsz, m.Sc1, HX.kslot, HX.sl,
                       HX.nbB, H.xtz, H.xtd, H.xcoef.p, H.xB.p, nullptr, H.xRi.p);
    KERNEL_CHECK();
    H.ndead.zero(st);
    block_factor_packed(m.nsz, H.xptr.p, HX.kslot, H.xRi.p, X.blk_Lf.p, H.ndead.p, st);
    mg_setup(X);
    const int gx = mgx_grid(m);
    ensure_full_csr(S);   // diag(AᵀA) of the z0 columns from GT
    hipLaunchKernelGGL(k_mgx_diag, dim3(gx), dim3(BLOCK), 0, st, m, S.colmap.p, S.GT.rp.p, S.GT.ci.p, S.GT.val.p, S.rs.p,
                       H.xdinv.p);
    H.d0.zero(st);
    hipLaunchKernelGGL(k_mgx_randvec, dim3(gx), dim3(BLOCK), 0, st, m, H.d0.p);
    HIP_CHECK(hipMemsetAsync(H.scal.p, 0, 2 * sizeof(double), st));
    const CgState* ms = H.mst.p;
    for (int k = 0; k < MG_POW; ++k) {
        mgx_op(S, H, ms, H.d0.p, S.cg_q.p);
        hipLaunchKernelGGL(k_mgx_smooth, dim3(gx), dim3(BLOCK), 0, st, ms, m, H.xdinv.p, nullptr, S.cg_q.p, H.d0.p,
                           H.d0.p, H.lam.p, MG_POWER, 0, H.part1.p, H.part2.p);
        hipLaunchKernelGGL(k_mg_power_scalar, dim3(1), dim3(BLOCK), 0, st, H.part1.p, H.part2.p, gx, k, H.lam.p, H.scal.p);
        hipLaunchKernelGGL(k_mgx_scale, dim3(gx), dim3(BLOCK), 0, st, m, H.scal.p, H.d0.p, H.d0.p);
    }
    KERNEL_CHECK();
    HIP_CHECK(hipMemsetAsync(H.scal.p, 0, 2 * sizeof(double), st));
    H.d0.zero(st);
    S.cg_q.zero(st);
    HIP_CHECK(hipStreamSynchronize(st));
}

// Algorithmic bytes of one preconditioner application (block update + V-cycle): per level, 2·deg
// operator applications (level 0: the CG normal + data byte model; coarse levels 32 B per column)
// and 2·deg block passes (r, q, x, d in and x, d out: 48 B per column + the fp32 factor; level 0's
// first is the block update's z = c₂M⁻¹s), plus restriction / prolongation (fine + coarse vector
// once each way; the coarse levels' residual r − q − Bx is formed inside the restriction).
double mg_bytes(const System& S, double op0_bytes) {
    const MgHier& H = *S.mg;
    if (H.mixed) {   // 2·deg fine operators, z0 smoothing (r, q, x, d, D⁻¹), transfers, the dz-lattice cycle
        const MgMix& m = H.mix;
        const double nsub = (double)m.nsz * (1 + m.nt);
        double xb[3];
        cg_kernel_bytes(*S.mx, 4, xb);
        return 2.0 * H.deg0 * (op0_bytes + 48.0 * (double)m.nz) + 16.0 * (double)S.n_full + 24.0 * nsub +
               16.0 * (double)S.n_full + xb[2];
    }
    const double npks = (double)lf_stride(H.kslot * (H.kslot + 1) / 2);
    // s −= αq, z = c₂M⁻¹s (q, s in, s, z out, factor) + x every CG_XK-th step
    double b = 48.0 * (double)S.G.n + ((double)sizeof(lf_t) * npks + 8.0) * (double)H.lev[0].geo.nodes;
    for (size_t l = 0; l < H.lev.size(); ++l) {
        const MgLevel& V = H.lev[l];
        const double nf = (double)V.geo.n_full, nb = (double)V.geo.nodes;
        if (V.coarsest) {
            b += 8.0 * (double)V.npad * (double)V.npad;
            continue;
        }
        const double deg = l ? H.deg : H.deg0;
        const double vb = (H.var && l) ? (8.0 * MG_VN + 24.0) * nb : 0.0;   // Galerkin z0 rows, p, q RMW
        b += 2.0 * deg * (l ? 32.0 * nf + 8.0 * (double)H.nbB * nb + vb : op0_bytes);
        b += (2.0 * deg - (l ? 0.0 : 1.0)) * (48.0 * nf + (double)sizeof(lf_t) * npks * nb);
        const double nc = (double)H.lev[l + 1].geo.n_full;
        b += 2.0 * (8.0 * nf + 8.0 * nc);
    }
    return b;
}

}  // namespace

// Test hooks (lsq_mg_info / lsq_mg_apply): the hierarchy of the current system and its level
// operators, for the GPU tests against a host Galerkin hierarchy.
int mg_info(System& S, int64_t* out, int64_t cap) {
    if (!cg_prepare(S, 4) || !S.mg) throw std::invalid_argument("multigrid unavailable: " + (S.cg_ok ? S.mg_why : S.cg_why));
    const MgHier& H = *S.mg;
    if (H.mixed) {   // the fine (z0-refined) level, then the dz-lattice hierarchy
        const MgHier& HX = *S.mx->mg;
        const int64_t L = 1 + (int64_t)HX.lev.size();
        if (cap < 1 + 4 * L) throw std::invalid_argument("lsq_mg_info: output too small");
        out[0] = L;
        out[1] = H.mix.Sf0;
        out[2] = H.mix.Sf1;
        out[3] = S.n_full;
        out[4] = H.mix.tref;
        for (int64_t l = 1; l < L; ++l) {
            out[1 + 4 * l] = HX.lev[l - 1].geo.S0;
            out[2 + 4 * l] = HX.lev[l - 1].geo.S1;
            out[3 + 4 * l] = HX.lev[l - 1].geo.n_full;
            out[4 + 4 * l] = HX.tref;
        }
        return 0;
    }
    const int64_t L = (int64_t)H.lev.size();
    if (cap < 1 + 4 * L) throw std::invalid_argument("lsq_mg_info: output too small");
    out[0] = L;
    for (int64_t l = 0; l < L; ++l) {
        out[1 + 4 * l] = H.lev[l].geo.S0;
        out[2 + 4 * l] = H.lev[l].geo.S1;
        out[3 + 4 * l] = H.lev[l].geo.n_full;
        out[4 + 4 * l] = H.tref;
    }
    return 0;
}

// what 0: y = N_ℓ x over level ℓ's full column space (ℓ ≥ 1: Galerkin stencil + lumped data;
// removed columns: 0); 1: y = V_ℓ(x), the cycle from level ℓ down (the coarsest level: its dense
// inverse; z0-refined systems: ℓ = 0 only); 2: y[0] = λ estimate of level ℓ; 3: y[0] = the kernel
// family of level ℓ's operator (0 ring + x-edge pass, 1 k_mg_direct, 2 k_mg_tile, 3 k_mg_tile_kt;
// −1: the coarsest level, no operator kernel)
void mg_test_apply(System& S, int level, int what, const double* hx, double* hy) {
    if (!cg_prepare(S, 4) || !S.mg) throw std::invalid_argument("multigrid unavailable: " + (S.cg_ok ? S.mg_why : S.cg_why));
    MgHier& H = *S.mg;
    hipStream_t st = S.stream;
    if (H.mixed) {   // the fine level: its operator (what 0), the V-cycle (1), λ (2)
        if (level != 0) throw std::invalid_argument("lsq_mg_apply: z0-refined systems expose their fine level only");
        cg_workspace(S);
        mg_setup(S);
        const int64_t nf = S.n_full;
        if (what == 2) {
            HIP_CHECK(hipMemcpyAsync(hy, H.lam.p, sizeof(double), hipMemcpyDeviceToHost, st));
        } else if (what == 0) {
            DBuf<double> dx(nf), dy(nf);
            dx.upload(hx, nf, st);
            mgx_op(S, H, H.mst.p, dx.p, dy.p);
            dy.download(hy, nf, st);
        } else if (what == 1) {
            S.cg_s.upload(hx, nf, st);
            mgx_vcycle(S, H, H.mst.p);
            S.cg_z.download(hy, nf, st);
        } else {
            throw std::invalid_argument("lsq_mg_apply: what must be 0, 1 or 2");
        }
        KERNEL_CHECK();
        HIP_CHECK(hipStreamSynchronize(st));
        S.cg_ready = false;
        return;
    }
    if (level < 0 || level >= (int)H.lev.size()) throw std::invalid_argument("lsq_mg_apply: level out of range");
    if (what == 3) {   // fixed at the hierarchy's build: no set-up needed
        const MgLevel& Vl = H.lev[level];
        hy[0] = Vl.coarsest ? -1.0 : Vl.tile ? (Vl.tile_kt ? 3.0 : 2.0) : Vl.direct ? 1.0 : 0.0;
        return;
    }
    cg_workspace(S);
    cg_dmf_prepare(S);
    mg_setup(S);
    const CgState* ms = H.mst.p;
    MgLevel& V = H.lev[level];
    const int64_t nf = V.geo.n_full;
    if (what == 2) {
        HIP_CHECK(hipMemcpyAsync(hy, H.lam.p + level, sizeof(double), hipMemcpyDeviceToHost, st));
    } else if (what == 0) {
        if (V.coarsest) throw std::invalid_argument("lsq_mg_apply: the coarsest level has no operator kernel");
        MgVec v = mg_vecs(S, H, level);
        DBuf<double> dx(nf);
        dx.upload(hx, nf, st);
        HIP_CHECK(hipMemsetAsync(const_cast<double*>(v.r), 0, sizeof(double) * nf, st));
        HIP_CHECK(hipMemsetAsync(v.res, 0, sizeof(double) * nf, st));
        mg_launch_op(S, H, level, ms, dx.p, nullptr, H.scal.p + 1, nullptr, v.q);
        MgVec vt = v;
        vt.x = dx.p;
        mg_launch_smooth(S, H, level, ms, vt, MG_RES, 0, nullptr, nullptr);   // res = 0 − q − B x
        std::vector<double> tmp(nf);
        HIP_CHECK(hipMemcpyAsync(tmp.data(), v.res, sizeof(double) * nf, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int64_t i = 0; i < nf; ++i) hy[i] = -tmp[i];
    } else if (what == 1) {
        if (level == 0) {
            S.cg_s.upload(hx, nf, st);
            S.cg_z.zero(st);
            mg_vcycle(S, H, 0, ms);
            S.cg_z.download(hy, nf, st);
        } else {   // the cycle from a coarse level (the coarsest: its dense inverse), on that level's own vectors
            V.r.upload(hx, nf, st);
            V.x.zero(st);
            mg_vcycle(S, H, level, ms);
            V.x.download(hy, nf, st);
        }
    } else {
        throw std::invalid_argument("lsq_mg_apply: what must be 0, 1, 2 or 3");
    }
    KERNEL_CHECK();
    HIP_CHECK(hipStreamSynchronize(st));
    S.cg_ready = false;
}

namespace {
