/*
 * lsqsurf.h — C ABI of lssurf_amd's MI355X (gfx950) least-squares solve path.
 *
 * This is the only public native surface (liblsqsurf.so).  It replaces, for LSsurf's
 * sparse regularized least-squares solve path:
 *
 *   sparseqr.solve(A, b)               LSsurf/smooth_fit.py:142 (iterate_fit),
 *                                      notebooks/smooth_fit_demo_aniso.ipynb cells 6,13,16,18,20
 *       -> lsq_create / lsq_set_col_map / lsq_set_matrix_coo / lsq_set_row_weight /
 *          lsq_set_row_mask / lsq_solve
 *   G_data.toCSR().dot(m0)             LSsurf/smooth_fit.py:146,662 (residual / z_est)
 *       -> lsq_spmv
 *   Gcoo = sp.vstack([...]).tocoo()·Ip_c, TCinv·Gcoo, Ip_r·(...)   smooth_fit.py:613-627,123-142
 *       -> formed on the device by lsq_set_matrix_coo (+col map, row weight, row mask)
 *   inv_tr_upper(R, nnz, tol)          LSsurf/inv_tr_upper.pyx:19-94 (smooth_fit.py:240-246)
 *       -> tri_upper_inv_csr
 *   propagate_qz_errors(R)             LSsurf/propagate_qz_errors.pyx:15-69
 *       -> tri_upper_rowrss_csr
 *   spsolve_tr_upper(A, b)             LSsurf/spsolve_tr_upper.pyx:11-54
 *       -> tri_upper_solve_csr
 *
 * Conventions
 *   - Ownership: the caller owns every host buffer; the library copies in and out and owns all
 *     device memory.  Pointers are plain host pointers, sizes are int64.
 *   - Errors: int return, 0 = ok, 1 = "not converged" (lsq_solve hit maxit) or "output buffer
 *     full" (tri_upper_inv_csr, same meaning as inv_tr_upper's status=1); < 0 = invalid
 *     argument / call order / HIP error, with lsq_last_error() describing it; -5 = declined for
 *     lack of resources (a band factor that does not fit the device or exceeds the width limit —
 *     the caller may choose another preconditioner).  There is no CPU fallback: without a
 *     usable gfx950 device every call fails.
 *   - Threading: one handle per host thread; calls on one handle are serialised.
 */
#ifndef LSQSURF_H
#define LSQSURF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lsq_handle lsq_handle;

/* Solver options.  Defaults (lsq_default_opts) reproduce scipy.sparse.linalg.lsqr's stopping
 * rules with atol = btol = 1e-10, conlim = 1e8, maxit = 4*n. */
typedef struct lsq_opts {
    int32_t method;        /* 0 = LSQR (Paige & Saunders 1982); 1 = CGNR: preconditioned CG on  */
                           /*     the normal equations with the fused normal-stencil operator   */
                           /*     (structured systems, single-GPU or structured ranks; precond  */
                           /*     1, 3 or 4; other single-GPU systems fall back to LSQR and     */
                           /*     report method 0 in lsq_stats)                                 */
    int32_t precond;       /* 0 = none, 1 = column (Jacobi) scaling, 2 = dense Cholesky R⁻¹   */
                           /*     (exact right preconditioner; n up to a few 10^4), 3 = block-  */
                           /*     Jacobi: R_b⁻¹ of every column block (lsq_set_column_blocks;   */
                           /*     SURVEY.md §8 a7.4 — no reference counterpart), 4 = geometric  */
                           /*     multigrid V-cycle over the (y, x) node lattice (method 1,     */
                           /*     smooth_fit systems with per-node column blocks, single GPU or */
                           /*     structured ranks with lsq_dist_set_global; DESIGN.md          */
                           /*     §Multigrid), 5 = banded Cholesky R̃⁻¹ in the order of         */
                           /*     lsq_set_band_order (LSQR, single GPU; band.hip)               */
    double  atol, btol, conlim;
    int64_t maxit;
    int32_t use_x0;        /* 1: x_inout holds a warm start (outer-iteration "resume")          */
    int32_t batch;         /* iterations per device batch between host convergence checks      */
    int32_t use_graph;     /* 1: replay each batch as a captured hipGraph                       */
    int32_t op;            /* operator the iteration streams: 0 = auto (the structured stencil  */
                           /*     operator when the matrix came from lsq_set_matrix_stencil and */
                           /*     precond < 2; else assembled SELL), 1 = assembled SELL always  */
    int64_t b_rows;        /* rows of b that may be non-zero: b[0, b_rows) is uploaded, the     */
                           /*     rest taken as zero (smooth_fit: the data rows, when no prior  */
                           /*     is non-zero); 0 = all m rows                                 */
    double  anorm0;        /* CGNR: an ‖A‖ estimate to start the stopping rule from — lsq_stats */
                           /*     .anorm of an earlier solve of the same operator and           */
                           /*     preconditioner (smooth_fit's later outer solves, warm         */
                           /*     starts).  The rule uses max(anorm0, the running Lanczos       */
                           /*     estimate), which only grows towards the true norm; without it */
                           /*     a re-solve from the solution iterates until the estimate has  */
                           /*     rebuilt.  0 = none (scipy's rule); ignored by LSQR            */
} lsq_opts;

/* Statistics (mirrors scipy's lsqr return tuple, plus timing and the byte model). */
typedef struct lsq_stats {
    int64_t iters;
    int32_t istop;         /* scipy istop: 1,2 converged; 3 cond limit; 4-6 machine precision; 7 maxit */
    int32_t method;        /* method that ran: 0 LSQR, 1 CGNR (acond is not estimated: 0)      */
    double  r1norm, r2norm, anorm, acond, arnorm, xnorm;
    double  time_s;        /* device-resident iteration time (A, b already in HBM)              */
    double  bytes_per_iter;/* algorithmic HBM bytes of one LSQR iteration (DESIGN.md byte model)*/
    double  setup_s;       /* CGNR: per-solve preconditioner set-up and initialisation (block   */
                           /*     factors, multigrid levels and λ estimates), host wall clock, */
                           /*     not part of time_s; LSQR: 0                                  */
    double  comm_bytes_per_iter; /* distributed CGNR: bytes one rank sends per iteration (halos   */
                           /*     and all-reduces; the busiest rank of a virtual / device group); */
                           /*     0 on one GPU                                                  */
} lsq_stats;

void        lsq_default_opts(lsq_opts* o);

/* ---- handle lifetime -------------------------------------------------------------------- */
lsq_handle* lsq_create(int32_t device);
void        lsq_destroy(lsq_handle* h);
const char* lsq_last_error(lsq_handle* h);     /* never NULL; "" when no error                 */

/* ---- matrix formation (replaces the scipy assembly of smooth_fit.py:613-627) ------------ */
/* Optional, before lsq_set_matrix_coo: keep only these columns of the full operator, in this
 * order (= Ip_c of build_reference_epoch_matrix, constraint_functions.py:112-151). keep_cols
 * must be strictly increasing in [0, n). */
int lsq_set_col_map(lsq_handle* h, int64_t n_full, const int64_t* keep_cols, int64_t n_keep);

/* Form A = diag(row_weight) * G * Ip_c on the device from COO triplets of G (m x n_full):
 * entries with v == 0 are dropped, duplicates are summed in input order, sums equal to 0 are
 * dropped, columns outside the col map are removed (lin_op.toCSR, lin_op.py:745-753, plus the
 * scipy products of smooth_fit.py:613-627).  row_weight may be NULL (= 1).  Builds A and Aᵀ. */
int lsq_set_matrix_coo(lsq_handle* h, int64_t m, int64_t n_full, int64_t nnz,
                       const int64_t* r, const int64_t* c, const double* v,
                       const double* row_weight);

/* Structured formation (no host triplets): the smooth_fit operator described by its fd_grids
 * and stencils, rows generated on the device exactly as lin_op would generate them.
 *   data rows 0..npts-1: sum over `n_interp` interpolation parts (lin_op.interp_mtx,
 *     lin_op.py:163-247) of point p = (py, px[, pt]) on grid interp_grid[k]; points must be
 *     inside every grid (bounds_error=True semantics);
 *   stencil part s covers rows [row0, row0+n_eq): centre k -> subscripts lo + unravel(k, hi-lo)
 *     ('ij' meshgrid order), entries col0 + ravel(centre + off[t]) with value val[t]
 *     (lin_op.diff_op, lin_op.py:80-132).
 * Then the same zero-drop / duplicate-sum / col-map rules as lsq_set_matrix_coo. */
typedef struct lsq_grid_desc {
    int32_t ndim, reserved;
    int64_t shape[3];
    int64_t col0;
    double  b0[3], delta[3];
} lsq_grid_desc;
typedef struct lsq_stencil_desc {
    int32_t grid, ntpl;
    int32_t off[8][3];
    double  val[8];
    int64_t row0, n_eq;
    int64_t lo[3], hi[3];
} lsq_stencil_desc;
int lsq_set_matrix_stencil(lsq_handle* h, int64_t m, int64_t n_full,
                           int32_t n_grids, const lsq_grid_desc* grids,
                           int32_t n_interp, const int32_t* interp_grid, int64_t npts,
                           const double* py, const double* px, const double* pt,
                           int32_t n_stencil, const lsq_stencil_desc* stencils,
                           const double* row_weight);

/* Field-valued (variable-coefficient) stencil part, staged before lsq_set_matrix_stencil: stencil
 * index `stencil` of that call keeps its grid, rows and centre box, and its template becomes the
 * ntpl (≤ 16) offsets off[3·t + d] with entry value val[t] · F[fsel[t]·n_eq + k] in the row of
 * centre k (k = ravel of centre − lo over the box, the row order of lin_op.diff_op).  F holds the
 * nfield exact per-row values (field-major).  This is the directional smoothing operator of
 * notebooks/smooth_fit_demo_aniso.ipynb cells 9-10: a lin_op.diff_op template whose rows
 * scale_op_by_2d_grid multiplies by the interpolated direction field (u², 2uv, v²), summed over
 * three templates on the same rows — one part here, 9 entries, F = the distinct |values|. */
int lsq_set_stencil_fields(lsq_handle* h, int32_t stencil, int32_t ntpl, const int32_t* off, const double* val,
                           int32_t nfield, const int32_t* fsel, int64_t n_eq, const double* F);

/* Extra sparse rows behind the stencil rows, staged before lsq_set_matrix_stencil (and after
 * lsq_set_col_map): the m_x rows of the CSR (indptr, cols_full, vals), columns = full-space ids,
 * become the LAST rows of the system, so m of lsq_set_matrix_stencil is data rows + stencil rows +
 * m_x.  These are rows that are neither interpolation rows nor stencil rows, e.g. smooth_fit's dz
 * priors (interp_dz(y, x, t) − interp_dz(y, x, t_ref) with their own σ and a non-zero b).
 * Formation follows lsq_set_matrix_coo: duplicates within a row are summed in input order, zeros and
 * zero sums are dropped, entries in columns the col map removes are dropped; a row may end up empty.
 * A row that keeps more than 32 entries returns −2 and the staging stays as it was.  m_x = 0 or a
 * null indptr clears the staging.  Row weights, the row mask and b address these rows at their
 * positions; lsq_shape counts them; lsq_get_csr / lsq_spmv / lsq_spmv_rows, the dense (2) and band
 * (5) factors and LSQR on the assembled operator (op = 1) cover them through the full CSR.
 * Matrix-free CGNR (method 1) carries them with precond 1 or 3: the normal operator gains
 * XᵀW_x²X (two small kernels per step, bitwise reproducible), the Jacobi norms and the node-block
 * factors gain the same sums, and lsq_normal_apply includes the term.  With lsq_opts.b_rows the
 * library also uploads b[m − m_x, m).  Refused with −2 and the reason: precond 4 unless the rows
 * are lumped (below; without it the multigrid's coarse levels would miss the term and
 * lsq_cg_available(h, 4) reports 0), LSQR on the structured stencil operator (op = 0 on a lazily
 * formed system), tile-mode CGNR, and every distributed, virtual or device-group rank (the
 * formation itself is refused there).  May be combined with lsq_set_data_bias: the two terms are
 * independent.
 * lsq_set_extra_rows_lumping(h, 1), after the rows are staged and before lsq_set_matrix_stencil
 * (cleared with the staging): precond 4 carries the rows.  Level 0 of the V-cycle applies XᵀW_x²X
 * exactly; on the coarse levels each row is lumped into the node blocks like a data row: with
 * τ_s = Σ_n x[n, s] and the (y, x) weights ω_n = Σ_s |x[n, s]| / Σ |x| (a separable row w ⊗ τ, w ≥ 0,
 * Σ w = 1 gives back w and τ), level 1 gains B_1[m] += rs² (Σ_n P[n, m] ω_n) τ τᵀ, restricted to the
 * levels below with the data rows' blocks, on every solve whose weights or mask changed, in a fixed
 * order without atomics.  A row is lumpable when its dz entries lie in at most two adjacent epochs
 * (the z0 entry is free).  Still refused with −2 and the reason: a row that is not lumpable (named
 * in the reason), the z0-refined hierarchy, tile-mode CGNR, distributed / virtual / group ranks.
 * Without the call nothing changes.
 * lsq_extra_rows_mg_info: out4 = {rows lumped, touched level-1 nodes, algorithmic bytes of one
 * lumping pass, device bytes of its tables}; zeros when precond 4 does not carry the rows.
 * lsq_profile_extra_rows_lumping: reps lumping passes of the set-up with device events between the
 * kernels: out2 = {ms of the extra rows' pass, ms of the data rows' k_mg_lump1 before it}.
 * lsq_extra_rows_info: out4 = {m_x, touched columns, algorithmic bytes of one CG step's two
 * kernels, device bytes of the rows and their transpose}.
 * lsq_profile_extra_rows: after lsq_iterate with the same precond (its live state), runs reps more
 * iterations with device events between the launches: out4 = {ms k_xr_fwd, ms k_xr_atq (with its
 * long-column kernel), ms of the data rows' Ad·p before them, ms of the node gather behind them}. */
int lsq_set_extra_rows(lsq_handle* h, int64_t m_x, const int64_t* indptr, const int64_t* cols_full,
                       const double* vals);
int lsq_set_extra_rows_lumping(lsq_handle* h, int32_t on);
int lsq_extra_rows_info(lsq_handle* h, double* out4);
int lsq_extra_rows_mg_info(lsq_handle* h, double* out4);
int lsq_profile_extra_rows_lumping(lsq_handle* h, int32_t reps, double* out2);
int lsq_profile_extra_rows(lsq_handle* h, int32_t reps, int32_t precond, double* out4);

/* Replace the row weights (TCinv of iterate_fit, smooth_fit.py:123-129) without re-forming. */
int lsq_set_row_weight(lsq_handle* h, const double* row_weight);
/* Row selection Ip_r (smooth_fit.py:132-135): rows with keep[i] == 0 are excluded from the
 * fit (treated as absent rows).  NULL keeps every row. */
int lsq_set_row_mask(lsq_handle* h, const uint8_t* keep);
/* Column blocks of the block-Jacobi preconditioner (precond 3): block b holds the compact
 * columns cols[block_ptr[b] .. block_ptr[b+1]) (at most 16, each column in at most one block);
 * unlisted columns are singleton blocks.  For smooth_fit a block is one (y, x) node: its z0
 * column and its dz columns of every kept epoch.  The factors R_b (AᵀA restricted to the block
 * = R_bᵀR_b, with the current row weights / mask) are rebuilt on the device when weights change;
 * R_b⁻¹ is kept rounded to bf16 (products in f64), the same M for CGNR and for every use LSQR
 * makes of it, so x is unaffected (any non-singular M gives the same least-squares solution).
 * NULL / 0 blocks clears the structure (every column its own block).  On a structured rank
 * (lsq_dist_set_halo) the blocks are the rank's owned nodes in its local compact ids, factored
 * from the rank's own rows; ghost columns stay outside every block. */
int lsq_set_column_blocks(lsq_handle* h, int64_t n_blocks, const int64_t* block_ptr, const int32_t* cols);
/* The same blocks given by their affine structure, as smooth_fit's node blocks are (single-GPU
 * handles): block b (0 <= b < n_blocks) holds the k <= 16 compact columns base[j] + b*stride[j],
 * whose full columns (lsq_set_col_map) are full_base[j] + b*full_stride[j].  The blocks must cover
 * every compact column exactly once (n_blocks*k == n).  The library forms the block arrays on the
 * device and checks all of this there (no 10^7-entry host column lists); on a violation it
 * returns < 0 and leaves no blocks set.  Replaces the explicit block_ptr / cols that
 * constraint_functions.node_column_blocks builds for the reference's Ip_c column space
 * (constraint_functions.py:112-151: every column except dz[:, :, reference_epoch]). */
int lsq_set_column_blocks_affine(lsq_handle* h, int64_t n_blocks, int32_t k, const int64_t* base, const int64_t* stride,
                                 const int64_t* full_base, const int64_t* full_stride);

int lsq_shape(lsq_handle* h, int64_t* m, int64_t* n, int64_t* nnz);
/* Download the formed A (selected rows only, in row order; canonical CSR, sorted columns). */
int lsq_get_csr(lsq_handle* h, int64_t* indptr, int32_t* indices, double* data);
/* Full CSR of a lazily formed system.  lsq_set_matrix_stencil on one GPU stores only the data rows
 * of G (the stencil rows live as part descriptors); these calls form the full G and Gᵀ on the
 * device and keep them: lsq_get_csr, lsq_spmv / lsq_spmv_rows past the data rows, the dense
 * (precond 2) and band (precond 5) factors, lsq_cov_band*, the mixed multigrid set-up, the
 * assembled SELL operator (precond 0/1 LSQR without the stencil operator) and the distributed
 * relabelling.  lsq_shape does not.  lsq_release_full_csr frees G / Gᵀ / the SELL copies again
 * (the factors already built stay valid); *released = 0 when there was nothing to free (formed
 * eagerly, never expanded, or relabelled for ranks). */
int lsq_release_full_csr(lsq_handle* h, int32_t* released);

/* ---- solve and products ----------------------------------------------------------------- */
/* x = argmin || A x - diag(row_weight)·mask·b ||.  b has length m (unweighted rhs, all rows);
 * x_inout has length n (compacted columns).  Returns 0 converged, 1 maxit reached. */
int lsq_solve(lsq_handle* h, const double* b, double* x_inout, const lsq_opts* o, lsq_stats* s);

/* y = G x (trans = 0; x length n, y length m, UNWEIGHTED rows, all rows) or
 * y = Gᵀ x (trans = 1).  G is the formed operator before row weights and row mask. */
int lsq_spmv(lsq_handle* h, int32_t trans, const double* x, double* y);
/* Rows [first, first + count) of G x only (e.g. the data rows: z_est / residuals, smooth_fit.py:146
 * and :662, without moving the constraint rows over PCIe). */
int lsq_spmv_rows(lsq_handle* h, int64_t first, int64_t count, const double* x, double* y);

/* Output statistics of smooth_fit's parse_model (smooth_fit.py:318-347) without moving the
 * operator to the host.  lsq_rows_sumsq: for each row range k, u = (G x) over rows
 * [first[k], first[k] + count[k]) (x in compacted columns) and sum_w[k] = Σ (w_i u_i)², sum_u[k]
 * = Σ u_i² with w the current row weights (R and RMS of each constraint type, smooth_fit.py:
 * 324-331).  lsq_data_colsum: out = G_dataᵀ f over the FULL column space (length n_full; f has
 * one value per data row, unweighted rows, removed columns included) — the per-node sums of the
 * count / misfit maps (smooth_fit.py:341-347); structured systems on one (y, x) lattice only. */
int lsq_rows_sumsq(lsq_handle* h, const double* x, int32_t n_ranges, const int64_t* first, const int64_t* count,
                   double* sum_w, double* sum_u);
int lsq_data_colsum(lsq_handle* h, const double* f, double* out);

/* Bench / profiling hook: run exactly `iters` LSQR iterations on the current system (no early
 * stop), starting from the state left by the previous call (first call initialises from b).
 * Times only the device iterations. */
int lsq_iterate(lsq_handle* h, const double* b, int64_t iters, const lsq_opts* o, lsq_stats* s);

/* ---- error propagation (replaces sparseqr.rz + inv_tr_upper + row RSS, smooth_fit.py:212-253)
 * Dense device Cholesky AᵀA = RᵀR of the current weighted, masked A (n up to a few 10^4):
 * lsq_sigma_x: E_j = sqrt(diag((AᵀA)^-1))_j = sqrt(row sums of R^-1 squared), length n;
 * lsq_get_rinv: R^-1 as a dense n x n row-major upper-triangular matrix. */
int lsq_sigma_x(lsq_handle* h, double* E);
int lsq_get_rinv(lsq_handle* h, double* Rinv);
/* Column order for precond 5 (band factor): perm[j] = the compact column at position j, chosen so
 * that AᵀA is banded (a grid system: its natural row-major order; others: e.g. reverse
 * Cuthill-McKee).  nullptr = natural order.  Precond 5 (LSQR on the assembled operator,
 * single GPU): M = P·S·R̃⁻¹ with R̃ the banded Cholesky factor of the equilibrated S·PᵀAᵀAP·S
 * (band.hip), applied by one band back / forward substitution per product — the large-n
 * counterpart of precond 2, for systems column scaling cannot precondition (the anisotropic
 * notebook: > 5·10⁴ column-scaled iterations).  Refused when the band is wider than 300 tiles. */
int lsq_set_band_order(lsq_handle* h, int64_t n, const int32_t* perm);

/* Error propagation without a dense factor (replaces sparseqr.rz + inv_tr_upper +
 * propagate_qz_errors at smooth_fit.py:218-253 and op.grid_error(Ip_c·Rinv) at :266-270).
 * perm (length n, nullable = identity): new position j -> compact column perm[j]; an order in
 * which AᵀA is banded (smooth_fit: node-major).  AᵀA of the current weighted, masked system is
 * equilibrated and factored inside its band (64×64 tiles, f64 MFMA); the rows of R⁻¹ needed are
 * formed by banded forward sweeps (never stored).  E[c] = sqrt(((AᵀA)⁻¹)_cc) per compact column.
 * For the n_ops rows of the CSR op (op_ptr[n_ops+1], op_col = compact columns, op_val):
 * op_err[i] = sqrt(op_i (AᵀA)⁻¹ op_iᵀ).  info (nullable, 6): band width in 64-column tiles, tile
 * rows, device bytes, 64×64 tile products of the sweeps, µs of the factorization and of the
 * sweeps (host wall clock).  Error -2 when the band does not fit the device's free memory. */
int lsq_cov_band(lsq_handle* h, const int32_t* perm, double* E, int64_t n_ops, const int64_t* op_ptr,
                 const int32_t* op_col, const double* op_val, double* op_err, int64_t* info);

/* lsq_cov_band for a banded system with a dense BORDER (smooth_fit's data and slope biases: a
 * bias column couples every node its track crosses, so no order makes the whole AᵀA banded).
 * perm has one entry per compact column: its first n - n_border positions are the band columns in
 * a banded order, its last n_border positions the border columns.  With
 *   AᵀA = [ N  Bᵗ ]    N = R̃ᵀR̃ (the band factor of the principal submatrix, as lsq_cov_band_window)
 *         [ B  C  ]    Y = R̃⁻ᵀBᵗ,  S = C − YᵀY = R_SᵀR_S (n_border × n_border dense),  V = R̃⁻¹(Y R_S⁻¹)
 *   var(band column j)   = (N⁻¹)_jj + ‖V_j·‖²   (the first term: lsq_cov_band's sweeps)
 *   var(border column j) = ‖(R_S⁻¹)_j·‖²
 *   var(op row q)        = q N⁻¹ qᵀ + ‖q V‖²     (op rows must hold band columns only)
 * on the equilibrated matrix; Y and V (n_pad × k_pad, k_pad = n_border rounded up to 64) are
 * stored, one workgroup per panel of 64 right-hand sides runs each substitution on f64 MFMA, and
 * every sum has a fixed order (results are bitwise equal run to run).  E per compact column and
 * op_err as lsq_cov_band.  n_border = 0 is lsq_cov_band itself.  At most LSQ_BORDER_MAX border
 * columns: beyond, and when Y and V (2·n_pad·k_pad·8 bytes, plus 2·k_pad²·8) do not fit 0.8 of the
 * device's free memory beside the band, the call is refused (-5) before the border is allocated.
 * -2: perm is not a permutation, an op row reaches a border column, n_border < 0 or > n, or the
 * border block S is not positive definite (a border column without a kept data row or a weighted
 * constraint row).  info (nullable, 10): [0..5] as lsq_cov_band ([5]: the band's sweeps only),
 * k_pad, device bytes of the border buffers, µs of the border steps (host wall clock), f64 flops
 * of the two substitutions. */
#define LSQ_BORDER_MAX 4096
int lsq_cov_band_bordered(lsq_handle* h, const int32_t* perm, int64_t n_border, double* E, int64_t n_ops,
                          const int64_t* op_ptr, const int32_t* op_col, const double* op_val, double* op_err,
                          int64_t* info);

/* The border term of compute_E where no band factor of the whole system fits (the tiled windows of
 * lsq_cov_band_windows, lssurf_amd/errors.py): Z = N⁻¹Bᵗ by k CGNR solves instead of the band factor.
 * The handle holds the GRID-ONLY structured system A_g with its current row weights and row mask
 * (W = weight × mask); the k border columns are passed here: B over the data rows as CSC (colptr[k+1],
 * rows strictly increasing within a column, vals UNWEIGHTED: W applies to these rows as to A_g's) and
 * c_con (k × k, row-major), the already weighted share of C from rows that touch border columns only
 * (smooth_fit's bias and slope constraint rows).  With N = A_gᵀW²A_g and C = BᵗW²B + c_con:
 *   z_j = argmin ‖W(A_g x − b_j)‖ = N⁻¹A_gᵀW²b_j        one lsq_solve-like CGNR solve per column, from x = 0,
 *                                                       with the options o (method 1; precond 1, 3 or 4)
 *   T = BᵗW²(A_d Z),  S = C − ½(T + Tᵀ),  S̃ = s_k S s_k = R̃ᵀR̃  (s_k = diag(C)^-½; dense.hip's tile kernels)
 *   var_add[j]    = ‖(Z s_k R̃⁻¹)_j·‖²     per compact column (n): add to the grid-only (N⁻¹)_jj
 *   var_border[j] = s_k[j]²‖(R̃⁻¹)_j·‖²     the border columns' variances (k)
 *   op_add[i]     = ‖(op_i Z) s_k R̃⁻¹‖²    per op row (compact columns, as lsq_cov_band): add to op_i N⁻¹ op_iᵀ
 * The row scales, the block factors or the multigrid levels and the ‖A‖ estimate are set up once for
 * all k solves.  Z (n_pad × k_pad, column-major; n_pad, k_pad = n, k rounded up to 64) stays on the
 * device, V = Z s_k R̃⁻¹ is never stored (f64 MFMA over 64-row panels of Z), and every sum has one
 * fixed order without atomics: a second call returns the same bits.
 * Returns -1 when a column's solve ends without istop 1 or 2 (the message names the column; a column
 * without a kept row stops at once with z_j = 0 and counts as solved); no output is written then.
 * -2: a bias, slope or sensor-grid elimination is set on the handle, the handle is a rank of a
 * group, there is no CGNR operator for o->precond (see lsq_cg_available), a malformed border or op
 * row, or S is not positive definite (as lsq_cov_band_bordered).  -5 before anything is allocated:
 * more than LSQ_BORDER_MAX columns, or n_pad·k_pad·8 + 3·k_pad²·8 bytes exceed 0.8 of the free device
 * memory beside the solver's buffers (the message names the largest k that fits; LSQ_BSOLVE_BUDGET,
 * a byte count read per call, overrides the budget for tests).  The handle stays usable after
 * every error.  info (nullable, 12 doubles): k_pad, device bytes, total and largest CG iterations
 * of a column, µs of the solves, of T, of S and its factor, of var_add, of op_add (host wall clock,
 * stream synchronised), asym = max_ij |T_ij − T_ji| s_i s_j (0 for exact solves: a free run-time
 * measure of their accuracy), the smallest pivot of S̃ (asym / pivot bounds what the solves' error
 * does to S̃⁻¹), µs of the var_add kernel alone (device events). */
int lsq_cov_border_solved(lsq_handle* h, int64_t k, const int64_t* colptr, const int32_t* rows, const double* vals,
                          const double* c_con, const lsq_opts* o, int64_t n_ops, const int64_t* op_ptr,
                          const int32_t* op_col, const double* op_val, double* var_add, double* var_border,
                          double* op_add, double* info);

/* The same for a WINDOW of the columns (compute_E at scale, lssurf_amd/errors.py method 'window'):
 * perm[0..n_win) lists the window's compact columns in a banded order; the principal submatrix
 * (AᵀA)_WW = A_WᵀA_W (the other columns held fixed) is factored and E[j] = sqrt(((AᵀA)_WW⁻¹)_jj)
 * in WINDOW order (n_win entries).  inner (nullable = every position): only the 64-column tiles
 * of the window order that hold a flagged position are swept (the interior whose σ the caller
 * keeps — the margin's sweeps are most of the work), and E is 0 at the other positions.  op rows
 * must lie inside the window.  (AᵀA)⁻¹'s correlations decay with node distance, so the window's
 * interior nodes carry diag((AᵀA)⁻¹) to a tolerance set by the margin (DESIGN.md §Error
 * propagation). */
int lsq_cov_band_window(lsq_handle* h, const int32_t* perm, int64_t n_win, const uint8_t* inner, double* E,
                        int64_t n_ops, const int64_t* op_ptr, const int32_t* op_col, const double* op_val,
                        double* op_err, int64_t* info);

/* Many windows at once (compute_E at scale): window w is perm[win_ptr[w] .. win_ptr[w+1]) with its
 * inner flags and E (window order) at the same positions, and the op rows [win_ops[w],
 * win_ops[w+1]) of the CSR op (op_ptr, op_pos = POSITIONS in window w, op_val; win_ops nullable:
 * none) with op_err per row.  Windows are independent: they run on LSQ_E_LANES (default 2) stream
 * lanes, one window's factorization (a latency-bound chain of tile steps) beside another's sweeps.
 * info (nullable, 6): widest band, most tile rows, device bytes, tile products, µs, lanes. */
int lsq_cov_band_windows(lsq_handle* h, int64_t n_windows, const int64_t* win_ptr, const int32_t* perm,
                         const uint8_t* inner, double* E, const int64_t* win_ops, const int64_t* op_ptr,
                         const int32_t* op_pos, const double* op_val, double* op_err, int64_t* info);

/* Many windows with their bottom margin eliminated first (compute_E at scale; DESIGN.md §Error
 * propagation, round 6): window w's columns are perm[win_ptr[w] .. win_ptr[w+1]) = A = [top margin
 * rows, interior rows] in ascending band order, its last nib[w] columns being Ib (the interior rows
 * the bottom margin's rows reach); bot_perm[bot_ptr[w] .. bot_ptr[w+1]) = B' = the band order of
 * [Ib, bottom margin] REVERSED (bot_ptr[w+1] = bot_ptr[w]: no bottom margin).  B' is factored, its
 * trailing Ib block gives the bottom margin's Schur complement onto Ib, which replaces A's (Ib, Ib)
 * block; A is then factored and swept over the tiles holding an inner position, so the sweeps end
 * at the interior.  E (window order, A's positions) equals lsq_cov_band_windows' E of the whole
 * window [A, bottom margin] to rounding.  Fails (-3, "a deeper Ib is needed") when a row holds a
 * column of A outside Ib and one of the bottom margin.  info as lsq_cov_band_windows. */
int lsq_cov_band_windows_schur(lsq_handle* h, int64_t n_windows, const int64_t* win_ptr, const int32_t* perm,
                               const uint8_t* inner, double* E, const int64_t* bot_ptr, const int32_t* bot_perm,
                               const int64_t* nib, int64_t* info);

/* The banded factor itself (replaces sparseqr.rz's R and E, smooth_fit.py:218 / the aniso notebook):
 * for the current weighted, masked A and the column order perm (nullable = natural),
 * (A·P)ᵀ(A·P) = RᵀR with R = R̃·S⁻¹, R̃ the upper band factor of the equilibrated S·Pᵀ(AᵀA)P·S.
 * info (3): n, T = tile rows (n padded to 64·T), w = tiles right of the diagonal per tile row.  When
 * R is non-null: R̃ as T·(w+1) row-major 64×64 tiles, tile (I, J) (I ≤ J ≤ I + w) at
 * (I·(w+1) + J − I)·4096 (use the upper triangle of diagonal tiles), sc = diag(S) (64·T), perm_out =
 * P (new position -> compact column, n).  Call once with R = NULL for the sizes.  -5 when the band
 * does not fit the device. */
int lsq_band_factor(lsq_handle* h, const int32_t* perm, int64_t* info, double* R, double* sc, int32_t* perm_out);

/* ---- multi-GPU (one process per GPU) --------------------------------------
 * lsq_dist_unique_id: rank 0 creates the 128-byte RCCL id; the caller broadcasts it (any
 * transport); every rank then calls lsq_create_dist.  Each rank forms only the rows it owns
 * (lsq_set_col_map + lsq_set_matrix_* with GLOBAL column ids), reads which columns its rows
 * reference, and installs its layout: col_local maps every global column to a local id
 * ([0, n_own) owned, [n_own, n_local) ghosts grouped by owning peer, -1 unused); for each
 * peer, send_idx lists the owned local columns that peer holds as ghosts (in the order of the
 * peer's ghost slots) and recv_cnt the number of ghosts it owns.  lsq_solve / lsq_iterate then
 * run one LSQR over all ranks: halo exchange of ghost v before A·v, reverse halo of ghost
 * partial sums after Aᵀu, RCCL all-reduce of the scalar norms; x_inout receives the owned
 * columns (length n_own). */
int lsq_dist_unique_id(uint8_t* id128);
lsq_handle* lsq_create_dist(int32_t device, int32_t rank, int32_t nranks, const uint8_t* id128);
/* What the rank's RCCL communicator and device report (bench.py's self-check of a multi-GPU run):
 * out[0] ncclCommCount, out[1] ncclCommUserRank, out[2] ncclCommCuDevice, out[3] the handle's
 * HIP device, out[4..6] its PCI domain / bus / device ids (a physical card: two ranks with equal
 * ids share one GPU).  A handle without a communicator reports count 0. */
int lsq_dist_comm_info(lsq_handle* h, int64_t* out7);
int lsq_dist_referenced_cols(lsq_handle* h, uint8_t* flags);
int lsq_dist_set_layout(lsq_handle* h, const int32_t* col_local, int64_t n_local, int64_t n_own,
                        int32_t n_peers, const int32_t* peers, const int64_t* send_cnt,
                        const int32_t* send_idx, const int64_t* recv_cnt);

/* Structured-operator ranks (systems formed by lsq_set_matrix_stencil): each rank forms its
 * window of node rows — owned rows ± halo rows, as sub-grids with their own column numbering —
 * and installs the halo: own_ranges = n_ranges [start, end) pairs of owned local full columns;
 * per peer, send_idx lists owned local columns that peer holds as ghosts and recv_idx the local
 * ghost columns that peer owns (both in ascending GLOBAL column order).  lsq_solve then returns
 * every local compact column in x_inout (length = the local compact width; ghosts come out 0). */
int lsq_dist_set_halo(lsq_handle* h, int32_t n_ranges, const int64_t* own_ranges, int32_t n_peers,
                      const int32_t* peers, const int64_t* send_cnt, const int32_t* send_idx,
                      const int64_t* recv_cnt, const int32_t* recv_idx);

/* Multigrid over ranks (precond 4, method 1): the global structure behind a structured rank's
 * window — the global grids and stencil parts (the descriptors of lsq_set_matrix_stencil for the
 * whole system; field-valued parts with ntpl = 0), local_of[s] = the rank's stencil index of global
 * stencil s (-1: the rank holds none of its rows), and the window in global node rows of dim 0:
 * window start, owned rows [own_row0, own_row1), rows of the lattice.  Level 0 of the V-cycle is
 * each rank's window (halo exchanges around every operator application), the coarse levels are
 * the global Galerkin levels replicated on every rank (the restricted residual summed over the
 * ranks once per cycle, the lumped data rows once per solve). */
int lsq_dist_set_global(lsq_handle* h, int64_t n_full, int32_t n_grids, const lsq_grid_desc* grids, int32_t n_stencil,
                        const lsq_stencil_desc* stencils, const int32_t* local_of, int32_t win_row0, int32_t own_row0,
                        int32_t own_row1, int32_t rows);

/* Virtual ranks: the same distributed solve with every rank of the partition in THIS process
 * on one device (exchanges become device copies).  Configure each rank's handle exactly as a
 * real rank (lsq_set_col_map, lsq_set_matrix_*, lsq_dist_referenced_cols,
 * lsq_dist_set_layout), then solve all ranks at once; b / x are per-rank arrays. */
typedef struct lsq_vgroup lsq_vgroup;
lsq_vgroup* lsq_vgroup_create(int32_t device, int32_t nranks);
lsq_handle* lsq_vgroup_rank(lsq_vgroup* g, int32_t rank);
int lsq_vgroup_solve(lsq_vgroup* g, const double* const* b, double* const* x, const lsq_opts* o,
                     lsq_stats* s);
int lsq_vgroup_iterate(lsq_vgroup* g, const double* const* b, int64_t iters, const lsq_opts* o,
                       lsq_stats* s);
const char* lsq_vgroup_last_error(lsq_vgroup* g);
void lsq_vgroup_destroy(lsq_vgroup* g);
/* Test hook: what rank `rank` of the group holds from its last multigrid solve (method 1, precond 4).
 * out[0] = levels L, out[1] = lp (levels 1 ... lp are partitioned over the ranks, the rest replicated),
 * then per level l three values: the smoother's lambda of that solve's set-up (0 for the coarsest level),
 * and the node rows [oa, ob) of the level the rank owns (level 0: of the global fine lattice).  cap must
 * hold 2 + 3L values.  Reads state only: no set-up, no solve path changes.  Returns the count written,
 * or -1 with the reason in lsq_vgroup_last_error (no multigrid solve yet, rank out of range, cap). */
int lsq_vgroup_mg_info(lsq_vgroup* g, int32_t rank, double* out, int64_t cap);

/* Device group: the distributed solve over N distinct devices from ONE process (smooth_fit's
 * n_gpus; SURVEY.md §8(b) "ranks invisible to Python").  One RCCL communicator per device
 * (ncclCommInitAll); each solve runs every rank on its own host thread with the kernels, halos
 * and all-reduces of a one-process-per-GPU rank.  Configure each rank's handle as a real rank
 * (lsq_set_col_map, lsq_set_matrix_stencil, lsq_dist_set_halo, lsq_dist_set_global ...).
 * Repeated devices are refused (NULL): one device runs the same ranks through lsq_vgroup. */
typedef struct lsq_dgroup lsq_dgroup;
lsq_dgroup* lsq_dgroup_create(int32_t n, const int32_t* devices);
lsq_handle* lsq_dgroup_rank(lsq_dgroup* g, int32_t rank);
int lsq_dgroup_solve(lsq_dgroup* g, const double* const* b, double* const* x, const lsq_opts* o, lsq_stats* s);
int lsq_dgroup_iterate(lsq_dgroup* g, const double* const* b, int64_t iters, const lsq_opts* o,
                       lsq_stats* s);
const char* lsq_dgroup_last_error(lsq_dgroup* g);
void lsq_dgroup_destroy(lsq_dgroup* g);
/* The rank threads of a device-group call meet at a host fence before every RCCL call; a rank
 * that fails poisons it, so the others return an error at their next collective instead of
 * blocking in it.  Self-test of that fence (no device): n threads pass `rounds` fences, thread
 * fail_rank (-1: none) throws before round fail_rank; returns the number of threads that left
 * on the poisoned fence (n - 1 when one rank failed, 0 otherwise). */
int lsq_fence_selftest(int32_t n, int32_t fail_rank, int32_t rounds);

/* ---- outlier editing (RDE.py:10-18, calc_sigma_extra.py:13-44) -----
 * calc_sigma_extra's bounded search evaluates RDE(r / sqrt(s² + σ²)) 25–30 times per outer
 * iteration.  lsq_rde_create uploads r and σ once (finite entries only); lsq_rde_order_stats
 * returns the requested order statistics (0-based ranks) of r / sqrt(s² + σ²), computed exactly
 * as numpy does, so the caller's percentile interpolation is bit-identical to RDE's. */
typedef struct lsq_rde lsq_rde;
lsq_rde* lsq_rde_create(int32_t device, int64_t n, const double* r, const double* sigma);
int lsq_rde_order_stats(lsq_rde* c, double sigma_extra, int64_t n_idx, const int64_t* idx, double* out);
const char* lsq_rde_last_error(lsq_rde* c);     /* c = NULL: why the last create_segments failed */
void lsq_rde_destroy(lsq_rde* c);

/* Binned sigma_extra (calc_sigma_extra_on_grid.py): many overlapping segments of one point set —
 * segment k = the points seg_idx[seg_ptr[k] .. seg_ptr[k+1]) (seg_ptr[0] = 0, fewer than 2^31
 * entries in all) — each with its four 0-based ranks seg_rank[4k..4k+4) = (j_lo, j_lo+1, j_hi,
 * j_hi+1).  lsq_rde_create_segments keeps segment-contiguous copies of r and σ on the device.
 * status (nullable): 0, -2 = invalid argument (non-monotone seg_ptr, index >= n, rank >= segment
 * size, ranks not two adjacent pairs), -5 = declined (the context does not fit about 0.8 of the
 * free device memory, or 2^31 entries), -3 = HIP error; NULL is returned unless 0.
 * lsq_rde_select: for the active segments seg[a] (each at most once) and their trial s[a], the
 * four order statistics of r / sqrt(s[a]² + σ²) — raw != 0: of r itself — over segment seg[a] go
 * to out[4a..4a+4), bit-identical to np.sort(x)[ranks] (±0 may differ in sign).  An MSB-first
 * radix select on order-preserving 64-bit keys, no sort: segments of up to lsq_rde_small_max()
 * points run one workgroup each with their keys in LDS, larger ones multi-workgroup histogram
 * passes with the bucket decisions taken on the device; one launch sequence and one
 * device-to-host copy per call.  A context of lsq_rde_create refuses lsq_rde_select and a
 * segmented one lsq_rde_order_stats (-2). */
lsq_rde* lsq_rde_create_segments(int32_t device, int64_t n, const double* r, const double* sigma,
                                 int64_t n_seg, const int64_t* seg_ptr, const int32_t* seg_idx,
                                 const int64_t* seg_rank, int* status);
int lsq_rde_select(lsq_rde* c, int64_t n_act, const int32_t* seg, const double* s, int32_t raw,
                   double* out);
int64_t lsq_rde_small_max(void);

/* Bench / profiling hooks.  lsq_profile_kernels times each iteration kernel of the operator
 * `op` (lsq_opts.op) in isolation (reps launches each, HIP events on the handle's stream):
 * out8 = {ms of x/w+A·v, ms of Aᵀu, ms of beta reduce, ms of rotation, algorithmic HBM bytes
 * per launch of x/w+A·v, of Aᵀu (DESIGN.md §Byte model), 0, 0}.  It clobbers the iteration
 * state.  lsq_sell_info: out8 = {m, n, nnz, SELL entries streamed by A·v, by Aᵀu, device bytes
 * of the operator copies, 1 if the structured stencil operator is available, n_full}. */
int lsq_profile_kernels(lsq_handle* h, int32_t reps, int32_t op, double* out8);
/* CGNR (method 1) hooks.  lsq_cg_available: 1 when method 1 runs CGNR on this system with this
 * preconditioner (it builds the normal-stencil tables), 0 when it would fall back to LSQR (the
 * reason is in lsq_last_error).  lsq_profile_cg: per-kernel HIP-event times of one CG iteration,
 * out8 = {ms data rows t = Ad·p, ms normal operator q = N p + Adᵀt, ms update + preconditioner,
 * ms of the two scalar kernels, algorithmic HBM bytes per launch of the first three, mode bits:
 * 1 matrix-free data rows, 2 wave-strip normal kernel, 4 column-mode operator (else tile mode),
 * 8 chunk mode (tile mode's step on tiles cut along the last grid dimension; bit 4 clear)}.
 * lsq_normal_apply: q = AᵀA p for the current row weights/mask, p and q over the FULL column
 * space (length n_full of lsq_set_col_map; test hook for the normal operator). */
int lsq_cg_available(lsq_handle* h, int32_t precond);
int lsq_profile_cg(lsq_handle* h, int32_t reps, int32_t precond, double* out8);
/* Chunk mode: CGNR on grids of 20 to 64 nodes along their last dimension (epochs), where a
 * tile-mode image of whole time columns exceeds 64 KB of LDS and method 1 otherwise falls back to
 * LSQR.  lsq_set_cg_chunks(h, 1) lets the layout cut such a grid's tiles along the last dimension
 * too (k_cg_normal_chunk); systems that run column or tile mode are laid out and solved exactly as
 * without it, and what tile mode refuses (multigrid, eliminated biases / slopes / sensor grids,
 * extra rows, more than 64 nodes) stays refused.  Callable any time after lsq_create; a change
 * drops the CGNR description, the captured iterations and the multigrid levels, and the next
 * lsq_cg_available / lsq_solve lays out afresh.  Returns −2 (reason in lsq_last_error) on a rank of
 * a distributed, virtual or device group.  Default: off.
 * lsq_cg_layout_info builds the description if needed: out8 = {mode (0 no CGNR operator — the
 * reason is in lsq_last_error —, 1 column, 2 tile, 3 chunk), rows per tile ty of the grid with the
 * longest last dimension, its chunk length tc, its chunks per tile, the LDS stride of its node
 * columns, LDS bytes of the largest tile, workgroups of one normal-operator launch, 0}. */
int lsq_set_cg_chunks(lsq_handle* h, int32_t on);
/* Tile and chunk mode on matrix-free data rows.  lsq_set_cg_tile_dmf(h, 1), called BEFORE the
 * formation (lsq_set_matrix_stencil), lets the formation keep the sorted point table for a 3-D
 * interpolation grid of up to 64 nodes along its last dimension (16 without it), and lets a tile- or
 * chunk-mode CGNR step (16 to 19 nodes; 20 to 64 with lsq_set_cg_chunks) run in column mode's order:
 * q = N_s p by k_cg_normal / k_cg_normal_chunk without the stored ATd rows, t = Ad·p from the points,
 * the elimination of data biases, slopes and sensor grids, then the node gather (k_cg_dmf_atq, or
 * k_cg_dmf_atq_long above 16 nodes).  lsq_set_data_bias, lsq_set_data_slope and lsq_set_sensor_grids
 * then run on such a handle; lsq_profile_cg reports mode bit 1 beside a clear bit 4.  Still refused
 * there: multigrid (precond 4), extra rows, more than 64 nodes, 20 or more without
 * lsq_set_cg_chunks.  Column-mode systems, and every system without the switch, run exactly as
 * before.  A change drops the CGNR description, the captured iterations and the multigrid levels.
 * Returns −2 (reason in lsq_last_error) on a rank of a distributed, virtual or device group.
 * Default: off. */
int lsq_set_cg_tile_dmf(lsq_handle* h, int32_t on);
int lsq_cg_layout_info(lsq_handle* h, int64_t* out8);
/* Per-row constraint scales inside CGNR.  A stencil part whose rows do not share one row scale
 * (weight × row mask) — the constraint rows of a masked fit, or of one with constraint scaling maps —
 * has no class-table normal stencil: lsq_cg_available is 0 ("a stencil part has per-row scales …")
 * and method 1 falls back to LSQR.  lsq_set_cg_scaled(h, 1) keeps such a part in the matrix-free
 * CGNR operator when its scale is one value per (y, x) node: the part is left out of the class table
 * and applied by k_cg_scaled from a squared-scale field over its (y, x) centre box, rebuilt from the
 * row scales whenever they are refreshed.  Refused with the key too (lsq_cg_available 0, the reason
 * names the part): scales that differ in any bit along the last dimension at one node, a reach beyond
 * ±2 in y or x, tile and chunk mode (16 nodes and more along the last dimension), ranks of a
 * distributed, virtual or device group; precond 4 is refused with "multigrid: per-row constraint
 * scales".  Systems whose parts all share one scale, and every system without the key, run exactly
 * as before.  Callable any time after lsq_create; a change drops the CGNR description, the captured
 * iterations and the multigrid levels.  Returns −2 on a rank of a distributed, virtual or device
 * group.  Default: off.
 * lsq_cg_scaled_info builds the description if needed: out4 = {scaled parts, bytes of their fields,
 * grids with scaled parts, workgroups of their launches} (zeros without the key or the operator).
 * lsq_profile_cg_scaled: after lsq_iterate with the same precond (its live state), reps more real
 * iterations with device events around k_cg_scaled: out4 = {ms of its launches per step, their
 * algorithmic bytes (24 B per column of the grids with scaled parts + 8 B per part and node of
 * field), ms of the normal kernel and the x-edge pass in front of them, ms of the whole step}. */
int lsq_set_cg_scaled(lsq_handle* h, int32_t on);
int lsq_cg_scaled_info(lsq_handle* h, int64_t* out4);
int lsq_profile_cg_scaled(lsq_handle* h, int32_t reps, int32_t precond, double* out4);
/* Multigrid (precond 4) test hooks.  lsq_mg_info: out[0] = levels L, then per level
 * (S0, S1, n_full, removed epoch) — cap must hold 1 + 4L values.  lsq_mg_apply on level l's full
 * column space (z0 grid then dz grid, in the system's order): what 0: y = N_l x (level 0: AᵀA;
 * coarse levels: Galerkin PᵀNP of the stencil rows + the (y, x)-lumped data rows), 1: y = the
 * V-cycle from level l down applied to x (the coarsest level: its dense inverse; a system with z0
 * on a refined lattice exposes level 0 only), 2: y[0] = the smoother's λ_max(M⁻¹N) estimate of level l,
 * 3: y[0] = the kernel family of level l's operator (0 ring kernel + x-edge pass, 1 k_mg_direct,
 * 2 k_mg_tile, 3 k_mg_tile_kt, −1 the coarsest level; systems with z0 on the dz lattice).
 * Both build the hierarchy for the current row weights / mask. */
int lsq_mg_info(lsq_handle* h, int64_t* out, int64_t cap);
int lsq_mg_apply(lsq_handle* h, int32_t level, int32_t what, const double* x, double* y);
int lsq_normal_apply(lsq_handle* h, const double* p, double* q);

/* Data biases: one additive unknown b_j per bias ID on the data rows (data row i gains a 1 in the
 * column of id[i]) with the constraint rows c_j b_j = 0 (c_j = 1 / the bias's expected size).  The
 * library never forms these columns: CGNR eliminates them exactly, solving the reduced problem in
 * the grid unknowns (normal operator AᵀA − A_dᵀ W Q W A_d, Q = W B D⁻¹ Bᵀ W, D_j = Σ_{i∈j} W_i² + c_j²,
 * W = the data rows' current weight × mask), so x keeps its length.
 * lsq_set_data_bias: call after lsq_set_matrix_stencil.  id[i] ∈ [0, nb) for data row i in the
 * caller's row order, c[j] > 0; npts must equal the system's data rows.  nb = 0 or a null pointer
 * clears the biases; setting or clearing them also clears the slopes of lsq_set_data_slope (below),
 * which index the bias IDs.  Returns −2 (the handle and any biases set before stay as they were) on an ID
 * out of range, a c that is not > 0, or a wrong npts.  The biases belong to the handle's matrix: a
 * handle takes one matrix (a second lsq_set_matrix_* returns −2 and changes nothing, the biases
 * included), and every formation of the operator starts without biases.
 * With biases set, lsq_solve / lsq_iterate run only as matrix-free CGNR on one GPU (method 1,
 * precond 1, 3 or 4, interpolation grids on one (y, x) lattice); anything else returns −2 with the
 * reason, and lsq_cg_available reports 0 with it.  lsq_normal_apply then applies the reduced
 * operator.  lsq_spmv / lsq_spmv_rows / lsq_get_csr stay the grid operator only.
 * lsq_get_data_bias: the nb biases that belong to the last lsq_solve's x,
 * b_j = Σ_{i∈j} W_i² (d_i − (A_d x)_i) / D_j (0 for an ID no row carries); −2 before any solve. */
int lsq_set_data_bias(lsq_handle* h, int64_t npts, const int32_t* id, int64_t nb, const double* c);
int lsq_get_data_bias(lsq_handle* h, double* b);

/* Slope biases: the data rows of slope group s gain two further unknowns γ_s (a tilt in x and in y,
 * smooth_fit's data_slope_sensors) with the coefficients u[2i], u[2i + 1] on row i and the constraint
 * rows c[2s] γ_s0 = 0, c[2s + 1] γ_s1 = 0.  They are eliminated together with the data biases: with
 * Z = [B U] (B the bias indicator columns, U the slope columns) and M = ZᵀW²Z + C², the normal operator
 * is AᵀA − A_dᵀ W² Z M⁻¹ Zᵀ W² A_d.  The layout must be nested: the rows of every bias ID lie in at most
 * one slope group (rows of group −1 do not count; always true when the sensor is among the bias
 * parameters and the groups are sensors).  M⁻¹ is then one 2 × 2 system per group.
 * lsq_set_data_slope: call after lsq_set_matrix_stencil and, if biases are used, after
 * lsq_set_data_bias.  grp[i] ∈ {−1} ∪ [0, ng) for data row i in the caller's row order; u is read only
 * where grp ≥ 0; c > 0.  ng = 0 or a null pointer clears the slopes (the biases stay, and solve as if
 * no slopes had ever been set, bit for bit).  lsq_set_data_bias, when it sets or clears the biases,
 * clears the slopes too.  Returns −2 with the handle unchanged on a group out of range, a u that is
 * not finite, a c that is not > 0, a wrong npts or a layout that is not nested.
 * Solves, lsq_cg_available and lsq_normal_apply follow the rules of the data biases above, with or
 * without biases set.  Every sum runs in a fixed order without atomics: results are bitwise equal
 * run to run.
 * lsq_get_data_slope: the 2·ng slopes that belong to the last lsq_solve's x (0 for a group no row
 * carries); −2 before any solve. */
int lsq_set_data_slope(lsq_handle* h, int64_t npts, const int32_t* grp, const double* u, int64_t ng, const double* c);
int lsq_get_data_slope(lsq_handle* h, double* g);
/* The slope elimination's kernels timed inside reps real iterations of the live lsq_iterate state
 * (method 1, this precond; HIP events between the launches): out8 = {ms of the chunk pass, of the
 * per-rank sums, of the per-group kernel, of the apply pass, and the algorithmic HBM bytes of each}.
 * −2 without such a state or without slopes in the operator. */
int lsq_profile_data_slope(lsq_handle* h, int32_t reps, int32_t precond, double* out8);

/* Sensor bias grids: the data rows of grid s gain the unknowns a_s, a coarse 2-D grid of additive bias
 * (smooth_fit's sensor_grid_bias_params), through the bilinear weights wt[4i .. 4i + 3] on the nodes
 * node[4i .. 4i + 3] (local to the grid; a weight of 0 pads a dropped corner), and the grid is held by
 * constraint rows C_s a_s = 0.  A row lies in one grid and C_s touches its own nodes only, so with
 * B the interpolation columns and M = BᵀW²B + K, K_s = C_sᵀC_s, the normal operator is
 * AᵀA − A_dᵀ W² B M⁻¹ Bᵀ W² A_d with one dense SPD block M_s per grid (x keeps its length).
 * lsq_set_sensor_grids: call after lsq_set_matrix_stencil.  grid[i] ∈ {−1} ∪ [0, ng) for data row i in
 * the caller's row order; node and wt are read only where grid ≥ 0.  K_s, already weighted and constant
 * over the outer iterations, is passed as the triplets k_ptr[s] … k_ptr[s + 1] (local rows and columns,
 * both triangles, duplicates summed in their order; k_ptr null: no K).  ng = 0 or a null pointer clears
 * the grids, and the handle then solves bit for bit as if none had been set.  Returns −2 with the handle
 * unchanged on a grid or node out of range, a weight or value that is not finite, a wrong npts, data
 * biases or slopes already set (lsq_set_data_bias / lsq_set_data_slope likewise return −2 while grids
 * are set), a node that shares rows with more than 9 nodes (the rows must be cells of a lattice), or a
 * grid over the size cap: at most LSQ_SGRID_MAX_NODES nodes per grid and LSQ_SGRID_MAX_FACTOR_BYTES for
 * all inverse factors together (each npad², npad = nodes rounded up to 64; the device holds two such
 * sets).  Every CG step reads each grid's inverse factor once: 8·npad² bytes, 32 MB at 2048 nodes, about
 * 10 µs of HBM time; all factors at the byte cap cost 0.3 ms per step, three quarters of an iteration of
 * a 2 M-point fit, beyond which the grids are better carried as ordinary columns.
 * Solves, lsq_cg_available and lsq_normal_apply follow the rules of the data biases above: method 1,
 * precond 1, 3 or 4, one GPU.  M_s is assembled and factored at the start of every solve for the
 * current weights and mask; a pivot that is not positive (below 1e-12 of its diagonal entry) makes
 * lsq_solve return −2 with a message that names the grid — a grid held by its curvature only whose
 * kept data do not pin its bilinear null space.  Every sum runs in a fixed order without atomics:
 * results are bitwise equal run to run.
 * lsq_get_sensor_grids: the node values a (grid after grid, Σ n_nodes) that belong to the last
 * lsq_solve's x; −2 before any solve. */
#define LSQ_SGRID_MAX_NODES 2048
#define LSQ_SGRID_MAX_FACTOR_BYTES (1ll << 30)
int lsq_set_sensor_grids(lsq_handle* h, int64_t npts, const int32_t* grid /* −1: none */,
                         const int32_t* node /* 4 per row, local to the grid */, const double* wt /* 4 per row */,
                         int32_t ng, const int64_t* n_nodes, const int64_t* k_ptr, const int32_t* k_row,
                         const int32_t* k_col, const double* k_val);
int lsq_get_sensor_grids(lsq_handle* h, double* a);
/* Sensor grids beside data biases and slopes.  The arguments of lsq_set_sensor_grids; call it after
 * lsq_set_matrix_stencil and after any lsq_set_data_bias / lsq_set_data_slope, whose layout it reads
 * from the handle.  With Z = [B_bias U_slope B_grid] and M = ZᵀW²Z + C the eliminated block stays block
 * diagonal when every bias ID and every slope group lies inside one grid's rows or outside every grid:
 *   - a bias ID with a row in a grid must have all its rows in that grid; the grid's block claims it as
 *     a dense node (coefficient 1 on its rows, c_j² on the diagonal);
 *   - a slope group with a row (grp ≥ 0) in a grid must have all of them in that grid; it is claimed as
 *     two dense nodes (coefficients u, c² on the diagonal);
 *   - the other IDs and groups stay on the bias / slope path, which the rows of every grid leave.
 * The two parts touch disjoint rows and their corrections add.  Returns −2 with the handle unchanged on
 * everything lsq_set_sensor_grids refuses except biases or slopes being set, on an ID or group that is
 * not nested in this sense, on more than LSQ_SGRID_MAX_DENSE dense nodes in one grid, on lattice plus
 * dense nodes over LSQ_SGRID_MAX_NODES, or on inverse factors (counted with the dense nodes) over
 * LSQ_SGRID_MAX_FACTOR_BYTES.  lsq_set_data_bias and lsq_set_data_slope go on returning −2 while grids
 * are set, their clearing forms (nb = 0, ng = 0) included: the blocks hold the claimed IDs and groups; ng = 0 (through either call) clears the grids, and the handle then solves with its biases
 * and slopes bit for bit as if no grid had been set.  Without biases and slopes the call sets exactly
 * what lsq_set_sensor_grids sets.  lsq_get_data_bias and lsq_get_data_slope return every bias and slope
 * of the last solve's x, the claimed ones from their block's solution; lsq_get_sensor_grids returns the
 * lattice nodes only.  The solve rules, lsq_normal_apply, the warm start and lsq_profile_sensor_grids
 * hold as for either part alone.  The step launches the bias path's sums, the blocks' three reduce
 * launches, the bias path's apply pass and the blocks' apply pass: lsq_profile_sensor_grids' first stage
 * then spans the bias path's sums and its fourth the bias path's apply pass as well, and
 * lsq_profile_data_slope's fourth stage spans the blocks' three reduce launches.
 * Every sum runs in a fixed order without atomics. */
#define LSQ_SGRID_MAX_DENSE 16
int lsq_set_sensor_grids_joint(lsq_handle* h, int64_t npts, const int32_t* grid, const int32_t* node,
                               const double* wt, int32_t ng, const int64_t* n_nodes, const int64_t* k_ptr,
                               const int32_t* k_row, const int32_t* k_col, const double* k_val);
/* The sensor grids' kernels timed inside reps real iterations of the live lsq_iterate state (method 1,
 * this precond; HIP events between the launches): out8 = {ms of s = Bᵀ td, of z = R⁻ᵀ s, of y = R⁻¹ z,
 * of the apply pass, and the algorithmic HBM bytes of each}.  −2 without such a state or without grids
 * in the operator. */
int lsq_profile_sensor_grids(lsq_handle* h, int32_t reps, int32_t precond, double* out8);
int lsq_sell_info(lsq_handle* h, int64_t* out8);

/* ---- triangular kernels (replace the Cython kernels; R upper triangular CSR, int32 indices,
 *      sorted column indices, diagonal first in each row) ------------------------------------ */
/* spsolve_tr_upper: x = R^-1 b. */
int tri_upper_solve_csr(int32_t device, int64_t N, const int32_t* indptr, const int32_t* indices,
                        const double* data, const double* b, double* x);
/* inv_tr_upper: columns col = N-1..0 of R^-1, entries emitted (col descending, row descending)
 * when row == col or |x| > tol (tol is a C float, as in the .pyx).  Returns 1 (buffer full)
 * exactly when inv_tr_upper returns status 1, with the same nnz_max entries in rr/cc/vv (the
 * last one zero).  *n_out = number of entries written. */
int tri_upper_inv_csr(int32_t device, int64_t N, const int32_t* indptr, const int32_t* indices,
                      const double* data, int64_t nnz_max, float tol,
                      int32_t* rr, int32_t* cc, double* vv, int64_t* n_out);
/* propagate_qz_errors: E_i = sqrt(sum over columns of (R^-1)_{i,col}^2). */
int tri_upper_rowrss_csr(int32_t device, int64_t N, const int32_t* indptr, const int32_t* indices,
                         const double* data, double* E);
/* Error string of the last failing tri_* call on this thread. */
const char* tri_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* LSQSURF_H */
