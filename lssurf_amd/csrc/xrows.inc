// xrows.inc — extra sparse rows behind the stencil rows (lsq_set_extra_rows), carried by the
// matrix-free CGNR operator.  Included by lsqr_cg.inc inside its anonymous namespace.
//
// The system's last m_x rows X (≤ XR_MAXW entries each, e.g. smooth_fit's dz priors: one
// interpolation row at (y, x, t) minus one at (y, x, t_ref)) are neither data rows nor stencil
// rows.  The normal operator gains XᵀW_x²X (W_x = the rows' weight × mask):
//   k_xr_fwd   t_x[r] = rs[r] · Σ v · p[col]   (SELL-64 slices, one wave per slice) and the
//              workgroups' partials of Σ t_x², appended to the data rows' partials of pᵀNp
//   k_xr_atq   q[c] += Σ_{r∋c} rs[r] · v · t_x[r], one lane per touched column over the transpose
//              (rows ascending); the columns over XR_LONG rows by a wave each (k_xr_atq_long)
// Both run between the data rows' Ad·p and the node gather q += Adᵀ td, whose fused α then sees the
// new partials.  Every sum has a fixed order and no atomics: two runs agree bit for bit.  Launch
// counts and grids depend on m_x and the touched columns only.
// With lsq_set_extra_rows_lumping the multigrid (precond 4) carries the rows too: level 0 of the
// V-cycle launches the same two kernels (mg.inc, mg_launch_xr) and the coarse levels take the rows
// lumped into their node blocks (xr_lump.hpp, k_mg_lump_xr).

// t[r] = rs[r] · ((b ? b[r] : 0) + sgn · Σ v · p[col]) per extra row and part[blockIdx.x] = Σ t².
// The CG step: b = null, sgn = 1; the initial residual: b, p = x0 (or null), sgn = −1.
__global__ __launch_bounds__(BLOCK) void k_xr_fwd(const CgState* __restrict__ st, int64_t m_x, int64_t nslices,
                                                  const int64_t* __restrict__ sp, const int32_t* __restrict__ ci,
                                                  const double* __restrict__ val, const double* __restrict__ rs,
                                                  const double* __restrict__ b, const double* __restrict__ p,
                                                  double sgn, double* __restrict__ t, double* part) {
    if (st && st->stop) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double acc = 0.0;
    for (int64_t s = (int64_t)blockIdx.x * (BLOCK / 64) + wid; s < nslices; s += (int64_t)gridDim.x * (BLOCK / 64)) {
        const int64_t r = s * SELL_C + lane;
        double d = 0.0;
        if (p) {
            const int64_t e = sp[s + 1];
            for (int64_t k = sp[s] + lane; k < e; k += SELL_C) d += val[k] * p[ci[k]];   // padding: val 0, col valid
        }
        if (r < m_x) {
            const double tv = rs[r] * ((b ? b[r] : 0.0) + sgn * d);
            t[r] = tv;
            acc += tv * tv;
        }
    }
    store_partial(acc, part, blockIdx.x);
}

// q[tc[j]] += Σ_e rs[cr[e]] · cv[e] · t[cr[e]] over column j's entries in row order; the columns over
// XR_LONG rows are left to k_xr_atq_long
__global__ __launch_bounds__(BLOCK) void k_xr_atq(const CgState* __restrict__ st, int64_t ntc,
                                                  const int32_t* __restrict__ tc, const int64_t* __restrict__ cp,
                                                  const int32_t* __restrict__ cr, const double* __restrict__ cv,
                                                  const double* __restrict__ rs, const double* __restrict__ t,
                                                  double* __restrict__ q) {
    if (st && st->stop) return;
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < ntc; j += (int64_t)gridDim.x * BLOCK) {
        const int64_t a = cp[j], e = cp[j + 1];
        if (e - a > XR_LONG) continue;
        double s = 0.0;
        for (int64_t k = a; k < e; ++k) {
            const int32_t r = cr[k];
            s += rs[r] * cv[k] * t[r];
        }
        q[tc[j]] += s;
    }
}

// a wave per long column: lane l adds entries l, l + 64, … in row order, then the fixed shuffle tree
__global__ __launch_bounds__(BLOCK) void k_xr_atq_long(const CgState* __restrict__ st, int64_t nlong,
                                                       const int32_t* __restrict__ long_col,
                                                       const int32_t* __restrict__ tc, const int64_t* __restrict__ cp,
                                                       const int32_t* __restrict__ cr, const double* __restrict__ cv,
                                                       const double* __restrict__ rs, const double* __restrict__ t,
                                                       double* __restrict__ q) {
    if (st && st->stop) return;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= nlong) return;   // whole waves leave
    const int32_t j = long_col[i];
    const int64_t e = cp[j + 1];
    double s = 0.0;
    for (int64_t k = cp[j] + lane; k < e; k += 64) {
        const int32_t r = cr[k];
        s += rs[r] * cv[k] * t[r];
    }
    s = wave_sum(s);
    if (lane == 0) q[tc[j]] += s;
}

// Jacobi: norm2[tc[j]] += Σ (rs · v)² over column j (full-space squared column norms)
__global__ __launch_bounds__(BLOCK) void k_xr_colnorm(int64_t ntc, const int32_t* __restrict__ tc,
                                                      const int64_t* __restrict__ cp, const int32_t* __restrict__ cr,
                                                      const double* __restrict__ cv, const double* __restrict__ rs,
                                                      double* __restrict__ norm2) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < ntc; j += (int64_t)gridDim.x * BLOCK) {
        double s = 0.0;
        for (int64_t k = cp[j]; k < cp[j + 1]; ++k) {
            const double a = rs[cr[k]] * cv[k];
            s += a * a;
        }
        norm2[tc[j]] += s;
    }
}

// the extra rows take part in this system's CGNR operator (column mode only: tile mode forms p
// inside its normal kernel, after the data rows)
inline bool xr_active(const System& S) { return S.xr.on && !S.dist && S.cgh.colmode; }

// t = rs · (b − X x) (or rs · X p), partials to part[0, S.xr.nbk)
void xr_launch_fwd(const System& S, const CgState* st, const double* b, const double* p, double sgn, double* part) {
    const XrData& X = S.xr;
    hipLaunchKernelGGL(k_xr_fwd, dim3(X.nbk), dim3(BLOCK), 0, S.stream, st, X.m_x, X.rows.nslices, X.rows.sp.p,
                       X.rows.ci.p, X.rows.val.p, S.rs.p + X.row0, b ? b + X.row0 : nullptr, p, sgn, X.t.p, part);
}

// q += Xᵀ (rs ∘ t)
void xr_launch_atq(const System& S, const CgState* st, double* q) {
    const XrData& X = S.xr;
    hipLaunchKernelGGL(k_xr_atq, dim3(grid_for(X.ntc)), dim3(BLOCK), 0, S.stream, st, X.ntc, X.tc.p, X.cp.p, X.cr.p,
                       X.cv.p, S.rs.p + X.row0, X.t.p, q);
    if (X.nlong)
        hipLaunchKernelGGL(k_xr_atq_long, dim3((unsigned)((X.nlong + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0,
                           S.stream, st, X.nlong, X.long_col.p, X.tc.p, X.cp.p, X.cr.p, X.cv.p, S.rs.p + X.row0,
                           X.t.p, q);
}

// algorithmic bytes of one step: the rows' entries (12 B) with their p gathers (8 B), rs and t per
// row (16 B), the transpose's entries (12 B row id + value, 16 B rs and t gathers), and per touched
// column its id, pointer and q read and written (28 B)
double xr_step_bytes(const System& S) {
    const XrData& X = S.xr;
    return 20.0 * (double)X.rows.nent + 16.0 * (double)X.m_x + 28.0 * (double)X.nnz + 28.0 * (double)X.ntc;
}
