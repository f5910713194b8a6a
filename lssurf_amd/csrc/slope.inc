// slope.inc — slope biases eliminated with the data biases (lsq_set_data_slope).  Included by
// bias.inc.
//
// Every row i of slope group s carries two further eliminated columns with the coefficients u_i (a
// tilt in x and in y per sensor), constrained by c_s γ_s = 0.  With Z = [B U], M = ZᵀW²Z + C² and the
// rows of every bias ID inside at most one group, M⁻¹ needs one 2 × 2 system per group:
//   per solve  e_j = Σ_{i∈j} w_i² u_i,  F_s = Σ_{i∈s} w_i² u_i u_iᵀ + diag(c_s²),
//              G_s = F_s − Σ_{j∈s} e_j e_jᵀ / D_j = L_s L_sᵀ
//   per step   s_j = Σ_{i∈j} td_i,  h_s = Σ_{i∈s} td_i u_i,  r_s = h_s − Σ_{j∈s} e_j s_j / D_j,
//              γ_s = G_s⁻¹ r_s,  β_j = (s_j − e_j·γ_s(j)) / D_j,
//              td_i −= w_i² (β_j(i) + u_i·γ_s(i)),  pᵀNp −= Σ_j s_j β_j + Σ_s h_s·γ_s
// The sums by ID are the chunk / slot sums of bias.inc with three channels (src, src·u₀, src·u₁:
// k_bias_chunk<3>, k_bias_long<3>); k_slope_rank adds each rank's slots in chunk order, k_slope_group
// adds a group's ranks in rank order (a wave per group, lane l takes the ranks l, l + 64, …, then the
// fixed shuffle tree) and solves.  No atomics, every order fixed: bitwise reproducible.
// Without biases (pseudo) the ranks only carry the sums: e = 0, β = 0, G = F.

// per rank: its channels' slot sums in chunk order into rsum (plane ch = ns doubles); three
// channels below nsr, one above.  mode 1: the ranks outside every group also get β = s / D (0 when
// pseudo) into sD and add −s β to the workgroup's partial.
__global__ __launch_bounds__(BLOCK) void k_slope_rank(const CgState* __restrict__ st, int64_t ns, int32_t nsr,
                                                      const int32_t* __restrict__ seg,
                                                      const int32_t* __restrict__ sbase,
                                                      const double* __restrict__ slots, int64_t nslots,
                                                      const int32_t* __restrict__ long_of,
                                                      const double* __restrict__ lsum, int64_t nlong, int mode,
                                                      int pseudo, const double* __restrict__ D,
                                                      double* __restrict__ rsum, double* __restrict__ sD, double* part) {
    if (st && st->stop) return;
    double acc = 0.0;
    const int64_t nsp = (ns + BLOCK - 1) / BLOCK * BLOCK;
    for (int64_t r0 = (int64_t)blockIdx.x * BLOCK; r0 < nsp; r0 += (int64_t)gridDim.x * BLOCK) {
        const int64_t r = r0 + threadIdx.x;
        if (r >= ns) continue;
        const int nch = r < nsr ? 3 : 1;
        const int32_t lo = long_of[r];
        const int32_t ca = seg[r] / BIAS_CHUNK, cb = (seg[r + 1] - 1) / BIAS_CHUNK;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;   // the three channels side by side: one chain of loads, not three
        if (lo >= 0) {
            s0 = lsum[lo];
            if (nch == 3) {
                s1 = lsum[nlong + lo];
                s2 = lsum[2 * nlong + lo];
            }
        } else {
            for (int32_t c = ca; c <= cb; ++c) {
                const int64_t k = (int64_t)sbase[c] + r;
                s0 += slots[k];
                if (nch == 3) {
                    s1 += slots[nslots + k];
                    s2 += slots[2 * nslots + k];
                }
            }
        }
        rsum[r] = s0;
        if (nch == 3) {
            rsum[ns + r] = s1;
            rsum[2 * ns + r] = s2;
        }
        if (mode == 1 && r >= nsr) {
            const double q = pseudo ? 0.0 : s0 / D[r];
            sD[r] = q;
            acc -= s0 * q;
        }
    }
    if (part) store_partial(acc, part, blockIdx.x);
}

// per solve, after the pass over w²: D_j = Σ w² + c_j² and e_j = Σ w² u (pseudo: D = 1, e = 0)
__global__ __launch_bounds__(BLOCK) void k_slope_de(int64_t ns, int32_t nsr, int pseudo,
                                                    const double* __restrict__ rsum, const double* __restrict__ c2,
                                                    double* __restrict__ D, double* __restrict__ e) {
    for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < ns; r += (int64_t)gridDim.x * BLOCK) {
        D[r] = pseudo ? 1.0 : rsum[r] + c2[r];
        if (r < nsr) {
            e[r] = pseudo ? 0.0 : rsum[ns + r];
            e[ns + r] = pseudo ? 0.0 : rsum[2 * ns + r];
        }
    }
}

// tmp = w² u_k per sorted point (the source of the passes that give F)
__global__ __launch_bounds__(BLOCK) void k_slope_w2u(int64_t npts, const double* __restrict__ w2,
                                                     const double2* __restrict__ u, int k, double* __restrict__ tmp) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < npts; i += (int64_t)gridDim.x * BLOCK) {
        const double2 uu = u[i];
        tmp[i] = w2[i] * (k ? uu.y : uu.x);
    }
}

// a wave per group over the group's ranks [gseg[g], gseg[g + 1]) in rank order.
// mode 0 (after the pass over w² u₀): F₀₀, F₀₁ = Σ_r channels 1, 2.
// mode 1 (after the pass over w² u₁): F₁₁ = Σ_r channel 2, then G = F + diag(c²) − Σ_r e eᵀ / D and
//   its Cholesky factor.
// mode 2 (the step): h = Σ_r channels 1, 2, r = h − Σ_r e s / D, γ = G⁻¹ r; then β_r = (s_r − e_r·γ) / D_r
//   into sD and the workgroup's partial of −(Σ_r s_r β_r + h·γ).
__global__ __launch_bounds__(BLOCK) void k_slope_group(const CgState* __restrict__ st, int64_t ng, int64_t ns,
                                                       const int32_t* __restrict__ gseg, int mode, int pseudo,
                                                       const double* __restrict__ rsum, const double* __restrict__ D,
                                                       const double* __restrict__ e, const double* __restrict__ gc2,
                                                       double* __restrict__ F, double* __restrict__ L,
                                                       double* __restrict__ gam, double* __restrict__ sD, double* part) {
    if (st && st->stop) return;
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (BLOCK / 64);
    double acc = 0.0;
    for (int64_t g = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); g < ng; g += nw) {
        const int32_t ra = gseg[g], rb = gseg[g + 1];
        double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        for (int32_t r = ra + lane; r < rb; r += 64) {
            a0 += rsum[ns + r];
            a1 += rsum[2 * ns + r];
            if (!pseudo && mode == 1) {
                const double e0 = e[r], e1 = e[ns + r], d = D[r];
                b0 += e0 * e0 / d;
                b1 += e0 * e1 / d;
                b2 += e1 * e1 / d;
            }
            if (!pseudo && mode == 2) {
                const double q = rsum[r] / D[r];
                b0 += e[r] * q;
                b1 += e[ns + r] * q;
            }
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        b0 = wave_sum(b0);
        b1 = wave_sum(b1);
        b2 = wave_sum(b2);
        if (mode == 0) {
            if (lane == 0) {
                F[3 * g] = a0;
                F[3 * g + 1] = a1;
            }
        } else if (mode == 1) {
            if (lane == 0) {
                F[3 * g + 2] = a1;
                const double g00 = F[3 * g] + gc2[2 * g] - b0, g01 = F[3 * g + 1] - b1, g11 = a1 + gc2[2 * g + 1] - b2;
                const double l00 = sqrt(g00), l10 = g01 / l00;
                L[3 * g] = l00;
                L[3 * g + 1] = l10;
                L[3 * g + 2] = sqrt(g11 - l10 * l10);
            }
        } else {
            const double l00 = L[3 * g], l10 = L[3 * g + 1], l11 = L[3 * g + 2];
            const double y0 = (a0 - b0) / l00, y1 = ((a1 - b1) - l10 * y0) / l11;
            const double g1 = y1 / l11, g0 = (y0 - l10 * g1) / l00;   // every lane holds the same sums
            if (lane == 0) {
                gam[2 * g] = g0;
                gam[2 * g + 1] = g1;
                acc -= a0 * g0 + a1 * g1;
            }
            for (int32_t r = ra + lane; r < rb; r += 64) {
                const double s = rsum[r];
                const double q = pseudo ? 0.0 : (s - (e[r] * g0 + e[ns + r] * g1)) / D[r];
                sD[r] = q;
                acc -= s * q;
            }
        }
    }
    if (part) store_partial(acc, part, blockIdx.x);
}

// mode 0: td −= w² (β[rank] + u·γ[group]) (the CG step and the cold start); mode 1: td = −w² (…)
// (the warm start's correction of s0).  u and γ are read for the rows of the ranks inside a group.
__global__ __launch_bounds__(BLOCK) void k_slope_apply(const CgState* __restrict__ st, int64_t npts, int32_t nsr,
                                                       const int32_t* __restrict__ rank_pt,
                                                       const int32_t* __restrict__ rgrp, const double* __restrict__ w2,
                                                       const double* __restrict__ sD, const double2* __restrict__ u,
                                                       const double* __restrict__ gam, double* __restrict__ td,
                                                       int mode) {
    if (st && st->stop) return;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < npts; i += (int64_t)gridDim.x * BLOCK) {
        const int32_t r = rank_pt[i];
        double v = sD[r];
        if (r < nsr) {
            const double2 uu = u[i];
            const int32_t g = rgrp[r];
            v += uu.x * gam[2 * g] + uu.y * gam[2 * g + 1];
        }
        const double d = w2[i] * v;
        td[i] = mode ? -d : td[i] - d;
    }
}
