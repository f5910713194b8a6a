// xr_lump.hpp — host side of the multigrid's lumped extra rows (mg.inc, k_mg_lump_xr): the
// classification of the formed extra rows and the transpose over the touched level-1 nodes.
// Plain C++ (no HIP): the tables are built on the host once per formation and level-0 geometry.
//
// A formed row (merged, zero-free, removed columns dropped) has entries x[n, s] at node n of the
// (y, x) lattice and slot s (z0, or a dz epoch).  Per row
//   τ_s = Σ_n x[n, s]              ω_n = Σ_s |x[n, s]| / Σ_{n,s} |x[n, s]|
// (a separable row x = w ⊗ τ with w ≥ 0, Σ w = 1 gives back w and τ), and the row is lumpable when
// its dz slots are at most two adjacent epochs (t, t + 1): what a node's arrow + tridiagonal block
// of 3·nt doubles can hold.  Level-1 weights w¹_m = Σ_n P[n, m] ω_n with the hierarchy's bilinear
// prolongation P (coarse node a on fine node 2a).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace lsq {

struct XrLumpGeom {   // level 0's column layout (MgGeom) and the level-1 lattice
    int32_t S0 = 0, S1 = 0, nt = 0, has_z = 0;
    int64_t colz = 0, cold = 0;
    int32_t S0c = 0, S1c = 0;
    bool operator==(const XrLumpGeom& o) const {
        return S0 == o.S0 && S1 == o.S1 && nt == o.nt && has_z == o.has_z && colz == o.colz && cold == o.cold &&
               S0c == o.S0c && S1c == o.S1c;
    }
};

struct XrLumpHost {
    bool ok = false;
    std::string why;                // !ok: the first row that is not lumpable
    int64_t nrows = 0;              // rows that kept an entry (the others contribute nothing)
    std::vector<double> tau;        // 4 per row: τ_z, τ_t, τ_{t+1}, t
    std::vector<int32_t> node;      // touched level-1 nodes, ascending
    std::vector<int64_t> ptr;       // node.size() + 1
    std::vector<int32_t> row;       // per entry: the local row (ascending inside a node) …
    std::vector<double> w;          // … and its w¹
    std::vector<int32_t> long_node; // positions in node of the nodes over `long_rows` rows
};

// rp / ci / val: the formed rows (full column ids, every column inside the level-0 lattice)
inline XrLumpHost xr_lump_build(const XrLumpGeom& G, int64_t m_x, const int64_t* rp, const int64_t* ci,
                                const double* val, int long_rows) {
    XrLumpHost L;
    const int64_t nodes = (int64_t)G.S0 * G.S1;
    L.tau.assign((size_t)std::max<int64_t>(4 * m_x, 4), 0.0);
    std::vector<std::pair<int64_t, double>> fine, coarse;   // a row's (node, weight) lists
    std::vector<int64_t> cnt((size_t)((int64_t)G.S0c * G.S1c) + 1, 0);
    std::vector<int32_t> erow, enode;   // entries in row order
    std::vector<double> ew;
    for (int64_t r = 0; r < m_x; ++r) {
        if (rp[r + 1] == rp[r]) continue;
        ++L.nrows;
        fine.clear();
        double tz = 0.0, tt[16] = {0.0}, tot = 0.0;
        int tlo = 1 << 30, thi = -1;
        for (int64_t e = rp[r]; e < rp[r + 1]; ++e) {
            const int64_t c = ci[e];
            int64_t n;
            int t = -1;
            if (G.has_z && c >= G.colz && c < G.colz + nodes) {
                n = c - G.colz;
                tz += val[e];
            } else if (G.nt > 0 && c >= G.cold && c < G.cold + nodes * G.nt) {
                n = (c - G.cold) / G.nt;
                t = (int)((c - G.cold) - n * G.nt);
                tt[t] += val[e];
                tlo = std::min(tlo, t);
                thi = std::max(thi, t);
            } else {
                L.why = "extra row " + std::to_string(r) + " has a column outside the z0 / dz grids";
                return L;
            }
            const double a = std::fabs(val[e]);
            tot += a;
            size_t k = 0;
            while (k < fine.size() && fine[k].first != n) ++k;
            if (k == fine.size()) fine.emplace_back(n, a);
            else fine[k].second += a;
        }
        if (thi - tlo > 1) {
            L.why = "extra row " + std::to_string(r) + " spans dz epochs " + std::to_string(tlo) + " to " +
                    std::to_string(thi) + ": a node block holds two adjacent epochs per row";
            return L;
        }
        // the pair (t, t + 1) inside [0, nt): a single epoch at nt − 1 takes the upper place
        int t0 = thi < 0 ? 0 : tlo;
        if (thi >= 0 && tlo == thi && t0 == G.nt - 1 && G.nt > 1) --t0;
        double* T = &L.tau[(size_t)(4 * r)];
        T[0] = tz;
        T[1] = thi >= 0 ? tt[t0] : 0.0;
        T[2] = (thi >= 0 && t0 + 1 < G.nt) ? tt[t0 + 1] : 0.0;
        T[3] = (double)t0;
        // w¹ over the ≤ 2 × 2 parents of every fine node, merged per row
        coarse.clear();
        for (const auto& f : fine) {
            const int fy = (int)(f.first / G.S1), fx = (int)(f.first - (int64_t)fy * G.S1);
            const int ay[2] = {fy >> 1, (fy + 1) >> 1}, ax[2] = {fx >> 1, (fx + 1) >> 1};
            const int ny = (fy & 1) ? 2 : 1, nx = (fx & 1) ? 2 : 1;
            for (int i = 0; i < ny; ++i)
                for (int j = 0; j < nx; ++j) {
                    const int64_t m = (int64_t)ay[i] * G.S1c + ax[j];
                    const double wv = (f.second / tot) * ((ny == 2 ? 0.5 : 1.0) * (nx == 2 ? 0.5 : 1.0));
                    size_t k = 0;
                    while (k < coarse.size() && coarse[k].first != m) ++k;
                    if (k == coarse.size()) coarse.emplace_back(m, wv);
                    else coarse[k].second += wv;
                }
        }
        for (const auto& c : coarse) {
            erow.push_back((int32_t)r);
            enode.push_back((int32_t)c.first);
            ew.push_back(c.second);
            ++cnt[(size_t)c.first + 1];
        }
    }
    // the transpose: rows ascend inside a node since the entries are walked in row order
    const int64_t nc = (int64_t)G.S0c * G.S1c, ne = (int64_t)erow.size();
    std::vector<int64_t> where((size_t)nc, -1);
    L.ptr.push_back(0);
    for (int64_t m = 0; m < nc; ++m)
        if (cnt[(size_t)m + 1]) {
            where[(size_t)m] = (int64_t)L.node.size();
            L.node.push_back((int32_t)m);
            L.ptr.push_back(L.ptr.back() + cnt[(size_t)m + 1]);
        }
    L.row.assign((size_t)std::max<int64_t>(ne, 1), 0);
    L.w.assign((size_t)std::max<int64_t>(ne, 1), 0.0);
    std::vector<int64_t> fill(L.ptr.begin(), L.ptr.end() - 1);
    for (int64_t e = 0; e < ne; ++e) {
        const int64_t k = fill[(size_t)where[(size_t)enode[(size_t)e]]]++;
        L.row[(size_t)k] = erow[(size_t)e];
        L.w[(size_t)k] = ew[(size_t)e];
    }
    for (size_t j = 0; j < L.node.size(); ++j)
        if (L.ptr[j + 1] - L.ptr[j] > long_rows) L.long_node.push_back((int32_t)j);
    L.ok = true;
    return L;
}

}  // namespace lsq
