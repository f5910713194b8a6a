// Stand-alone host program around csrc/xr_lump.hpp (no HIP): reads formed extra rows, runs the
// classification and the level-1 transpose builder, writes the tables.  Built by
// tools/xr_lump_check.py, with -fsanitize=address,undefined when asked.
//
// in : int64 {S0, S1, nt, has_z, colz, cold, S0c, S1c, long_rows, m_x, nnz}, int64 rp[m_x + 1],
//      int64 ci[nnz], double val[nnz]
// out: int64 {ok, nrows, nnodes, nent, nlong}, double tau[4 m_x], int32 node[nnodes],
//      int64 ptr[nnodes + 1], int32 row[nent], double w[nent], int32 long_node[nlong]; !ok: the reason
#include <cstdio>
#include <cstdlib>

#include "../lssurf_amd/csrc/xr_lump.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
}
template <class T>
static void wr(FILE* f, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "short write\n");
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: xr_lump_check IN OUT\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[11];
    rd(f, h, 11);
    lsq::XrLumpGeom G;
    G.S0 = (int32_t)h[0], G.S1 = (int32_t)h[1], G.nt = (int32_t)h[2], G.has_z = (int32_t)h[3];
    G.colz = h[4], G.cold = h[5];
    G.S0c = (int32_t)h[6], G.S1c = (int32_t)h[7];
    const int64_t m_x = h[9], nnz = h[10];
    std::vector<int64_t> rp((size_t)m_x + 1), ci((size_t)nnz);
    std::vector<double> val((size_t)nnz);
    rd(f, rp.data(), rp.size());
    rd(f, ci.data(), ci.size());
    rd(f, val.data(), val.size());
    fclose(f);
    const lsq::XrLumpHost L = lsq::xr_lump_build(G, m_x, rp.data(), ci.data(), val.data(), (int)h[8]);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const int64_t ne = L.ok ? L.ptr.back() : 0;
    const int64_t head[5] = {L.ok ? 1 : 0, L.nrows, (int64_t)L.node.size(), ne, (int64_t)L.long_node.size()};
    wr(o, head, 5);
    if (L.ok) {
        wr(o, L.tau.data(), (size_t)(4 * m_x));
        wr(o, L.node.data(), L.node.size());
        wr(o, L.ptr.data(), L.ptr.size());
        wr(o, L.row.data(), (size_t)ne);
        wr(o, L.w.data(), (size_t)ne);
        wr(o, L.long_node.data(), L.long_node.size());
    } else {
        wr(o, L.why.data(), L.why.size());
    }
    fclose(o);
    return 0;
}
