// Host build of the nearest-point math shared with the kernels (fluidlab_amd/csrc/fe_nearest.h: fe_nn_point_ok, fe_nn_d2, fe_nn_plan,
// fe_nn_cell_axis, fe_nn_ring_bound, fe_nn_quant and the ring search fe_nn_search that k_nn_query runs).  No checks in here: the program reads
// cases (a mask, an "nn_cells", a set of points, queries) from a file and writes what the functions give; tests/test_chamfer_math.py compares
// that with numpy.  The index is built the way the kernels build it -- count, exclusive scan, fill -- with the members of a cell in reverse
// order of arrival, one of the orders the atomics may leave.
//   nearest_math_test <in> <out>
//   in:  int32 n_cases; per case int32 mask, nn_cells, M, Q; float32 points[M][3]; float32 queries[Q][3]
//   out: per case, all as fp64: lo[3] h[3] h_min n[3]; bound[65] (of a query inside the box: gap2 = 0); ok[M]; cell[M][3]; qok[Q]; qcell[Q][3]; d2[Q][M]; per query nn, best, last ring;
//        quant[Q][3] = fe_nn_quant(query - point 0) on every axis; hi[3]; gap2[Q]; qbound[Q][65] = the bounds of that query
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/fluidengine_ext.h"
#define FE_NEAREST_MATH_ONLY
#include "../../fluidlab_amd/csrc/fe_nearest.h"

template <class T>
static bool rd(std::FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
static void wr(std::FILE* f, const std::vector<double>& v) { if (!v.empty()) std::fwrite(v.data(), sizeof(double), v.size(), f); }

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: nearest_math_test <in> <out>\n"); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::printf("cannot open the files\n"); return 2; }
    int n_cases = 0;
    if (!rd(in, &n_cases, 1)) return 2;
    for (int c = 0; c < n_cases; c++) {
        int head[4];
        if (!rd(in, head, 4)) return 2;
        const int mask = head[0], nn_cells = head[1], M = head[2], Q = head[3];
        std::vector<float> P((size_t)M * 3), X((size_t)Q * 3);
        if (!rd(in, P.data(), P.size()) || !rd(in, X.data(), X.size())) return 2;
        // the box of the members, the grid
        float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
        int count = 0;
        std::vector<int> ok((size_t)M);
        for (int j = 0; j < M; j++) {
            ok[j] = fe_nn_point_ok(&P[3 * (size_t)j], mask) ? 1 : 0;
            if (!ok[j]) continue;
            for (int a = 0; a < 3; a++) {
                const float v = P[3 * (size_t)j + a];
                if (count == 0 || v < lo[a]) lo[a] = v;
                if (count == 0 || v > hi[a]) hi[a] = v;
            }
            count++;
        }
        FeNnGrid g;
        fe_nn_plan(lo, hi, count, mask, nn_cells, g);
        const int cells = fe_nn_cells(g);
        if (cells < 1 || cells > FE_NN_MAX_CELLS) { std::printf("case %d: %d cells\n", c, cells); return 1; }
        // count, scan, fill
        std::vector<int> cnt((size_t)cells, 0), start((size_t)cells + 1, 0);
        for (int j = 0; j < M; j++) if (ok[j]) cnt[fe_nn_cell_of(g, &P[3 * (size_t)j])]++;
        for (int k = 0; k < cells; k++) start[k + 1] = start[k] + cnt[k];
        std::vector<float4> pts((size_t)(count > 0 ? count : 1));
        for (int j = 0; j < M; j++) {
            if (!ok[j]) continue;
            const int k = fe_nn_cell_of(g, &P[3 * (size_t)j]);
            float4 p = {P[3 * (size_t)j], P[3 * (size_t)j + 1], P[3 * (size_t)j + 2], 0.f};
            std::memcpy(&p.w, &j, sizeof(int));
            pts[(size_t)(start[k] + --cnt[k])] = p;
        }
        std::vector<double> o;
        for (int a = 0; a < 3; a++) o.push_back(g.lo[a]);
        for (int a = 0; a < 3; a++) o.push_back(g.h[a]);
        o.push_back(g.h_min);
        for (int a = 0; a < 3; a++) o.push_back((double)g.n[a]);
        for (int r = 0; r <= FE_NN_AXIS_CELLS; r++) o.push_back(fe_nn_ring_bound(g, r, 0.0));
        for (int j = 0; j < M; j++) o.push_back((double)ok[j]);
        for (int j = 0; j < M; j++) for (int a = 0; a < 3; a++) o.push_back((double)fe_nn_cell_axis(g, a, P[3 * (size_t)j + a]));
        for (int i = 0; i < Q; i++) o.push_back(fe_nn_point_ok(&X[3 * (size_t)i], mask) ? 1.0 : 0.0);
        for (int i = 0; i < Q; i++) for (int a = 0; a < 3; a++) o.push_back((double)fe_nn_cell_axis(g, a, X[3 * (size_t)i + a]));
        for (int i = 0; i < Q; i++) for (int j = 0; j < M; j++) o.push_back(fe_nn_d2(&X[3 * (size_t)i], &P[3 * (size_t)j], mask));
        for (int i = 0; i < Q; i++) {
            double best = 0.0; int bid = -1; float4 bp;
            int r = -1;
            if (fe_nn_point_ok(&X[3 * (size_t)i], mask)) r = fe_nn_search(g, start.data(), pts.data(), count, &X[3 * (size_t)i], mask, best, bid, bp);
            if (bid < 0) best = 0.0;
            o.push_back((double)bid); o.push_back(best); o.push_back((double)r);
        }
        for (int i = 0; i < Q; i++)
            for (int a = 0; a < 3; a++) o.push_back(M > 0 ? (double)fe_nn_quant((double)X[3 * (size_t)i + a] - (double)P[a]) : 0.0);
        for (int a = 0; a < 3; a++) o.push_back(g.hi[a]);
        for (int i = 0; i < Q; i++) o.push_back(fe_nn_gap2(g, &X[3 * (size_t)i]));
        for (int i = 0; i < Q; i++) for (int r = 0; r <= FE_NN_AXIS_CELLS; r++) o.push_back(fe_nn_ring_bound(g, r, fe_nn_gap2(g, &X[3 * (size_t)i])));
        wr(out, o);
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("%d cases\n", n_cases);
    return 0;
}
