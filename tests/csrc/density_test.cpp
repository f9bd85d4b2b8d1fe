// Host check of the density math shared with the kernels (fluidlab_amd/csrc/fe_density.h: fe_dn_stencil, fe_dn_weight, fe_dn_dweight, fe_dn_quant,
// fe_dn_value, fe_dn_index, fe_dn_grad -- the functions k_density_scatter, k_density_resid and k_task_bwd run) against the definition written out
// in plain loops: weights and derivatives, the dropped cells, the non-finite guard, the llrint quantisation and the index order on a non-cubic
// field.  Weights are compared to 4 ulp of 1 (the two sides may associate the products differently); the fixed-point field of the plain loops
// must be EQUAL word for word whatever the order of accumulation.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>
#include "../../include/fluidengine_ext.h"
#define FE_DENSITY_MATH_ONLY
#include "../../fluidlab_amd/csrc/fe_density.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the definition, one axis: cells b, b + 1, b + 2 with their weights and derivatives
static void plain_axis(double x, double origin, double cell, int n, long long& b, double* w, double* dw) {
    if (n == 1) { b = 0; w[0] = 1.0; w[1] = w[2] = 0.0; dw[0] = dw[1] = dw[2] = 0.0; return; }
    const double u = (x - origin) / cell, s = u - 0.5;
    const double fb = std::floor(s - 0.5), t = s - fb;
    b = (long long)fb;
    w[0] = 0.5 * (1.5 - t) * (1.5 - t); w[1] = 0.75 - (t - 1.0) * (t - 1.0); w[2] = 0.5 * (t - 0.5) * (t - 0.5);
    dw[0] = -(1.5 - t) / cell; dw[1] = -2.0 * (t - 1.0) / cell; dw[2] = (t - 0.5) / cell;
}

int main() {
    std::mt19937 rng(4321);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    const double EPS = 4.0 * std::numeric_limits<double>::epsilon();
    CHECK(sizeof(FeDensitySpec) == 64, "sizeof(FeDensitySpec) = %zu", sizeof(FeDensitySpec));

    const FeDensitySpec specs[] = {{{0.2, 0.0, 0.3}, {0.05, 1.0, 0.04}, {8, 1, 8}, 0},            // projected on y
                                   {{0.25, 0.2, 0.3}, {0.06, 0.09, 0.08}, {6, 5, 4}, 0},           // non-cubic: a transposed index cannot pass
                                   {{0.0, 0.0, 0.0}, {1.0 / 16, 1.0 / 16, 1.0 / 16}, {16, 16, 16}, 0}};
    for (const FeDensitySpec& sp : specs) {
        const long long cells = fe_dn_cells(sp);
        CHECK(cells == (long long)sp.n[0] * sp.n[1] * sp.n[2], "cells");
        CHECK(fe_dn_index(sp, sp.n[0] - 1, sp.n[1] - 1, sp.n[2] - 1) == cells - 1 && fe_dn_index(sp, 0, 0, 1) == 1 && fe_dn_index(sp, 0, 1, 0) == sp.n[2] &&
              fe_dn_index(sp, 1, 0, 0) == (long long)sp.n[1] * sp.n[2], "index order (i n1 + j) n2 + k");
        std::vector<unsigned long long> fwd(cells, 0ull), rev(cells, 0ull), plain(cells, 0ull);
        std::vector<double> r(cells);
        for (double& v : r) v = (double)U(rng) - 0.5;
        const int n_pts = 3000;
        std::vector<float> pts(3 * n_pts);
        for (int p = 0; p < n_pts; p++)
            for (int a = 0; a < 3; a++) {
                pts[3 * p + a] = U(rng);
                if (&sp == &specs[2]) pts[3 * p + a] = (float)((int)(U(rng) * 64.f) / 64.0);      // dyadic: on the stencil switch points too
            }
        long long dropped = 0, kept = 0;
        for (int pass = 0; pass < 2; pass++)
            for (int q = 0; q < n_pts; q++) {
                const int p = pass == 0 ? q : n_pts - 1 - q;
                const float* x = &pts[3 * p];
                FeDensityStencil st;
                CHECK(fe_dn_stencil(sp, x, st), "a finite point has a stencil");
                long long b[3]; double w[3][3], dw[3][3];
                for (int a = 0; a < 3; a++) plain_axis((double)x[a], sp.origin[a], sp.cell[a], sp.n[a], b[a], w[a], dw[a]);
                double g[3] = {0, 0, 0}, gw[3];
                fe_dn_grad(sp, st, r.data(), gw);
                for (int a = 0; a < 3; a++) {
                    CHECK(st.base[a] == b[a], "base of axis %d: %d, want %lld", a, st.base[a], b[a]);
                    double sum = 0.0, dsum = 0.0;
                    for (int i = 0; i < 3; i++) {
                        CHECK(std::fabs(st.w[a][i] - w[a][i]) <= EPS && std::fabs(st.dw[a][i] - dw[a][i]) <= EPS / sp.cell[a], "weight / derivative of axis %d cell %d", a, i);
                        CHECK(st.w[a][i] >= 0.0 && st.w[a][i] <= 0.75 + (sp.n[a] == 1 ? 0.25 : 0.0), "weight range");
                        sum += st.w[a][i]; dsum += st.dw[a][i];
                    }
                    CHECK(std::fabs(sum - 1.0) <= EPS && std::fabs(dsum) <= EPS / sp.cell[a], "partition of unity on axis %d: %.17g, %.3g", a, sum, dsum);
                }
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++)
                        for (int k = 0; k < 3; k++) {
                            const long long ci = b[0] + i, cj = b[1] + j, ck = b[2] + k;
                            const bool in = ci >= 0 && ci < sp.n[0] && cj >= 0 && cj < sp.n[1] && ck >= 0 && ck < sp.n[2];
                            CHECK(in == (fe_dn_in(sp, 0, st.base[0] + i) && fe_dn_in(sp, 1, st.base[1] + j) && fe_dn_in(sp, 2, st.base[2] + k)), "the dropped cells");
                            if (!in) { if (pass == 0 && w[0][i] * w[1][j] * w[2][k] > 0) dropped++; continue; }
                            const double wt = w[0][i] * w[1][j] * w[2][k];
                            const long long c = (ci * sp.n[1] + cj) * sp.n[2] + ck;
                            CHECK(fe_dn_index(sp, (int)ci, (int)cj, (int)ck) == c, "index");
                            CHECK(std::fabs(fe_dn_weight(st, i, j, k) - wt) <= EPS, "weight product");
                            const unsigned long long qd = fe_dn_quant(fe_dn_weight(st, i, j, k));
                            CHECK(std::fabs((double)qd - fe_dn_weight(st, i, j, k) * 1099511627776.0) <= 0.5, "llrint quantisation");
                            if (&sp == &specs[2]) CHECK((double)qd == wt * 1099511627776.0, "a dyadic weight is exact times 2^40");
                            (pass == 0 ? fwd : rev)[c] += qd;
                            if (pass == 0) { plain[c] += (unsigned long long)std::llrint(wt * 1099511627776.0); kept++; }
                            const double d[3] = {dw[0][i] * w[1][j] * w[2][k], w[0][i] * dw[1][j] * w[2][k], w[0][i] * w[1][j] * dw[2][k]};
                            for (int a = 0; a < 3; a++) {
                                CHECK(std::fabs(fe_dn_dweight(st, i, j, k, a) - d[a]) <= EPS / sp.cell[a], "derivative of the product, axis %d", a);
                                g[a] += 2.0 * r[c] * d[a];
                            }
                        }
                for (int a = 0; a < 3; a++) CHECK(std::fabs(gw[a] - g[a]) <= 27 * EPS / sp.cell[a], "gather axis %d: %.17g vs %.17g", a, gw[a], g[a]);
                if (sp.n[1] == 1) CHECK(gw[1] == 0.0, "no gradient along a projected axis");
            }
        CHECK(fwd == rev, "the field does not depend on the order of accumulation");
        if (&sp == &specs[2]) CHECK(fwd == plain, "dyadic positions: the same words as the plain loops");
        long long diff = 0;
        for (long long c = 0; c < cells; c++) diff += fwd[c] > plain[c] ? fwd[c] - plain[c] : plain[c] - fwd[c];
        CHECK(diff <= kept, "fixed-point fields agree to one unit per deposit (%lld over %lld deposits)", diff, kept);
        CHECK(kept > 0 && (dropped > 0 || &sp == &specs[2]), "kept %lld and dropped %lld deposits both occur", kept, dropped);
        CHECK(fe_dn_value(1ull << 40) == 1.0 && fe_dn_value(3ull << 39) == 1.5, "word to value");
    }

    // ---- the guard: non-finite words and |u| > 2^30 deposit nothing; a projected axis takes any finite coordinate
    {
        const FeDensitySpec& sp = specs[0];
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        FeDensityStencil st;
        const float bad[][3] = {{nan, 0.5f, 0.5f}, {0.5f, nan, 0.5f}, {0.5f, 0.5f, inf}, {-inf, 0.5f, 0.5f}, {1e9f, 0.5f, 0.5f}, {0.5f, 0.5f, -1e9f}, {3.4e38f, 0.5f, 0.5f}};
        for (const auto& x : bad) CHECK(!fe_dn_stencil(sp, x, st), "guard (%g, %g, %g)", x[0], x[1], x[2]);
        const float far_y[3] = {0.4f, 1e30f, 0.5f};
        CHECK(fe_dn_stencil(sp, far_y, st) && st.base[1] == 0 && st.w[1][0] == 1.0 && st.dw[1][0] == 0.0, "a projected axis ignores the coordinate");
        const float edge[3] = {(float)(0.2 + 0.05 * 1073741000.0), 0.5f, 0.5f};          // |u| just below 2^30: a stencil far outside the field, every cell dropped
        CHECK(fe_dn_stencil(sp, edge, st) && !fe_dn_in(sp, 0, st.base[0]) && !fe_dn_in(sp, 0, st.base[0] + 2), "a far finite point keeps an integer base");
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
