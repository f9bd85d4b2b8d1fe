// Host check of the observation-field math shared with the kernels (fluidlab_amd/csrc/fe_field_obs.h: fe_fo_v_ok, fe_fo_quant, fe_fo_value,
// fe_fo_grad -- the functions k_field_obs_scatter and k_field_obs_grad run) against the definition written out in plain loops: the velocity
// guard at its edge, the sign handling of the two's-complement momentum word, order independence of the fixed-point field, and the
// per-particle adjoint sum for one and for four channels, against central differences of the plain field too.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>
#include "../../include/fluidengine_ext.h"
#define FE_DENSITY_MATH_ONLY
#include "../../fluidlab_amd/csrc/fe_density.h"
#include "../../fluidlab_amd/csrc/fe_field_obs.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the definition: sum_c G_ch[c] field_ch[c] of one point in plain fp64, no quantisation
static double plain_dot(const FeDensitySpec& sp, const double* x, const double* v, const std::vector<float>& G, long long cells, int channels) {
    long long b[3]; double w[3][3];
    for (int a = 0; a < 3; a++) {
        if (sp.n[a] == 1) { b[a] = 0; w[a][0] = 1.0; w[a][1] = w[a][2] = 0.0; continue; }
        const double u = (x[a] - sp.origin[a]) / sp.cell[a], s = u - 0.5, fb = std::floor(s - 0.5), t = s - fb;
        b[a] = (long long)fb;
        w[a][0] = 0.5 * (1.5 - t) * (1.5 - t); w[a][1] = 0.75 - (t - 1.0) * (t - 1.0); w[a][2] = 0.5 * (t - 0.5) * (t - 0.5);
    }
    double acc = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) {
                const long long ci = b[0] + i, cj = b[1] + j, ck = b[2] + k;
                if (ci < 0 || ci >= sp.n[0] || cj < 0 || cj >= sp.n[1] || ck < 0 || ck >= sp.n[2]) continue;
                const long long c = (ci * sp.n[1] + cj) * sp.n[2] + ck;
                const double wt = w[0][i] * w[1][j] * w[2][k];
                acc += (double)G[c] * wt;
                for (int ch = 1; ch < channels; ch++) acc += (double)G[ch * cells + c] * wt * v[ch - 1];
            }
    return acc;
}

int main() {
    std::mt19937 rng(97531);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    // ---- the velocity guard: non-finite words, |v| = 2^10 kept, the next float above it dropped, on every axis and with either sign
    {
        const float edge = 1024.f, above = std::nextafter(1024.f, inf);
        CHECK(above > edge && above - edge == 1024.f * std::numeric_limits<float>::epsilon(), "the next float above 2^10");
        for (int a = 0; a < 3; a++)
            for (float sgn : {1.f, -1.f}) {
                float v[3] = {0.5f, -0.25f, 3.f};
                CHECK(fe_fo_v_ok(v), "an ordinary velocity passes");
                v[a] = sgn * edge;  CHECK(fe_fo_v_ok(v), "|v_%d| = 2^10 is kept", a);
                v[a] = sgn * above; CHECK(!fe_fo_v_ok(v), "the next float above 2^10 on axis %d is dropped", a);
                v[a] = sgn * inf;   CHECK(!fe_fo_v_ok(v), "inf on axis %d is dropped", a);
                v[a] = nan;         CHECK(!fe_fo_v_ok(v), "nan on axis %d is dropped", a);
                v[a] = sgn * 3.4e38f; CHECK(!fe_fo_v_ok(v), "a huge finite word on axis %d is dropped", a);
            }
        const float z[3] = {0.f, -0.f, 0.f};
        CHECK(fe_fo_v_ok(z), "zeros pass");
    }

    // ---- the momentum word: llrint(w v 2^28) as a signed integer in a two's-complement word
    {
        CHECK(fe_fo_quant(1.0, 1.f) == (1ull << 28) && fe_fo_value(1ull << 28) == 1.0, "w v = 1 is 2^28");
        CHECK(fe_fo_quant(1.0, -1.f) == ~(1ull << 28) + 1ull && fe_fo_value(~(1ull << 28) + 1ull) == -1.0, "w v = -1 is the two's complement of 2^28");
        CHECK(fe_fo_quant(0.5, -3.f) + fe_fo_quant(0.5, 3.f) == 0ull, "opposite deposits cancel to the zero word");
        CHECK(fe_fo_quant(0.25, 0.f) == 0ull && fe_fo_quant(0.25, -0.f) == 0ull, "zero velocity deposits the zero word");
        CHECK(fe_fo_value(fe_fo_quant(1.0, 1024.f)) == 1024.0 && fe_fo_value(fe_fo_quant(1.0, -1024.f)) == -1024.0, "the edge of the guard is exact");
        // 2^23 deposits of the largest magnitude stay inside the signed word: 2^23 2^10 2^28 = 2^61
        unsigned long long acc = 0ull;
        const unsigned long long big = fe_fo_quant(1.0, -1024.f);
        for (int i = 0; i < (1 << 23); i++) acc += big;
        CHECK(fe_fo_value(acc) == -1024.0 * 8388608.0, "2^23 deposits of -2^10: %.17g", fe_fo_value(acc));
        // tie to even, both signs (llrint in the default rounding mode)
        CHECK(fe_fo_quant(1.0, 1.5f / 268435456.f) == 2ull && fe_fo_quant(1.0, 2.5f / 268435456.f) == 2ull, "ties to even");
        CHECK((long long)fe_fo_quant(1.0, -1.5f / 268435456.f) == -2ll && (long long)fe_fo_quant(1.0, -2.5f / 268435456.f) == -2ll, "ties to even, negative");
        std::uniform_real_distribution<double> W(0.0, 1.0);
        for (int i = 0; i < 20000; i++) {
            const double w = W(rng); const float v = (U(rng) - 0.5f) * 80.f;
            const long long q = (long long)fe_fo_quant(w, v);
            CHECK(std::fabs((double)q - w * (double)v * 268435456.0) <= 0.5, "llrint quantisation");
            CHECK(std::fabs(fe_fo_value((unsigned long long)q) - w * (double)v) <= 1.0 / 536870912.0, "a deposit is within 2^-29 of exact");
            CHECK((q < 0) == (w * (double)v * 268435456.0 < -0.5) || q == 0, "the sign of the word is the sign of the deposit");
        }
    }

    // ---- fields in either order of accumulation, and the per-particle adjoint sum
    const FeDensitySpec specs[] = {{{0.2, 0.0, 0.3}, {0.05, 1.0, 0.04}, {8, 1, 8}, 0},            // projected on y
                                   {{0.25, 0.2, 0.3}, {0.06, 0.09, 0.08}, {6, 5, 4}, 0}};          // non-cubic, partly outside
    for (const FeDensitySpec& sp : specs)
        for (int channels : {1, 4}) {
            const long long cells = fe_dn_cells(sp);
            std::vector<float> G((size_t)(channels * cells));
            for (float& g : G) g = U(rng) - 0.5f;
            const int n_pts = 2000;
            std::vector<float> pts(3 * n_pts), vel(3 * n_pts);
            for (int q = 0; q < 3 * n_pts; q++) { pts[q] = U(rng); vel[q] = (U(rng) - 0.5f) * 20.f; }
            std::vector<unsigned long long> fwd((size_t)(channels * cells), 0ull), rev((size_t)(channels * cells), 0ull);
            std::vector<double> plain((size_t)(channels * cells), 0.0);
            std::vector<long long> count((size_t)cells, 0);
            for (int pass = 0; pass < 2; pass++)
                for (int q = 0; q < n_pts; q++) {
                    const int p = pass == 0 ? q : n_pts - 1 - q;
                    const float *x = &pts[3 * p], *v = &vel[3 * p];
                    FeDensityStencil st;
                    CHECK(fe_dn_stencil(sp, x, st) && fe_fo_v_ok(v), "a finite point passes both guards");
                    for (int i = 0; i < 3; i++)
                        for (int j = 0; j < 3; j++)
                            for (int k = 0; k < 3; k++) {
                                if (!fe_dn_in(sp, 0, st.base[0] + i) || !fe_dn_in(sp, 1, st.base[1] + j) || !fe_dn_in(sp, 2, st.base[2] + k)) continue;
                                const long long c = fe_dn_index(sp, st.base[0] + i, st.base[1] + j, st.base[2] + k);
                                const double w = fe_dn_weight(st, i, j, k);
                                std::vector<unsigned long long>& dst = pass == 0 ? fwd : rev;
                                dst[(size_t)c] += fe_dn_quant(w);
                                for (int b = 0; b < channels - 1; b++) dst[(size_t)((1 + b) * cells + c)] += fe_fo_quant(w, v[b]);
                                if (pass == 0) {
                                    plain[(size_t)c] += w; count[(size_t)c]++;
                                    for (int b = 0; b < channels - 1; b++) plain[(size_t)((1 + b) * cells + c)] += w * (double)v[b];
                                }
                            }
                    if (pass == 1) continue;
                    // the adjoint sum against the plain loops
                    double gx[3], gv[3], wx[3] = {0, 0, 0}, wv[3] = {0, 0, 0}, scale = 0.0;
                    fe_fo_grad(sp, st, G.data(), cells, channels, v, gx, gv);
                    for (int i = 0; i < 3; i++)
                        for (int j = 0; j < 3; j++)
                            for (int k = 0; k < 3; k++) {
                                if (!fe_dn_in(sp, 0, st.base[0] + i) || !fe_dn_in(sp, 1, st.base[1] + j) || !fe_dn_in(sp, 2, st.base[2] + k)) continue;
                                const long long c = fe_dn_index(sp, st.base[0] + i, st.base[1] + j, st.base[2] + k);
                                double coef = (double)G[(size_t)c];
                                for (int b = 0; b < channels - 1; b++) {
                                    coef += (double)G[(size_t)((1 + b) * cells + c)] * (double)v[b];
                                    wv[b] += (double)G[(size_t)((1 + b) * cells + c)] * st.w[0][i] * st.w[1][j] * st.w[2][k];
                                }
                                const double d[3] = {st.dw[0][i] * st.w[1][j] * st.w[2][k], st.w[0][i] * st.dw[1][j] * st.w[2][k], st.w[0][i] * st.w[1][j] * st.dw[2][k]};
                                for (int a = 0; a < 3; a++) { wx[a] += coef * d[a]; scale += std::fabs(coef * d[a]); }
                            }
                    for (int a = 0; a < 3; a++) {
                        CHECK(std::fabs(gx[a] - wx[a]) <= 1e-14 * (scale + 1.0), "adjoint sum, x axis %d: %.17g vs %.17g", a, gx[a], wx[a]);
                        CHECK(std::fabs(gv[a] - wv[a]) <= 1e-14, "adjoint sum, v axis %d: %.17g vs %.17g", a, gv[a], wv[a]);
                        if (channels == 1) CHECK(gv[a] == 0.0, "one channel: no velocity adjoint");
                        if (sp.n[a] == 1) CHECK(gx[a] == 0.0, "no gradient along a projected axis");
                    }
                    // ... and against central differences of the plain field, away from the stencil switches
                    if (q < 200) {
                        const double h = 1e-6;
                        bool smooth = true;
                        for (int a = 0; a < 3; a++) {
                            if (sp.n[a] == 1) continue;
                            const double u = ((double)x[a] - sp.origin[a]) / sp.cell[a], fr = u - std::floor(u);
                            if (std::fabs(fr) < 4 * h / sp.cell[a] || std::fabs(fr - 1.0) < 4 * h / sp.cell[a]) smooth = false;
                        }
                        if (smooth)
                            for (int a = 0; a < 3; a++) {
                                double xp[3] = {x[0], x[1], x[2]}, xm[3] = {x[0], x[1], x[2]}, vd[3] = {v[0], v[1], v[2]};
                                xp[a] += h; xm[a] -= h;
                                const double fd = (plain_dot(sp, xp, vd, G, cells, channels) - plain_dot(sp, xm, vd, G, cells, channels)) / (2 * h);
                                CHECK(std::fabs(fd - gx[a]) <= 1e-6 * (scale + 1.0), "x adjoint against central differences, axis %d: %.12g vs %.12g", a, gx[a], fd);
                                if (channels == 4) {
                                    double x0[3] = {x[0], x[1], x[2]}, vp[3] = {v[0], v[1], v[2]}, vm[3] = {v[0], v[1], v[2]};
                                    vp[a] += 1.0; vm[a] -= 1.0;                   // (linear in v: any step)
                                    const double fv = (plain_dot(sp, x0, vp, G, cells, channels) - plain_dot(sp, x0, vm, G, cells, channels)) / 2.0;
                                    CHECK(std::fabs(fv - gv[a]) <= 1e-12, "v adjoint against differences, axis %d: %.12g vs %.12g", a, gv[a], fv);
                                }
                            }
                    }
                }
            CHECK(fwd == rev, "the field does not depend on the order of accumulation");
            long long hit = 0;
            for (long long c = 0; c < channels * cells; c++) {
                const double val = c < cells ? fe_dn_value(fwd[(size_t)c]) : fe_fo_value(fwd[(size_t)c]);
                const double bound = (double)count[(size_t)(c % cells)] / 536870912.0 + 1e-12;
                CHECK(std::fabs(val - plain[(size_t)c]) <= bound, "word %lld decodes to %.17g, plain %.17g (k_c %lld)", c, val, plain[(size_t)c], count[(size_t)(c % cells)]);
                hit += count[(size_t)(c % cells)] > 0;
            }
            CHECK(hit > 0, "the points reach the field");
        }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
