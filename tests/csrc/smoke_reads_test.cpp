// Host check of the smoke reads' shared math (fluidlab_amd/csrc/fe_smoke_reads.h: fe_sl_value, fe_sl_grad, fe_ss_cell, fe_ss_merge_lane,
// fe_ss_merge_lanes, fe_ss_finish -- the same functions the kernels run) against plain fp64 loops.
//   loss     L1 and SQ value and gradient of planted detectors, d == 0 and a NaN / inf q included
//   summary  a slab of random cells with a NaN planted in v of one cell and an inf in q of another, for q_dim 1 and 3: counts and extremes
//            exact, sums within (n - 1) 2^-53 sum |terms|
//   merge    the cells split into 1, 63, 64, 65 and 1,000 partial records, merged in the fixed order of k_smoke_summary_merge, against the
//            sequential sum within (n - 1) 2^-53 sum |terms| (n = the number of cells: every grouping of them is an fp64 summation)
//   empty    no cell at all, and a slab whose cells are all non-finite: zeros apart from the two counts
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>
#include "../../include/fluidengine_ext.h"
#define FE_SUMMARY_MATH_ONLY
#include "../../fluidlab_amd/csrc/fe_summary.h"
#define FE_TASK_LOSS_MATH_ONLY
#include "../../fluidlab_amd/csrc/fe_task_loss.h"
#define FE_SMOKE_READS_MATH_ONLY
#include "../../fluidlab_amd/csrc/fe_smoke_reads.h"

static int failures = 0;
static void exact(const char* what, int a, int b, double got, double want) {
    if (!(got == want)) { failures++; std::printf("[%d, %d] %s = %.17g, expected exactly %.17g\n", a, b, what, got, want); }
}
static void within(const char* what, int a, int b, double got, double want, double bound) {
    if (!(std::fabs(got - want) <= bound)) { failures++; std::printf("[%d, %d] %s = %.17g, expected %.17g (bound %.3g)\n", a, b, what, got, want, bound); }
}
static void expect(const char* what, bool ok) {
    if (!ok) { failures++; std::printf("%s\n", what); }
}

static void test_loss() {
    const float q[6] = {0.25f, 0.7f, -1.5f, 0.1f, 3.0f, 0.5f};
    const double t[6] = {1.0, 0.7f /* exactly the fp32 word: d == 0 */, 0.0, 0.1 /* not the fp32 word */, 2.0, 0.5};
    const double w[6] = {1.0, 2.0, -0.5, 3.0, 0.125, -7.0};
    const double scale = 0.37;
    for (int i = 0; i < 6; i++) {
        const double d = (double)q[i] - t[i];
        exact("L1 value", i, 0, fe_sl_value(FE_SMOKE_L1, q[i], t[i], w[i]), w[i] * std::fabs(d));
        exact("SQ value", i, 0, fe_sl_value(FE_SMOKE_SQ, q[i], t[i], w[i]), w[i] * (d * d));
        bool add = false;
        const double sg = d > 0 ? 1.0 : (d < 0 ? -1.0 : 0.0);
        exact("L1 grad", i, 0, fe_sl_grad(FE_SMOKE_L1, q[i], t[i], w[i], scale, add), (float)(scale * w[i] * sg));
        expect("L1 grad of a finite q is added", add);
        exact("SQ grad", i, 0, fe_sl_grad(FE_SMOKE_SQ, q[i], t[i], w[i], scale, add), (float)(scale * w[i] * (2.0 * d)));
        expect("SQ grad of a finite q is added", add);
    }
    bool add = true;
    exact("L1 grad at d == 0", 1, 0, fe_sl_grad(FE_SMOKE_L1, q[1], t[1], w[1], scale, add), 0.0);
    exact("L1 grad at d == 0, sign", 5, 0, fe_sl_grad(FE_SMOKE_L1, q[5], t[5], w[5], scale, add), 0.0);
    const float bad[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    for (int i = 0; i < 3; i++)
        for (int kind = 0; kind < 2; kind++) {
            expect("the value at a non-finite q is non-finite", !std::isfinite(fe_sl_value(kind, bad[i], 0.5, 2.0)));
            add = true;
            const float g = fe_sl_grad(kind, bad[i], 0.5, 2.0, scale, add);
            expect("a non-finite q adds no gradient", !add && g == 0.f);
        }
}

struct Cell { float v[3], q[3]; };
struct Ref { long long n = 0, bad = 0; double v_max = 0, kin = 0, a_kin = 0, q_sum[3] = {0, 0, 0}, a_q[3] = {0, 0, 0}, q_min[3] = {0, 0, 0}, q_max[3] = {0, 0, 0}; bool any = false; };

static Ref reference(const std::vector<Cell>& cs, int qd) {
    Ref r;
    for (const Cell& c : cs) {
        r.n++;
        bool ok = std::isfinite(c.v[0]) && std::isfinite(c.v[1]) && std::isfinite(c.v[2]);
        for (int d = 0; d < qd; d++) ok = ok && std::isfinite(c.q[d]);
        if (!ok) { r.bad++; continue; }
        if (!r.any) { for (int d = 0; d < qd; d++) r.q_min[d] = r.q_max[d] = c.q[d]; r.any = true; }
        double vv = 0;
        for (int d = 0; d < 3; d++) { const double v = c.v[d]; vv += v * v; r.v_max = std::fmax(r.v_max, std::fabs(v)); }
        r.kin += 0.5 * vv; r.a_kin += 0.5 * vv;
        for (int d = 0; d < qd; d++) { const double q = c.q[d]; r.q_sum[d] += q; r.a_q[d] += std::fabs(q); r.q_min[d] = std::fmin(r.q_min[d], q); r.q_max[d] = std::fmax(r.q_max[d], q); }
    }
    return r;
}
// the cells dealt out to `parts` records round-robin-by-block (as a grid-stride pass would), then the kernel's fixed-order merge
static FeSmokeSummary summarise(const std::vector<Cell>& cs, int qd, int parts, double dt) {
    std::vector<FeSmokeAcc> partial((size_t)parts);
    for (auto& p : partial) fe_ss_clear(p);
    for (size_t i = 0; i < cs.size(); i++) fe_ss_cell(partial[(i / 7) % (size_t)parts], cs[i].v, cs[i].q, qd);
    FeSmokeAcc lanes[FE_SS_LANES], a;
    for (int l = 0; l < FE_SS_LANES; l++) fe_ss_merge_lane(partial.data(), parts, l, lanes[l]);
    fe_ss_merge_lanes(lanes, a);
    FeSmokeSummary o;
    fe_ss_finish(a, dt, qd, o);
    return o;
}
static void check(const std::vector<Cell>& cs, int qd, int parts) {
    const double dt = 0.03f, u = std::ldexp(1.0, -53);
    const Ref r = reference(cs, qd);
    const FeSmokeSummary o = summarise(cs, qd, parts, dt);
    const double nm1 = (double)(cs.size() > 0 ? cs.size() - 1 : 0);
    exact("n_cells", qd, parts, (double)o.n_cells, (double)r.n);
    exact("n_nonfinite", qd, parts, (double)o.n_nonfinite, (double)r.bad);
    exact("v_max", qd, parts, o.v_max, r.v_max);
    exact("courant", qd, parts, o.courant, dt * r.v_max);
    within("kinetic", qd, parts, o.kinetic, r.kin, nm1 * u * r.a_kin);      // (a cell's term 1/2 ((v0^2 + v1^2) + v2^2) is formed the same way on both sides)
    for (int d = 0; d < 3; d++) {
        if (d < qd) {
            within("q_sum", qd, parts, o.q_sum[d], r.q_sum[d], nm1 * u * r.a_q[d]);
            exact("q_min", qd, parts, o.q_min[d], r.q_min[d]);
            exact("q_max", qd, parts, o.q_max[d], r.q_max[d]);
        } else {
            exact("q_sum beyond q_dim", qd, parts, o.q_sum[d], 0.0);
            exact("q_min beyond q_dim", qd, parts, o.q_min[d], 0.0);
            exact("q_max beyond q_dim", qd, parts, o.q_max[d], 0.0);
        }
    }
}

// n partial records with sums of mixed sign, merged in the kernel's fixed order, against their sequential sum: within (n - 1) 2^-53 sum |terms|;
// counts and extremes exact
static void test_merge(int n) {
    std::mt19937 rng(77 + n);
    std::uniform_real_distribution<double> us(-1e3, 1e3);
    std::vector<FeSmokeAcc> part((size_t)n);
    long long cells = 0, bad = 0;
    double kin = 0, a_kin = 0, qs[3] = {0, 0, 0}, a_qs[3] = {0, 0, 0}, v_max = 0, lo = 1e300, hi = -1e300;
    for (int i = 0; i < n; i++) {
        FeSmokeAcc& p = part[(size_t)i];
        fe_ss_clear(p);
        p.n_cells = 256 + i; p.n_nonfinite = i % 3;
        p.kin = std::fabs(us(rng)); p.v_max = std::fabs(us(rng));
        for (int d = 0; d < 3; d++) { p.q_sum[d] = us(rng); p.q_min[d] = us(rng); p.q_max[d] = p.q_min[d] + 1.0; }
        cells += p.n_cells; bad += p.n_nonfinite;
        kin += p.kin; a_kin += std::fabs(p.kin);
        for (int d = 0; d < 3; d++) { qs[d] += p.q_sum[d]; a_qs[d] += std::fabs(p.q_sum[d]); }
        v_max = std::fmax(v_max, p.v_max); lo = std::fmin(lo, p.q_min[1]); hi = std::fmax(hi, p.q_max[1]);
    }
    FeSmokeAcc lanes[FE_SS_LANES], a;
    for (int l = 0; l < FE_SS_LANES; l++) fe_ss_merge_lane(part.data(), n, l, lanes[l]);
    fe_ss_merge_lanes(lanes, a);
    const double u = std::ldexp(1.0, -53);
    exact("merge n_cells", n, 0, (double)a.n_cells, (double)cells);
    exact("merge n_nonfinite", n, 0, (double)a.n_nonfinite, (double)bad);
    exact("merge v_max", n, 0, a.v_max, v_max);
    exact("merge q_min", n, 0, a.q_min[1], lo);
    exact("merge q_max", n, 0, a.q_max[1], hi);
    within("merge kin", n, 0, a.kin, kin, (n - 1) * u * a_kin);
    for (int d = 0; d < 3; d++) within("merge q_sum", n, d, a.q_sum[d], qs[d], (n - 1) * u * a_qs[d]);
}

int main() {
    test_loss();
    for (int n : {1, 63, 64, 65, 1000}) test_merge(n);
    std::mt19937 rng(20240607);
    std::uniform_real_distribution<float> uv(-3.f, 3.f), uq(-0.5f, 1.5f);
    std::vector<Cell> cs(7200);
    for (auto& c : cs) { for (int d = 0; d < 3; d++) { c.v[d] = uv(rng); c.q[d] = uq(rng); } }
    cs[0].v[1] = -7.5f;                                       // the maximum of |v|, negative, in the first cell
    cs.back().q[0] = -2.25f;                                  // the minimum of q in the last
    cs[100].v[2] = std::numeric_limits<float>::quiet_NaN();
    cs[4000].q[0] = std::numeric_limits<float>::infinity();
    cs[4001].q[2] = -std::numeric_limits<float>::infinity();  // (counts only when q_dim is 3)
    const int parts[5] = {1, 63, 64, 65, 1000};
    for (int qd = 1; qd <= 3; qd += 2)
        for (int p = 0; p < 5; p++) check(cs, qd, parts[p]);
    // a finite-only run so that the sums of every partial count have all 7,200 terms
    std::vector<Cell> fin(cs);
    fin[100].v[2] = 1.f; fin[4000].q[0] = 0.5f; fin[4001].q[2] = 0.5f;
    for (int p = 0; p < 5; p++) check(fin, 3, parts[p]);
    // empty slab; all cells non-finite
    for (int p = 0; p < 2; p++) check(std::vector<Cell>(), 1, parts[p]);
    std::vector<Cell> allbad(130);
    for (auto& c : allbad) { for (int d = 0; d < 3; d++) { c.v[d] = std::numeric_limits<float>::quiet_NaN(); c.q[d] = 1.f; } }
    for (int p = 0; p < 3; p++) check(allbad, 1, parts[p]);
    {
        const FeSmokeSummary o = summarise(allbad, 1, 64, 0.03);
        exact("all non-finite: n_cells", 1, 64, (double)o.n_cells, 130.0);
        exact("all non-finite: n_nonfinite", 1, 64, (double)o.n_nonfinite, 130.0);
        exact("all non-finite: v_max", 1, 64, o.v_max, 0.0);
        exact("all non-finite: kinetic", 1, 64, o.kinetic, 0.0);
        exact("all non-finite: q_min", 1, 64, o.q_min[0], 0.0);
        exact("all non-finite: q_max", 1, 64, o.q_max[0], 0.0);
        const FeSmokeSummary e = summarise(std::vector<Cell>(), 3, 1, 0.03);
        exact("empty: n_cells", 3, 1, (double)e.n_cells, 0.0);
        exact("empty: q_min", 3, 1, e.q_min[1], 0.0);
        exact("empty: courant", 3, 1, e.courant, 0.0);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
