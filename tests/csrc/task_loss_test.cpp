// Host check of the task-loss math shared with the kernels (fluidlab_amd/csrc/fe_task_loss.h: fe_tl_selected, fe_tl_sep_value, fe_tl_sep_grad,
// fe_tl_pair, fe_tl_pair_grad, fe_tl_merge -- the functions k_task_sep_fwd, k_task_pair, k_task_bwd and k_task_merge run) against plain fp64
// loops.  Values that are sums of the same fp64 terms in the same order must be EQUAL; the merge, which re-orders, must agree with the plain
// sum to 1e-13 x sum |terms| on random data (a few thousand terms of fp64 rounding 1.1e-16 each) and exactly on dyadic data.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>
#include "../../include/fluidengine_ext.h"
#define FE_TASK_LOSS_MATH_ONLY
#include "../../fluidlab_amd/csrc/fe_task_loss.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main() {
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> U(0.f, 1.f);

    // ---- the selection test, against its definition written out
    {
        const FeLossSel sels[] = {{0, 10, -1, 0}, {3, 7, -1, 0}, {0, 10, 2, 0}, {0, 10, -1, 1}, {2, 9, 5, 1}, {4, 4, -1, 0}};
        for (const FeLossSel& s : sels)
            for (int pid = -1; pid <= 10; pid++)
                for (int mat = 0; mat < 7; mat++)
                    for (int used = 0; used < 2; used++) {
                        const bool want = pid >= s.pid_lo && pid < s.pid_hi && (s.mat == -1 || mat == s.mat) && (s.require_used == 0 || used != 0);
                        CHECK(fe_tl_selected(s, pid, mat, used) == want, "selected pid %d mat %d used %d", pid, mat, used);
                    }
    }

    // ---- value and gradient of each separable kind, every axis mask
    {
        const int kinds[3] = {FE_TERM_L1_CONST, FE_TERM_SQ_CONST, FE_TERM_L1_REF};
        for (int k = 0; k < 3; k++)
            for (int mask = 1; mask < 8; mask++)
                for (int rep = 0; rep < 200; rep++) {
                    FeLossTerm t{};
                    t.kind = kinds[k]; t.axis_mask = mask; t.weight = -0.37 + rep * 0.01;
                    for (int a = 0; a < 3; a++) t.c[a] = (double)U(rng);
                    float x[3], ref[3];
                    for (int a = 0; a < 3; a++) { x[a] = U(rng); ref[a] = U(rng); }
                    if (rep % 5 == 0) { ref[1] = x[1]; t.c[1] = (double)x[1]; }        // a tie: |d|' = 0
                    double want = 0.0, wg[3] = {0, 0, 0};
                    for (int a = 0; a < 3; a++) {
                        if (!((mask >> a) & 1)) continue;
                        const double d = (double)x[a] - (t.kind == FE_TERM_L1_REF ? (double)ref[a] : t.c[a]);
                        if (t.kind == FE_TERM_SQ_CONST) { want += d * d; wg[a] = 2.0 * d * t.weight; }
                        else { want += std::fabs(d); wg[a] = (d > 0 ? 1.0 : d < 0 ? -1.0 : 0.0) * t.weight; }
                    }
                    CHECK(fe_tl_sep_value(t, x, ref) == want, "sep value kind %d mask %d", t.kind, mask);
                    for (int a = 0; a < 3; a++) CHECK(fe_tl_sep_grad(t, x, ref, a) == wg[a], "sep grad kind %d mask %d axis %d", t.kind, mask, a);
                    CHECK(fe_tl_separable(t.kind), "separable");
                }
        CHECK(!fe_tl_separable(FE_TERM_PAIR_L1), "pair is not separable");
    }

    // ---- the pair contribution: points on multiples of 1/64 (many ties), self pairs with i == j included
    {
        const int n = 97;
        std::vector<float> p(n);
        std::uniform_int_distribution<int> Q(0, 63);
        for (float& v : p) v = Q(rng) / 64.f;
        double total = 0.0, want_total = 0.0;
        long long ties = 0;
        for (int i = 0; i < n; i++) {
            int cnt = 0, want_cnt = 0;
            for (int j = 0; j < n; j++) {
                double ad; int sg;
                fe_tl_pair(p[i], p[j], ad, sg);
                total += ad; cnt += sg;
                want_total += std::fabs((double)p[i] - (double)p[j]);
                want_cnt += (p[j] < p[i]) - (p[j] > p[i]);
                if (p[i] == p[j]) { ties++; CHECK(ad == 0.0 && sg == 0, "a tie contributes nothing"); }
            }
            CHECK(cnt == want_cnt, "pair count of point %d: %d, want %d", i, cnt, want_cnt);
            FeLossTerm self{}; self.kind = FE_TERM_PAIR_L1; self.b.pid_lo = -1; self.weight = -7e-5;
            FeLossTerm two = self; two.b.pid_lo = 0;
            CHECK(fe_tl_pair_grad(self, cnt) == -7e-5 * (2.0 * cnt), "self-pair gradient");
            CHECK(fe_tl_pair_grad(two, cnt) == -7e-5 * (double)cnt, "two-set gradient");
        }
        CHECK(total == want_total, "pair total %.17g, want %.17g", total, want_total);
        CHECK(ties > n, "the data has ties beside i == j (%lld)", ties);
    }

    // ---- the fixed-order merge of partials
    {
        const int sizes[] = {0, 1, 63, 64, 65, 1000, 4097};
        for (int n : sizes) {
            std::vector<double> r(n), q(n);
            double sum = 0.0, asum = 0.0, qsum = 0.0;
            std::uniform_int_distribution<int> Q(-4096, 4096);
            for (int i = 0; i < n; i++) { r[i] = (double)U(rng) - 0.5; sum += r[i]; asum += std::fabs(r[i]); q[i] = Q(rng) / 64.0; qsum += q[i]; }
            const double m = fe_tl_merge(r.data(), n);
            CHECK(std::fabs(m - sum) <= 1e-13 * asum, "merge of %d: %.17g vs %.17g", n, m, sum);
            CHECK(fe_tl_merge(r.data(), n) == m, "merge repeats bit for bit");
            CHECK(fe_tl_merge(q.data(), n) == qsum, "merge of %d dyadic partials is exact", n);
            double lanes = 0.0;                                // the lane sums cover every partial once
            for (int l = 0; l < FE_TL_LANES; l++) lanes += fe_tl_lane_sum(q.data(), n, l);
            CHECK(lanes == qsum, "lane sums of %d", n);
        }
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
