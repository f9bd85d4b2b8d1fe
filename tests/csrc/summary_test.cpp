// Host check of the frame summary's shared math (fluidlab_amd/csrc/fe_summary.h: fe_sum_particle, fe_sum_merge, fe_sum_finish -- the same
// functions k_frame_summary runs) against a plain fp64 loop: ~1,000 random particles in 5 groups, one of them empty, some in no group (-1),
// some unused, a handful with NaN or +-inf in one word of x, v, C or F.  Counts and extremes must agree exactly, sums to 1e-12 x sum |terms|
// (the fp64 reordering bound for 1,000 terms is ~1e-13).  The data is also split into 1, 7 and 64 partial records and merged.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>
#include "../../include/fluidengine_ext.h"
#define FE_SUMMARY_MATH_ONLY
#include "../../fluidlab_amd/csrc/fe_summary.h"

struct P { float m, x[3], v[3], C[9], F[9]; int used, group; };
static const int NG = 5, EMPTY = 3;

struct Ref {                                                  // the plain loop: fp64 sums in particle order, and the sums of |terms| for the bounds
    long long n_used = 0, n_bad = 0;
    double mass = 0, mx[3] = {0, 0, 0}, mom[3] = {0, 0, 0}, kin = 0, v_max = 0, lo[3], hi[3], J_min = 0, J_max = 0;
    double a_mass = 0, a_mx[3] = {0, 0, 0}, a_mom[3] = {0, 0, 0}, a_kin = 0;
    bool any = false;
};

static Ref reference(const std::vector<P>& ps, int g) {       // g == NG: every used particle
    Ref r;
    for (const P& p : ps) {
        if (!p.used || (g != NG && p.group != g)) continue;
        r.n_used++;
        bool ok = true;
        for (int d = 0; d < 3; d++) ok = ok && std::isfinite(p.x[d]) && std::isfinite(p.v[d]);
        for (int d = 0; d < 9; d++) ok = ok && std::isfinite(p.C[d]) && std::isfinite(p.F[d]);
        if (!ok) { r.n_bad++; continue; }
        const double m = p.m;
        double F[9]; for (int d = 0; d < 9; d++) F[d] = p.F[d];
        const double J = F[0] * (F[4] * F[8] - F[5] * F[7]) - F[1] * (F[3] * F[8] - F[5] * F[6]) + F[2] * (F[3] * F[7] - F[4] * F[6]);
        if (!r.any) { for (int d = 0; d < 3; d++) r.lo[d] = r.hi[d] = p.x[d]; r.J_min = r.J_max = J; r.any = true; }
        r.mass += m; r.a_mass += std::fabs(m);
        double vv = 0;
        for (int d = 0; d < 3; d++) {
            const double x = p.x[d], v = p.v[d];
            r.mx[d] += m * x; r.a_mx[d] += std::fabs(m * x);
            r.mom[d] += m * v; r.a_mom[d] += std::fabs(m * v);
            vv += v * v;
            r.v_max = std::fmax(r.v_max, std::fabs(v));
            r.lo[d] = std::fmin(r.lo[d], x); r.hi[d] = std::fmax(r.hi[d], x);
        }
        r.kin += 0.5 * m * vv; r.a_kin += 0.5 * m * vv;
        r.J_min = std::fmin(r.J_min, J); r.J_max = std::fmax(r.J_max, J);
    }
    if (!r.any) for (int d = 0; d < 3; d++) r.lo[d] = r.hi[d] = 0;
    return r;
}

static int failures = 0;
static void exact(const char* what, int g, int parts, double got, double want) {
    if (!(got == want)) { failures++; std::printf("group %d, %d partials: %s = %.17g, expected exactly %.17g\n", g, parts, what, got, want); }
}
static void close_to(const char* what, int g, int parts, double got, double want, double sum_abs) {
    if (!(std::fabs(got - want) <= 1e-12 * sum_abs)) { failures++; std::printf("group %d, %d partials: %s = %.17g, expected %.17g (bound %.3g)\n", g, parts, what, got, want, 1e-12 * sum_abs); }
}

int main() {
    std::mt19937_64 rng(11);
    std::normal_distribution<double> nrm(0.0, 1.0);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    const int N = 1003;
    std::vector<P> ps(N);
    for (int i = 0; i < N; i++) {
        P& p = ps[i];
        p.m = (float)(1e-4 * (0.5 + uni(rng)));
        for (int d = 0; d < 3; d++) { p.x[d] = (float)(0.1 + 0.8 * uni(rng)); p.v[d] = (float)(2.0 * nrm(rng)); }
        for (int d = 0; d < 9; d++) { p.C[d] = (float)(5.0 * nrm(rng)); p.F[d] = (float)((d % 4 == 0 ? 1.0 : 0.0) + 0.2 * nrm(rng)); }
        p.used = (i % 11 == 5) ? 0 : 1;
        p.group = (i % 13 == 0) ? -1 : (int)(rng() % NG);
        if (p.group == EMPTY) p.group = 4;                    // group 3 stays empty
        if (!p.used) { p.x[0] = p.x[1] = p.x[2] = -100.f; }   // (a parked particle: must not reach the bounding box)
    }
    const float bad[3] = {NAN, INFINITY, -INFINITY};
    int nb = 0;
    for (int i = 7; i < N && nb < 12; i += 61) {             // one bad word each, in turn in x, v, C, F, in used particles
        P& p = ps[i];
        if (!p.used) continue;
        float* field = nb % 4 == 0 ? p.x : nb % 4 == 1 ? p.v : nb % 4 == 2 ? p.C : p.F;
        field[(nb * 5) % (nb % 4 < 2 ? 3 : 9)] = bad[nb % 3];
        nb++;
    }
    const double dt = 2e-4, dx = 1.0 / 64;
    const int splits[3] = {1, 7, 64};
    for (int parts : splits) {
        // partial k holds the particles i with i % parts == k, per group and for the whole frame; then the partials are merged in order
        std::vector<FeSumAcc> acc((size_t)parts * (NG + 1));
        for (FeSumAcc& a : acc) fe_sum_clear(a);
        for (int i = 0; i < N; i++) {
            const P& p = ps[i];
            if (!p.used) continue;
            FeSumAcc* mine = &acc[(size_t)(i % parts) * (NG + 1)];
            if (p.group >= 0) fe_sum_particle(mine[p.group], p.m, p.x, p.v, p.C, p.F);
            fe_sum_particle(mine[NG], p.m, p.x, p.v, p.C, p.F);
        }
        for (int g = 0; g <= NG; g++) {
            FeSumAcc tot;
            fe_sum_clear(tot);
            for (int k = 0; k < parts; k++) fe_sum_merge(tot, acc[(size_t)k * (NG + 1) + g]);
            FeFrameSummary s;
            fe_sum_finish(tot, dt, dx, s);
            const Ref r = reference(ps, g);
            exact("n_used", g, parts, (double)s.n_used, (double)r.n_used);
            exact("n_nonfinite", g, parts, (double)s.n_nonfinite, (double)r.n_bad);
            exact("v_max", g, parts, s.v_max, r.v_max);
            exact("courant", g, parts, s.courant, dt * r.v_max / dx);
            exact("J_min", g, parts, s.J_min, r.J_min);
            exact("J_max", g, parts, s.J_max, r.J_max);
            close_to("mass", g, parts, s.mass, r.mass, r.a_mass);
            close_to("kinetic", g, parts, s.kinetic, r.kin, r.a_kin);
            for (int d = 0; d < 3; d++) {
                exact("lo", g, parts, s.lo[d], r.lo[d]);
                exact("hi", g, parts, s.hi[d], r.hi[d]);
                close_to("com * mass", g, parts, s.com[d] * s.mass, r.mx[d], r.a_mx[d]);
                close_to("momentum", g, parts, s.momentum[d], r.mom[d], r.a_mom[d]);
            }
            if (g == EMPTY && (s.n_used != 0 || s.mass != 0.0 || s.kinetic != 0.0 || s.lo[0] != 0.0 || s.hi[2] != 0.0 || s.J_min != 0.0 || s.J_max != 0.0 || s.com[1] != 0.0)) {
                failures++; std::printf("the empty group's record is not all zeros (%d partials)\n", parts);
            }
        }
    }
    {   // a group whose particles are all non-finite: zeros apart from the counts
        FeSumAcc a; fe_sum_clear(a);
        P p = ps[1]; p.v[1] = NAN;
        fe_sum_particle(a, p.m, p.x, p.v, p.C, p.F);
        FeFrameSummary s; fe_sum_finish(a, dt, dx, s);
        if (s.n_used != 1 || s.n_nonfinite != 1 || s.mass != 0.0 || s.lo[0] != 0.0 || s.hi[0] != 0.0 || s.J_min != 0.0 || s.J_max != 0.0 || s.v_max != 0.0 || s.courant != 0.0) {
            failures++; std::printf("an all-non-finite group is not zeros apart from its counts\n");
        }
    }
    if (reference(ps, NG).n_bad != 12 || reference(ps, EMPTY).n_used != 0) { failures++; std::printf("the test data is not what it is meant to be\n"); }
    std::printf("%d failures\n", failures);
    return failures != 0;
}
