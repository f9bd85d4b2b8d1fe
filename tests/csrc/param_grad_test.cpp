// Host check (fp64) of the material-parameter adjoint of one particle's p2g deposit: constitutive_param_grad and the node sums
// k_param_grad forms (fe_param_grad.h) against central finite differences of the deposit itself,
//   L(mu, lam, mass) = sum over the 27 nodes of  gg.xyz . w (mass v + affine dpos) + gg.w w mass      (mpm:339-353)
// for every material class, including the inviscid liquid at mu = 0 whose forward pass skips the SVD.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <random>
#include "../../fluidlab_amd/csrc/fe_math.h"

static std::mt19937_64 rng(7);
static double rnd(double s) { return std::normal_distribution<double>(0.0, s)(rng); }

struct Case { m3 C, F; real x[3], v[3]; real gg[27][4]; int cls; real dt, dx, scale; };

static real deposit(const Case& c, real mu, real lam, real mass) {
    Constitutive k;
    constitutive_eval(c.C, c.F, c.dt, mu, lam, mass, c.cls, c.scale, k);
    Stencil st; stencil_make(c.x, R_(1.0) / c.dx, st);
    real L = 0;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) for (int kk = 0; kk < 3; kk++) {
        const real w = st.w[i][0] * st.w[j][1] * st.w[kk][2];
        const real dpos[3] = {(i - st.fx[0]) * c.dx, (j - st.fx[1]) * c.dx, (kk - st.fx[2]) * c.dx};
        const real* g = c.gg[(i * 3 + j) * 3 + kk];
        for (int a = 0; a < 3; a++) L += g[a] * w * (mass * c.v[a] + k.affine.a[a][0] * dpos[0] + k.affine.a[a][1] * dpos[1] + k.affine.a[a][2] * dpos[2]);
        L += g[3] * w * mass;
    }
    return L;
}

int main() {
    int failures = 0;
    const int classes[4] = {FE_MAT_LIQUID_, FE_MAT_LIQUID_, FE_MAT_ELASTIC_, FE_MAT_PLASTO_ELASTIC_};
    for (int t = 0; t < 400; t++) {
        Case c; c.cls = classes[t % 4]; c.dt = 2e-4; c.dx = 1.0 / 16; c.scale = -c.dt * (0.5 * c.dx) * (0.5 * c.dx) * 4 / (c.dx * c.dx);
        const real mu = (t % 4 == 0) ? 0.0 : 300.0 + rnd(50), lam = 277.78, mass = 1e-3 * (1 + 0.3 * std::fabs(rnd(1)));
        for (int a = 0; a < 3; a++) { c.x[a] = 0.3 + 0.4 * std::fabs(std::sin(t * 1.7 + a)); c.v[a] = rnd(0.5);
            for (int b = 0; b < 3; b++) { c.C.a[a][b] = rnd(2.0); c.F.a[a][b] = (a == b) + rnd(0.03); } }
        for (auto& g : c.gg) for (real& q : g) q = rnd(1.0);
        // the kernel's sums
        Stencil st; stencil_make(c.x, R_(1.0) / c.dx, st);
        real Gv[3] = {0, 0, 0}, Gm = 0; m3 M = m3_zero(), GA;
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) for (int kk = 0; kk < 3; kk++) {
            const real w = st.w[i][0] * st.w[j][1] * st.w[kk][2]; const real* g = c.gg[(i * 3 + j) * 3 + kk];
            Gm += w * g[3];
            for (int a = 0; a < 3; a++) { Gv[a] += w * g[a]; M.a[a][0] += i * w * g[a]; M.a[a][1] += j * w * g[a]; M.a[a][2] += kk * w * g[a]; }
        }
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) GA.a[a][b] = c.dx * (M.a[a][b] - st.fx[b] * Gv[a]);
        double g_mu, g_lam, g_mass;
        constitutive_param_grad(c.C, c.F, c.dt, c.scale, GA, c.v, Gv, Gm, g_mu, g_lam, g_mass);
        const real hm = 1e-3, hl = 1e-3, hs = 1e-7;         // (L is linear in each of the three: any step gives the derivative)
        const real fd[3] = {(deposit(c, mu + hm, lam, mass) - deposit(c, mu - hm, lam, mass)) / (2 * hm),
                            (deposit(c, mu, lam + hl, mass) - deposit(c, mu, lam - hl, mass)) / (2 * hl),
                            (deposit(c, mu, lam, mass + hs) - deposit(c, mu, lam, mass - hs)) / (2 * hs)};
        const real got[3] = {g_mu, g_lam, g_mass};
        for (int q = 0; q < 3; q++) {
            const real err = std::fabs(got[q] - fd[q]), ref = std::fabs(fd[q]) + 1e-12;
            if (!(err <= 1e-7 * ref + 1e-13)) { failures++; std::printf("case %d cls %d param %d: got %.12e fd %.12e\n", t, c.cls, q, (double)got[q], (double)fd[q]); }
        }
    }
    std::printf("%d failures\n", failures);
    return failures != 0;
}
