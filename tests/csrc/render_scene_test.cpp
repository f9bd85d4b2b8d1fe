// Host check of the scene math shared with the kernels (fluidlab_amd/csrc/fe_render_scene.h: fe_rs_ray, fe_rs_sample, fe_rs_march, fe_rs_shade,
// fe_rs_cell_* -- the functions k_render_sdf, k_render_smoke and k_render_shade_scene run) against the definitions of
// include/fluidengine_ext.h written out in plain loops over a 33 x 21 image: the ray and its map into voxels, the trilinear sample, the clipped
// fixed-step march with its bisection (every sample taken, no early stop), the early stop's promise, the shading, the cells.
// Built twice by tests/test_render_scene_math.py: plain, and with -fsanitize=address,undefined (the voxel reads are heap reads here).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "../../include/fluidengine_ext.h"
#define FE_RENDER_MATH_ONLY
#include "../../fluidlab_amd/csrc/fe_render.h"
#include "../../fluidlab_amd/csrc/fe_render_scene.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; if (failures < 40) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const int W = 33, H = 21;

static FeRenderCamera make_cam(const double* pos, const double* at, double fov_deg) {
    FeRenderCamera c;
    std::memset(&c, 0, sizeof(c));
    double f[3] = {at[0] - pos[0], at[1] - pos[1], at[2] - pos[2]};
    const double n = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (double& v : f) v /= n;
    const double up[3] = {0, 1, 0};
    double r[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    const double rn = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (double& v : r) v /= rn;
    const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
    for (int a = 0; a < 3; a++) { c.pos[a] = pos[a]; c.right[a] = r[a]; c.up[a] = u[a]; c.fwd[a] = f[a]; }
    c.focal = 0.5 * H / std::tan(fov_deg * M_PI / 360.0);
    c.near = 0.01; c.max_radius_px = 32.0; c.width = W; c.height = H;
    return c;
}
static FeRenderLights make_lights() {
    FeRenderLights L;
    std::memset(&L, 0, sizeof(L));
    for (int a = 0; a < 3; a++) { L.ambient[a] = 0.1; L.background[a] = 1.0; L.color[0][a] = L.color[1][a] = 0.5; }
    L.pos[0][0] = 0.5; L.pos[0][1] = 1.5; L.pos[0][2] = 0.5;
    L.pos[1][0] = 0.5; L.pos[1][1] = 1.5; L.pos[1][2] = 1.5;
    L.n_lights = 2;
    return L;
}

// A volume over a heap block of exactly res^3 floats: voxel (a, b, c) sits at mesh point (lo + a h_x, lo + b h_y, lo + c h_z).
struct Vol {
    std::vector<float> vox; FeRenderVol V; double lo[3], h[3];
};
template <class F> static void make_vol(Vol& v, int res, const double* lo, const double* hi, F sdf) {
    v.vox.resize((size_t)res * res * res);
    std::memset(&v.V, 0, sizeof(v.V));
    for (int a = 0; a < 3; a++) { v.lo[a] = lo[a]; v.h[a] = (hi[a] - lo[a]) / (res - 1); }
    for (int a = 0; a < res; a++) for (int b = 0; b < res; b++) for (int c = 0; c < res; c++)
        v.vox[((size_t)a * res + b) * res + c] = (float)sdf(lo[0] + a * v.h[0], lo[1] + b * v.h[1], lo[2] + c * v.h[2]);
    v.V.res = res; v.V.vox = v.vox.data();
    for (int a = 0; a < 3; a++) {
        v.V.T[a * 4 + a] = (float)(1.0 / v.h[a]); v.V.T[a * 4 + 3] = (float)(-lo[a] / v.h[a]);
        v.V.Rinv[a * 3 + a] = (float)v.h[a];
    }
    v.V.q[0] = 1.f; v.V.rgba = 0xff2060c0u;
}

// ---- the definitions, plainly
static void plain_qrot(const double* v, const double* q, double* o) {       // v + 2 q_w (q_v x v) + 2 q_v x (q_v x v), with geom.py's signs
    const double u[3] = {q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]};
    const double w[3] = {q[2] * u[2] - q[3] * u[1], q[3] * u[0] - q[1] * u[2], q[1] * u[1] - q[2] * u[0]};
    for (int a = 0; a < 3; a++) o[a] = v[a] + 2.0 * (q[0] * u[a] + w[a]);
}
static void plain_dir(const FeRenderCamera& c, int i, int j, double* d) {
    for (int a = 0; a < 3; a++) d[a] = c.fwd[a] + ((i + 0.5 - W / 2.0) / c.focal) * c.right[a] - ((j + 0.5 - H / 2.0) / c.focal) * c.up[a];
}
static void plain_to_voxels(const FeRenderVol& V, const double* P, double* pv) {    // a WORLD point into voxels: inverse pose, then T
    double m[3] = {P[0], P[1], P[2]};
    if (V.posed) {
        const double qn = std::sqrt((double)V.q[0] * V.q[0] + (double)V.q[1] * V.q[1] + (double)V.q[2] * V.q[2] + (double)V.q[3] * V.q[3]);
        const double qi[4] = {V.q[0] / qn, -V.q[1] / qn, -V.q[2] / qn, -V.q[3] / qn};
        const double rel[3] = {P[0] - V.p[0], P[1] - V.p[1], P[2] - V.p[2]};
        plain_qrot(rel, qi, m);
    }
    for (int a = 0; a < 3; a++) pv[a] = V.T[a * 4] * m[0] + V.T[a * 4 + 1] * m[1] + V.T[a * 4 + 2] * m[2] + V.T[a * 4 + 3];
}
static double plain_sample(const FeRenderVol& V, const double* pv) {
    int b[3];
    for (int a = 0; a < 3; a++) { b[a] = (int)std::floor(pv[a]); if (b[a] < 0 || b[a] >= V.res - 1) return 1.0; }
    double sd = 0.0;
    for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) for (int k = 0; k < 2; k++) {
        const double f[3] = {pv[0] - b[0], pv[1] - b[1], pv[2] - b[2]};
        const double w = (i ? f[0] : 1.0 - f[0]) * (j ? f[1] : 1.0 - f[1]) * (k ? f[2] : 1.0 - f[2]);
        sd += w * V.vox[((size_t)(b[0] + i) * V.res + (b[1] + j)) * V.res + (b[2] + k)];
    }
    return sd;
}
// the march of the contract with every sample taken; k_hit = -1: no hit
static bool plain_march(const FeRenderCamera& c, const FeRenderVol& V, const FeRenderRay& r, double step, int iters, float& depth, int& k_hit, double& dt_out) {
    const double top = V.res - 1;
    double t0 = c.near, t1 = std::numeric_limits<double>::infinity();
    k_hit = -1;
    for (int a = 0; a < 3; a++) {
        if (r.dv[a] == 0.0) { if (r.ov[a] < 0.0 || r.ov[a] > top) return false; continue; }
        const double ta = (0.0 - r.ov[a]) / r.dv[a], tb = (top - r.ov[a]) / r.dv[a];
        t0 = std::fmax(t0, std::fmin(ta, tb)); t1 = std::fmin(t1, std::fmax(ta, tb));
    }
    if (!(t0 <= t1)) return false;
    const double dt = step / std::sqrt(r.dv[0] * r.dv[0] + r.dv[1] * r.dv[1] + r.dv[2] * r.dv[2]);
    dt_out = dt;
    auto sd_at = [&](double t) { const double pv[3] = {r.ov[0] + t * r.dv[0], r.ov[1] + t * r.dv[1], r.ov[2] + t * r.dv[2]}; return plain_sample(V, pv); };
    for (int k = 0; t0 + k * dt <= t1 && k <= FE_RENDER_MAX_MARCH; k++) {
        if (!(sd_at(t0 + k * dt) <= 0.0)) continue;
        double lo = t0 + (k - 1) * dt, hi = t0 + k * dt;
        if (k > 0) for (int it = 0; it < iters; it++) { const double mid = 0.5 * (lo + hi); if (sd_at(mid) <= 0.0) hi = mid; else lo = mid; }
        depth = (float)hi; k_hit = k;
        return true;
    }
    return false;
}

static void check_volume(const char* name, const FeRenderCamera& cam, const FeRenderLights& L, const Vol& vol, double step, int iters, bool analytic_sphere, const double* centre, double radius,
                         int* n_hit_out) {
    std::mt19937 rng(7);
    const FeRenderVol& V = vol.V;
    int n_hit = 0, n_k0 = 0;
    for (int j = 0; j < H; j++) for (int i = 0; i < W; i++) {
        FeRenderRay r;
        fe_rs_ray(cam, V, i, j, r);
        double d[3];
        plain_dir(cam, i, j, d);
        for (int a = 0; a < 3; a++) CHECK(std::fabs(r.d[a] - d[a]) <= 1e-14, "%s: d[%d] at (%d, %d)", name, a, i, j);
        for (double t : {0.0, 0.37, 2.5}) {                  // the voxel position is linear in t and is the map of the world point
            const double P[3] = {cam.pos[0] + t * d[0], cam.pos[1] + t * d[1], cam.pos[2] + t * d[2]};
            double pv[3];
            plain_to_voxels(V, P, pv);
            for (int a = 0; a < 3; a++) CHECK(std::fabs((r.ov[a] + t * r.dv[a]) - pv[a]) <= 1e-9 * (1.0 + std::fabs(pv[a])), "%s: pv[%d](%g) at (%d, %d): %.17g vs %.17g", name, a, t, i, j, r.ov[a] + t * r.dv[a], pv[a]);
            CHECK(std::fabs(fe_rs_sample(V, pv[0], pv[1], pv[2]) - plain_sample(V, pv)) <= 1e-12, "%s: sample at (%d, %d)", name, i, j);
        }
        float dep = -1.f, dep_p = -1.f;
        int k_hit; double dt = 0.0;
        const bool hit = fe_rs_march(cam, V, r, step, iters, std::numeric_limits<float>::infinity(), dep);
        const bool hit_p = plain_march(cam, V, r, step, iters, dep_p, k_hit, dt);
        CHECK(hit == hit_p, "%s: hit %d vs %d at (%d, %d)", name, (int)hit, (int)hit_p, i, j);
        if (!(hit && hit_p)) continue;
        n_hit++; n_k0 += k_hit == 0;
        CHECK(fe_rd_float_bits(dep) == fe_rd_float_bits(dep_p), "%s: depth %.9g vs %.9g at (%d, %d)", name, dep, dep_p, i, j);
        CHECK(dep >= (float)cam.near, "%s: a hit in front of near", name);
        // the early stop: a limit at or behind the hit gives the same hit, one in front of it gives nothing or something behind the limit
        const float stops[3] = {dep, std::nextafter(dep, 0.f), dep * std::uniform_real_distribution<float>(0.3f, 1.7f)(rng)};
        for (float stop : stops) {
            float d2 = -1.f;
            const bool h2 = fe_rs_march(cam, V, r, step, iters, stop, d2);
            if (dep <= stop) CHECK(h2 && fe_rd_float_bits(d2) == fe_rd_float_bits(dep), "%s: a stop behind the hit changed it at (%d, %d)", name, i, j);
            else CHECK(!h2 || d2 > stop, "%s: a stop in front of the hit produced a nearer one", name);
        }
        // the hit is not outside the solid (where the solid ends inside the box: on a face of the box the fp32 depth may round out of it)
        if (analytic_sphere) CHECK(fe_rs_sample_t(V, r, (double)dep_p) <= 1e-6, "%s: sd at the hit %g", name, fe_rs_sample_t(V, r, (double)dep_p));
        if (analytic_sphere && k_hit > 0) {                  // within one voxel length along the ray of the analytic root
            const double oc[3] = {cam.pos[0] - centre[0], cam.pos[1] - centre[1], cam.pos[2] - centre[2]};
            const double A = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], B = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2], C = oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2] - radius * radius;
            const double disc = B * B - A * C;
            if (disc > 0.0) CHECK(std::fabs((double)dep - (-B - std::sqrt(disc)) / A) <= 2.0 * dt, "%s: depth %g, analytic %g, one voxel along the ray %g at (%d, %d)", name, dep, (-B - std::sqrt(disc)) / A, 2.0 * dt, i, j);
        }
        // the shading: the plain formula on the same hit point
        unsigned char out[3];
        fe_rs_shade(cam, L, V, r, dep, out);
        const double t = (double)dep;
        const double P[3] = {cam.pos[0] + t * d[0], cam.pos[1] + t * d[1], cam.pos[2] + t * d[2]};
        double pv[3], g[3], nm[3], n[3];
        plain_to_voxels(V, P, pv);
        for (int a = 0; a < 3; a++) {
            double inc[3] = {pv[0], pv[1], pv[2]}, dec[3] = {pv[0], pv[1], pv[2]};
            inc[a] += 1e-2; dec[a] -= 1e-2;
            g[a] = (plain_sample(V, inc) - plain_sample(V, dec)) / 2e-2;
        }
        for (int a = 0; a < 3; a++) nm[a] = V.Rinv[a * 3] * g[0] + V.Rinv[a * 3 + 1] * g[1] + V.Rinv[a * 3 + 2] * g[2];
        if (V.posed) {
            const double qn = std::sqrt((double)V.q[0] * V.q[0] + (double)V.q[1] * V.q[1] + (double)V.q[2] * V.q[2] + (double)V.q[3] * V.q[3]);
            const double q[4] = {V.q[0] / qn, V.q[1] / qn, V.q[2] / qn, V.q[3] / qn};
            plain_qrot(nm, q, n);
        } else for (int a = 0; a < 3; a++) n[a] = nm[a];
        double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (len > 0.0) for (double& v : n) v /= len; else for (int a = 0; a < 3; a++) n[a] = -cam.fwd[a];
        if (n[0] * d[0] + n[1] * d[1] + n[2] * d[2] > 0.0) for (double& v : n) v = -v;
        for (int a = 0; a < 3; a++) {
            double acc = L.ambient[a];
            for (int k = 0; k < L.n_lights; k++) {
                const double l[3] = {L.pos[k][0] - P[0], L.pos[k][1] - P[1], L.pos[k][2] - P[2]};
                const double ll = std::sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
                acc += L.color[k][a] * std::fmax(0.0, (n[0] * l[0] + n[1] * l[1] + n[2] * l[2]) / ll);
            }
            const double cval = std::fmin(1.0, std::fmax(0.0, ((V.rgba >> (8 * a)) & 0xffu) / 255.0 * acc));
            CHECK(std::abs((int)out[a] - (int)(cval * 255.0 + 0.5)) <= 1, "%s: channel %d is %d, plain %g at (%d, %d)", name, a, (int)out[a], cval * 255.0, i, j);
        }
    }
    std::printf("%s: %d hits, %d at sample 0\n", name, n_hit, n_k0);
    *n_hit_out = n_hit;
}

int main() {
    const double pos[3] = {0.4, 0.9, 2.1}, at[3] = {0.5, 0.45, 0.5};
    const FeRenderCamera cam = make_cam(pos, at, 30.0);
    const FeRenderLights L = make_lights();
    int n;
    {   // an analytic sphere sampled at res 24 in a box with three different voxel sizes
        Vol v;
        const double lo[3] = {0.1, 0.15, 0.05}, hi[3] = {0.9, 0.8, 0.95}, c[3] = {0.5, 0.45, 0.5};
        make_vol(v, 24, lo, hi, [&](double x, double y, double z) { return std::sqrt((x - c[0]) * (x - c[0]) + (y - c[1]) * (y - c[1]) + (z - c[2]) * (z - c[2])) - 0.25; });
        check_volume("sphere", cam, L, v, 0.5, 10, true, c, 0.25, &n);
        CHECK(n > 20 && n < W * H, "sphere: %d hits", n);
        check_volume("sphere, step 1, no bisection", cam, L, v, 1.0, 0, false, c, 0.25, &n);
    }
    {   // a posed box: quaternion not normalised, pose away from the origin
        Vol v;
        const double lo[3] = {-0.3, -0.3, -0.3}, hi[3] = {0.3, 0.3, 0.3};
        make_vol(v, 12, lo, hi, [&](double x, double y, double z) { return 3.0 * (std::fmax(std::fabs(x) - 0.15, std::fmax(std::fabs(y) - 0.1, std::fabs(z) - 0.2))); });
        v.V.posed = 1; v.V.p[0] = 0.55f; v.V.p[1] = 0.5f; v.V.p[2] = 0.45f;
        v.V.q[0] = 1.8f; v.V.q[1] = 0.4f; v.V.q[2] = -0.7f; v.V.q[3] = 0.3f;
        check_volume("posed box", cam, L, v, 0.5, 10, false, lo, 0.0, &n);
        CHECK(n > 10 && n < W * H, "posed box: %d hits", n);
    }
    {   // 2^3 cells, solid throughout: every hit is at sample 0, the gradient vanishes inside; and a camera inside a solid
        Vol v;
        const double lo[3] = {0.3, 0.3, 0.3}, hi[3] = {0.7, 0.6, 0.7};
        make_vol(v, 3, lo, hi, [&](double, double, double) { return -1.0; });
        check_volume("solid res 3", cam, L, v, 0.5, 10, false, lo, 0.0, &n);
        CHECK(n > 5, "solid: %d hits", n);
        Vol big;
        const double blo[3] = {-1.0, -1.0, -1.0}, bhi[3] = {3.0, 3.0, 3.0};
        make_vol(big, 5, blo, bhi, [&](double, double, double) { return -0.5; });
        FeRenderRay r;
        fe_rs_ray(cam, big.V, 16, 10, r);
        float dep = 0.f;
        CHECK(fe_rs_march(cam, big.V, r, 0.5, 10, std::numeric_limits<float>::infinity(), dep) && dep == (float)cam.near, "camera inside: the hit is at t0 = near, got %g", dep);
    }
    {   // a ray that misses the box, and one parallel to an axis outside it
        Vol v;
        const double lo[3] = {5.0, 5.0, 5.0}, hi[3] = {6.0, 6.0, 6.0};
        make_vol(v, 4, lo, hi, [&](double, double, double) { return -1.0; });
        float dep;
        for (int j = 0; j < H; j++) for (int i = 0; i < W; i++) { FeRenderRay r; fe_rs_ray(cam, v.V, i, j, r); CHECK(!fe_rs_march(cam, v.V, r, 0.5, 10, std::numeric_limits<float>::infinity(), dep), "a hit off the box"); }
        FeRenderRay r;
        fe_rs_ray(cam, v.V, 0, 0, r);
        r.dv[1] = 0.0; r.ov[1] = -0.5;
        CHECK(!fe_rs_march(cam, v.V, r, 0.5, 10, std::numeric_limits<float>::infinity(), dep), "a ray parallel to a slab and outside it");
    }
    {   // cells
        float x[3];
        fe_rs_cell_centre(16, 0, 7, 15, x);
        CHECK(x[0] == 0.5f / 16.f && x[1] == 7.5f / 16.f && x[2] == 15.5f / 16.f, "cell centre");
        const double cold[3] = {0.0, 0.55, 1.0}, hot[3] = {1.0, 0.45, 0.14};
        unsigned char b[3];
        fe_rs_cell_colour(cold, hot, 0.f, b);
        CHECK(b[0] == 0 && b[1] == 140 && b[2] == 255, "cold %d %d %d", b[0], b[1], b[2]);
        fe_rs_cell_colour(cold, hot, 1.f, b);
        CHECK(b[0] == 255 && b[1] == 115 && b[2] == 36, "hot %d %d %d", b[0], b[1], b[2]);
        fe_rs_cell_colour(cold, hot, std::numeric_limits<float>::quiet_NaN(), b);
        CHECK(b[0] == 0 && b[1] == 0 && b[2] == 0, "NaN %d %d %d", b[0], b[1], b[2]);
        fe_rs_cell_colour(cold, hot, 3.f, b);
        CHECK(b[0] == 255 && b[2] == 0, "q = 3: %d %d %d", b[0], b[1], b[2]);
        CHECK(fe_rs_vol_id0(0) == FE_RENDER_MAX_SETS * FE_RENDER_MAX_POINTS && fe_rs_cell_id0(5) == 5 + FE_RENDER_MAX_SETS * FE_RENDER_MAX_POINTS + FE_RENDER_MAX_VOLUMES, "id bases");
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
