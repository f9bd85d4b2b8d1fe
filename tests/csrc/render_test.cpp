// Host check of the renderer's math shared with the kernels (fluidlab_amd/csrc/fe_render.h: fe_rd_project, fe_rd_fragment, fe_rd_key, fe_rd_shade --
// the functions k_render_splat, k_render_points and k_render_shade run) against the definitions of include/fluidengine_ext.h written out in
// plain loops over the WHOLE image: projection, the box and its clipping, coverage with the centre-pixel rule, key packing and ordering, shading.
// The image of the plain loops (every pixel tested against every sphere) must be EQUAL word for word to the one drawn box by box.
// Built twice by tests/test_render_math.py: plain, and with -fsanitize=address,undefined.
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

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static FeRenderCamera make_cam(int W, int H, const double* pos, const double* at, double fov_deg, double near, double max_r) {
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
    c.near = near; c.max_radius_px = max_r; c.width = W; c.height = H;
    return c;
}

// the definition for one sphere and one pixel of the image, with no box: is the pixel covered, and by which fragment
struct Plain { bool drawn; double zc, px, py, rp; };
static Plain plain_project(const FeRenderCamera& c, const float* x, double R) {
    Plain p = {false, 0, 0, 0, 0};
    for (int a = 0; a < 3; a++) if (!std::isfinite(x[a])) return p;
    const double d[3] = {(double)x[0] - c.pos[0], (double)x[1] - c.pos[1], (double)x[2] - c.pos[2]};
    const double zc = d[0] * c.fwd[0] + d[1] * c.fwd[1] + d[2] * c.fwd[2];
    const double xc = d[0] * c.right[0] + d[1] * c.right[1] + d[2] * c.right[2];
    const double yc = d[0] * c.up[0] + d[1] * c.up[1] + d[2] * c.up[2];
    if (!(zc > c.near + R)) return p;
    p.drawn = true; p.zc = zc;
    p.px = c.width / 2.0 + c.focal * xc / zc;
    p.py = c.height / 2.0 - c.focal * yc / zc;
    p.rp = std::fmin(c.focal * R / zc, c.max_radius_px);
    return p;
}
static bool plain_fragment(const Plain& p, double R, int i, int j, double& u, double& v, double& nz, float& depth) {
    u = (i + 0.5 - p.px) / p.rp; v = (j + 0.5 - p.py) / p.rp;
    double s = u * u + v * v;
    const bool centre = (double)i <= p.px && p.px < (double)i + 1.0 && (double)j <= p.py && p.py < (double)j + 1.0;
    if (!(s <= 1.0) && !centre) return false;
    if (s > 1.0) s = 1.0;
    nz = std::sqrt(1.0 - s);
    depth = (float)(p.zc - R * nz);
    return true;
}

static void check_scene(const char* name, const FeRenderCamera& cam, const std::vector<float>& xs, const std::vector<double>& Rs, const FeRenderLights& L) {
    const int W = cam.width, H = cam.height, n = (int)Rs.size();
    std::vector<unsigned long long> box((size_t)W * H, FE_RENDER_BG), all((size_t)W * H, FE_RENDER_BG);
    for (int k = 0; k < n; k++) {
        const float* x = &xs[3 * (size_t)k];
        FeRenderSphere sp;
        const bool drawn = fe_rd_project(cam, x, Rs[k], sp);
        const Plain p = plain_project(cam, x, Rs[k]);
        CHECK(drawn == p.drawn, "%s sphere %d: drawn %d, definition %d", name, k, (int)drawn, (int)p.drawn);
        if (!drawn) continue;
        CHECK(sp.zc == p.zc && sp.px == p.px && sp.py == p.py && sp.rp == p.rp, "%s sphere %d: projection", name, k);
        CHECK(sp.i0 >= 0 && sp.j0 >= 0 && sp.i1 <= W - 1 && sp.j1 <= H - 1, "%s sphere %d: box [%d, %d] x [%d, %d] leaves the image", name, k, sp.i0, sp.i1, sp.j0, sp.j1);
        CHECK(fe_rd_box_pixels(sp) == (long long)fe_rd_box_w(sp) * fe_rd_box_h(sp), "%s box pixels", name);
        for (int j = sp.j0; j <= sp.j1; j++)
            for (int i = sp.i0; i <= sp.i1; i++) {
                FeRenderFrag fr;
                if (!fe_rd_fragment(sp, i, j, fr)) continue;
                const unsigned long long key = fe_rd_key(fr.depth, k);
                unsigned long long& w = box[(size_t)j * W + i];
                if (key < w) w = key;
            }
        // the definition over the whole image: nothing outside the box may be covered
        for (int j = 0; j < H; j++)
            for (int i = 0; i < W; i++) {
                double u, v, nz; float depth;
                if (!plain_fragment(p, Rs[k], i, j, u, v, nz, depth)) continue;
                CHECK(i >= sp.i0 && i <= sp.i1 && j >= sp.j0 && j <= sp.j1, "%s sphere %d: pixel (%d, %d) is covered but outside the box", name, k, i, j);
                CHECK(depth > 0.f, "%s depth not positive", name);
                unsigned bits; std::memcpy(&bits, &depth, 4);
                const unsigned long long key = ((unsigned long long)bits << 32) | (unsigned)k;
                unsigned long long& w = all[(size_t)j * W + i];
                if (key < w) w = key;
            }
    }
    int diff = 0, covered = 0;
    for (size_t p = 0; p < box.size(); p++) { diff += box[p] != all[p]; covered += all[p] != FE_RENDER_BG; }
    CHECK(diff == 0, "%s: %d pixel words differ between the boxes and the whole-image loops", name, diff);
    // discs cross each of the four edges: the first and last row and column are covered, and by spheres whose centre lies outside the image
    int edge_px[4] = {0, 0, 0, 0}, edge_out[4] = {0, 0, 0, 0};
    for (int i = 0; i < W; i++) { edge_px[0] += all[i] != FE_RENDER_BG; edge_px[1] += all[(size_t)(H - 1) * W + i] != FE_RENDER_BG; }
    for (int j = 0; j < H; j++) { edge_px[2] += all[(size_t)j * W] != FE_RENDER_BG; edge_px[3] += all[(size_t)j * W + W - 1] != FE_RENDER_BG; }
    for (int k = 0; k < n; k++) {
        FeRenderSphere sp;
        if (!fe_rd_project(cam, &xs[3 * (size_t)k], Rs[k], sp) || fe_rd_box_pixels(sp) == 0) continue;
        edge_out[0] += sp.py < 0.0; edge_out[1] += sp.py >= (double)H; edge_out[2] += sp.px < 0.0; edge_out[3] += sp.px >= (double)W;
    }
    const char* edge_name[4] = {"top", "bottom", "left", "right"};
    for (int e = 0; e < 4; e++)
        CHECK(edge_px[e] > 0 && edge_out[e] > 0, "%s: %s edge: %d pixels covered, %d discs drawn from a centre beyond it", name, edge_name[e], edge_px[e], edge_out[e]);
    CHECK(covered > 0, "%s: nothing drawn", name);
    // shade every covered pixel from its winner, against the definition
    int shade_bad = 0;
    for (int j = 0; j < H; j++)
        for (int i = 0; i < W; i++) {
            const unsigned long long key = box[(size_t)j * W + i];
            if (key == FE_RENDER_BG) continue;
            const int k = fe_rd_key_id(key);
            FeRenderSphere sp; FeRenderFrag fr;
            const bool ok = fe_rd_project(cam, &xs[3 * (size_t)k], Rs[k], sp) && fe_rd_fragment(sp, i, j, fr);
            CHECK(ok, "%s: the winner of (%d, %d) has no fragment there", name, i, j);
            if (!ok) continue;
            CHECK(fe_rd_float_bits(fr.depth) == (unsigned)(key >> 32) && fe_rd_key_depth(key) == fr.depth, "%s: depth of the key", name);
            const unsigned char base[3] = {(unsigned char)(40 + 7 * k % 200), (unsigned char)(250 - 3 * k % 200), 128};
            unsigned char got[3];
            fe_rd_shade(cam, L, sp, fr, base, got);
            double nrm[3], P[3];
            for (int a = 0; a < 3; a++) { nrm[a] = fr.u * cam.right[a] - fr.v * cam.up[a] - fr.nz * cam.fwd[a]; P[a] = (double)xs[3 * (size_t)k + a] + Rs[k] * nrm[a]; }
            for (int a = 0; a < 3; a++) {
                double acc = L.ambient[a];
                for (int q = 0; q < L.n_lights; q++) {
                    const double l[3] = {L.pos[q][0] - P[0], L.pos[q][1] - P[1], L.pos[q][2] - P[2]};
                    const double len = std::sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
                    acc += L.color[q][a] * std::fmax(0.0, (nrm[0] * l[0] + nrm[1] * l[1] + nrm[2] * l[2]) / len);
                }
                const double c = std::fmin(1.0, std::fmax(0.0, base[a] / 255.0 * acc));
                const int want = (int)(c * 255.0 + 0.5);
                if (std::abs(want - (int)got[a]) > 1) shade_bad++;          // (the plain loop may contract or associate differently: one level)
            }
        }
    CHECK(shade_bad == 0, "%s: %d shaded channels off by more than one level", name, shade_bad);
    std::printf("%s: %d spheres, %d covered pixels\n", name, n, covered);
}

int main() {
    CHECK(sizeof(FeRenderCamera) == 128, "sizeof(FeRenderCamera) = %zu", sizeof(FeRenderCamera));
    CHECK(sizeof(FeRenderLights) == 248, "sizeof(FeRenderLights) = %zu", sizeof(FeRenderLights));
    FeRenderLights L;
    std::memset(&L, 0, sizeof(L));
    for (int a = 0; a < 3; a++) { L.ambient[a] = 0.1; L.background[a] = 1.0; L.color[0][a] = 0.5; L.color[1][a] = 0.5; }
    L.pos[0][0] = 0.5; L.pos[0][1] = 1.5; L.pos[0][2] = 0.5; L.pos[1][0] = 0.5; L.pos[1][1] = 1.5; L.pos[1][2] = 1.5;
    L.n_lights = 2;

    // a sphere on the optical axis: a disc about (W/2, H/2) of radius focal R / zc, on a non-square image
    {
        const double pos[3] = {0.5, 0.5, 3.0}, at[3] = {0.5, 0.5, 0.5};
        const FeRenderCamera cam = make_cam(80, 48, pos, at, 40.0, 0.01, 64.0);
        const float x[3] = {0.5f, 0.5f, 1.0f};
        const double R = 0.2;
        FeRenderSphere sp;
        CHECK(fe_rd_project(cam, x, R, sp), "axis sphere dropped");
        CHECK(std::fabs(sp.px - 40.0) < 1e-12 && std::fabs(sp.py - 24.0) < 1e-12, "axis sphere centre (%.17g, %.17g)", sp.px, sp.py);
        const double want_rp = cam.focal * R / 2.0;
        CHECK(std::fabs(sp.rp - want_rp) < 1e-12, "axis sphere radius %.17g, analytic %.17g", sp.rp, want_rp);
        int n_cov = 0, n_def = 0;
        for (int j = 0; j < 48; j++)
            for (int i = 0; i < 80; i++) {
                FeRenderFrag fr;
                const bool in_box = i >= sp.i0 && i <= sp.i1 && j >= sp.j0 && j <= sp.j1;
                const bool cov = in_box && fe_rd_fragment(sp, i, j, fr);
                const double dx = i + 0.5 - 40.0, dy = j + 0.5 - 24.0;
                const bool def = dx * dx + dy * dy <= want_rp * want_rp;
                n_cov += cov; n_def += def;
                if (std::fabs(std::sqrt(dx * dx + dy * dy) - want_rp) > 1e-9) CHECK(cov == def, "axis disc pixel (%d, %d)", i, j);
                if (cov && i == 40 && j == 24) CHECK(std::fabs(fr.depth - (float)(2.0 - R * fr.nz)) == 0.f && fr.nz > 0.99, "axis disc centre depth");
            }
        CHECK(n_cov == n_def && n_cov > 100, "axis disc: %d pixels, definition %d", n_cov, n_def);
    }
    // keys: nearer wins, the lower id wins among equal depths, the background loses to everything
    {
        CHECK(fe_rd_key(1.0f, 7) < fe_rd_key(1.0000001f, 3), "nearer depth must give the smaller key");
        CHECK(fe_rd_key(2.5f, 3) < fe_rd_key(2.5f, 4), "lower id must give the smaller key");
        CHECK(fe_rd_key(3.0e38f, 0x7fffffff) < FE_RENDER_BG, "the background word must be the largest");
        CHECK(fe_rd_key_id(fe_rd_key(0.25f, 123456)) == 123456 && fe_rd_key_depth(fe_rd_key(0.25f, 123456)) == 0.25f, "key round trip");
        std::mt19937 rng(7);
        std::uniform_real_distribution<float> U(1e-3f, 100.f);
        for (int t = 0; t < 10000; t++) {
            const float a = U(rng), b = U(rng);
            if (a != b) CHECK((a < b) == (fe_rd_key(a, 5) < fe_rd_key(b, 1)), "positive floats must order like their bits");
        }
    }
    // non-finite words, zc on both sides of near + R, the radius clamp, the sub-pixel sphere
    {
        const double pos[3] = {0.5, 0.5, 3.0}, at[3] = {0.5, 0.5, 0.5};
        const FeRenderCamera cam = make_cam(64, 64, pos, at, 40.0, 0.1, 8.0);
        FeRenderSphere sp;
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        for (int a = 0; a < 3; a++) {
            float x[3] = {0.5f, 0.5f, 1.0f};
            x[a] = inf; CHECK(!fe_rd_project(cam, x, 0.05, sp), "+inf word drawn");
            x[a] = -inf; CHECK(!fe_rd_project(cam, x, 0.05, sp), "-inf word drawn");
            x[a] = nan; CHECK(!fe_rd_project(cam, x, 0.05, sp), "nan word drawn");
        }
        const float behind[3] = {0.5f, 0.5f, 3.5f}, at_near[3] = {0.5f, 0.5f, 2.85f}, past_near[3] = {0.5f, 0.5f, 2.84f}, just[3] = {0.5f, 0.5f, 2.86f};
        CHECK(!fe_rd_project(cam, behind, 0.05, sp), "a sphere behind the camera is drawn");
        CHECK(!fe_rd_project(cam, just, 0.05, sp), "zc = 0.14 < near + R = 0.15 is drawn");
        CHECK(!fe_rd_project(cam, at_near, 0.05, sp) || sp.zc > 0.15, "zc <= near + R is drawn");
        CHECK(fe_rd_project(cam, past_near, 0.05, sp) && sp.zc > 0.15, "zc = 0.16 > near + R = 0.15 is dropped");
        CHECK(sp.rp == 8.0, "the radius clamp: rp = %.17g", sp.rp);
        CHECK(fe_rd_box_w(sp) <= 18 && fe_rd_box_h(sp) <= 18, "a clamped sphere's box is %d x %d", fe_rd_box_w(sp), fe_rd_box_h(sp));
        const float far_[3] = {0.53f, 0.52f, -40.0f};
        CHECK(fe_rd_project(cam, far_, 0.001, sp) && sp.rp < 0.5, "the far sphere is not sub-pixel");
        int n = 0;
        for (int j = sp.j0; j <= sp.j1; j++) for (int i = sp.i0; i <= sp.i1; i++) { FeRenderFrag fr; if (fe_rd_fragment(sp, i, j, fr)) { n++; CHECK(i == sp.ci && j == sp.cj, "sub-pixel sphere covers a pixel that is not its centre's"); } }
        CHECK(n == 1, "a sub-pixel sphere must cover exactly its centre pixel, covers %d", n);
        const float off[3] = {40.0f, 0.5f, 1.0f};                 // far off the image: an empty box, no overflow
        CHECK(fe_rd_project(cam, off, 0.05, sp) && fe_rd_box_pixels(sp) == 0, "a sphere off the image has a box");
        const float huge_[3] = {3.0e38f, -3.0e38f, -3.0e38f};
        CHECK(fe_rd_project(cam, huge_, 0.05, sp) && fe_rd_box_pixels(sp) == 0, "a sphere at 3e38 has a box");
    }
    // whole scenes against the whole-image loops: discs across each of the four edges and the corners, overlaps, an identical pair
    {
        const double pos[3] = {0.45, 0.62, 2.2}, at[3] = {0.5, 0.5, 0.5};
        const FeRenderCamera cam = make_cam(96, 64, pos, at, 40.0, 0.01, 8.0);
        std::mt19937 rng(99);
        std::uniform_real_distribution<float> U(0.f, 1.f);
        std::vector<float> xs; std::vector<double> Rs;
        for (int k = 0; k < 400; k++) { xs.push_back(-0.6f + 2.2f * U(rng)); xs.push_back(-0.3f + 1.6f * U(rng)); xs.push_back(0.2f + 0.6f * U(rng)); Rs.push_back(0.03); }
        for (int k = 0; k < 20; k++) { xs.push_back(0.42f + 0.06f * U(rng)); xs.push_back(0.58f + 0.06f * U(rng)); xs.push_back(1.9f + 0.1f * U(rng)); Rs.push_back(0.03); }      // close to the lens: clamped
        for (int k = 0; k < 2; k++) { xs.push_back(0.5f); xs.push_back(0.5f); xs.push_back(0.9f); Rs.push_back(0.03); }                                                   // an identical pair
        check_scene("scene 96x64", cam, xs, Rs, L);
        // the identical pair: the lower id owns every pixel both cover
        const FeRenderCamera cam2 = make_cam(33, 57, pos, at, 55.0, 0.01, 32.0);
        check_scene("scene 33x57", cam2, xs, Rs, L);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
