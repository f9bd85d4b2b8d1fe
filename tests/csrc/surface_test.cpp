// Host check of the liquid-surface math shared with the kernels (fluidlab_amd/csrc/fe_surface.h: fe_sf_thick, fe_sf_smooth, fe_sf_ray, fe_sf_tangent,
// fe_sf_shade -- the functions k_surface_splat, k_surface_smooth and k_surface_shade run) against the definitions of include/fluidengine_ext.h
// written out in plain loops over whole small images (37 x 23: neither side a multiple of the 16-pixel tile): the smoothing pass by its definition,
// the same pass through staged tiles with halos as the kernel stages them (the result must not depend on the tiling), what a pass may and may not
// blend, the tangent's choice of neighbour, the normal of a flat and of a tilted sheet, the highlight's power, the opacity and the composite.
// Built twice by tests/test_surface_math.py: plain, and with -fsanitize=address,undefined (the images are heap blocks of exactly W * H words here).
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
#include "../../fluidlab_amd/csrc/fe_surface.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; if (failures < 40) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const int W = 37, H = 23;
static const float INF = std::numeric_limits<float>::infinity();

static FeRenderCamera make_cam() {
    FeRenderCamera c;
    std::memset(&c, 0, sizeof(c));
    c.pos[0] = 0.5; c.pos[1] = 0.5; c.pos[2] = 3.0;
    c.right[0] = 1.0; c.up[1] = 1.0; c.fwd[2] = -1.0;
    c.focal = 0.5 * H / std::tan(30.0 * M_PI / 360.0);
    c.near = 0.01; c.max_radius_px = 32.0; c.width = W; c.height = H;
    return c;
}
static FeRenderLights one_light(double x, double y, double z) {
    FeRenderLights L;
    std::memset(&L, 0, sizeof(L));
    for (int a = 0; a < 3; a++) { L.background[a] = 1.0; L.color[0][a] = 1.0; }
    L.pos[0][0] = x; L.pos[0][1] = y; L.pos[0][2] = z;
    L.n_lights = 1;
    return L;
}
static FeSurfaceParams make_params() {
    FeSurfaceParams S;
    std::memset(&S, 0, sizeof(S));
    S.radius_scale = 1.5; S.range = 0.05; S.absorb = 40.0; S.alpha_min = 0.25; S.specular = 0.3;
    S.smooth_iters = 2; S.smooth_radius_px = 5; S.shininess_log2 = 5;
    return S;
}
static unsigned fbits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

// a whole image on the heap, exactly W * H floats
struct Img {
    const float* z;
    float operator()(int i, int j) const { return z[(size_t)j * W + i]; }
};
// a staged tile with its halo, as k_surface_smooth stages it: side * side floats, entry (0, 0) is pixel (i0, j0)
struct Tile {
    const float* t; int i0, j0, side;
    float operator()(int i, int j) const { return t[(size_t)(j - j0) * side + (i - i0)]; }
};

// two sheets more than `range` apart, holes, an isolated pixel and a jitter of `amp`
static std::vector<float> make_depth(double range, double amp, unsigned seed) {
    std::vector<float> z((size_t)W * H, INF);
    std::mt19937 g(seed);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    for (int j = 0; j < H; j++)
        for (int i = 0; i < W; i++) {
            const bool hole = (i % 9 == 4 && j % 7 == 3) || (i > 30 && j > 18 && !(i == 34 && j == 21));
            if (hole) continue;
            if (i > 30 && j > 18) { z[(size_t)j * W + i] = 2.0f; continue; }
            const double sheet = i < 20 ? 2.0 : 2.0 + 3.0 * range;
            z[(size_t)j * W + i] = (float)(sheet + amp * U(g));
        }
    for (int j = 17; j < H; j++) for (int i = 29; i < W; i++) z[(size_t)j * W + i] = INF;      // a cleared corner ...
    z[(size_t)21 * W + 34] = 2.0f;                                                               // ... with one liquid pixel alone in it
    return z;
}

// the pass by the header's text, every step spelled out
static float smooth_def(const std::vector<float>& z, int i, int j, int r, double range, double* den_out, double* lo, double* hi) {
    const double zp = (double)z[(size_t)j * W + i];
    double num = 0.0, den = 0.0;
    *lo = 1e300; *hi = -1e300;
    for (int dj = -r; dj <= r; dj++)
        for (int di = -r; di <= r; di++) {
            const int qi = i + di, qj = j + dj;
            if (qi < 0 || qi >= W || qj < 0 || qj >= H) continue;
            const float zq = z[(size_t)qj * W + qi];
            if (std::isinf(zq)) continue;
            const double s2 = (double)(di * di + dj * dj) / (double)((r + 1) * (r + 1));
            if (s2 >= 1.0) continue;
            const double dz = ((double)zq - zp) / range;
            if (dz * dz >= 1.0) continue;
            const double w = ((1.0 - s2) * (1.0 - s2)) * ((1.0 - dz * dz) * (1.0 - dz * dz));
            num = num + w * (double)zq;
            den = den + w;
            if ((double)zq < *lo) *lo = (double)zq;
            if ((double)zq > *hi) *hi = (double)zq;
        }
    *den_out = den;
    return (float)(num / den);
}

static void test_smooth() {
    const double range = 0.05;
    for (int r : {1, 5, 8}) {
        std::vector<float> z = make_depth(range, 0.004, 7u + (unsigned)r);
        for (int it = 0; it < 3; it++) {
            std::vector<float> whole((size_t)W * H, INF), tiled((size_t)W * H, INF);
            const Img img = {z.data()};
            for (int j = 0; j < H; j++)
                for (int i = 0; i < W; i++) {
                    const float zp = z[(size_t)j * W + i];
                    if (!fe_sf_liquid(zp)) continue;
                    double den, lo, hi;
                    const float want = smooth_def(z, i, j, r, range, &den, &lo, &hi);
                    const float got = fe_sf_smooth(img, i, j, W, H, r, range, zp);
                    whole[(size_t)j * W + i] = got;
                    CHECK(fbits(got) == fbits(want), "smooth r %d it %d (%d, %d): %.9g, by definition %.9g", r, it, i, j, got, want);
                    CHECK(den >= 1.0, "den %.17g < 1 at (%d, %d)", den, i, j);
                    CHECK((double)got >= lo - 1e-6 && (double)got <= hi + 1e-6, "smooth leaves the range of what it blends at (%d, %d)", i, j);
                    // sheets further apart than `range` do not blend: every pixel stays with its own sheet
                    CHECK(std::fabs((double)got - (double)zp) < range, "(%d, %d) moved by %.9g >= range", i, j, (double)got - (double)zp);
                }
            // the kernel's road: 16 x 16 tiles, each staged with its halo (out-of-image entries +inf) in a block of exactly side^2 floats
            const int side = FE_SURFACE_TILE + 2 * r;
            for (int tj = 0; tj * FE_SURFACE_TILE < H; tj++)
                for (int ti = 0; ti * FE_SURFACE_TILE < W; ti++) {
                    std::vector<float> t((size_t)side * side);
                    const int i0 = ti * FE_SURFACE_TILE - r, j0 = tj * FE_SURFACE_TILE - r;
                    for (int e = 0; e < side * side; e++) {
                        const int qi = i0 + e % side, qj = j0 + e / side;
                        t[(size_t)e] = (qi >= 0 && qi < W && qj >= 0 && qj < H) ? z[(size_t)qj * W + qi] : INF;
                    }
                    const Tile tile = {t.data(), i0, j0, side};
                    for (int k = 0; k < FE_SURFACE_TILE * FE_SURFACE_TILE; k++) {
                        const int i = ti * FE_SURFACE_TILE + k % FE_SURFACE_TILE, j = tj * FE_SURFACE_TILE + k / FE_SURFACE_TILE;
                        if (i >= W || j >= H) continue;
                        const float zp = tile(i, j);
                        tiled[(size_t)j * W + i] = fe_sf_liquid(zp) ? fe_sf_smooth(tile, i, j, W, H, r, range, zp) : INF;
                    }
                }
            for (size_t p = 0; p < whole.size(); p++) CHECK(fbits(whole[p]) == fbits(tiled[p]), "tiling changes pixel %zu (r %d)", p, r);
            CHECK(fbits(whole[(size_t)21 * W + 34]) == fbits(2.0f), "the isolated pixel moved");      // its window holds its centre only
            z = whole;
        }
    }
    // a flat sheet with jitter: a pass lowers the variance
    std::vector<float> z((size_t)W * H);
    std::mt19937 g(3);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    for (float& v : z) v = (float)(2.0 + 0.004 * U(g));
    auto var = [](const std::vector<float>& a) { double m = 0, s = 0; for (float v : a) m += v; m /= a.size(); for (float v : a) s += (v - m) * (v - m); return s / a.size(); };
    std::vector<float> out(z.size());
    const Img img = {z.data()};
    for (int j = 0; j < H; j++) for (int i = 0; i < W; i++) out[(size_t)j * W + i] = fe_sf_smooth(img, i, j, W, H, 3, range, z[(size_t)j * W + i]);
    CHECK(var(out) < 0.25 * var(z), "variance %.3g -> %.3g", var(z), var(out));
}

static void test_thick() {
    CHECK(fe_sf_thick(0.01, 0.0) == 0ull, "zero chord");
    CHECK(fe_sf_thick(0.5, 1.0) == 4294967296ull, "unit chord");
    unsigned long long prev = 0;
    for (int k = 0; k <= 1000; k++) {
        const double nz = k / 1000.0;
        const unsigned long long q = fe_sf_thick(0.01125, nz);
        CHECK(q == (unsigned long long)std::llrint((2.0 * 0.01125 * nz) * 4294967296.0), "quantum at nz %g", nz);
        CHECK(q >= prev, "not monotone at nz %g", nz);
        prev = q;
    }
}

static void test_tangent() {
    const FeRenderCamera cam = make_cam();
    double d[3], dm[3], dp[3], t[3];
    const int i = 10, j = 9;
    fe_sf_ray(cam, i, j, d); fe_sf_ray(cam, i - 1, j, dm); fe_sf_ray(cam, i + 1, j, dp);
    // the ray by the header's text
    for (int c = 0; c < 3; c++) {
        const double want = (cam.fwd[c] + ((i + 0.5 - 0.5 * W) / cam.focal) * cam.right[c]) - ((j + 0.5 - 0.5 * H) / cam.focal) * cam.up[c];
        CHECK(d[c] == want, "ray component %d", c);
    }
    const double z = 2.0, range = 0.05;
    auto expect = [&](float zm, float zp, double zn, const double* dn, const char* what) {
        fe_sf_tangent(cam, z, d, zm, zp, dm, dp, range, t);
        for (int c = 0; c < 3; c++) CHECK(t[c] == (cam.pos[c] + zn * dn[c]) - (cam.pos[c] + z * d[c]), "%s: component %d", what, c);
    };
    expect(2.01f, 2.02f, (double)2.01f, dm, "the nearer neighbour is at -1");
    expect(2.02f, 1.99f, (double)1.99f, dp, "the nearer neighbour is at +1");
    expect(2.01f, 2.01f, (double)2.01f, dp, "a tie goes to +1");
    expect(2.0f - 0.0078125f, 2.0f + 0.0078125f, 2.0078125, dp, "a tie in |dz| goes to +1");
    expect(2.2f, 2.01f, (double)2.01f, dp, "-1 is out of range");
    expect(2.01f, 2.2f, (double)2.01f, dm, "+1 is out of range");
    expect(INF, 2.01f, (double)2.01f, dp, "-1 is not liquid");
    expect(2.01f, INF, (double)2.01f, dm, "+1 is not liquid");
    expect(INF, INF, z, dp, "no neighbour: the own depth on the ray at +1");
    expect(2.2f, 1.8f, z, dp, "both out of range: the own depth on the ray at +1");
}

// one pixel of fe_sf_shade over an image z, with the neighbour rule of k_surface_shade
static void shade_at(const FeRenderCamera& cam, const FeRenderLights& L, const FeSurfaceParams& S, const std::vector<float>& z, int i, int j, const unsigned char* base,
                     unsigned long long word, const unsigned char* behind, unsigned char* out) {
    const size_t p = (size_t)j * W + i;
    const float zs[5] = {z[p], i > 0 ? z[p - 1] : INF, i + 1 < W ? z[p + 1] : INF, j > 0 ? z[p - W] : INF, j + 1 < H ? z[p + W] : INF};
    fe_sf_shade(cam, L, S, i, j, zs, base, word, behind, out);
}

static void test_shade() {
    const FeRenderCamera cam = make_cam();
    const unsigned char white[3] = {255, 255, 255}, black[3] = {0, 0, 0}, behind[3] = {13, 200, 77};
    const unsigned long long thick = (unsigned long long)(0.05 * 4294967296.0);
    // a sheet z = z0 + gx i + gy j: its normal from the cross product of the exact tangents, and n.l of one white light through the bytes
    // (ambient 0, base white, no highlight, alpha_min 1: out = byte(max(0, n.l)))
    for (int tilt = 0; tilt < 3; tilt++) {
        const double gx = tilt == 1 ? 0.002 : 0.0, gy = tilt == 2 ? -0.003 : 0.0;
        std::vector<float> z((size_t)W * H);
        for (int j = 0; j < H; j++) for (int i = 0; i < W; i++) z[(size_t)j * W + i] = (float)(2.0 + gx * i + gy * j);
        FeSurfaceParams S = make_params();
        S.alpha_min = 1.0; S.specular = 0.0;
        const FeRenderLights L = one_light(0.7, 1.5, 3.5);
        for (int j = 0; j < H; j++)
            for (int i = 0; i < W; i++) {
                unsigned char out[3];
                shade_at(cam, L, S, z, i, j, white, thick, behind, out);
                // the plane through P(i, j), P(i + 1, j), P(i, j + 1) of the exact (unrounded) sheet
                auto P = [&](int a, int b, double* o) { double d[3]; fe_sf_ray(cam, a, b, d); const double zz = 2.0 + gx * a + gy * b; for (int c = 0; c < 3; c++) o[c] = cam.pos[c] + zz * d[c]; };
                double p0[3], px[3], py[3];
                P(i, j, p0); P(i + 1, j, px); P(i, j + 1, py);
                const double tx[3] = {px[0] - p0[0], px[1] - p0[1], px[2] - p0[2]}, ty[3] = {py[0] - p0[0], py[1] - p0[1], py[2] - p0[2]};
                double n[3] = {ty[1] * tx[2] - ty[2] * tx[1], ty[2] * tx[0] - ty[0] * tx[2], ty[0] * tx[1] - ty[1] * tx[0]};
                const double ln = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                double d[3]; fe_sf_ray(cam, i, j, d);
                double sgn = (n[0] * d[0] + n[1] * d[1] + n[2] * d[2]) > 0 ? -1.0 : 1.0;
                double l[3] = {L.pos[0][0] - p0[0], L.pos[0][1] - p0[1], L.pos[0][2] - p0[2]};
                const double ll = std::sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
                double ndl = sgn * (n[0] * l[0] + n[1] * l[1] + n[2] * l[2]) / (ln * ll);
                if (ndl < 0) ndl = 0;
                // (the sheet is stored in fp32: a depth step of 2^-22 over a pixel of about 1/40 tilts the normal by up to 1e-5 rad)
                for (int c = 0; c < 3; c++) CHECK(std::abs((int)out[c] - (int)(ndl * 255.0 + 0.5)) <= 1, "tilt %d (%d, %d): byte %d, n.l %.6f", tilt, i, j, out[c], ndl);
            }
    }
    // the highlight: base black, specular 1, alpha_min 1: out = byte(max(0, n.h)^(2^k)), n = -fwd on a sheet of constant depth
    std::vector<float> flat((size_t)W * H, 2.0f);
    for (int k : {0, 1, 5, 10}) {
        FeSurfaceParams S = make_params();
        S.alpha_min = 1.0; S.specular = 1.0; S.shininess_log2 = k;
        const FeRenderLights L = one_light(0.52, 0.55, 3.4);
        for (int j = 0; j < H; j += 3)
            for (int i = 0; i < W; i += 3) {
                unsigned char out[3];
                shade_at(cam, L, S, flat, i, j, black, thick, behind, out);
                double d[3]; fe_sf_ray(cam, i, j, d);
                const double dl = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                double l[3], hv[3];
                for (int c = 0; c < 3; c++) l[c] = L.pos[0][c] - (cam.pos[c] + 2.0 * d[c]);
                const double ll = std::sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
                for (int c = 0; c < 3; c++) hv[c] = l[c] / ll - d[c] / dl;
                const double hl = std::sqrt(hv[0] * hv[0] + hv[1] * hv[1] + hv[2] * hv[2]);
                double s = -(cam.fwd[0] * hv[0] + cam.fwd[1] * hv[1] + cam.fwd[2] * hv[2]) / hl;
                s = s > 0 ? std::pow(s, (double)(1 << k)) : 0.0;
                for (int c = 0; c < 3; c++) CHECK(std::abs((int)out[c] - (int)(std::min(s, 1.0) * 255.0 + 0.5)) <= 1, "highlight k %d (%d, %d): byte %d, %.6f", k, i, j, out[c], s);
            }
    }
    // opacity and composite
    {
        FeSurfaceParams S = make_params();
        const FeRenderLights L = one_light(0.7, 1.5, 3.5);
        unsigned char out[3];
        S.alpha_min = 0.0; S.absorb = 0.0;                    // alpha = 0: the opaque picture's bytes come back as they were
        for (int b = 0; b < 256; b++) {
            const unsigned char bh[3] = {(unsigned char)b, (unsigned char)(255 - b), (unsigned char)((b * 7) & 255)};
            shade_at(cam, L, S, flat, 5, 5, white, thick, bh, out);
            CHECK(out[0] == bh[0] && out[1] == bh[1] && out[2] == bh[2], "alpha 0 changes byte %d", b);
        }
        S.alpha_min = 0.0; S.absorb = 40.0;
        shade_at(cam, L, S, flat, 5, 5, white, 0ull, behind, out);      // no thickness: alpha_min
        CHECK(out[0] == behind[0] && out[1] == behind[1] && out[2] == behind[2], "zero thickness with alpha_min 0 is not the opaque picture");
        // black liquid over white, no light: out = byte(1 - alpha), falling with the thickness and never below 1 - 1 = 0 nor above 1 - alpha_min
        S.alpha_min = 0.25; S.specular = 0.0;
        FeRenderLights dark = L; dark.n_lights = 0;
        int prev = 256;
        for (int k = 0; k <= 64; k++) {
            const double t = 0.004 * k;
            shade_at(cam, dark, S, flat, 5, 5, black, (unsigned long long)std::llrint(t * 4294967296.0), white, out);
            const double at = 40.0 * t, alpha = 0.25 + (0.75 * at) / (1.0 + at);
            CHECK(std::abs((int)out[0] - (int)((1.0 - alpha) * 255.0 + 0.5)) <= 1, "alpha at t %.3f: byte %d, 1 - alpha %.6f", t, out[0], 1.0 - alpha);
            CHECK((int)out[0] <= prev && (int)out[0] <= 192 && alpha < 1.0, "opacity not monotone at t %.3f", t);
            prev = out[0];
        }
    }
    // the image border and an isolated pixel: every neighbour missing, nothing read outside the block, the normal falls back and stays finite
    {
        std::vector<float> lone((size_t)W * H, INF);
        const int at[5][2] = {{0, 0}, {W - 1, 0}, {0, H - 1}, {W - 1, H - 1}, {17, 11}};
        for (const auto& q : at) lone[(size_t)q[1] * W + q[0]] = 2.0f;
        FeSurfaceParams S = make_params();
        S.alpha_min = 1.0; S.specular = 0.0;
        const FeRenderLights L = one_light(0.5, 0.5, 4.0);
        for (const auto& q : at) {
            unsigned char out[3];
            shade_at(cam, L, S, lone, q[0], q[1], white, thick, behind, out);
            CHECK(out[0] > 200, "lone pixel (%d, %d) is lit from the front: byte %d", q[0], q[1], out[0]);
        }
    }
}

int main() {
    test_thick();
    test_smooth();
    test_tangent();
    test_shade();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
