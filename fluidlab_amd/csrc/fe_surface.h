// fe_surface.h -- liquids as one smoothed, translucent screen-space surface in the picture of fe_render.h / fe_render_scene.h
// (include/fluidengine_ext.h: fe_surface_set, fe_surface_frame, fe_surface_get).  The selected particles are taken out of the opaque picture and
// drawn as a second layer: nearest fragment and summed thickness per pixel, a depth-aware smoothing of that layer's depth, normals from the
// smoothed depth, one lit colour per pixel blended over the opaque picture by the thickness.
// Included from the last line of the kernel part of fe_render_scene.h (tests/test_render_scene_abi.py allows no fe_*.h behind that header in
// fe_engine.hip).  Its kernels are template instantiations (<0>) that take their arguments as one struct and read no blockDim / gridDim, and their
// first uses stand at the very end of fe_engine.hip, behind fe_field_obs.h's: they are the last code of the object and every other kernel keeps
// its address (fe_render_scene.h, fe_field_obs.h say why that matters).
//
// The rules of fe_render.h hold: fp64 formed from fp32 words with + - * / and sqrt under fp contract(off), no exp or pow (the highlight is raised
// to 2^k by k squarings), integer atomics only.  The per-pixel math is __host__ __device__ code above the FE_RENDER_MATH_ONLY guard
// (tests/csrc/surface_test.cpp compiles it for the host; tests/surface_ref.py restates it).
#ifndef FE_SURFACE_H
#define FE_SURFACE_H

#define FE_SURFACE_TILE 16                                   /* k_surface_smooth: pixels along a side of a workgroup's tile */
#define FE_SURFACE_MAX_R 8                                   /* the largest smooth_radius_px: tile + halo is at most 32 x 32 */
#define FE_SURFACE_FIX 4294967296.0                          /* 2^32: a thickness word counts in units of 2^-32 */

// the thickness a fragment with normal component nz of a sphere of radius Rs adds to its pixel's word: the chord 2 Rs nz in units of 2^-32
__host__ __device__ inline unsigned long long fe_sf_thick(double Rs, double nz) {
#pragma clang fp contract(off)
    return (unsigned long long)llrint((2.0 * Rs * nz) * FE_SURFACE_FIX);
}
__host__ __device__ inline bool fe_sf_liquid(float z) { return fe_rd_finite(z); }      // (a depth image of the liquid layer holds +inf elsewhere)

// One smoothing pass at the liquid pixel (i, j) of depth zp.  z(qi, qj) is the depth image of the pass before at a pixel inside the image.
// Window offsets dj = -r .. r (outer), di = -r .. r (inner), in that order; the centre has weight 1, so den >= 1.
template <class Z>
__host__ __device__ inline float fe_sf_smooth(const Z& z, int i, int j, int W, int H, int r, double range, float zpf) {
#pragma clang fp contract(off)
    const double zp = (double)zpf;
    const double rr = (double)((r + 1) * (r + 1));
    double num = 0.0, den = 0.0;
    for (int dj = -r; dj <= r; dj++) {
        const int qj = j + dj;
        if (qj < 0 || qj >= H) continue;
        for (int di = -r; di <= r; di++) {
            const int qi = i + di;
            if (qi < 0 || qi >= W) continue;
            const float zqf = z(qi, qj);
            if (!fe_sf_liquid(zqf)) continue;
            const double s2 = (double)(di * di + dj * dj) / rr;
            if (s2 >= 1.0) continue;
            const double zq = (double)zqf;
            const double dz = (zq - zp) / range;
            const double dz2 = dz * dz;
            if (dz2 >= 1.0) continue;
            const double a = 1.0 - s2, b = 1.0 - dz2;
            const double w = (a * a) * (b * b);
            num = num + w * zq;
            den = den + w;
        }
    }
    return (float)(num / den);
}

// d of pixel (i, j): the ray of the scene section, not normalised (t is the depth along fwd)
__host__ __device__ inline void fe_sf_ray(const FeRenderCamera& cam, int i, int j, double* d) {
#pragma clang fp contract(off)
    const double a = (((double)i + 0.5) - 0.5 * (double)cam.width) / cam.focal;
    const double b = (((double)j + 0.5) - 0.5 * (double)cam.height) / cam.focal;
    for (int c = 0; c < 3; c++) d[c] = (cam.fwd[c] + a * cam.right[c]) - b * cam.up[c];
}
// The tangent along one image direction: zm / zp are the smoothed depths of the neighbours at -1 / +1 (+inf: outside the image or not liquid),
// dm / dp their rays.  The neighbour with |z_n - z| < range and the smaller |z_n - z| (a tie: +1) gives P(neighbour) - P; with none, the pixel's
// own depth on the ray at +1.
__host__ __device__ inline void fe_sf_tangent(const FeRenderCamera& cam, double z, const double* d, float zm, float zp, const double* dm, const double* dp, double range, double* t) {
#pragma clang fp contract(off)
    double am = -1.0, ap = -1.0;                             // |z_n - z| of a usable neighbour, -1: none
    if (fe_sf_liquid(zm)) { double a = (double)zm - z; if (a < 0.0) a = 0.0 - a; if (a < range) am = a; }
    if (fe_sf_liquid(zp)) { double a = (double)zp - z; if (a < 0.0) a = 0.0 - a; if (a < range) ap = a; }
    double zn = z;
    const double* dn = dp;
    if (ap >= 0.0 && (am < 0.0 || ap <= am)) zn = (double)zp;
    else if (am >= 0.0) { zn = (double)zm; dn = dm; }
    for (int c = 0; c < 3; c++) t[c] = (cam.pos[c] + zn * dn[c]) - (cam.pos[c] + z * d[c]);
}
// The colour of the liquid pixel (i, j): zs = {centre, x - 1, x + 1, y - 1, y + 1} smoothed depths (+inf as above), base the colour bytes of the
// layer's winning particle, word the pixel's thickness word, behind the opaque layer's bytes.  out[0..2]; alpha is the caller's.
__host__ __device__ inline void fe_sf_shade(const FeRenderCamera& cam, const FeRenderLights& L, const FeSurfaceParams& S, int i, int j, const float* zs,
                                            const unsigned char* base, unsigned long long word, const unsigned char* behind, unsigned char* out) {
#pragma clang fp contract(off)
    const double z = (double)zs[0];
    double d[3], dxm[3], dxp[3], dym[3], dyp[3], tx[3], ty[3], n[3], P[3];
    fe_sf_ray(cam, i, j, d);
    fe_sf_ray(cam, i - 1, j, dxm); fe_sf_ray(cam, i + 1, j, dxp);
    fe_sf_ray(cam, i, j - 1, dym); fe_sf_ray(cam, i, j + 1, dyp);
    fe_sf_tangent(cam, z, d, zs[1], zs[2], dxm, dxp, S.range, tx);
    fe_sf_tangent(cam, z, d, zs[3], zs[4], dym, dyp, S.range, ty);
    n[0] = ty[1] * tx[2] - ty[2] * tx[1];
    n[1] = ty[2] * tx[0] - ty[0] * tx[2];
    n[2] = ty[0] * tx[1] - ty[1] * tx[0];
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (len > 0.0 && len < 1e300) { n[0] = n[0] / len; n[1] = n[1] / len; n[2] = n[2] / len; }
    else { n[0] = 0.0 - cam.fwd[0]; n[1] = 0.0 - cam.fwd[1]; n[2] = 0.0 - cam.fwd[2]; }
    if ((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2] > 0.0) { n[0] = 0.0 - n[0]; n[1] = 0.0 - n[1]; n[2] = 0.0 - n[2]; }
    const double dl = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);      // (>= 1: d = fwd + something orthogonal to it)
    double diff[3], spec[3];
    for (int c = 0; c < 3; c++) { P[c] = cam.pos[c] + z * d[c]; diff[c] = L.ambient[c]; spec[c] = 0.0; }
    for (int k = 0; k < L.n_lights; k++) {
        double l[3] = {L.pos[k][0] - P[0], L.pos[k][1] - P[1], L.pos[k][2] - P[2]};
        const double ll = sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]);
        if (!(ll > 0.0)) continue;
        l[0] = l[0] / ll; l[1] = l[1] / ll; l[2] = l[2] / ll;
        const double ndl = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2];
        if (ndl > 0.0)
            for (int c = 0; c < 3; c++) diff[c] = diff[c] + L.color[k][c] * ndl;
        const double hv[3] = {l[0] - d[0] / dl, l[1] - d[1] / dl, l[2] - d[2] / dl};
        const double hl = sqrt((hv[0] * hv[0] + hv[1] * hv[1]) + hv[2] * hv[2]);
        if (!(hl > 0.0)) continue;
        double s = ((n[0] * hv[0] + n[1] * hv[1]) + n[2] * hv[2]) / hl;
        if (!(s > 0.0)) continue;
        for (int q = 0; q < S.shininess_log2; q++) s = s * s;
        for (int c = 0; c < 3; c++) spec[c] = spec[c] + L.color[k][c] * s;
    }
    const double t = (double)word / FE_SURFACE_FIX;
    const double at = S.absorb * t;
    const double alpha = S.alpha_min + ((1.0 - S.alpha_min) * at) / (1.0 + at);
    for (int c = 0; c < 3; c++) {
        const double lit = ((double)base[c] / 255.0) * diff[c] + S.specular * spec[c];
        out[c] = fe_rd_byte(lit * alpha + ((double)behind[c] / 255.0) * (1.0 - alpha));
    }
}

#ifndef FE_RENDER_MATH_ONLY

// Step 1, the particles of the opaque layer: k_render_splat with the selected particles left out (the same words for the rest).
struct SurfaceOpaqueArgs { int N; unsigned Np; float* fr; const int* pid_of_slot; const unsigned char* sel; FeRenderCamera cam; double R; int lane_pixels, stride; unsigned long long* pix; };
template <int TAIL> __global__ __launch_bounds__(FE_RENDER_WG) void k_surface_opaque(SurfaceOpaqueArgs a) {
    const FrameV fr = frame_view(a.fr, a.Np);
    const int rounds = (a.N + FE_RENDER_WG - 1) / FE_RENDER_WG;
    for (int r = blockIdx.x; r < rounds; r += a.stride) {    // (uniform; stride = the number of workgroups launched)
        const int s = r * FE_RENDER_WG + (int)threadIdx.x;
        bool have = false;
        int pid = -1;
        float x[3] = {0.f, 0.f, 0.f};
        FeRenderSphere sp;
        if (s < a.N) {
            pid = a.pid_of_slot[s];
            if ((unsigned)pid < (unsigned)a.N && fr.used[s] != 0 && a.sel[pid] == 0) {
                const float4 a0 = fr.A0[s];
                x[0] = a0.x; x[1] = a0.y; x[2] = a0.z;
                have = fe_rd_project(a.cam, x, a.R, sp) && fe_rd_box_pixels(sp) > 0;
            }
        }
        fe_rd_splat_wave(a.cam, have, sp, x, a.R, pid, a.lane_pixels, a.pix);
    }
}

// Step 2, the liquid layer: every selected used particle with radius Rs.  A fragment counts when it lies in front of the opaque picture's depth
// at its pixel (+inf on background; that picture is finished: stream order); it lowers the pixel's word of `liq` and adds its chord to `thick`.
// Each road visits every pixel of a box once, so both add the same integers.  (i, j) lies inside the clipped box, that is inside the image.
struct SurfaceSplatArgs { int N; unsigned Np; float* fr; const int* pid_of_slot; const unsigned char* sel; FeRenderCamera cam; double Rs; int lane_pixels, stride;
                          const float* opaque; unsigned long long* liq; unsigned long long* thick; };
__device__ __forceinline__ void fe_sf_emit(const FeRenderSphere& sp, int id, int i, int j, int W, const float* __restrict__ opaque, unsigned long long* liq, unsigned long long* thick) {
    FeRenderFrag fr;
    if (!fe_rd_fragment(sp, i, j, fr)) return;
    const size_t p = (size_t)j * (size_t)W + (size_t)i;
    if (!(fr.depth < opaque[p])) return;
    const unsigned long long key = fe_rd_key(fr.depth, id);
    if (key < __atomic_load_n(liq + p, __ATOMIC_RELAXED)) atomicMin(liq + p, key);
    const unsigned long long q = fe_sf_thick(sp.R, fr.nz);
    if (q != 0ull) atomicAdd(thick + p, q);
}
template <int TAIL> __global__ __launch_bounds__(FE_RENDER_WG) void k_surface_splat(SurfaceSplatArgs a) {
    const FrameV fr = frame_view(a.fr, a.Np);
    const int rounds = (a.N + FE_RENDER_WG - 1) / FE_RENDER_WG;
    const int lane = (int)(threadIdx.x & 63u);
    for (int r = blockIdx.x; r < rounds; r += a.stride) {    // (uniform)
        const int s = r * FE_RENDER_WG + (int)threadIdx.x;
        bool have = false;
        int pid = -1;
        float x[3] = {0.f, 0.f, 0.f};
        FeRenderSphere mine;
        if (s < a.N) {
            pid = a.pid_of_slot[s];
            if ((unsigned)pid < (unsigned)a.N && fr.used[s] != 0 && a.sel[pid] != 0) {
                const float4 a0 = fr.A0[s];
                x[0] = a0.x; x[1] = a0.y; x[2] = a0.z;
                have = fe_rd_project(a.cam, x, a.Rs, mine) && fe_rd_box_pixels(mine) > 0;
            }
        }
        const long long npx = have ? fe_rd_box_pixels(mine) : 0;
        const bool big = npx > (long long)a.lane_pixels;
        if (have && !big) {                                   // the lane road
            for (int j = mine.j0; j <= mine.j1; j++)
                for (int i = mine.i0; i <= mine.i1; i++) fe_sf_emit(mine, pid, i, j, a.cam.width, a.opaque, a.liq, a.thick);
        }
        unsigned long long m = __ballot(big);
        while (m) {                                           // (uniform) the wave road: one large sphere at a time, its box strided over the 64 lanes
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            const float xs[3] = {__shfl(x[0], src), __shfl(x[1], src), __shfl(x[2], src)};
            const int ids = __shfl(pid, src);
            FeRenderSphere sp;
            if (!fe_rd_project(a.cam, xs, a.Rs, sp)) continue;      // (the same words give the same sphere as in lane src: never taken)
            const int w = fe_rd_box_w(sp);
            const int cnt = w * fe_rd_box_h(sp);
            for (int k = lane; k < cnt; k += 64) fe_sf_emit(sp, ids, sp.i0 + k % w, sp.j0 + k / w, a.cam.width, a.opaque, a.liq, a.thick);
        }
    }
}

// The raw depth image of the liquid layer: the depth of each pixel's word, +inf where there is none.  One thread per pixel.
struct SurfaceDepthArgs { int n_pix; const unsigned long long* liq; float* z; };
template <int TAIL> __global__ __launch_bounds__(FE_RENDER_WG) void k_surface_depth(SurfaceDepthArgs a) {
    const int p = blockIdx.x * FE_RENDER_WG + (int)threadIdx.x;
    if (p >= a.n_pix) return;
    const unsigned long long key = a.liq[p];
    a.z[p] = key == FE_RENDER_BG ? __builtin_inff() : fe_rd_key_depth(key);
}

// Step 3, one smoothing pass: a 16 x 16 tile per workgroup (thread t owns pixel (t % 16, t / 16) of it), the tile and its halo of r pixels staged
// in LDS by one cooperative load, out-of-image entries +inf.  The sums of fe_sf_smooth run in a fixed order per pixel: the result does not
// depend on the tiling.
struct SurfaceSmoothArgs { int W, H, r, tiles_x; double range; const float* src; float* dst; };
struct SurfaceTileZ {
    const float* t; int i0, j0, side;                        // the LDS tile: entry (0, 0) is pixel (i0, j0)
    __device__ __forceinline__ float operator()(int qi, int qj) const { return t[(qj - j0) * side + (qi - i0)]; }
};
template <int TAIL> __global__ __launch_bounds__(FE_RENDER_WG) void k_surface_smooth(SurfaceSmoothArgs a) {
    __shared__ float tile[(FE_SURFACE_TILE + 2 * FE_SURFACE_MAX_R) * (FE_SURFACE_TILE + 2 * FE_SURFACE_MAX_R)];
    const int tid = (int)threadIdx.x;
    const int r = a.r < 0 ? 0 : (a.r > FE_SURFACE_MAX_R ? FE_SURFACE_MAX_R : a.r);      // (the tile holds no more)
    const int side = FE_SURFACE_TILE + 2 * r;
    const int ti = (int)blockIdx.x % a.tiles_x, tj = (int)blockIdx.x / a.tiles_x;
    const int i0 = ti * FE_SURFACE_TILE - r, j0 = tj * FE_SURFACE_TILE - r;
    for (int e = tid; e < side * side; e += FE_RENDER_WG) {
        const int qi = i0 + e % side, qj = j0 + e / side;
        tile[e] = (qi >= 0 && qi < a.W && qj >= 0 && qj < a.H) ? a.src[(size_t)qj * (size_t)a.W + (size_t)qi] : __builtin_inff();
    }
    __syncthreads();
    const int i = ti * FE_SURFACE_TILE + tid % FE_SURFACE_TILE, j = tj * FE_SURFACE_TILE + tid / FE_SURFACE_TILE;
    if (i >= a.W || j >= a.H) return;
    const SurfaceTileZ z = {tile, i0, j0, side};
    const float zp = z(i, j);
    a.dst[(size_t)j * (size_t)a.W + (size_t)i] = fe_sf_liquid(zp) ? fe_sf_smooth(z, i, j, a.W, a.H, r, a.range, zp) : __builtin_inff();
}

// Step 4, shade and composite: one thread per pixel.  A pixel with a word in `liq` whose id is a particle's is blended over the opaque picture
// and takes the layer's depth and id; every other pixel keeps the opaque picture's bytes.
struct SurfaceShadeArgs { int N; FeRenderCamera cam; FeRenderLights lights; FeSurfaceParams S; const unsigned* colors; const unsigned long long* liq; const unsigned long long* thick;
                          const float* z; unsigned* rgba; float* depth; int* ids; };
template <int TAIL> __global__ __launch_bounds__(FE_RENDER_WG) void k_surface_shade(SurfaceShadeArgs a) {
    const int W = a.cam.width, H = a.cam.height;
    const int p = blockIdx.x * FE_RENDER_WG + (int)threadIdx.x;
    if (p >= W * H) return;
    const unsigned long long key = a.liq[p];
    if (key == FE_RENDER_BG) return;
    const int kid = fe_rd_key_id(key);
    if (kid < 0 || kid >= a.N) return;                       // (never: only particle ids are splatted into liq)
    const int i = p % W, j = p / W;
    const float inf = __builtin_inff();
    const float zs[5] = {a.z[p], i > 0 ? a.z[p - 1] : inf, i + 1 < W ? a.z[p + 1] : inf, j > 0 ? a.z[p - W] : inf, j + 1 < H ? a.z[p + W] : inf};
    if (!fe_sf_liquid(zs[0])) return;                        // (never: a pixel with a word has a depth)
    const unsigned col = a.colors[kid], old = a.rgba[p];
    const unsigned char base[3] = {(unsigned char)(col & 0xffu), (unsigned char)((col >> 8) & 0xffu), (unsigned char)((col >> 16) & 0xffu)};
    const unsigned char behind[3] = {(unsigned char)(old & 0xffu), (unsigned char)((old >> 8) & 0xffu), (unsigned char)((old >> 16) & 0xffu)};
    unsigned char out[3];
    fe_sf_shade(a.cam, a.lights, a.S, i, j, zs, base, a.thick[p], behind, out);
    a.rgba[p] = (unsigned)out[0] | ((unsigned)out[1] << 8) | ((unsigned)out[2] << 16) | 0xff000000u;
    a.depth[p] = zs[0];
    a.ids[p] = kid;
}

// fe_surface_get_dev: the thickness words as lengths (word / 2^32: exact in fp64 below 2^53)
struct SurfaceThickArgs { int n_pix; const unsigned long long* words; double* out; };
template <int TAIL> __global__ __launch_bounds__(FE_RENDER_WG) void k_surface_thickness(SurfaceThickArgs a) {
    const int p = blockIdx.x * FE_RENDER_WG + (int)threadIdx.x;
    if (p < a.n_pix) a.out[p] = (double)a.words[p] / FE_SURFACE_FIX;
}

// ---------------------------------------------------------------------------------------------------------------- host
struct SurfaceState {
    unsigned char* sel = nullptr;                            // [N] by particle id on the device (allocated by the first fe_surface_set with a selection)
    bool on = false;                                         // a selection with at least one particle is set
    FeSurfaceParams P;
    size_t n_pix = 0;                                        // pixels the five images below hold
    unsigned long long* liq = nullptr; unsigned long long* thick = nullptr;
    float* z_raw = nullptr; float* z_a = nullptr; float* z_b = nullptr;
    const float* z_smooth = nullptr;                         // where the last fe_surface_frame left the smoothed depth (z_raw with smooth_iters == 0)
    bool drawn = false;                                      // fe_surface_frame has drawn a surface since the last fe_render_setup
    SurfaceState() { P = FeSurfaceParams(); }
};
static void surface_free_images(FeEngine* h, SurfaceState* Q) {
    render_free(h, Q->liq, Q->n_pix); render_free(h, Q->thick, Q->n_pix);
    render_free(h, Q->z_raw, Q->n_pix); render_free(h, Q->z_a, Q->n_pix); render_free(h, Q->z_b, Q->n_pix);
    Q->n_pix = 0; Q->z_smooth = nullptr; Q->drawn = false;
}
static void surface_drop(FeEngine* h) {                      // fe_destroy
    SurfaceState* Q = h->surface;
    if (!Q) return;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    surface_free_images(h, Q);
    render_free(h, Q->sel, (size_t)h->N);
    delete Q;
    h->surface = nullptr;
}
static void surface_invalidate(FeEngine* h) {                // fe_render_setup: the pictures of the old camera are gone
    if (h->surface) h->surface->drawn = false;
}
// the five images for the renderer's current size, built aside: a failure leaves the old ones
static int surface_images(FeEngine* h, SurfaceState* Q) {
    const size_t n_pix = (size_t)h->render->cam.width * (size_t)h->render->cam.height;
    if (Q->liq && Q->n_pix == n_pix) return 0;
    unsigned long long* liq = nullptr; unsigned long long* thick = nullptr; float* z_raw = nullptr; float* z_a = nullptr; float* z_b = nullptr;
    if (dev_alloc(h, &liq, n_pix, false) || dev_alloc(h, &thick, n_pix, false) || dev_alloc(h, &z_raw, n_pix, false) || dev_alloc(h, &z_a, n_pix, false) ||
        dev_alloc(h, &z_b, n_pix, false) || hipStreamSynchronize(h->stream) != hipSuccess) {      // (an earlier picture may still be in flight)
        render_free(h, liq, n_pix); render_free(h, thick, n_pix); render_free(h, z_raw, n_pix); render_free(h, z_a, n_pix); render_free(h, z_b, n_pix);
        if (h->err.empty()) h->err = "fe_surface: allocation failed (the previous buffers stay)";
        return 1;
    }
    surface_free_images(h, Q);
    Q->liq = liq; Q->thick = thick; Q->z_raw = z_raw; Q->z_a = z_a; Q->z_b = z_b; Q->n_pix = n_pix;
    return 0;
}
// The launches, defined at the end of fe_engine.hip behind every other first use of a template kernel (see the head of this file)
static void surface_launch_opaque(FeEngine* h, int f);       // the particle splat of fe_render_frame with the selection left out
static void surface_launch_layer(FeEngine* h, int f);        // steps 2 to 4 on top of a finished opaque picture
static void surface_launch_thickness(FeEngine* h, double* out);

static bool surface_unit(double v) { return std::isfinite(v) && v >= 0.0 && v <= 1.0; }

extern "C" {

int fe_surface_set(FeEngine* h, const unsigned char* sel, const FeSurfaceParams* params, int params_size) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (!h->render) FAIL(h, "fe_surface_set: no renderer: fe_render_setup first");
    if (!sel) {
        if (h->surface) h->surface->on = false;
        return 0;
    }
    if (!params || params_size != (int)sizeof(FeSurfaceParams)) FAIL(h, "fe_surface_set: FeSurfaceParams size mismatch (the surface is unchanged)");
    const FeSurfaceParams& p = *params;
    if (!std::isfinite(p.radius_scale) || p.radius_scale < 1.0) FAIL(h, "fe_surface_set: radius_scale must be finite and >= 1 (the surface is unchanged)");
    if (p.smooth_iters < 0 || p.smooth_iters > 8) FAIL(h, "fe_surface_set: smooth_iters must be in [0, 8] (the surface is unchanged)");
    if (p.smooth_radius_px < 1 || p.smooth_radius_px > FE_SURFACE_MAX_R) FAIL(h, "fe_surface_set: smooth_radius_px must be in [1, 8] (the surface is unchanged)");
    if (!render_pos(p.range)) FAIL(h, "fe_surface_set: range must be finite and positive (the surface is unchanged)");
    if (!std::isfinite(p.absorb) || p.absorb < 0.0) FAIL(h, "fe_surface_set: absorb must be finite and >= 0 (the surface is unchanged)");
    if (!surface_unit(p.alpha_min)) FAIL(h, "fe_surface_set: alpha_min must be in [0, 1] (the surface is unchanged)");
    if (!surface_unit(p.specular)) FAIL(h, "fe_surface_set: specular must be in [0, 1] (the surface is unchanged)");
    if (p.shininess_log2 < 0 || p.shininess_log2 > 10) FAIL(h, "fe_surface_set: shininess_log2 must be in [0, 10] (the surface is unchanged)");
    bool any = false;
    for (int i = 0; i < h->N; i++) any = any || sel[i] != 0;
    SurfaceState* Q = h->surface;
    if (!any) {                                               // an empty selection: off, nothing allocated for it
        if (Q) Q->on = false;
        return 0;
    }
    unsigned char* d = nullptr;
    if (dev_alloc(h, &d, (size_t)h->N, false)) return 1;
    if (hipMemcpyOnStream(h, d, sel, (size_t)h->N, hipMemcpyHostToDevice) != hipSuccess) { render_free(h, d, (size_t)h->N); FAIL(h, "fe_surface_set: hipMemcpy failed (the surface is unchanged)"); }
    if (!Q) Q = h->surface = new SurfaceState();
    if (surface_images(h, Q)) { render_free(h, d, (size_t)h->N); h->err = "fe_surface_set: " + h->err + " (the surface is unchanged)"; return 1; }
    render_free(h, Q->sel, (size_t)h->N);                    // (the stream has drained: hipMemcpyOnStream)
    Q->sel = d; Q->P = p; Q->P.pad = 0; Q->on = true;
    return 0;
}

int fe_surface_frame(FeEngine* h, int f, int s) {
    if (!h) return 1;
    FE_ENTRY(h);
    RenderState* R = h->render;
    if (!R) FAIL(h, "fe_surface_frame: no renderer: fe_render_setup first");
    SurfaceState* Q = h->surface;
    if (!Q || !Q->on) {                                       // off: exactly fe_render_scene_frame, and no surface picture from here on
        if (render_scene_frame_with(h, f, s, false)) return 1;
        if (Q) Q->drawn = false;
        return 0;
    }
    // the thickness word of a pixel holds at most N chords of 2 Rs 2^32 each
    const double Rs = Q->P.radius_scale * R->R;
    if (!(2.0 * Rs * (double)h->N < 2147483648.0)) FAIL(h, "fe_surface_frame: radius_scale * radius is too large for the thickness words");
    if (surface_images(h, Q)) return 1;                      // (fe_render_setup has changed the image since fe_surface_set)
    if (render_scene_frame_with(h, f, s, true)) return 1;
    surface_launch_layer(h, f);
    Q->drawn = true;
    return check_async(h);
}

static int surface_copy(FeEngine* h, const char* who, float* z_raw, float* z_smooth, double* thickness, bool to_host) {
    RenderState* R = h->render;
    SurfaceState* Q = h->surface;
    if (!R) { h->err = std::string(who) + ": no renderer: fe_render_setup first"; return 1; }
    if (!Q || !Q->drawn || !R->drawn) { h->err = std::string(who) + ": no surface picture: fe_surface_frame with a selection first"; return 1; }
    const size_t n_pix = Q->n_pix;
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (z_raw) HIPCK(h, hipMemcpyAsync(z_raw, Q->z_raw, sizeof(float) * n_pix, kind, h->stream));
    if (z_smooth) HIPCK(h, hipMemcpyAsync(z_smooth, Q->z_smooth, sizeof(float) * n_pix, kind, h->stream));
    if (thickness) {
        if (to_host) {                                        // the words, decoded here: word / 2^32 is exact in fp64 below 2^53
            std::vector<unsigned long long> words(n_pix);
            HIPCK(h, hipMemcpyAsync(words.data(), Q->thick, sizeof(unsigned long long) * n_pix, kind, h->stream));
            HIPCK(h, hipStreamSynchronize(h->stream));
            for (size_t p = 0; p < n_pix; p++) thickness[p] = (double)words[p] / FE_SURFACE_FIX;
        } else surface_launch_thickness(h, thickness);
    }
    return 0;
}
int fe_surface_get(FeEngine* h, float* z_raw, float* z_smooth, double* thickness) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (surface_copy(h, "fe_surface_get", z_raw, z_smooth, thickness, true)) return 1;
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    return check_device_errors(h);
}
int fe_surface_get_dev(FeEngine* h, float* z_raw, float* z_smooth, double* thickness) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (surface_copy(h, "fe_surface_get_dev", z_raw, z_smooth, thickness, false)) return 1;
    return check_async(h);
}

}  // extern "C"
#endif /* FE_RENDER_MATH_ONLY */
#endif /* FE_SURFACE_H */
