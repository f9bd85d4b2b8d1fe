// fe_render.h -- the headless particle renderer (include/fluidengine_ext.h: fe_render_*).  Included by fe_engine.hip after every other piece of
// device code, so that the kernels here come last in the code object and the substep kernels keep their place.
// The first part -- projection of one sphere, its clipped box, one fragment, the pixel word and the shading of one pixel -- is plain
// __host__ __device__ code: tests/csrc/render_test.cpp compiles it for the host with FE_RENDER_MATH_ONLY defined and checks it against plain loops.
//
// Everything is fp64 formed from the fp32 position words with + - * / and sqrt, under fp contract(off): no fused multiply-add, nothing that
// rounds differently on the host, the device or in a restatement that performs the same operations in the same order (tests/render_ref.py).
// A pixel is one unsigned 64-bit word, (bits of the fp32 depth << 32) | id, lowered with integer atomicMin: positive floats order like their
// bits, so the smallest word is the nearest fragment and, among equal depths, the lowest id.  No floating-point atomics: an image does not
// depend on launch order.
#ifndef FE_RENDER_H
#define FE_RENDER_H

#define FE_RENDER_BG 0xffffffffffffffffull                  /* the background word */

// One projected sphere: what a fragment and the shading need of it.
struct FeRenderSphere {
    double x[3], R;                                          // centre (widened fp32 words) and world radius
    double zc, px, py, rp;                                   // depth along fwd, centre in pixels, radius in pixels (clamped)
    int i0, i1, j0, j1;                                      // the box clipped to the image, inclusive; empty when i0 > i1 or j0 > j1
    int ci, cj;                                              // the pixel that contains (px, py) (may lie outside the image)
};
struct FeRenderFrag { double u, v, nz; float depth; };

__host__ __device__ inline bool fe_rd_finite(float v) { return v - v == 0.0f; }
__host__ __device__ inline double fe_rd_floor(double a) {   // (a is finite and |a| < 2^31 wherever this is called)
    const double t = (double)(long long)a;
    return t > a ? t - 1.0 : t;
}
__host__ __device__ inline double fe_rd_ceil(double a) {
    const double t = (double)(long long)a;
    return t < a ? t + 1.0 : t;
}
__host__ __device__ inline double fe_rd_clampd(double a, double lo, double hi) { return a < lo ? lo : (a > hi ? hi : a); }

// false: the sphere draws nothing (a non-finite word, or not in front of near + R).  The box may still be empty (off the image).
__host__ __device__ inline bool fe_rd_project(const FeRenderCamera& cam, const float* xf, double R, FeRenderSphere& sp) {
#pragma clang fp contract(off)
    if (!fe_rd_finite(xf[0]) || !fe_rd_finite(xf[1]) || !fe_rd_finite(xf[2])) return false;
    const double W = (double)cam.width, H = (double)cam.height;
    sp.x[0] = (double)xf[0]; sp.x[1] = (double)xf[1]; sp.x[2] = (double)xf[2]; sp.R = R;
    const double d0 = sp.x[0] - cam.pos[0], d1 = sp.x[1] - cam.pos[1], d2 = sp.x[2] - cam.pos[2];
    const double zc = (d0 * cam.fwd[0] + d1 * cam.fwd[1]) + d2 * cam.fwd[2];
    const double xc = (d0 * cam.right[0] + d1 * cam.right[1]) + d2 * cam.right[2];
    const double yc = (d0 * cam.up[0] + d1 * cam.up[1]) + d2 * cam.up[2];
    if (!(zc > cam.near + R)) return false;
    sp.zc = zc;
    sp.px = 0.5 * W + (cam.focal * xc) / zc;
    sp.py = 0.5 * H - (cam.focal * yc) / zc;
    double rp = (cam.focal * R) / zc;
    if (rp > cam.max_radius_px) rp = cam.max_radius_px;
    sp.rp = rp;
    // (clamped in fp64 before the conversion: px may be far outside the image)
    sp.i0 = (int)fe_rd_floor(fe_rd_clampd((sp.px - rp) - 0.5, 0.0, W));
    sp.i1 = (int)fe_rd_ceil(fe_rd_clampd((sp.px + rp) - 0.5, -1.0, W - 1.0));
    sp.j0 = (int)fe_rd_floor(fe_rd_clampd((sp.py - rp) - 0.5, 0.0, H));
    sp.j1 = (int)fe_rd_ceil(fe_rd_clampd((sp.py + rp) - 0.5, -1.0, H - 1.0));
    sp.ci = (int)fe_rd_floor(fe_rd_clampd(sp.px, -1.0, W));
    sp.cj = (int)fe_rd_floor(fe_rd_clampd(sp.py, -1.0, H));
    return true;
}
__host__ __device__ inline int fe_rd_box_w(const FeRenderSphere& sp) { return sp.i1 >= sp.i0 ? sp.i1 - sp.i0 + 1 : 0; }
__host__ __device__ inline int fe_rd_box_h(const FeRenderSphere& sp) { return sp.j1 >= sp.j0 ? sp.j1 - sp.j0 + 1 : 0; }
__host__ __device__ inline long long fe_rd_box_pixels(const FeRenderSphere& sp) { return (long long)fe_rd_box_w(sp) * fe_rd_box_h(sp); }

// The fragment of the sphere at pixel (i, j) of its box; false: not covered.
__host__ __device__ inline bool fe_rd_fragment(const FeRenderSphere& sp, int i, int j, FeRenderFrag& fr) {
#pragma clang fp contract(off)
    const double u = (((double)i + 0.5) - sp.px) / sp.rp;
    const double v = (((double)j + 0.5) - sp.py) / sp.rp;
    double s = u * u + v * v;
    bool covered = s <= 1.0;
    if (i == sp.ci && j == sp.cj) {                          // the pixel of the centre: always covered
        covered = true;
        if (!(s <= 1.0)) s = 1.0;
    }
    if (!covered) return false;
    fr.u = u; fr.v = v;
    fr.nz = sqrt(1.0 - s);
    fr.depth = (float)(sp.zc - sp.R * fr.nz);               // (> near > 0: a positive float)
    return true;
}
__host__ __device__ inline unsigned fe_rd_float_bits(float f) {
    union { float f; unsigned u; } c; c.f = f; return c.u;
}
__host__ __device__ inline float fe_rd_bits_float(unsigned u) {
    union { float f; unsigned u; } c; c.u = u; return c.f;
}
__host__ __device__ inline unsigned long long fe_rd_key(float depth, int id) { return ((unsigned long long)fe_rd_float_bits(depth) << 32) | (unsigned long long)(unsigned)id; }
__host__ __device__ inline int fe_rd_key_id(unsigned long long key) { return (int)(unsigned)(key & 0xffffffffull); }
__host__ __device__ inline float fe_rd_key_depth(unsigned long long key) { return fe_rd_bits_float((unsigned)(key >> 32)); }

__host__ __device__ inline unsigned char fe_rd_byte(double c) {
#pragma clang fp contract(off)
    if (!(c >= 0.0)) c = 0.0;
    if (c > 1.0) c = 1.0;
    return (unsigned char)(int)(c * 255.0 + 0.5);
}
// The colour of the fragment fr of sphere sp with base colour base[3] (bytes): out[0..2], alpha is the caller's.
__host__ __device__ inline void fe_rd_shade(const FeRenderCamera& cam, const FeRenderLights& L, const FeRenderSphere& sp, const FeRenderFrag& fr,
                                            const unsigned char* base, unsigned char* out) {
#pragma clang fp contract(off)
    double n[3], P[3], acc[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        n[a] = (fr.u * cam.right[a] - fr.v * cam.up[a]) - fr.nz * cam.fwd[a];
        P[a] = sp.x[a] + sp.R * n[a];
        acc[a] = L.ambient[a];
    }
    for (int k = 0; k < L.n_lights; k++) {
        const double l0 = L.pos[k][0] - P[0], l1 = L.pos[k][1] - P[1], l2 = L.pos[k][2] - P[2];
        const double len = sqrt((l0 * l0 + l1 * l1) + l2 * l2);
        if (!(len > 0.0)) continue;
        const double ndl = ((n[0] * l0 + n[1] * l1) + n[2] * l2) / len;
        if (!(ndl > 0.0)) continue;
#pragma unroll
        for (int a = 0; a < 3; a++) acc[a] = acc[a] + L.color[k][a] * ndl;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) out[a] = fe_rd_byte(((double)base[a] / 255.0) * acc[a]);
}

#ifndef FE_RENDER_MATH_ONLY
#define FE_RENDER_WG 256
#define FE_RENDER_MAX_WGS 2048

// what the kernels need of the static point sets: id_base[k] .. id_base[k] + n[k] are the ids of set k
struct RenderSets {
    const float* xyz[FE_RENDER_MAX_SETS]; int n[FE_RENDER_MAX_SETS]; int id_base[FE_RENDER_MAX_SETS];
    double R[FE_RENDER_MAX_SETS]; unsigned rgba[FE_RENDER_MAX_SETS];
};

__global__ __launch_bounds__(FE_RENDER_WG) void k_render_clear(int n_pix, unsigned long long* __restrict__ pix) {
    for (int p = blockIdx.x * FE_RENDER_WG + threadIdx.x; p < n_pix; p += gridDim.x * FE_RENDER_WG) pix[p] = FE_RENDER_BG;
}

// One fragment: a load first, the atomic only when the key is smaller (words only ever decrease, so a stale load can only cost an
// atomic that changes nothing).  The load is a relaxed atomic one: other waves lower the word at the same time, and the compiler must
// neither tear nor keep it.  (i, j) lies inside the clipped box, that is inside the image.
__device__ __forceinline__ void fe_rd_emit(const FeRenderSphere& sp, int id, int i, int j, int W, unsigned long long* pix) {
    FeRenderFrag fr;
    if (!fe_rd_fragment(sp, i, j, fr)) return;
    const unsigned long long key = fe_rd_key(fr.depth, id);
    unsigned long long* p = pix + ((size_t)j * (size_t)W + (size_t)i);
    if (key < __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMin(p, key);
}
// The two roads for the sphere each lane holds (have: this lane has one with a non-empty box).  Called by all 64 lanes of a wave together.
__device__ __forceinline__ void fe_rd_splat_wave(const FeRenderCamera& cam, bool have, const FeRenderSphere& mine, const float* xmine, double R, int id, int lane_pixels,
                                                 unsigned long long* pix) {
    const long long npx = have ? fe_rd_box_pixels(mine) : 0;
    const bool big = npx > (long long)lane_pixels;
    if (have && !big) {
        for (int j = mine.j0; j <= mine.j1; j++)
            for (int i = mine.i0; i <= mine.i1; i++) fe_rd_emit(mine, id, i, j, cam.width, pix);
    }
    unsigned long long m = __ballot(big);
    const int lane = (int)(threadIdx.x & 63u);
    while (m) {                                               // (uniform) one large sphere at a time, its box strided over the 64 lanes
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        const float xs[3] = {__shfl(xmine[0], src), __shfl(xmine[1], src), __shfl(xmine[2], src)};
        const int ids = __shfl(id, src);
        FeRenderSphere sp;
        if (!fe_rd_project(cam, xs, R, sp)) continue;        // (the same words give the same sphere as in lane src: never taken)
        const int w = fe_rd_box_w(sp);
        const int cnt = w * fe_rd_box_h(sp);
        for (int k = lane; k < cnt; k += 64) fe_rd_emit(sp, ids, sp.i0 + k % w, sp.j0 + k / w, cam.width, pix);
    }
}

// The splat of frame f's particles: a grid-stride pass over the slots; id = the particle id of the slot.
__global__ __launch_bounds__(FE_RENDER_WG) void k_render_splat(int N, size_t Np, float* fr_, const int* __restrict__ pid_of_slot, FeRenderCamera cam, double R, int lane_pixels,
                                                               unsigned long long* pix) {
    const FrameV fr = frame_view(fr_, Np);
    const int rounds = (N + FE_RENDER_WG - 1) / FE_RENDER_WG;
    for (int r = blockIdx.x; r < rounds; r += gridDim.x) {   // (uniform: every lane of a wave makes the same rounds)
        const int s = r * FE_RENDER_WG + (int)threadIdx.x;
        bool have = false;
        int pid = -1;
        float x[3] = {0.f, 0.f, 0.f};
        FeRenderSphere sp;
        if (s < N) {
            pid = pid_of_slot[s];
            if ((unsigned)pid < (unsigned)N && fr.used[s] != 0) {
                const float4 a0 = fr.A0[s];
                x[0] = a0.x; x[1] = a0.y; x[2] = a0.z;
                have = fe_rd_project(cam, x, R, sp) && fe_rd_box_pixels(sp) > 0;
            }
        }
        fe_rd_splat_wave(cam, have, sp, x, R, pid, lane_pixels, pix);
    }
}
// The same for one static point set: id = id_base + the point's index.
__global__ __launch_bounds__(FE_RENDER_WG) void k_render_points(int n, const float* __restrict__ xyz, int id_base, FeRenderCamera cam, double R, int lane_pixels,
                                                                unsigned long long* pix) {
    const int rounds = (n + FE_RENDER_WG - 1) / FE_RENDER_WG;
    for (int r = blockIdx.x; r < rounds; r += gridDim.x) {
        const int s = r * FE_RENDER_WG + (int)threadIdx.x;
        bool have = false;
        float x[3] = {0.f, 0.f, 0.f};
        FeRenderSphere sp;
        if (s < n) {
            x[0] = xyz[3 * (size_t)s]; x[1] = xyz[3 * (size_t)s + 1]; x[2] = xyz[3 * (size_t)s + 2];
            have = fe_rd_project(cam, x, R, sp) && fe_rd_box_pixels(sp) > 0;
        }
        fe_rd_splat_wave(cam, have, sp, x, R, id_base + s, lane_pixels, pix);
    }
}

// One thread per pixel: the winning id's sphere again (a particle through the frame's own slot_of_pid, as k_obs_gather finds it), its
// fragment at this pixel, the colour.
__global__ __launch_bounds__(FE_RENDER_WG) void k_render_shade(int N, size_t Np, float* fr_, const int* __restrict__ slot_of_pid, FeRenderCamera cam, FeRenderLights lights,
                                                               double R, const unsigned* __restrict__ colors, RenderSets sets, const unsigned long long* __restrict__ pix,
                                                               unsigned* __restrict__ rgba, float* __restrict__ depth, int* __restrict__ ids) {
    const int n_pix = cam.width * cam.height;
    const int p = blockIdx.x * FE_RENDER_WG + (int)threadIdx.x;
    if (p >= n_pix) return;
    const unsigned long long key = pix[p];
    unsigned char out[3] = {fe_rd_byte(lights.background[0]), fe_rd_byte(lights.background[1]), fe_rd_byte(lights.background[2])};
    float dep = __builtin_inff();
    int id = -1;
    if (key != FE_RENDER_BG) {
        const int kid = fe_rd_key_id(key);
        float x[3] = {0.f, 0.f, 0.f};
        double Rs = R;
        unsigned col = 0u;
        bool found = false;
        if (kid >= 0 && kid < N) {
            const int s = slot_of_pid[kid];
            if ((unsigned)s < (unsigned)N) {
                const float4 a0 = frame_view(fr_, Np).A0[s];
                x[0] = a0.x; x[1] = a0.y; x[2] = a0.z;
                col = colors[kid];
                found = true;
            }
        } else {
#pragma unroll
            for (int k = 0; k < FE_RENDER_MAX_SETS; k++) {
                const int o = kid - sets.id_base[k];
                if (o >= 0 && o < sets.n[k]) {
                    x[0] = sets.xyz[k][3 * (size_t)o]; x[1] = sets.xyz[k][3 * (size_t)o + 1]; x[2] = sets.xyz[k][3 * (size_t)o + 2];
                    Rs = sets.R[k]; col = sets.rgba[k];
                    found = true;
                }
            }
        }
        FeRenderSphere sp;
        FeRenderFrag fr;
        const int i = p % cam.width, j = p / cam.width;
        if (found && fe_rd_project(cam, x, Rs, sp) && fe_rd_fragment(sp, i, j, fr)) {
            const unsigned char base[3] = {(unsigned char)(col & 0xffu), (unsigned char)((col >> 8) & 0xffu), (unsigned char)((col >> 16) & 0xffu)};
            fe_rd_shade(cam, lights, sp, fr, base, out);
            dep = fe_rd_key_depth(key);
            id = kid;
        }
    }
    rgba[p] = (unsigned)out[0] | ((unsigned)out[1] << 8) | ((unsigned)out[2] << 16) | 0xff000000u;
    depth[p] = dep;
    ids[p] = id;
}

// ---------------------------------------------------------------------------------------------------------------- host
struct RenderPointSet { int n = 0; float* xyz = nullptr; double R = 0.0; unsigned rgba = 0u; };
struct RenderState {
    FeRenderCamera cam; FeRenderLights lights;
    unsigned long long* pix = nullptr;                       // [H][W] pixel words
    unsigned* rgba = nullptr; float* depth = nullptr; int* ids = nullptr;     // [H][W] each: what k_render_shade writes
    unsigned* colors = nullptr; double R = 0.0;              // fe_render_set_colors: [N] by particle id
    RenderPointSet set[FE_RENDER_MAX_SETS];
    bool drawn = false;                                      // fe_render_frame has run since the last setup
};

// hipFree of a buffer dev_alloc gave, taken off the engine's byte count again (dev_alloc counts at least one element)
template <typename T>
static void render_free(FeEngine* h, T*& p, size_t count) {
    if (!p) return;
    (void)hipFree(p);
    const size_t bytes = count ? count * sizeof(T) : sizeof(T);
    h->bytes -= bytes < h->bytes ? bytes : h->bytes;
    p = nullptr;
}
static void render_drop(FeEngine* h) {                       // fe_destroy
    RenderState* R = h->render;
    if (!R) return;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    const size_t n_pix = (size_t)R->cam.width * (size_t)R->cam.height;
    render_free(h, R->pix, n_pix); render_free(h, R->rgba, n_pix); render_free(h, R->depth, n_pix); render_free(h, R->ids, n_pix);
    render_free(h, R->colors, (size_t)h->N);
    for (auto& S : R->set) render_free(h, S.xyz, (size_t)3 * S.n);
    delete R;
    h->render = nullptr;
}
static bool render_finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
static bool render_pos(double v) { return std::isfinite(v) && v > 0.0; }
// fe_surface.h (included behind fe_render_scene.h): what the two functions below need of it
static void surface_invalidate(FeEngine* h);                 // fe_render_setup: no surface picture any more
static void surface_launch_opaque(FeEngine* h, int f);       // the particle splat without the selected particles

extern "C" {

int fe_render_setup(FeEngine* h, const FeRenderCamera* camera, int camera_size, const FeRenderLights* lights, int lights_size) {
    FE_ENTRY(h);
    if (!camera || camera_size != (int)sizeof(FeRenderCamera)) FAIL(h, "fe_render_setup: FeRenderCamera size mismatch");
    if (!lights || lights_size != (int)sizeof(FeRenderLights)) FAIL(h, "fe_render_setup: FeRenderLights size mismatch");
    const FeRenderCamera& c = *camera;
    if (c.width < 1 || c.width > FE_RENDER_MAX_SIZE || c.height < 1 || c.height > FE_RENDER_MAX_SIZE) FAIL(h, "fe_render_setup: width and height must be in [1, 4096]");
    if (!render_pos(c.focal) || !render_pos(c.near) || !render_pos(c.max_radius_px)) FAIL(h, "fe_render_setup: focal, near and max_radius_px must be finite and positive");
    if (!render_finite3(c.pos) || !render_finite3(c.right) || !render_finite3(c.up) || !render_finite3(c.fwd)) FAIL(h, "fe_render_setup: the camera position or basis is not finite");
    const FeRenderLights& l = *lights;
    if (l.n_lights < 0 || l.n_lights > FE_RENDER_MAX_LIGHTS) FAIL(h, "fe_render_setup: n_lights must be in [0, FE_RENDER_MAX_LIGHTS]");
    bool ok = render_finite3(l.ambient) && render_finite3(l.background);
    for (int k = 0; k < l.n_lights; k++) ok = ok && render_finite3(l.pos[k]) && render_finite3(l.color[k]);
    if (!ok) FAIL(h, "fe_render_setup: a light, the ambient or the background colour is not finite");
    RenderState* R = h->render;
    const size_t n_pix = (size_t)c.width * (size_t)c.height;
    if (!R || (size_t)R->cam.width * (size_t)R->cam.height != n_pix) {       // (built aside: a failure leaves the old buffers as they were)
        unsigned long long* pix = nullptr; unsigned* rgba = nullptr; float* depth = nullptr; int* ids = nullptr;
        if (dev_alloc(h, &pix, n_pix, false) || dev_alloc(h, &rgba, n_pix) || dev_alloc(h, &depth, n_pix) || dev_alloc(h, &ids, n_pix) ||
            hipStreamSynchronize(h->stream) != hipSuccess) {  // (an earlier picture may still be in flight)
            render_free(h, pix, n_pix); render_free(h, rgba, n_pix); render_free(h, depth, n_pix); render_free(h, ids, n_pix);
            if (h->err.empty()) h->err = "fe_render_setup: allocation failed (the previous buffers stay)";
            return 1;
        }
        if (!R) R = h->render = new RenderState();
        else {
            const size_t old_pix = (size_t)R->cam.width * (size_t)R->cam.height;
            render_free(h, R->pix, old_pix); render_free(h, R->rgba, old_pix); render_free(h, R->depth, old_pix); render_free(h, R->ids, old_pix);
        }
        R->pix = pix; R->rgba = rgba; R->depth = depth; R->ids = ids;
    }
    R->cam = c; R->lights = l;
    for (int k = l.n_lights; k < FE_RENDER_MAX_LIGHTS; k++) for (int a = 0; a < 3; a++) R->lights.pos[k][a] = R->lights.color[k][a] = 0.0;
    R->drawn = false;
    surface_invalidate(h);
    return 0;
}

int fe_render_set_colors(FeEngine* h, const unsigned char* rgba, double radius) {
    FE_ENTRY(h);
    RenderState* R = h->render;
    if (!R) FAIL(h, "fe_render_set_colors: no renderer: fe_render_setup first");
    if (!rgba) FAIL(h, "fe_render_set_colors: null colours");
    if (!render_pos(radius)) FAIL(h, "fe_render_set_colors: the radius must be finite and positive");
    if (!R->colors && dev_alloc(h, &R->colors, (size_t)h->N, false)) return 1;
    if (h->N > 0 && hipMemcpyOnStream(h, R->colors, rgba, sizeof(unsigned) * (size_t)h->N, hipMemcpyHostToDevice) != hipSuccess) FAIL(h, "fe_render_set_colors: hipMemcpy failed");
    R->R = radius;
    return 0;
}

int fe_render_set_points(FeEngine* h, int set, const float* xyz, int n, const unsigned char* rgba, double radius) {
    FE_ENTRY(h);
    RenderState* R = h->render;
    if (!R) FAIL(h, "fe_render_set_points: no renderer: fe_render_setup first");
    if (set < 0 || set >= FE_RENDER_MAX_SETS) FAIL(h, "fe_render_set_points: set index out of range");
    if (n < 0) FAIL(h, "fe_render_set_points: n < 0 (the set is unchanged)");
    if (n > FE_RENDER_MAX_POINTS) FAIL(h, "fe_render_set_points: more than FE_RENDER_MAX_POINTS points (the set is unchanged)");
    RenderPointSet& S = R->set[set];
    if (!xyz || n == 0) {
        if (S.xyz) { HIPCK(h, hipStreamSynchronize(h->stream)); render_free(h, S.xyz, (size_t)3 * S.n); }
        S = RenderPointSet();
        return 0;
    }
    if (!rgba) FAIL(h, "fe_render_set_points: null colour (the set is unchanged)");
    if (!render_pos(radius)) FAIL(h, "fe_render_set_points: the radius must be finite and positive (the set is unchanged)");
    float* d = nullptr;
    if (dev_alloc(h, &d, (size_t)3 * n, false)) return 1;
    if (hipMemcpyOnStream(h, d, xyz, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) { render_free(h, d, (size_t)3 * n); FAIL(h, "fe_render_set_points: hipMemcpy failed (the set is unchanged)"); }
    render_free(h, S.xyz, (size_t)3 * S.n);                  // (the stream has drained: hipMemcpyOnStream)
    S.xyz = d; S.n = n; S.R = radius;
    S.rgba = (unsigned)rgba[0] | ((unsigned)rgba[1] << 8) | ((unsigned)rgba[2] << 16) | ((unsigned)rgba[3] << 24);
    return 0;
}

// The picture of frame f, enqueued.  surface: the particles are splatted by k_surface_opaque (fe_surface.h), which leaves the selected ones
// to the liquid layer; everything else is the same launches.
static int render_frame_with(FeEngine* h, int f, bool surface) {
    RenderState* R = h->render;
    if (!R) FAIL(h, "fe_render_frame: no renderer: fe_render_setup first");
    CHECK_FRAME(h, f);
    if (!R->colors) FAIL(h, "fe_render_frame: no colours: fe_render_set_colors first");
    const int n_pix = R->cam.width * R->cam.height;
    const int pix_wgs = (n_pix + FE_RENDER_WG - 1) / FE_RENDER_WG;
    hipLaunchKernelGGL(k_render_clear, dim3(std::min(pix_wgs, FE_RENDER_MAX_WGS)), dim3(FE_RENDER_WG), 0, h->stream, n_pix, R->pix);
    if (h->N > 0 && surface) surface_launch_opaque(h, f);
    else if (h->N > 0)
        hipLaunchKernelGGL(k_render_splat, dim3(std::min((h->N + FE_RENDER_WG - 1) / FE_RENDER_WG, FE_RENDER_MAX_WGS)), dim3(FE_RENDER_WG), 0, h->stream, h->N, (size_t)h->Np, h->frame(f),
                           h->pid_of(f), R->cam, R->R, h->render_lane_pixels, R->pix);
    RenderSets sets;
    for (int k = 0; k < FE_RENDER_MAX_SETS; k++) {
        const RenderPointSet& S = R->set[k];
        sets.xyz[k] = S.xyz; sets.n[k] = S.n; sets.id_base[k] = h->N + k * FE_RENDER_MAX_POINTS; sets.R[k] = S.R; sets.rgba[k] = S.rgba;
        if (S.n > 0)
            hipLaunchKernelGGL(k_render_points, dim3(std::min((S.n + FE_RENDER_WG - 1) / FE_RENDER_WG, FE_RENDER_MAX_WGS)), dim3(FE_RENDER_WG), 0, h->stream, S.n, (const float*)S.xyz,
                               sets.id_base[k], R->cam, S.R, h->render_lane_pixels, R->pix);
    }
    hipLaunchKernelGGL(k_render_shade, dim3(pix_wgs), dim3(FE_RENDER_WG), 0, h->stream, h->N, (size_t)h->Np, h->frame(f), (const int*)h->tables[h->tbl_of_frame[f]].slot_of_pid, R->cam,
                       R->lights, R->R, (const unsigned*)R->colors, sets, (const unsigned long long*)R->pix, R->rgba, R->depth, R->ids);
    R->drawn = true;
    return check_async(h);
}
int fe_render_frame(FeEngine* h, int f) {
    FE_ENTRY(h);
    return render_frame_with(h, f, false);
}

static int render_copy(FeEngine* h, const char* who, unsigned char* rgba, float* depth, int* id, hipMemcpyKind kind) {
    RenderState* R = h->render;
    if (!R) { h->err = std::string(who) + ": no renderer: fe_render_setup first"; return 1; }
    if (!R->drawn) { h->err = std::string(who) + ": no picture: fe_render_frame first"; return 1; }
    const size_t n_pix = (size_t)R->cam.width * (size_t)R->cam.height;
    if (rgba) HIPCK(h, hipMemcpyAsync(rgba, R->rgba, 4 * n_pix, kind, h->stream));
    if (depth) HIPCK(h, hipMemcpyAsync(depth, R->depth, sizeof(float) * n_pix, kind, h->stream));
    if (id) HIPCK(h, hipMemcpyAsync(id, R->ids, sizeof(int) * n_pix, kind, h->stream));
    return 0;
}
int fe_render_get(FeEngine* h, unsigned char* rgba, float* depth, int* id) {
    FE_ENTRY(h);
    if (render_copy(h, "fe_render_get", rgba, depth, id, hipMemcpyDeviceToHost)) return 1;
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    return check_device_errors(h);
}
int fe_render_get_dev(FeEngine* h, unsigned char* rgba, float* depth, int* id) {
    FE_ENTRY(h);
    if (render_copy(h, "fe_render_get_dev", rgba, depth, id, hipMemcpyDeviceToDevice)) return 1;
    return check_async(h);
}

}  // extern "C"
#endif /* FE_RENDER_MATH_ONLY */
#endif /* FE_RENDER_H */
