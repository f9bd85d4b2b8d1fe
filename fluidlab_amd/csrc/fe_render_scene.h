// fe_render_scene.h -- what the fluid touches, in the picture of fe_render.h: the SDF colliders ("volumes": the engine's statics, the posed
// meshes of Rigid effectors, the renderer's own copies of visual-only statics) and the smoke field (include/fluidengine_ext.h:
// fe_render_set_volume, fe_render_set_scene, fe_render_scene_frame).  Included by fe_engine.hip directly after fe_render.h.  Its three kernels
// are written as templates with one instantiation (<0>): the compiler emits plain kernels first, in source order, and template instantiations
// behind them, so as plain kernels their 26 KB would sit behind k_render_shade and push the whole 16 KB-aligned substep group one notch up; as
// instantiations they go to the tail of the code object, behind the substep and smoke kernels, which keep their addresses and their bytes
// (only the four small loss-term instantiations that used to end the code object, k_density_scatter and k_task_pair, come after them now).
//
// The rules of fe_render.h hold: fp64 formed from the fp32 words with + - * / and sqrt under fp contract(off), no floating-point atomics, the
// per-pixel math is __host__ __device__ code above the FE_RENDER_MATH_ONLY guard (tests/csrc/render_scene_test.cpp compiles it for the
// host; tests/render_scene_ref.py restates it).  Volume and cell fragments go into the same 64-bit depth|id pixel words as the particles.
//
// A volume is found by marching the ray of the pixel through the voxel box with a FIXED step and taking the first sample whose SDF is not
// positive, then bisecting.  Only the SIGN of the SDF is used: the stand-in SDFs of this repository are scaled ("only sign and direction
// matter"), so sphere tracing by the SDF's value would overshoot.  A wall thinner than the march step can be missed; that is part of the
// contract.  The march takes at most FE_RENDER_MAX_MARCH steps per volume (4096: a box of about 2300 voxels across its diagonal at the
// default step of 0.5); what lies behind that many steps is not drawn.
#ifndef FE_RENDER_SCENE_H
#define FE_RENDER_SCENE_H

#define FE_RENDER_MAX_MARCH 4096

// One volume as a pixel sees it: the SDF block, the pose (posed == 0: none) and the colour.
struct FeRenderVol {
    int res; const float* vox;
    float T[12], Rinv[9];
    int posed; float p[3], q[4];
    unsigned rgba;
};
// The ray of a pixel in world and in voxel coordinates: P(t) = pos + t d, pv(t) = ov + t dv.  q[4] is the normalised pose quaternion.
struct FeRenderRay { double d[3], ov[3], dv[3], q[4]; };

__host__ __device__ inline void fe_rs_qrot(const double* v, const double* q, double* out) {      // t_quat_rotate (fe_math.h), in fp64
#pragma clang fp contract(off)
    const double ux = q[2] * v[2] - q[3] * v[1], uy = q[3] * v[0] - q[1] * v[2], uz = q[1] * v[1] - q[2] * v[0];
    const double wx = q[2] * uz - q[3] * uy, wy = q[3] * ux - q[1] * uz, wz = q[1] * uy - q[2] * ux;
    out[0] = v[0] + 2.0 * (q[0] * ux + wx);
    out[1] = v[1] + 2.0 * (q[0] * uy + wy);
    out[2] = v[2] + 2.0 * (q[0] * uz + wz);
}
// The ray of pixel (i, j): d = fwd + ((i + 0.5 - W/2) / focal) right - ((j + 0.5 - H/2) / focal) up -- not normalised, so that t is the depth
// along fwd the particle fragments use -- mapped into the volume's voxels: the inverse pose first (t_dynamic_collide), then rows 0..2 of T.
__host__ __device__ inline void fe_rs_ray(const FeRenderCamera& cam, const FeRenderVol& V, int i, int j, FeRenderRay& r) {
#pragma clang fp contract(off)
    const double a = (((double)i + 0.5) - 0.5 * (double)cam.width) / cam.focal;
    const double b = (((double)j + 0.5) - 0.5 * (double)cam.height) / cam.focal;
    double o[3], dm[3];
    for (int c = 0; c < 3; c++) {
        r.d[c] = (cam.fwd[c] + a * cam.right[c]) - b * cam.up[c];
        o[c] = cam.pos[c]; dm[c] = r.d[c];
    }
    r.q[0] = 1.0; r.q[1] = r.q[2] = r.q[3] = 0.0;
    if (V.posed) {
        const double q0 = (double)V.q[0], q1 = (double)V.q[1], q2 = (double)V.q[2], q3 = (double)V.q[3];
        const double qn = 1.0 / sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
        r.q[0] = q0 * qn; r.q[1] = q1 * qn; r.q[2] = q2 * qn; r.q[3] = q3 * qn;
        const double qi[4] = {r.q[0], -r.q[1], -r.q[2], -r.q[3]};
        const double rel[3] = {cam.pos[0] - (double)V.p[0], cam.pos[1] - (double)V.p[1], cam.pos[2] - (double)V.p[2]};
        fe_rs_qrot(rel, qi, o);
        fe_rs_qrot(r.d, qi, dm);
    }
    for (int c = 0; c < 3; c++) {
        r.ov[c] = (((double)V.T[c * 4] * o[0] + (double)V.T[c * 4 + 1] * o[1]) + (double)V.T[c * 4 + 2] * o[2]) + (double)V.T[c * 4 + 3];
        r.dv[c] = ((double)V.T[c * 4] * dm[0] + (double)V.T[c * 4 + 1] * dm[1]) + (double)V.T[c * 4 + 2] * dm[2];
    }
}
// t_sdf_sample (fe_math.h) in fp64, its order of operations: 1 outside the voxel box.
__host__ __device__ inline double fe_rs_sample(const FeRenderVol& V, double p0, double p1, double p2) {
#pragma clang fp contract(off)
    const double top = (double)(V.res - 1);
    if (!(p0 >= 0.0 && p0 < top && p1 >= 0.0 && p1 < top && p2 >= 0.0 && p2 < top)) return 1.0;
    const int b0 = (int)p0, b1 = (int)p1, b2 = (int)p2;      // (non-negative: truncation is floor)
    const double f0 = p0 - (double)b0, f1 = p1 - (double)b1, f2 = p2 - (double)b2;
    const double g0 = 1.0 - f0, g1 = 1.0 - f1, g2 = 1.0 - f2;
    const size_t sy = (size_t)V.res, sx = (size_t)V.res * (size_t)V.res;
    const float* v = V.vox + ((size_t)b0 * sx + (size_t)b1 * sy) + (size_t)b2;
    double sd = g0 * g1 * g2 * (double)v[0];
    sd = sd + g0 * g1 * f2 * (double)v[1];
    sd = sd + g0 * f1 * g2 * (double)v[sy];
    sd = sd + g0 * f1 * f2 * (double)v[sy + 1];
    sd = sd + f0 * g1 * g2 * (double)v[sx];
    sd = sd + f0 * g1 * f2 * (double)v[sx + 1];
    sd = sd + f0 * f1 * g2 * (double)v[sx + sy];
    sd = sd + f0 * f1 * f2 * (double)v[sx + sy + 1];
    return sd;
}
__host__ __device__ inline double fe_rs_sample_t(const FeRenderVol& V, const FeRenderRay& r, double t) {
#pragma clang fp contract(off)
    return fe_rs_sample(V, r.ov[0] + t * r.dv[0], r.ov[1] + t * r.dv[1], r.ov[2] + t * r.dv[2]);
}
// The hit of the ray with the volume: false = none.  The ray is clipped against [0, res - 1]^3 (slab test) and t >= near, the interval
// [t0, t1] is marched with `step` voxels per sample (sample k at t0 + k dt, dt = step / |dv|, k <= FE_RENDER_MAX_MARCH); the first sample with
// sd <= 0 is a hit: at t0 when k == 0, else the bracket [t_(k-1), t_k] is bisected `iters` times and the hit is its upper end (the last end
// with sd <= 0).  `stop`: the depth of the pixel so far -- the march ends where no hit could lie in front of it any more ((float)t is monotone
// in t, so nothing the caller would keep is lost).
__host__ __device__ inline bool fe_rs_march(const FeRenderCamera& cam, const FeRenderVol& V, const FeRenderRay& r, double step, int iters, float stop, float& depth) {
#pragma clang fp contract(off)
    const double top = (double)(V.res - 1);
    double t0 = cam.near, t1 = 1e300;
    for (int c = 0; c < 3; c++) {
        if (r.dv[c] == 0.0) {
            if (r.ov[c] < 0.0 || r.ov[c] > top) return false;
            continue;
        }
        double ta = (0.0 - r.ov[c]) / r.dv[c], tb = (top - r.ov[c]) / r.dv[c];
        if (ta > tb) { const double s = ta; ta = tb; tb = s; }
        if (ta > t0) t0 = ta;
        if (tb < t1) t1 = tb;
    }
    if (!(t0 <= t1)) return false;
    const double dt = step / sqrt((r.dv[0] * r.dv[0] + r.dv[1] * r.dv[1]) + r.dv[2] * r.dv[2]);
    const double kd = (t1 - t0) / dt;
    const int K = kd >= (double)FE_RENDER_MAX_MARCH ? FE_RENDER_MAX_MARCH : (int)kd;
    double tp = t0;
    for (int k = 0; k <= K; k++) {
        const double t = t0 + (double)k * dt;
        if ((float)tp > stop) return false;                  // (tp: the lower end of the bracket a hit at sample k would have)
        if (fe_rs_sample_t(V, r, t) <= 0.0) {
            double lo = tp, hi = t;
            if (k > 0)
                for (int it = 0; it < iters; it++) {
                    const double mid = 0.5 * (lo + hi);
                    if (fe_rs_sample_t(V, r, mid) <= 0.0) hi = mid; else lo = mid;
                }
            depth = (float)hi;
            return true;
        }
        tp = t;
    }
    return false;
}
// The colour of a volume at the stored depth of its hit: P = pos + (double)depth d, no second march.  Normal: central differences of the SDF
// at P with delta = 1e-2 voxels, mapped back by Rinv, rotated by the pose, normalised (a vanishing gradient -- the inside of a solid block --
// gives -fwd), flipped to face the camera; the lighting is fe_rd_shade's.
__host__ __device__ inline void fe_rs_shade(const FeRenderCamera& cam, const FeRenderLights& L, const FeRenderVol& V, const FeRenderRay& r, float depth, unsigned char* out) {
#pragma clang fp contract(off)
    const double t = (double)depth, delta = 1e-2;
    const double pv[3] = {r.ov[0] + t * r.dv[0], r.ov[1] + t * r.dv[1], r.ov[2] + t * r.dv[2]};
    double g[3], nm[3], n[3], P[3], acc[3];
    g[0] = (fe_rs_sample(V, pv[0] + delta, pv[1], pv[2]) - fe_rs_sample(V, pv[0] - delta, pv[1], pv[2])) / (2.0 * delta);
    g[1] = (fe_rs_sample(V, pv[0], pv[1] + delta, pv[2]) - fe_rs_sample(V, pv[0], pv[1] - delta, pv[2])) / (2.0 * delta);
    g[2] = (fe_rs_sample(V, pv[0], pv[1], pv[2] + delta) - fe_rs_sample(V, pv[0], pv[1], pv[2] - delta)) / (2.0 * delta);
    for (int c = 0; c < 3; c++) nm[c] = ((double)V.Rinv[c * 3] * g[0] + (double)V.Rinv[c * 3 + 1] * g[1]) + (double)V.Rinv[c * 3 + 2] * g[2];
    if (V.posed) fe_rs_qrot(nm, r.q, n);
    else { n[0] = nm[0]; n[1] = nm[1]; n[2] = nm[2]; }
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (len > 0.0 && len < 1e300) { n[0] = n[0] / len; n[1] = n[1] / len; n[2] = n[2] / len; }
    else { n[0] = 0.0 - cam.fwd[0]; n[1] = 0.0 - cam.fwd[1]; n[2] = 0.0 - cam.fwd[2]; }
    if ((n[0] * r.d[0] + n[1] * r.d[1]) + n[2] * r.d[2] > 0.0) { n[0] = 0.0 - n[0]; n[1] = 0.0 - n[1]; n[2] = 0.0 - n[2]; }
    for (int c = 0; c < 3; c++) { P[c] = cam.pos[c] + t * r.d[c]; acc[c] = L.ambient[c]; }
    for (int k = 0; k < L.n_lights; k++) {
        const double l0 = L.pos[k][0] - P[0], l1 = L.pos[k][1] - P[1], l2 = L.pos[k][2] - P[2];
        const double ll = sqrt((l0 * l0 + l1 * l1) + l2 * l2);
        if (!(ll > 0.0)) continue;
        const double ndl = ((n[0] * l0 + n[1] * l1) + n[2] * l2) / ll;
        if (!(ndl > 0.0)) continue;
        for (int c = 0; c < 3; c++) acc[c] = acc[c] + L.color[k][c] * ndl;
    }
    const unsigned char base[3] = {(unsigned char)(V.rgba & 0xffu), (unsigned char)((V.rgba >> 8) & 0xffu), (unsigned char)((V.rgba >> 16) & 0xffu)};
    for (int c = 0; c < 3; c++) out[c] = fe_rd_byte(((double)base[c] / 255.0) * acc[c]);
}
// The smoke cell (i, j, k) of an n^3 grid: its centre words, and its base colour from q (a non-finite q gives 0 through fe_rd_byte).
__host__ __device__ inline void fe_rs_cell_centre(int n, int i, int j, int k, float* x) {
#pragma clang fp contract(off)
    const float inv = 1.f / (float)n;
    x[0] = ((float)i + 0.5f) * inv; x[1] = ((float)j + 0.5f) * inv; x[2] = ((float)k + 0.5f) * inv;
}
__host__ __device__ inline void fe_rs_cell_colour(const double* cold, const double* hot, float qf, unsigned char* base) {
#pragma clang fp contract(off)
    const double q = (double)qf;
    for (int a = 0; a < 3; a++) base[a] = fe_rd_byte(cold[a] * (1.0 - q) + hot[a] * q);
}
// ids: particles [0, N), point sets behind them (fe_render.h), then the volumes, then the cells
__host__ __device__ inline int fe_rs_vol_id0(int N) { return N + FE_RENDER_MAX_SETS * FE_RENDER_MAX_POINTS; }
__host__ __device__ inline int fe_rs_cell_id0(int N) { return fe_rs_vol_id0(N) + FE_RENDER_MAX_VOLUMES; }

#ifndef FE_RENDER_MATH_ONLY

// a slot of the volume table on the device: the pose words of an effector are read where they lie, at the frame drawn
struct RenderVolRec { SdfP s; const float* pos; const float* quat; unsigned rgba; int on; };

__device__ __forceinline__ void fe_rs_load_vol(const RenderVolRec& R, int f, FeRenderVol& V) {
    V.res = R.s.res; V.vox = R.s.vox; V.rgba = R.rgba;
#pragma unroll
    for (int c = 0; c < 12; c++) V.T[c] = R.s.T[c];
#pragma unroll
    for (int c = 0; c < 9; c++) V.Rinv[c] = R.s.Rinv[c];
    V.posed = R.pos != nullptr;
    V.p[0] = V.p[1] = V.p[2] = 0.f; V.q[0] = 1.f; V.q[1] = V.q[2] = V.q[3] = 0.f;
    if (V.posed) {
        for (int c = 0; c < 3; c++) V.p[c] = R.pos[(size_t)f * 3 + c];
        for (int c = 0; c < 4; c++) V.q[c] = R.quat[(size_t)f * 4 + c];
    }
}

// One sphere per cell of the slab lo < j < hi of an n^3 grid (every cell, free or not: the walls win by depth), both roads of fe_rd_splat_wave.
template <int TAIL> __global__ __launch_bounds__(FE_RENDER_WG) void k_render_smoke(int n, int lo, int hi, int id0, FeRenderCamera cam, double R, int lane_pixels, unsigned long long* pix) {
    const int nj = hi - lo - 1;
    const long long cells = (long long)n * nj * n;
    const long long rounds = (cells + FE_RENDER_WG - 1) / FE_RENDER_WG;
    for (long long r = blockIdx.x; r < rounds; r += gridDim.x) {      // (uniform)
        const long long t = r * FE_RENDER_WG + (long long)threadIdx.x;
        bool have = false;
        float x[3] = {0.f, 0.f, 0.f};
        FeRenderSphere sp;
        int id = -1;
        if (t < cells) {
            const int k = (int)(t % n), j = lo + 1 + (int)((t / n) % nj), i = (int)(t / ((long long)n * nj));
            fe_rs_cell_centre(n, i, j, k, x);
            id = id0 + (i * n + j) * n + k;
            have = fe_rd_project(cam, x, R, sp) && fe_rd_box_pixels(sp) > 0;
        }
        fe_rd_splat_wave(cam, have, sp, x, R, id, lane_pixels, pix);
    }
}

// One thread per pixel, one loop over the volumes.  The splats of this picture have finished (stream order) and no other thread touches
// this pixel's word: it is read once, lowered in a register and written once.
template <int TAIL> __global__ __launch_bounds__(FE_RENDER_WG) void k_render_sdf(const RenderVolRec* __restrict__ vols, int f, int id0, FeRenderCamera cam, double step, int iters, unsigned long long* pix) {
    const int n_pix = cam.width * cam.height;
    const int p = blockIdx.x * FE_RENDER_WG + (int)threadIdx.x;
    if (p >= n_pix) return;
    const int i = p % cam.width, j = p / cam.width;
    const unsigned long long key0 = pix[p];
    unsigned long long key = key0;
    for (int c = 0; c < FE_RENDER_MAX_VOLUMES; c++) {
        if (!vols[c].on) continue;
        FeRenderVol V;
        FeRenderRay r;
        fe_rs_load_vol(vols[c], f, V);
        fe_rs_ray(cam, V, i, j, r);
        float depth;
        const float stop = key == FE_RENDER_BG ? __builtin_inff() : fe_rd_key_depth(key);
        if (!fe_rs_march(cam, V, r, step, iters, stop, depth)) continue;
        const unsigned long long kc = fe_rd_key(depth, id0 + c);
        if (kc < key) key = kc;
    }
    if (key != key0) pix[p] = key;
}

// After k_render_shade (which left the background on every pixel whose id it does not know): the pixels of volumes and cells.
template <int TAIL> __global__ __launch_bounds__(FE_RENDER_WG) void k_render_shade_scene(const RenderVolRec* __restrict__ vols, int f, int N, int n, const float* __restrict__ q, int qd, FeRenderCamera cam,
                                                                     FeRenderLights lights, FeRenderScene sc, const unsigned long long* __restrict__ pix,
                                                                     unsigned* __restrict__ rgba, float* __restrict__ depth, int* __restrict__ ids) {
    const int n_pix = cam.width * cam.height;
    const int p = blockIdx.x * FE_RENDER_WG + (int)threadIdx.x;
    if (p >= n_pix) return;
    const unsigned long long key = pix[p];
    if (key == FE_RENDER_BG) return;
    const int kid = fe_rd_key_id(key);
    const int v0 = fe_rs_vol_id0(N), c0 = fe_rs_cell_id0(N);
    if (kid < v0) return;
    const int i = p % cam.width, j = p / cam.width;
    unsigned char out[3];
    if (kid < c0) {
        if (!vols || !vols[kid - v0].on) return;
        FeRenderVol V;
        FeRenderRay r;
        fe_rs_load_vol(vols[kid - v0], f, V);
        fe_rs_ray(cam, V, i, j, r);
        fe_rs_shade(cam, lights, V, r, fe_rd_key_depth(key), out);
    } else {
        const long long cell = (long long)kid - c0;
        if (!q || cell >= (long long)n * n * n) return;
        const int ck = (int)(cell % n), cj = (int)((cell / n) % n), ci = (int)(cell / ((long long)n * n));
        float x[3];
        unsigned char base[3];
        fe_rs_cell_centre(n, ci, cj, ck, x);
        fe_rs_cell_colour(sc.cold, sc.hot, q[(size_t)cell * qd], base);
        FeRenderSphere sp;
        FeRenderFrag fr;
        if (!fe_rd_project(cam, x, sc.smoke_radius, sp) || !fe_rd_fragment(sp, i, j, fr)) return;
        fe_rd_shade(cam, lights, sp, fr, base, out);
    }
    rgba[p] = (unsigned)out[0] | ((unsigned)out[1] << 8) | ((unsigned)out[2] << 16) | 0xff000000u;
    depth[p] = fe_rd_key_depth(key);
    ids[p] = kid;
}

// ---------------------------------------------------------------------------------------------------------------- host
struct RenderSceneState {
    RenderVolRec vol[FE_RENDER_MAX_VOLUMES];                 // the table (on == 0: an empty slot), and its copy on the device
    float* own[FE_RENDER_MAX_VOLUMES]; size_t own_n[FE_RENDER_MAX_VOLUMES];      // voxels of the renderer's own copies
    RenderVolRec* vol_dev = nullptr;
    int n_on = 0;
    bool has_scene = false; FeRenderScene sc;
    RenderSceneState() { for (int c = 0; c < FE_RENDER_MAX_VOLUMES; c++) { vol[c] = RenderVolRec(); vol[c].on = 0; vol[c].pos = vol[c].quat = nullptr; own[c] = nullptr; own_n[c] = 0; } sc = FeRenderScene(); }
};
static int build_sdf(FeEngine* h, const FeSdfDesc* d, const fe_real* voxels, SdfP& s, float** vox_out);

static void render_scene_drop(FeEngine* h) {                 // fe_destroy
    RenderSceneState* Q = h->render_scene;
    if (!Q) return;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (int c = 0; c < FE_RENDER_MAX_VOLUMES; c++) render_free(h, Q->own[c], Q->own_n[c]);
    render_free(h, Q->vol_dev, (size_t)FE_RENDER_MAX_VOLUMES);
    delete Q;
    h->render_scene = nullptr;
}

extern "C" {

int fe_render_set_volume(FeEngine* h, int slot, int source, int index, const FeSdfDesc* desc, const fe_real* voxels, const unsigned char* rgba) {
    FE_ENTRY(h);
    if (!h->render) FAIL(h, "fe_render_set_volume: no renderer: fe_render_setup first");
    if (slot < 0 || slot >= FE_RENDER_MAX_VOLUMES) FAIL(h, "fe_render_set_volume: slot out of range (the slot is unchanged)");
    RenderVolRec rec = RenderVolRec();
    rec.pos = rec.quat = nullptr; rec.on = 0;
    float* vox = nullptr; size_t vox_n = 0;
    if (source == FE_RENDER_VOL_STATIC) {
        if (index < 0 || index >= (int)h->statics_host.size()) FAIL(h, "fe_render_set_volume: static index out of range (the slot is unchanged)");
        rec.s = h->statics_host[index];
    } else if (source == FE_RENDER_VOL_EFFECTOR) {
        if (index < 0 || index >= (int)h->effs.size()) FAIL(h, "fe_render_set_volume: effector index out of range (the slot is unchanged)");
        if (!h->effs[index].p.has_mesh) FAIL(h, "fe_render_set_volume: the effector has no mesh: fe_eff_set_mesh first (the slot is unchanged)");
        rec.s = h->effs[index].p.mesh; rec.pos = h->effs[index].p.pos; rec.quat = h->effs[index].p.quat;
    } else if (source == FE_RENDER_VOL_OWN) {
        if (!desc || !voxels) FAIL(h, "fe_render_set_volume: an own copy needs a FeSdfDesc and voxels (the slot is unchanged)");
    } else if (source != FE_RENDER_VOL_NONE) FAIL(h, "fe_render_set_volume: unknown source (the slot is unchanged)");
    if (source != FE_RENDER_VOL_NONE) {
        if (!rgba) FAIL(h, "fe_render_set_volume: null colour (the slot is unchanged)");
        rec.rgba = (unsigned)rgba[0] | ((unsigned)rgba[1] << 8) | ((unsigned)rgba[2] << 16) | ((unsigned)rgba[3] << 24);
        rec.on = 1;
    }
    if (source == FE_RENDER_VOL_OWN) {
        if (build_sdf(h, desc, voxels, rec.s, &vox)) { h->err = "fe_render_set_volume: " + h->err + " (the slot is unchanged)"; return 1; }
        vox_n = (size_t)desc->res * desc->res * desc->res;
    }
    RenderSceneState* Q = h->render_scene;
    if (!Q) Q = h->render_scene = new RenderSceneState();
    if (!Q->vol_dev && dev_alloc(h, &Q->vol_dev, (size_t)FE_RENDER_MAX_VOLUMES)) { render_free(h, vox, vox_n); return 1; }
    const RenderVolRec old = Q->vol[slot];
    Q->vol[slot] = rec;
    if (hipMemcpyOnStream(h, Q->vol_dev, Q->vol, sizeof(Q->vol), hipMemcpyHostToDevice) != hipSuccess) {
        Q->vol[slot] = old; render_free(h, vox, vox_n);
        FAIL(h, "fe_render_set_volume: hipMemcpy failed (the slot is unchanged)");
    }
    render_free(h, Q->own[slot], Q->own_n[slot]);            // (the stream has drained: hipMemcpyOnStream)
    Q->own[slot] = vox; Q->own_n[slot] = vox_n;
    Q->n_on = 0;
    for (int c = 0; c < FE_RENDER_MAX_VOLUMES; c++) Q->n_on += Q->vol[c].on;
    return 0;
}

int fe_render_set_scene(FeEngine* h, const FeRenderScene* scene, int scene_size) {
    FE_ENTRY(h);
    if (!h->render) FAIL(h, "fe_render_set_scene: no renderer: fe_render_setup first");
    if (!scene) {
        if (h->render_scene) h->render_scene->has_scene = false;
        return 0;
    }
    if (scene_size != (int)sizeof(FeRenderScene)) FAIL(h, "fe_render_set_scene: FeRenderScene size mismatch");
    const FeRenderScene& s = *scene;
    if (!render_pos(s.march_step) || s.march_step > 1.0) FAIL(h, "fe_render_set_scene: march_step must be finite and in (0, 1] (the scene is unchanged)");
    if (s.bisect_iters < 0 || s.bisect_iters > 32) FAIL(h, "fe_render_set_scene: bisect_iters must be in [0, 32] (the scene is unchanged)");
    if (s.draw_smoke) {
        if (!h->smoke) FAIL(h, "fe_render_set_scene: draw_smoke without a smoke field: fe_smoke_create first (the scene is unchanged)");
        const int n = h->smoke->P.n;
        if (!render_pos(s.smoke_radius)) FAIL(h, "fe_render_set_scene: the smoke radius must be finite and positive (the scene is unchanged)");
        if (s.lo < -1 || s.hi > n || s.lo >= s.hi) FAIL(h, "fe_render_set_scene: the slab lo < j < hi lies outside the grid (the scene is unchanged)");
        if (!render_finite3(s.cold) || !render_finite3(s.hot)) FAIL(h, "fe_render_set_scene: the cold or hot colour is not finite (the scene is unchanged)");
        if ((long long)fe_rs_cell_id0(h->N) + (long long)n * n * n - 1 > 2147483647ll) FAIL(h, "fe_render_set_scene: the grid's largest cell id does not fit a positive int (the scene is unchanged)");
    }
    if (!h->render_scene) h->render_scene = new RenderSceneState();
    h->render_scene->sc = s;
    h->render_scene->has_scene = true;
    return 0;
}

// surface: render_frame_with's (fe_surface_frame draws the opaque layer through here)
static int render_scene_frame_with(FeEngine* h, int f, int s, bool surface) {
    RenderState* R = h->render;
    if (!R) FAIL(h, "fe_render_scene_frame: no renderer: fe_render_setup first");
    RenderSceneState* Q = h->render_scene;
    const bool smoke = Q && Q->has_scene && Q->sc.draw_smoke;
    const bool vols = Q && Q->n_on > 0;
    if (smoke) {
        if (!h->smoke) FAIL(h, "fe_render_scene_frame: the smoke field is gone");
        if (s < 0 || s > h->smoke->P.S) FAIL(h, "fe_render_scene_frame: smoke frame s outside [0, max_steps_local]");
    }
    if (render_frame_with(h, f, surface)) return 1;
    if (!smoke && !vols) return 0;
    const int n_pix = R->cam.width * R->cam.height;
    const int pix_wgs = (n_pix + FE_RENDER_WG - 1) / FE_RENDER_WG;
    FeRenderScene sc = Q->has_scene ? Q->sc : FeRenderScene();
    if (!Q->has_scene) { sc.march_step = 0.5; sc.bisect_iters = 10; }
    int n = 0, qd = 1;
    const float* q = nullptr;
    if (smoke) {
        const SmokeP& P = h->smoke->P;
        n = P.n; qd = P.qd;
        q = P.q + (size_t)s * P.n3 * (size_t)P.qd;
        const int lo = sc.lo, hi = sc.hi;
        const long long cells = (long long)n * (hi - lo - 1) * n;
        if (cells > 0)
            hipLaunchKernelGGL(k_render_smoke<0>, dim3((unsigned)std::min<long long>((cells + FE_RENDER_WG - 1) / FE_RENDER_WG, FE_RENDER_MAX_WGS)), dim3(FE_RENDER_WG), 0, h->stream, n, lo, hi,
                               fe_rs_cell_id0(h->N), R->cam, sc.smoke_radius, h->render_lane_pixels, R->pix);
    }
    if (vols)
        hipLaunchKernelGGL(k_render_sdf<0>, dim3(pix_wgs), dim3(FE_RENDER_WG), 0, h->stream, (const RenderVolRec*)Q->vol_dev, f, fe_rs_vol_id0(h->N), R->cam, sc.march_step, sc.bisect_iters, R->pix);
    hipLaunchKernelGGL(k_render_shade_scene<0>, dim3(pix_wgs), dim3(FE_RENDER_WG), 0, h->stream, (const RenderVolRec*)(vols ? Q->vol_dev : nullptr), f, h->N, n, q, qd, R->cam, R->lights, sc,
                       (const unsigned long long*)R->pix, R->rgba, R->depth, R->ids);
    return check_async(h);
}
int fe_render_scene_frame(FeEngine* h, int f, int s) {
    FE_ENTRY(h);
    return render_scene_frame_with(h, f, s, false);
}

}  // extern "C"
// (the liquid surface drawn over this picture: included here because no fe_*.h may follow this header in fe_engine.hip -- tests/test_render_scene_abi.py --
// and because it builds on the host functions above; its kernels' first uses are at the end of fe_engine.hip)
#include "fe_surface.h"
#endif /* FE_RENDER_MATH_ONLY */
#endif /* FE_RENDER_SCENE_H */
