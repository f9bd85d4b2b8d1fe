// The geometry and contact half of fluidlab_amd/csrc/fe_math.h as the GPU compiles it: SDF sampling and normal, the contact law and its
// pull-back, the static and the moving collider (value and all 20 forward-mode columns), the quaternion helpers, the boundaries and the
// B-spline stencil.  Thin kernels, one lane per case, no LDS, no atomics; the header is included unchanged.
// Built three ways by tests/geom_cases.py, like math_device_test.hip:
//   device library  hipcc + the engine's flags, FE_T = float: gdt_run(entry, device = 1, ...) launches the kernel of the entry (host pointers
//                   in and out; the return value is the first HIP error), device = 0 runs the same lane function on the CPU in fp32;
//   fp64 library    --offload-host-only -DFE_T=double -DGDT_HOST_ONLY: the CPU evaluation only, plus the `classify` entry.
// One calling convention for every entry: in[slot] / out[slot] / iout[slot] are arrays of `width` reals (ints) per case, case i at offset
// width * i; the widths are the table gdt_widths() returns, so the Python side sizes every buffer from the table the kernels index with.
#include <cstddef>
#include "../../fluidlab_amd/csrc/fe_math.h"

enum { GDT_SDF, GDT_CONTACT_LAW, GDT_STATIC_COLLIDE, GDT_DYNAMIC_COLLIDE, GDT_MOVE_QUAT, GDT_QUAT, GDT_BOUNDARY, GDT_STENCIL, GDT_CLASSIFY, GDT_ENTRIES };
#define GDT_IN 4
#define GDT_OUT 4
#define GDT_IOUT 2

// what a launch shares among its cases (friction and softness are per case: they ride in an input slot)
struct GdtParams {
    int res; const real* vox; real T[12], Rinv[9];            // the collider's voxels (res^3 reals) and transforms
    BoundaryP bnd;
    real dt, inv_dx; int n_grid;
};
struct GdtIO { const real* in[GDT_IN]; real* out[GDT_OUT]; int* iout[GDT_IOUT]; };

// widths per entry: GDT_IN inputs, GDT_OUT outputs, GDT_IOUT int outputs (0 = slot unused)
static const int gdt_w[GDT_ENTRIES][GDT_IN + GDT_OUT + GDT_IOUT] = {
    /* sdf             in: pv                          out: sdf_sample, t_sdf_sample<real>, sdf_normal */ {3, 0, 0, 0, 1, 1, 3, 0, 0, 0},
    /* contact_law     in: n, rv, g, friction          out: out, g pulled back                          */ {3, 3, 3, 1, 3, 3, 0, 0, 0, 0},
    /* static_collide  in: pos, v, g, friction         out: v, g pulled back                            */ {3, 3, 3, 1, 3, 3, 0, 0, 0, 0},
    /* dynamic_collide in: (p0 q0 p1 q1 pos mv), (friction softness)   out: out, J[3][20]; hit          */ {20, 2, 0, 0, 3, 60, 0, 0, 1, 0},
    /* move_quat       in: (w q)                       out: q', J[4][7]                                 */ {7, 0, 0, 0, 4, 28, 0, 0, 0, 0},
    /* quat            in: q, r, aa, v                 out: quat_mul(q, r), quat_from_w(aa), quat_rotate(v, q) */ {4, 4, 3, 3, 4, 4, 3, 0, 0, 0},
    /* boundary        in: x, v                        out: v', k, xn, J[3][3]; is_out                  */ {3, 3, 0, 0, 3, 3, 3, 9, 1, 0},
    /* stencil         in: x                           out: fx, w[3][3], dw[3][3]; base, inside         */ {3, 0, 0, 0, 3, 9, 9, 0, 3, 1},
    /* classify        in: as dynamic_collide          out: sd pv[3] pv+[3] pv-[3] |g| nc vtn t infl n[3] cv[3]; hit */ {20, 2, 0, 0, 22, 0, 0, 0, 1, 0},
};

FE_HD SdfP gdt_sdf_of(const GdtParams& p, real friction, real softness) {
    SdfP s;
    s.res = p.res; s.vox = p.vox;
    for (int i = 0; i < 12; i++) s.T[i] = p.T[i];
    for (int i = 0; i < 9; i++) s.Rinv[i] = p.Rinv[i];
    s.friction = friction; s.softness = softness;
    return s;
}

// ---- one lane's work: the kernels and the CPU entries call the same functions
FE_HD void gdt_sdf_one(const GdtIO& a, const GdtParams& p, size_t i) {
    const SdfP s = gdt_sdf_of(p, R_(0.0), R_(0.0));
    const real pv[3] = {a.in[0][3 * i], a.in[0][3 * i + 1], a.in[0][3 * i + 2]};
    real n[3];
    a.out[0][i] = sdf_sample(s, pv);
    a.out[1][i] = t_sdf_sample<real>(s, pv);
    sdf_normal(s, pv, n);
    for (int d = 0; d < 3; d++) a.out[2][3 * i + d] = n[d];
}
FE_HD void gdt_contact_law_one(const GdtIO& a, const GdtParams&, size_t i) {
    real n[3], rv[3], g[3], out[3];
    for (int d = 0; d < 3; d++) { n[d] = a.in[0][3 * i + d]; rv[d] = a.in[1][3 * i + d]; g[d] = a.in[2][3 * i + d]; }
    contact_law(n, a.in[3][i], rv, out, g);
    for (int d = 0; d < 3; d++) { a.out[0][3 * i + d] = out[d]; a.out[1][3 * i + d] = g[d]; }
}
FE_HD void gdt_static_collide_one(const GdtIO& a, const GdtParams& p, size_t i) {
    const SdfP s = gdt_sdf_of(p, a.in[3][i], R_(0.0));
    real pos[3], v[3], g[3];
    for (int d = 0; d < 3; d++) { pos[d] = a.in[0][3 * i + d]; v[d] = a.in[1][3 * i + d]; g[d] = a.in[2][3 * i + d]; }
    static_collide(s, pos, v, g);
    for (int d = 0; d < 3; d++) { a.out[0][3 * i + d] = v[d]; a.out[1][3 * i + d] = g[d]; }
}
// the 20 inputs in the order of the engine's chain: p0[3] q0[4] p1[3] q1[4] pos[3] mv[3]
template <class T> FE_HD bool gdt_dyn_call(const SdfP& s, const T* x, real dt, T out[3]) {
    return t_dynamic_collide<T>(s, x, x + 3, x + 7, x + 10, x + 14, x + 17, dt, out);
}
FE_HD void gdt_dynamic_collide_one(const GdtIO& a, const GdtParams& p, size_t i) {
    const SdfP s = gdt_sdf_of(p, a.in[1][2 * i], a.in[1][2 * i + 1]);
    real x[20], out[3];
#pragma unroll
    for (int j = 0; j < 20; j++) x[j] = a.in[0][20 * i + j];
    const bool hit = gdt_dyn_call<real>(s, x, p.dt, out);
    for (int d = 0; d < 3; d++) a.out[0][3 * i + d] = out[d];
    a.iout[0][i] = hit ? 1 : 0;
    for (int c = 0; c < 20; c++) {                           // one forward-mode column per call, as collide_chain_grad_row assembles them
        Dual xd[20], od[3];
#pragma unroll
        for (int j = 0; j < 20; j++) xd[j] = Dual(x[j], j == c ? R_(1.0) : R_(0.0));
        gdt_dyn_call<Dual>(s, xd, p.dt, od);
        for (int d = 0; d < 3; d++) a.out[1][60 * i + 20 * d + c] = od[d].d;
    }
}
FE_HD void gdt_move_quat_one(const GdtIO& a, const GdtParams&, size_t i) {
    real x[7], o[4];
#pragma unroll
    for (int j = 0; j < 7; j++) x[j] = a.in[0][7 * i + j];
    t_move_quat<real>(x, x + 3, o);
    for (int d = 0; d < 4; d++) a.out[0][4 * i + d] = o[d];
    for (int c = 0; c < 7; c++) {
        Dual xd[7], od[4];
#pragma unroll
        for (int j = 0; j < 7; j++) xd[j] = Dual(x[j], j == c ? R_(1.0) : R_(0.0));
        t_move_quat<Dual>(xd, xd + 3, od);
        for (int d = 0; d < 4; d++) a.out[1][28 * i + 7 * d + c] = od[d].d;
    }
}
FE_HD void gdt_quat_one(const GdtIO& a, const GdtParams&, size_t i) {
    real q[4], r[4], aa[3], v[3], o4[4], o3[3];
    for (int d = 0; d < 4; d++) { q[d] = a.in[0][4 * i + d]; r[d] = a.in[1][4 * i + d]; }
    for (int d = 0; d < 3; d++) { aa[d] = a.in[2][3 * i + d]; v[d] = a.in[3][3 * i + d]; }
    quat_mul(q, r, o4);
    for (int d = 0; d < 4; d++) a.out[0][4 * i + d] = o4[d];
    quat_from_w(aa, o4);
    for (int d = 0; d < 4; d++) a.out[1][4 * i + d] = o4[d];
    quat_rotate(v, q, o3);
    for (int d = 0; d < 3; d++) a.out[2][3 * i + d] = o3[d];
}
FE_HD void gdt_boundary_one(const GdtIO& a, const GdtParams& p, size_t i) {
    real x[3], v[3], k[3], xn[3], J[3][3];
    for (int d = 0; d < 3; d++) { x[d] = a.in[0][3 * i + d]; v[d] = a.in[1][3 * i + d]; }
    boundary_v(p.bnd, x, v, k);
    boundary_x(p.bnd, x, xn, J);
    for (int d = 0; d < 3; d++) { a.out[0][3 * i + d] = v[d]; a.out[1][3 * i + d] = k[d]; a.out[2][3 * i + d] = xn[d]; }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) a.out[3][9 * i + 3 * r + c] = J[r][c];
    a.iout[0][i] = boundary_is_out(p.bnd, x) ? 1 : 0;
}
FE_HD void gdt_stencil_one(const GdtIO& a, const GdtParams& p, size_t i) {
    const real x[3] = {a.in[0][3 * i], a.in[0][3 * i + 1], a.in[0][3 * i + 2]};
    Stencil s;
    stencil_make(x, p.inv_dx, s);
#pragma unroll
    for (int d = 0; d < 3; d++) {
        a.iout[0][3 * i + d] = s.base[d];
        a.out[0][3 * i + d] = s.fx[d];
#pragma unroll
        for (int k = 0; k < 3; k++) { a.out[1][9 * i + 3 * k + d] = s.w[k][d]; a.out[2][9 * i + 3 * k + d] = stencil_dw(s, k, d); }
    }
    a.iout[1][i] = stencil_inside(s, p.n_grid) ? 1 : 0;
}
#ifdef GDT_HOST_ONLY
// The quantities the case classes take their margins on, of one dynamic-collide case: the header's own pieces in the header's order, up
// to the selects.  (fp64 build only: a margin decided in fp32 would be decided by the rounding it is meant to keep away from.)
static void gdt_classify_one(const GdtIO& a, const GdtParams& p, size_t i) {
    const SdfP s = gdt_sdf_of(p, a.in[1][2 * i], a.in[1][2 * i + 1]);
    const real *x = a.in[0] + 20 * i, *p0 = x, *q0 = x + 3, *p1 = x + 7, *q1 = x + 10, *pos = x + 14, *mv = x + 17;
    real* o = a.out[0] + 22 * i;
    const real rel0[3] = {pos[0] - p0[0], pos[1] - p0[1], pos[2] - p0[2]};
    const real qn = R_(1.0) / sqrt(q0[0] * q0[0] + q0[1] * q0[1] + q0[2] * q0[2] + q0[3] * q0[3]);
    const real qi[4] = {q0[0] * qn, -(q0[1] * qn), -(q0[2] * qn), -(q0[3] * qn)};
    real pm[3], pv[3], pn[3], cv[3], g[3], nm[3], n[3];
    t_quat_rotate<real>(rel0, qi, pm);
    sdf_to_voxels(s, pm, pv);
    const real sd = t_sdf_sample<real>(s, pv);
    real infl = exp(-sd * s.softness);
    if (infl > R_(1.0)) infl = R_(1.0);
    a.iout[0][i] = (sd <= R_(0.0) || (s.softness > R_(0.0) && infl > R_(0.1))) ? 1 : 0;
    t_quat_rotate<real>(pm, q1, pn);
    for (int d = 0; d < 3; d++) cv[d] = (pn[d] + p1[d] - pos[d]) / p.dt;
    const real delta = R_(1e-2);
    for (int d = 0; d < 3; d++) {
        real inc[3] = {pv[0], pv[1], pv[2]}, dec[3] = {pv[0], pv[1], pv[2]};
        inc[d] += delta; dec[d] -= delta;
        o[4 + d] = inc[d]; o[7 + d] = dec[d];
        g[d] = (t_sdf_sample<real>(s, inc) - t_sdf_sample<real>(s, dec)) / (R_(2.0) * delta);
    }
    const real gn = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    t_normalize3<real>(g);
    for (int d = 0; d < 3; d++) nm[d] = s.Rinv[d * 3] * g[0] + s.Rinv[d * 3 + 1] * g[1] + s.Rinv[d * 3 + 2] * g[2];
    t_quat_rotate<real>(nm, q0, n);
    t_normalize3<real>(n);
    const real rel[3] = {mv[0] - cv[0], mv[1] - cv[1], mv[2] - cv[2]};
    const real nc = rel[0] * n[0] + rel[1] * n[1] + rel[2] * n[2];
    const real am = nc < R_(0.0) ? nc : R_(0.0);
    const real vt[3] = {rel[0] - am * n[0], rel[1] - am * n[1], rel[2] - am * n[2]};
    const real vtn = sqrt(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
    o[0] = sd; o[1] = pv[0]; o[2] = pv[1]; o[3] = pv[2];
    o[10] = gn; o[11] = nc; o[12] = vtn; o[13] = vtn + nc * s.friction; o[14] = infl;
    for (int d = 0; d < 3; d++) { o[15 + d] = n[d]; o[18 + d] = cv[d]; }
}
#endif

FE_HD void gdt_one(int entry, const GdtIO& a, const GdtParams& p, size_t i) {
    switch (entry) {
    case GDT_SDF: gdt_sdf_one(a, p, i); break;
    case GDT_CONTACT_LAW: gdt_contact_law_one(a, p, i); break;
    case GDT_STATIC_COLLIDE: gdt_static_collide_one(a, p, i); break;
    case GDT_DYNAMIC_COLLIDE: gdt_dynamic_collide_one(a, p, i); break;
    case GDT_MOVE_QUAT: gdt_move_quat_one(a, p, i); break;
    case GDT_QUAT: gdt_quat_one(a, p, i); break;
    case GDT_BOUNDARY: gdt_boundary_one(a, p, i); break;
    case GDT_STENCIL: gdt_stencil_one(a, p, i); break;
    default: break;
    }
}

extern "C" int gdt_real_bytes() { return (int)sizeof(real); }
extern "C" int gdt_entries() { return GDT_ENTRIES; }
extern "C" int gdt_widths(int entry, int* w) {
    if (entry < 0 || entry >= GDT_ENTRIES) return 1;
    for (int j = 0; j < GDT_IN + GDT_OUT + GDT_IOUT; j++) w[j] = gdt_w[entry][j];
    return 0;
}
#ifdef GDT_HOST_ONLY
extern "C" int gdt_has_device() { return 0; }
#else
extern "C" int gdt_has_device() { return 1; }
#endif

static int gdt_run_host(int entry, int n, const GdtIO& a, const GdtParams& p) {
    for (int i = 0; i < n; i++) {
#ifdef GDT_HOST_ONLY
        if (entry == GDT_CLASSIFY) { gdt_classify_one(a, p, (size_t)i); continue; }
#endif
        gdt_one(entry, a, p, (size_t)i);
    }
    return 0;
}

#ifndef GDT_HOST_ONLY
// ---- the kernels: one lane per case, 64-lane workgroups (a workgroup is one wave, so the caller decides who shares a wave)
template <int ENTRY>
__global__ void k_geom(GdtIO a, GdtParams p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gdt_one(ENTRY, a, p, (size_t)i);
}

// Every buffer is sized from n and the width table; the first HIP error is kept, nothing is launched or copied after it, everything is freed.
struct GdtBufs {
    void* p[16]; int np = 0; hipError_t err = hipSuccess;
    void note(hipError_t e) { if (err == hipSuccess && e != hipSuccess) err = e; }
    void* raw(size_t bytes) {
        void* d = nullptr;
        if (err != hipSuccess || np >= 16) { note(hipErrorOutOfMemory); return nullptr; }
        note(hipMalloc(&d, bytes));
        if (err != hipSuccess) return nullptr;
        p[np++] = d;
        return d;
    }
    template <class T> T* in(const T* h, size_t count) {
        T* d = (T*)raw(count * sizeof(T));
        if (d) note(hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    template <class T> T* out(size_t count) {                     // filled with 0xFF: a float that no lane wrote reads as NaN
        T* d = (T*)raw(count * sizeof(T));
        if (d) note(hipMemset(d, 0xFF, count * sizeof(T)));
        return d;
    }
    bool ok() const { return err == hipSuccess; }
    void ran() { note(hipGetLastError()); note(hipDeviceSynchronize()); }
    template <class T> void back(T* h, const T* d, size_t count) { if (ok()) note(hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost)); }
    int done() { for (int i = 0; i < np; i++) note(hipFree(p[i])); return (int)err; }
};

static int gdt_run_device(int entry, int n, const GdtIO& h, const GdtParams& hp) {
    const int* w = gdt_w[entry];
    const size_t N = (size_t)n;
    GdtBufs b;
    GdtIO d = {};
    GdtParams p = hp;
    if (hp.vox) p.vox = b.in(hp.vox, (size_t)hp.res * hp.res * hp.res);
    for (int s = 0; s < GDT_IN; s++) if (w[s]) d.in[s] = b.in(h.in[s], N * w[s]);
    for (int s = 0; s < GDT_OUT; s++) if (w[GDT_IN + s]) d.out[s] = b.out<real>(N * w[GDT_IN + s]);
    for (int s = 0; s < GDT_IOUT; s++) if (w[GDT_IN + GDT_OUT + s]) d.iout[s] = b.out<int>(N * w[GDT_IN + GDT_OUT + s]);
    if (b.ok()) {
        const dim3 grid((unsigned)((N + 63) / 64)), block(64);
        switch (entry) {
#define GDT_LAUNCH(E) case E: hipLaunchKernelGGL(k_geom<E>, grid, block, 0, 0, d, p, n); break;
        GDT_LAUNCH(GDT_SDF) GDT_LAUNCH(GDT_CONTACT_LAW) GDT_LAUNCH(GDT_STATIC_COLLIDE) GDT_LAUNCH(GDT_DYNAMIC_COLLIDE)
        GDT_LAUNCH(GDT_MOVE_QUAT) GDT_LAUNCH(GDT_QUAT) GDT_LAUNCH(GDT_BOUNDARY) GDT_LAUNCH(GDT_STENCIL)
#undef GDT_LAUNCH
        default: break;
        }
        b.ran();
    }
    for (int s = 0; s < GDT_OUT; s++) if (w[GDT_IN + s]) b.back(h.out[s], d.out[s], N * w[GDT_IN + s]);
    for (int s = 0; s < GDT_IOUT; s++) if (w[GDT_IN + GDT_OUT + s]) b.back(h.iout[s], d.iout[s], N * w[GDT_IN + GDT_OUT + s]);
    return b.done();
}
#endif

// in / out / iout: GDT_IN / GDT_OUT / GDT_IOUT host pointers (unused slots may be null).  device = 1 needs the device library.
// Returns 0, the first HIP error, or -1 for an entry this build does not have.
extern "C" int gdt_run(int entry, int device, int n, const real* const* in, real* const* out, int* const* iout, const GdtParams* prm) {
    if (entry < 0 || entry >= GDT_ENTRIES || n < 0) return -1;
    if (n == 0) return 0;
    const int* w = gdt_w[entry];
    const bool needs_vox = entry == GDT_SDF || entry == GDT_STATIC_COLLIDE || entry == GDT_DYNAMIC_COLLIDE || entry == GDT_CLASSIFY;
    if (needs_vox && (!prm->vox || prm->res < 2)) return -1;
    GdtIO a = {};
    for (int s = 0; s < GDT_IN; s++) { if (w[s] && !in[s]) return -1; a.in[s] = in[s]; }
    for (int s = 0; s < GDT_OUT; s++) { if (w[GDT_IN + s] && !out[s]) return -1; a.out[s] = out[s]; }
    for (int s = 0; s < GDT_IOUT; s++) { if (w[GDT_IN + GDT_OUT + s] && !iout[s]) return -1; a.iout[s] = iout[s]; }
#ifdef GDT_HOST_ONLY
    if (device) return -1;
    return gdt_run_host(entry, n, a, *prm);
#else
    if (entry == GDT_CLASSIFY) return -1;
    return device ? gdt_run_device(entry, n, a, *prm) : gdt_run_host(entry, n, a, *prm);
#endif
}
