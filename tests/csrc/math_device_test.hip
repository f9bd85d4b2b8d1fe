// fluidlab_amd/csrc/fe_math.h as the GPU compiles it: thin kernels around fe_cbrt_pos / fe_pow_m23 (the hardware's log2, exp2 and
// reciprocal), svd3 (rotations and sweeps that end on a wave-wide vote) and constitutive_eval_t / constitutive_grad_t (FMA contraction,
// the device's operation order), one lane per case, no LDS, no atomics.  The header is included unchanged.
// Built twice by tests/math_cases.py:
//   device library  hipcc + the engine's flags, FE_T = float: mdt_cbrt / mdt_svd / mdt_constitutive run the kernels (host pointers in and
//                   out; the return value is the first HIP error), mdt_*_host run the same lane functions on the CPU in fp32;
//   fp64 library    --offload-host-only -DFE_T=double -DMDT_HOST_ONLY: only mdt_*_host, the build tests/test_csrc_math.py checks against
//                   finite differences -- the reference of the adjoints.
// Layout: a 3x3 matrix is 9 consecutive reals, row-major, case i at offset 9 i; sig is 3 reals per case.
#include <cstddef>
#include "../../fluidlab_amd/csrc/fe_math.h"

FE_HD m3 mdt_ld(const real* p) { m3 r;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) r.a[a][b] = p[a * 3 + b];
    return r; }
FE_HD void mdt_st(real* p, const m3& x) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) p[a * 3 + b] = x.a[a][b];
}

// ---- one lane's work: the kernels and the host entries call the same functions
FE_HD void mdt_cbrt_one(const real* J, real* cb, real* pm, int i) {
    cb[i] = fe_cbrt_pos(J[i]);
    pm[i] = fe_pow_m23(J[i]);
}

FE_HD void mdt_svd_one(const real* F, const int* mask, real* U, real* sig, real* V, int i) {
    if (mask[i]) {                                   // (the call sits in a branch, as it does in the engine: if (k.full))
        m3 u, v; real s[3];
        svd3(mdt_ld(F + 9 * (size_t)i), u, s, v);
        mdt_st(U + 9 * (size_t)i, u); mdt_st(V + 9 * (size_t)i, v);
        sig[3 * (size_t)i] = s[0]; sig[3 * (size_t)i + 1] = s[1]; sig[3 * (size_t)i + 2] = s[2];
    }
}

struct MdtConstitutive {
    const real *C, *F, *mu, *lam; const int* cls; const real *GA, *Fg;          // per case
    real *affine, *Fnew, *J; int* full; real *sig, *gC, *gF;                    // per case; sig is zero where the SVD was not needed
};
template <bool GENERAL>
FE_HD void mdt_constitutive_one(const MdtConstitutive& a, real dt, real mass, real scale, int i) {
    const size_t o = 9 * (size_t)i;
    const m3 C = mdt_ld(a.C + o), F = mdt_ld(a.F + o), GA = mdt_ld(a.GA + o), Fg = mdt_ld(a.Fg + o);
    const real mu = a.mu[i], lam = a.lam[i];
    const int cls = a.cls[i];
    Constitutive k;
    constitutive_eval_t<GENERAL>(C, F, dt, mu, lam, mass, cls, scale, k);
    m3 gC, gF;
    constitutive_grad_t<GENERAL>(C, F, dt, mu, lam, mass, cls, scale, k, GA, Fg, gC, gF);
    mdt_st(a.affine + o, k.affine); mdt_st(a.Fnew + o, k.Fnew); mdt_st(a.gC + o, gC); mdt_st(a.gF + o, gF);
    a.J[i] = k.J;
    a.full[i] = k.full ? 1 : 0;
#pragma unroll
    for (int d = 0; d < 3; d++) a.sig[3 * (size_t)i + d] = k.full ? k.sig[d] : R_(0.0);
}

// ---- the CPU evaluation (fp32 in the device library, fp64 in the host-only one)
extern "C" int mdt_cbrt_host(const real* J, real* cb, real* pm, int n) {
    for (int i = 0; i < n; i++) mdt_cbrt_one(J, cb, pm, i);
    return 0;
}
extern "C" int mdt_svd_host(const real* F, const int* mask, real* U, real* sig, real* V, int n) {
    for (int i = 0; i < n; i++) mdt_svd_one(F, mask, U, sig, V, i);
    return 0;
}
extern "C" int mdt_constitutive_host(int general, const real* C, const real* F, const real* mu, const real* lam, const int* cls,
                                     const real* GA, const real* Fg, real dt, real mass, real scale,
                                     real* affine, real* Fnew, real* J, int* full, real* sig, real* gC, real* gF, int n) {
    const MdtConstitutive a = {C, F, mu, lam, cls, GA, Fg, affine, Fnew, J, full, sig, gC, gF};
    for (int i = 0; i < n; i++) {
        if (general) mdt_constitutive_one<true>(a, dt, mass, scale, i);
        else mdt_constitutive_one<false>(a, dt, mass, scale, i);
    }
    return 0;
}
extern "C" int mdt_real_bytes() { return (int)sizeof(real); }

#ifndef MDT_HOST_ONLY
// ---- the kernels: one lane per case
__global__ void k_cbrt(const real* J, real* cb, real* pm, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mdt_cbrt_one(J, cb, pm, i);
}
// launched with 64-lane workgroups: a workgroup is one wave, so the caller decides who shares a wave
__global__ void k_svd(const real* F, const int* mask, real* U, real* sig, real* V, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mdt_svd_one(F, mask, U, sig, V, i);
}
template <bool GENERAL>
__global__ void k_constitutive(MdtConstitutive a, real dt, real mass, real scale, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mdt_constitutive_one<GENERAL>(a, dt, mass, scale, i);
}

// ---- launchers.  Every buffer is sized from n; the first HIP error is kept, nothing is launched or copied after it, everything is freed.
struct MdtBufs {
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
static unsigned mdt_grid(int n, int block) { return (unsigned)(((size_t)n + block - 1) / block); }

extern "C" int mdt_cbrt(const real* J, real* cb, real* pm, int n) {
    if (n <= 0) return 0;
    MdtBufs b;
    const size_t N = (size_t)n;
    const real* dJ = b.in(J, N);
    real *dcb = b.out<real>(N), *dpm = b.out<real>(N);
    if (b.ok()) { hipLaunchKernelGGL(k_cbrt, dim3(mdt_grid(n, 256)), dim3(256), 0, 0, dJ, dcb, dpm, n); b.ran(); }
    b.back(cb, dcb, N); b.back(pm, dpm, N);
    return b.done();
}
extern "C" int mdt_svd(const real* F, const int* mask, real* U, real* sig, real* V, int n) {
    if (n <= 0) return 0;
    MdtBufs b;
    const size_t N = (size_t)n;
    const real* dF = b.in(F, 9 * N);
    const int* dm = b.in(mask, N);
    real *dU = b.out<real>(9 * N), *ds = b.out<real>(3 * N), *dV = b.out<real>(9 * N);
    if (b.ok()) { hipLaunchKernelGGL(k_svd, dim3(mdt_grid(n, 64)), dim3(64), 0, 0, dF, dm, dU, ds, dV, n); b.ran(); }
    b.back(U, dU, 9 * N); b.back(sig, ds, 3 * N); b.back(V, dV, 9 * N);
    return b.done();
}
extern "C" int mdt_constitutive(int general, const real* C, const real* F, const real* mu, const real* lam, const int* cls,
                                const real* GA, const real* Fg, real dt, real mass, real scale,
                                real* affine, real* Fnew, real* J, int* full, real* sig, real* gC, real* gF, int n) {
    if (n <= 0) return 0;
    MdtBufs b;
    const size_t N = (size_t)n;
    MdtConstitutive a;
    a.C = b.in(C, 9 * N); a.F = b.in(F, 9 * N); a.mu = b.in(mu, N); a.lam = b.in(lam, N); a.cls = b.in(cls, N);
    a.GA = b.in(GA, 9 * N); a.Fg = b.in(Fg, 9 * N);
    a.affine = b.out<real>(9 * N); a.Fnew = b.out<real>(9 * N); a.J = b.out<real>(N); a.full = b.out<int>(N);
    a.sig = b.out<real>(3 * N); a.gC = b.out<real>(9 * N); a.gF = b.out<real>(9 * N);
    if (b.ok()) {
        // 64-lane workgroups here too: the mixed-material test decides which classes share a wave
        if (general) hipLaunchKernelGGL(k_constitutive<true>, dim3(mdt_grid(n, 64)), dim3(64), 0, 0, a, dt, mass, scale, n);
        else hipLaunchKernelGGL(k_constitutive<false>, dim3(mdt_grid(n, 64)), dim3(64), 0, 0, a, dt, mass, scale, n);
        b.ran();
    }
    b.back(affine, a.affine, 9 * N); b.back(Fnew, a.Fnew, 9 * N); b.back(J, a.J, N); b.back(full, a.full, N);
    b.back(sig, a.sig, 3 * N); b.back(gC, a.gC, 9 * N); b.back(gF, a.gF, 9 * N);
    return b.done();
}
#endif
