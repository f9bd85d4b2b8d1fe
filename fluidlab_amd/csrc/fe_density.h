// fe_density.h -- density fields of a frame and the density term of the loss-term programs (include/fluidengine_ext.h: fe_density_*,
// FE_TERM_DENSITY_SQ).  Included by fe_task_loss.h between its helpers (the selection test, workgroup sums, frame views), which the kernels here use, and k_task_bwd.
// The first part -- the quadratic B-spline stencil of one particle on one field, its derivative, the guard and the fixed-point deposit -- is
// plain __host__ __device__ code: tests/csrc/density_test.cpp compiles it for the host with FE_DENSITY_MATH_ONLY defined and checks it against
// plain loops.
//
// A field is accumulated in unsigned 64-bit integers, q = llrint(w 2^40) per deposit: integer addition does not depend on order, so a field is
// the same bits however it was accumulated (LDS copies per workgroup or global atomics, any number of workgroups).  With N <= 2^23 particles
// and w <= 1 a cell word stays below 2^63.  No floating-point atomics anywhere.
#ifndef FE_DENSITY_H
#define FE_DENSITY_H

#define FE_DENSITY_FIX 1099511627776.0                      /* 2^40 */
#define FE_DENSITY_MAX_U 1073741824.0                       /* 2^30: |u| above it deposits nothing */

// One particle's stencil on one field: on axis a the cells base[a], base[a] + 1, base[a] + 2 with weights w[a][] and derivatives dw[a][] with
// respect to x_a.  A cell outside [0, n[a]) is dropped by the caller (fe_dn_in); on a projected axis that leaves cell 0 alone, with weight 1.
struct FeDensityStencil { int base[3]; double w[3][3]; double dw[3][3]; };

__host__ __device__ inline bool fe_dn_finite(float v) { return v - v == 0.0f; }
__host__ __device__ inline long long fe_dn_cells(const FeDensitySpec& sp) { return (long long)sp.n[0] * sp.n[1] * sp.n[2]; }
__host__ __device__ inline long long fe_dn_index(const FeDensitySpec& sp, int i, int j, int k) { return ((long long)i * sp.n[1] + j) * sp.n[2] + k; }
__host__ __device__ inline bool fe_dn_in(const FeDensitySpec& sp, int a, int i) { return i >= 0 && i < sp.n[a]; }
// one axis of the stencil; false: |u| > 2^30 (tested in floating point, before the conversion to integer)
__host__ __device__ inline bool fe_dn_axis(double x, double origin, double cell, int n, int& base, double* w, double* dw) {
    if (n == 1) {                                             // projected: weight 1, derivative 0, wherever the particle is
        base = 0;
        w[0] = 1.0; w[1] = 0.0; w[2] = 0.0;
        dw[0] = 0.0; dw[1] = 0.0; dw[2] = 0.0;
        return true;
    }
    const double u = (x - origin) / cell;
    if (!(u >= -FE_DENSITY_MAX_U && u <= FE_DENSITY_MAX_U)) return false;
    const double s = u - 0.5;
    const double b = floor(s - 0.5);
    const double t = s - b;                                   // in [0.5, 1.5)
    const double inv = 1.0 / cell;
    base = (int)b;
    w[0] = 0.5 * (1.5 - t) * (1.5 - t);
    w[1] = 0.75 - (t - 1.0) * (t - 1.0);
    w[2] = 0.5 * (t - 0.5) * (t - 0.5);
    dw[0] = -(1.5 - t) * inv;
    dw[1] = -2.0 * (t - 1.0) * inv;
    dw[2] = (t - 0.5) * inv;
    return true;
}
// false: the particle deposits nothing and gets no gradient (a non-finite position word, or |u| > 2^30 on an unprojected axis)
__host__ __device__ inline bool fe_dn_stencil(const FeDensitySpec& sp, const float* x, FeDensityStencil& st) {
    if (!fe_dn_finite(x[0]) || !fe_dn_finite(x[1]) || !fe_dn_finite(x[2])) return false;
    const bool ok0 = fe_dn_axis((double)x[0], sp.origin[0], sp.cell[0], sp.n[0], st.base[0], st.w[0], st.dw[0]);
    const bool ok1 = fe_dn_axis((double)x[1], sp.origin[1], sp.cell[1], sp.n[1], st.base[1], st.w[1], st.dw[1]);
    const bool ok2 = fe_dn_axis((double)x[2], sp.origin[2], sp.cell[2], sp.n[2], st.base[2], st.w[2], st.dw[2]);
    return ok0 && ok1 && ok2;
}
// the weight of stencil cell (i, j, k) and its fixed-point deposit
__host__ __device__ inline double fe_dn_weight(const FeDensityStencil& st, int i, int j, int k) { return st.w[0][i] * st.w[1][j] * st.w[2][k]; }
__host__ __device__ inline unsigned long long fe_dn_quant(double w) { return (unsigned long long)llrint(w * FE_DENSITY_FIX); }
__host__ __device__ inline double fe_dn_value(unsigned long long word) { return (double)word / FE_DENSITY_FIX; }
// d weight(i, j, k) / d x_a
__host__ __device__ inline double fe_dn_dweight(const FeDensityStencil& st, int i, int j, int k, int a) {
    return (a == 0 ? st.dw[0][i] : st.w[0][i]) * (a == 1 ? st.dw[1][j] : st.w[1][j]) * (a == 2 ? st.dw[2][k] : st.w[2][k]);
}
// The UNWEIGHTED gradient of sum_c r_c^2 with respect to the particle's position: g[a] = the sum over the in-range stencil cells, in the
// fixed order i, j, k, of 2 r_c d w_c / d x_a.  r: the field's residual D - T by linear cell index.
__host__ __device__ inline void fe_dn_grad(const FeDensitySpec& sp, const FeDensityStencil& st, const double* r, double* g /* [3] */) {
    g[0] = g[1] = g[2] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (!fe_dn_in(sp, 0, st.base[0] + i)) continue;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            if (!fe_dn_in(sp, 1, st.base[1] + j)) continue;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (!fe_dn_in(sp, 2, st.base[2] + k)) continue;
                const double rc = 2.0 * r[fe_dn_index(sp, st.base[0] + i, st.base[1] + j, st.base[2] + k)];
#pragma unroll
                for (int a = 0; a < 3; a++) g[a] += rc * fe_dn_dweight(st, i, j, k, a);
            }
        }
    }
}

#ifndef FE_DENSITY_MATH_ONLY
#define FE_DENSITY_WG 256
static_assert(FE_DENSITY_WG == FE_TL_WG, "k_density_resid sums its workgroup with fe_tl_wg_sum");
#define FE_DENSITY_MAX_WGS 512
// what k_task_bwd needs of the program's density terms, in term order: the field and the residual k_density_resid left
struct TaskDensity { FeDensitySpec spec[FE_TASK_LOSS_MAX_DENSITY_TERMS]; const double* r[FE_TASK_LOSS_MAX_DENSITY_TERMS]; };

// The scatter: one pass over the slots of the frame, grid-stride; every selected particle adds its deposits to the cell words.
//   LDS = true:  the workgroup accumulates a private copy of the field in dynamic LDS (n_cells words, 64-bit integer LDS adds) and, after a
//                barrier, adds its non-zero cells to `field` with one 64-bit integer global atomic each.
//   LDS = false: straight to 64-bit integer global atomics.
// `field` was zeroed on the stream.  Both roads add the same integers, so they give the same words.
template <bool LDS>
__global__ __launch_bounds__(FE_DENSITY_WG) void k_density_scatter(int N, size_t Np, float* fr_, const int* __restrict__ pid_of_slot, const float4* __restrict__ pinfo,
                                                                   FeDensitySpec sp, FeLossSel sel, int n_cells, unsigned long long* __restrict__ field) {
    extern __shared__ unsigned long long dn_cells[];
    if (LDS) {
        for (int c = threadIdx.x; c < n_cells; c += FE_DENSITY_WG) dn_cells[c] = 0ull;
        __syncthreads();
    }
    unsigned long long* dst = LDS ? dn_cells : field;
    const FrameV fr = frame_view(fr_, Np);
    for (int base = blockIdx.x * FE_DENSITY_WG; base < N; base += gridDim.x * FE_DENSITY_WG) {
        const int s = base + threadIdx.x;
        if (s >= N) continue;
        const int pid = pid_of_slot[s];
        if ((unsigned)pid >= (unsigned)N) continue;
        if (!fe_tl_selected(sel, pid, fe_tl_mat(pinfo, pid), fr.used[s])) continue;
        const float4 a0 = fr.A0[s];
        const float x[3] = {a0.x, a0.y, a0.z};
        FeDensityStencil st;
        if (!fe_dn_stencil(sp, x, st)) continue;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (!fe_dn_in(sp, 0, st.base[0] + i)) continue;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                if (!fe_dn_in(sp, 1, st.base[1] + j)) continue;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    if (!fe_dn_in(sp, 2, st.base[2] + k)) continue;
                    const unsigned long long q = fe_dn_quant(fe_dn_weight(st, i, j, k));
                    const long long c = fe_dn_index(sp, st.base[0] + i, st.base[1] + j, st.base[2] + k);      // (in [0, n_cells): every axis index was tested)
                    if (q != 0ull) atomicAdd(&dst[c], q);
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int c = threadIdx.x; c < n_cells; c += FE_DENSITY_WG) {
            const unsigned long long v = dn_cells[c];
            if (v != 0ull) atomicAdd(&field[c], v);
        }
    }
}

// Per cell: r = D - T in fp64, stored for the adjoint; partial[blockIdx.x] = the workgroup's sum of r^2 (nullptr: not wanted).  k_task_merge
// adds the partials in fixed order.
__global__ __launch_bounds__(FE_DENSITY_WG) void k_density_resid(int n_cells, const unsigned long long* __restrict__ field, const double* __restrict__ target,
                                                                 double* __restrict__ r, double* __restrict__ partial) {
    __shared__ double lds[FE_DENSITY_WG / 64];
    double acc = 0.0;
    for (int c = blockIdx.x * FE_DENSITY_WG + threadIdx.x; c < n_cells; c += gridDim.x * FE_DENSITY_WG) {
        const double d = fe_dn_value(field[c]) - target[c];
        r[c] = d;
        acc += d * d;
    }
    if (!partial) return;                                     // (uniform)
    const double v = fe_tl_wg_sum(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
}
#endif /* FE_DENSITY_MATH_ONLY */
#endif /* FE_DENSITY_H */
