// fe_density.h -- density fields of a frame and the density term of the loss-term programs (include/fluidengine_ext.h: fe_density_*,
// FE_TERM_DENSITY_SQ).  Included by fe_task_loss.h between its helpers (the selection test, workgroup sums, frame views), which the kernels here use, and k_task_bwd.
// The first part -- the quadratic B-spline stencil of one particle on one field, its derivative, the guard and the fixed-point deposit -- is
// plain __host__ __device__ code: tests/csrc/density_test.cpp compiles it for the host with FE_DENSITY_MATH_ONLY defined and checks it against
// plain loops.  Behind the kernels: the state (DensityState, one pointer in FeEngine), density_drop for fe_destroy and the fe_density_* entries.
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

// ---------------------------------------------------------------------------------------------------------------- host
#define FE_DN_SLOTS (FE_TASK_LOSS_MAX_DENSITY_TERMS + 1)    /* users of a field's buffers: the program's density terms in term order, then fe_density_get */
struct DensityState {
    FeDensitySpec spec[FE_DENSITY_MAX_FIELDS] = {};           // the fields (n[0] == 0: not set)
    double* target[FE_DENSITY_MAX_FIELDS] = {}; bool has_target[FE_DENSITY_MAX_FIELDS] = {};     // their targets, [cells] fp64 on the device
    unsigned long long* words[FE_DN_SLOTS] = {}; double* r[FE_DN_SLOTS] = {}; size_t cap[FE_DN_SLOTS] = {};     // per user: the cell words and the residual D - T (grown on demand)
};
// every entry starts from the state, empty at first: no field is set in it, which is what an entry called before any set-up is told
static DensityState* density_state(FeEngine* h) {
    if (!h->density) h->density = new DensityState();
    return h->density;
}
static void density_drop(FeEngine* h) {                       // fe_destroy
    DensityState* D = h->density;
    if (!D) return;
    for (double* q : D->target) if (q) (void)hipFree(q);
    for (int k = 0; k < FE_DN_SLOTS; k++) for (void* q : {(void*)D->words[k], (void*)D->r[k]}) if (q) (void)hipFree(q);
    delete D;
    h->density = nullptr;
}
// room for `cells` cell words and residuals of field user `slot`
static int density_reserve(FeEngine* h, int slot, size_t cells) {
    DensityState* D = density_state(h);
    if (cells <= D->cap[slot]) return 0;
    HIPCK(h, hipStreamSynchronize(h->stream));               // (an earlier step may still use the old buffers)
    if (D->words[slot]) (void)hipFree(D->words[slot]);
    if (D->r[slot]) (void)hipFree(D->r[slot]);
    D->words[slot] = nullptr; D->r[slot] = nullptr; D->cap[slot] = 0;
    if (dev_alloc(h, &D->words[slot], cells, false) || dev_alloc(h, &D->r[slot], cells, false)) return 1;
    D->cap[slot] = cells;
    return 0;
}
// the field of frame f from the particles of `sel`, into the cell words of user `slot` (zeroed on the stream first).  Defined in fe_engine.hip behind
// every extension header: it is the first use of k_density_scatter<>, and template kernels sit in the code object in the order of their first use
static void density_scatter(FeEngine* h, int f, const FeDensitySpec& sp, const FeLossSel& sel, int slot);
static int density_resid_wgs(const FeDensitySpec& sp) { return (int)std::max<long long>(1, std::min<long long>((fe_dn_cells(sp) + FE_DENSITY_WG - 1) / FE_DENSITY_WG, FE_DENSITY_MAX_WGS)); }

extern "C" {

int fe_density_set_field(FeEngine* h, int field, const FeDensitySpec* spec, int spec_size) {
    FE_ENTRY(h);
    DensityState* D = density_state(h);
    if (field < 0 || field >= FE_DENSITY_MAX_FIELDS) FAIL(h, "fe_density_set_field: field id out of range (nothing is changed)");
    if (spec) {
        if (spec_size != (int)sizeof(FeDensitySpec)) FAIL(h, "fe_density_set_field: spec_size is not sizeof(FeDensitySpec) (the field is unchanged)");
        if (h->N > (1 << 23)) FAIL(h, "fe_density_set_field: engines with N > 2^23 particles are refused (a cell word could overflow)");
        long long cells = 1;
        for (int a = 0; a < 3; a++) {
            if (spec->n[a] < 1) FAIL(h, "fe_density_set_field: n[a] must be >= 1 on every axis (the field is unchanged)");
            if (spec->n[a] > FE_DENSITY_MAX_CELLS) FAIL(h, "fe_density_set_field: more than FE_DENSITY_MAX_CELLS cells (the field is unchanged)");
            cells *= spec->n[a];
            if (cells > FE_DENSITY_MAX_CELLS) FAIL(h, "fe_density_set_field: more than FE_DENSITY_MAX_CELLS cells (the field is unchanged)");
            if (!(spec->cell[a] > 0.0) || !(spec->cell[a] - spec->cell[a] == 0.0)) FAIL(h, "fe_density_set_field: cell must be finite and positive on every axis (the field is unchanged)");
            if (!(spec->origin[a] - spec->origin[a] == 0.0)) FAIL(h, "fe_density_set_field: origin must be finite (the field is unchanged)");
        }
    }
    HIPCK(h, hipStreamSynchronize(h->stream));               // (an earlier step may still read the old target)
    if (D->target[field]) (void)hipFree(D->target[field]);
    D->target[field] = nullptr; D->has_target[field] = false;
    if (spec) { D->spec[field] = *spec; D->spec[field].pad = 0; }
    else D->spec[field] = FeDensitySpec{};
    return 0;
}
int fe_density_set_target(FeEngine* h, int field, const double* target, long long n_cells) {
    FE_ENTRY(h);
    DensityState* D = density_state(h);
    if (field < 0 || field >= FE_DENSITY_MAX_FIELDS) FAIL(h, "fe_density_set_target: field id out of range (nothing is changed)");
    if (D->spec[field].n[0] == 0) FAIL(h, "fe_density_set_target: the field is not set: fe_density_set_field first");
    if (n_cells != fe_dn_cells(D->spec[field])) FAIL(h, "fe_density_set_target: n_cells does not match the field (the target is unchanged)");
    if (!target) FAIL(h, "fe_density_set_target: null target (the target is unchanged)");
    double* d_t = nullptr;                                    // (a buffer of its own, swapped in once it is complete)
    if (dev_alloc(h, &d_t, (size_t)n_cells, false)) return 1;
    if (hipMemcpyOnStream(h, d_t, target, sizeof(double) * (size_t)n_cells, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_t); FAIL(h, "fe_density_set_target: hipMemcpy failed (the target is unchanged)"); }
    if (D->target[field]) (void)hipFree(D->target[field]);
    D->target[field] = d_t; D->has_target[field] = true;
    return 0;
}
int fe_density_get(FeEngine* h, int f, int field, const FeLossSel* sel, double* out, long long n_cells) {
    FE_ENTRY(h);
    DensityState* D = density_state(h);
    CHECK_FRAME(h, f);
    if (field < 0 || field >= FE_DENSITY_MAX_FIELDS) FAIL(h, "fe_density_get: field id out of range");
    const FeDensitySpec& sp = D->spec[field];
    if (sp.n[0] == 0) FAIL(h, "fe_density_get: the field is not set: fe_density_set_field first");
    if (n_cells != fe_dn_cells(sp)) FAIL(h, "fe_density_get: n_cells does not match the field");
    if (!out) FAIL(h, "fe_density_get: null output");
    const FeLossSel all = {0, h->N, -1, 1};
    const FeLossSel S = sel ? *sel : all;
    if (!tl_sel_ok(S, h->N)) FAIL(h, "fe_density_get: pid range of the selection outside [0, N]");
    const int slot = FE_TASK_LOSS_MAX_DENSITY_TERMS;
    if (density_reserve(h, slot, (size_t)n_cells)) return 1;
    density_scatter(h, f, sp, S, slot);
    std::vector<unsigned long long> words((size_t)n_cells);
    HIPCK(h, hipMemcpyAsync(words.data(), D->words[slot], sizeof(unsigned long long) * (size_t)n_cells, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    for (long long c = 0; c < n_cells; c++) out[c] = fe_dn_value(words[(size_t)c]);
    return check_device_errors(h);
}

}  // extern "C"
#endif /* FE_DENSITY_MATH_ONLY */
#endif /* FE_DENSITY_H */
