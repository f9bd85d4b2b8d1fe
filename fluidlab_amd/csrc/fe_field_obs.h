// fe_field_obs.h -- Eulerian observations of a particle frame for closed-loop policies (include/fluidengine_ext.h: fe_field_obs_*): a small grid of
// "how much material is where, and how is it moving" -- density and momentum on the cells of a FeDensitySpec box, from the particles of a FeLossSel --
// and the adjoint of that grid back into the frame's x and v adjoints.  The stencil, the edge rules and the projected axes are those of the density
// fields (fe_density.h: fe_dn_stencil, fe_dn_in); channel 0 is the same words as fe_density_get of the same box and selection.
// Included by fe_engine.hip behind fe_policy_io.h.  Its kernels are template instantiations that take their arguments as one struct and read no
// blockDim / gridDim, and their first uses stand at the very end of fe_engine.hip, for the reason given in fe_policy_io.h and fe_render_scene.h:
// they land at the tail of the code object and every other kernel keeps its place.
// The first part -- the velocity guard, the momentum deposit and the per-particle adjoint sum -- is plain __host__ __device__ code:
// tests/csrc/field_obs_test.cpp compiles it for the host with FE_DENSITY_MATH_ONLY defined and checks it against plain loops.
//
// Fixed point (the contract): a density deposit is fe_dn_quant exactly, llrint(w 2^40) into an unsigned 64-bit word.  A momentum deposit is
// llrint(w v_a 2^28) as a signed 64-bit integer, added in two's complement to a 64-bit word, and decoded as (double)(long long)word / 2^28.  A
// particle deposits nothing in any channel, and gets no gradient, when the density guard drops it (a non-finite position word, |u| > 2^30), when
// a velocity word is not finite or when |v_a| > 2^10 on any axis.  With N <= 2^23 a momentum word stays below 2^23 2^10 2^28 = 2^61.  Every
// deposit is within 2^-29 of exact, a cell with k_c deposits within k_c 2^-29.  Integer addition does not depend on order: a field is the same
// bits on the LDS road and on the global road, with any number of workgroups.  No floating-point atomics, only integer LDS and global atomics
// and plain vector stores.
#ifndef FE_FIELD_OBS_H
#define FE_FIELD_OBS_H

#define FE_FIELD_OBS_FIX 268435456.0                        /* 2^28 */
#define FE_FIELD_OBS_MAX_V 1024.0                           /* 2^10: |v_a| above it deposits nothing */

// false: the particle deposits nothing in any channel and gets no gradient (a non-finite velocity word, or |v_a| > 2^10)
__host__ __device__ inline bool fe_fo_v_ok(const float* v) {
    if (!fe_dn_finite(v[0]) || !fe_dn_finite(v[1]) || !fe_dn_finite(v[2])) return false;
    return fabs((double)v[0]) <= FE_FIELD_OBS_MAX_V && fabs((double)v[1]) <= FE_FIELD_OBS_MAX_V && fabs((double)v[2]) <= FE_FIELD_OBS_MAX_V;
}
// the momentum deposit of weight w and velocity word va: a signed integer in a two's-complement word; and the word's value
__host__ __device__ inline unsigned long long fe_fo_quant(double w, float va) { return (unsigned long long)llrint(w * (double)va * FE_FIELD_OBS_FIX); }
__host__ __device__ inline double fe_fo_value(unsigned long long word) { return (double)(long long)word / FE_FIELD_OBS_FIX; }
// The adjoint of one particle for a cotangent G[channels][n_cells]: over the in-field stencil cells in the fixed order i, j, k, in fp64,
//   gx[a] = sum_c (G_0[c] + sum_b G_{1+b}[c] v_b) d w_c / d x_a,    gv[b] = sum_c G_{1+b}[c] w_c  (channels == 4; else gv = 0)
template <typename T>
__host__ __device__ inline void fe_fo_grad(const FeDensitySpec& sp, const FeDensityStencil& st, const T* G, long long n_cells, int channels, const float* v, double* gx /* [3] */, double* gv /* [3] */) {
    gx[0] = gx[1] = gx[2] = 0.0;
    gv[0] = gv[1] = gv[2] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (!fe_dn_in(sp, 0, st.base[0] + i)) continue;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            if (!fe_dn_in(sp, 1, st.base[1] + j)) continue;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (!fe_dn_in(sp, 2, st.base[2] + k)) continue;
                const long long c = fe_dn_index(sp, st.base[0] + i, st.base[1] + j, st.base[2] + k);
                double coef = (double)G[c];
                if (channels == 4) {
                    const double w = fe_dn_weight(st, i, j, k);
#pragma unroll
                    for (int b = 0; b < 3; b++) {
                        const double gb = (double)G[(1 + b) * n_cells + c];
                        coef += gb * (double)v[b];
                        gv[b] += gb * w;
                    }
                }
#pragma unroll
                for (int a = 0; a < 3; a++) gx[a] += coef * fe_dn_dweight(st, i, j, k, a);
            }
        }
    }
}

#ifndef FE_DENSITY_MATH_ONLY
#define FE_FIELD_OBS_WG 256

// The scatter: one pass over the slots of the frame, grid-stride (a.stride threads in the grid); every selected particle that passes the guards
// computes its stencil once and adds its deposits to the words of all channels, words[ch * n_cells + c].
//   LDS = true:  the workgroup accumulates private copies of all channels in dynamic LDS (channels * n_cells words, 64-bit integer LDS adds) and,
//                after a barrier, adds its non-zero words to `words` with one 64-bit integer global atomic each.
//   LDS = false: straight to 64-bit integer global atomics.
// `words` was zeroed on the stream.  Both roads add the same integers, so they give the same words.
struct FieldObsScatterArgs { int N; unsigned Np; float* fr; const int* pid_of_slot; const float4* pinfo; FeDensitySpec sp; FeLossSel sel; int n_cells, channels, stride; unsigned long long* words; };
template <bool LDS>
__global__ __launch_bounds__(FE_FIELD_OBS_WG) void k_field_obs_scatter(FieldObsScatterArgs a) {
    extern __shared__ unsigned long long fo_cells[];
    const int n_words = a.channels * a.n_cells;
    if (LDS) {
        for (int c = threadIdx.x; c < n_words; c += FE_FIELD_OBS_WG) fo_cells[c] = 0ull;
        __syncthreads();
    }
    unsigned long long* dst = LDS ? fo_cells : a.words;
    const FrameV fr = frame_view(a.fr, a.Np);
    for (int base = blockIdx.x * FE_FIELD_OBS_WG; base < a.N; base += a.stride) {
        const int s = base + threadIdx.x;
        if (s >= a.N) continue;
        const int pid = a.pid_of_slot[s];
        if ((unsigned)pid >= (unsigned)a.N) continue;
        if (!fe_tl_selected(a.sel, pid, fe_tl_mat(a.pinfo, pid), fr.used[s])) continue;
        const float4 a0 = fr.A0[s];
        const float x[3] = {a0.x, a0.y, a0.z};
        FeDensityStencil st;
        if (!fe_dn_stencil(a.sp, x, st)) continue;
        const float4 a1 = fr.A1[s];
        const float v[3] = {a0.w, a1.x, a1.y};
        if (!fe_fo_v_ok(v)) continue;                         // (with one channel too: channel 0 is the same field whatever the channel count)
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (!fe_dn_in(a.sp, 0, st.base[0] + i)) continue;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                if (!fe_dn_in(a.sp, 1, st.base[1] + j)) continue;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    if (!fe_dn_in(a.sp, 2, st.base[2] + k)) continue;
                    const double w = fe_dn_weight(st, i, j, k);
                    const long long c = fe_dn_index(a.sp, st.base[0] + i, st.base[1] + j, st.base[2] + k);      // (in [0, n_cells): every axis index was tested)
                    const unsigned long long q = fe_dn_quant(w);
                    if (q != 0ull) atomicAdd(&dst[c], q);
                    if (a.channels == 4) {
#pragma unroll
                        for (int b = 0; b < 3; b++) {
                            const unsigned long long m = fe_fo_quant(w, v[b]);
                            if (m != 0ull) atomicAdd(&dst[(size_t)(1 + b) * a.n_cells + c], m);
                        }
                    }
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int c = threadIdx.x; c < n_words; c += FE_FIELD_OBS_WG) {
            const unsigned long long v = fo_cells[c];
            if (v != 0ull) atomicAdd(&a.words[c], v);
        }
    }
}

// words -> fe_real values [channels][n0][n1][n2], through fp64: channel 0 as fe_dn_value, the momentum channels as fe_fo_value
struct FieldObsDecodeArgs { int n_cells, channels; const unsigned long long* words; fe_real* out; };
template <int TAIL>
__global__ __launch_bounds__(FE_FIELD_OBS_WG) void k_field_obs_decode(FieldObsDecodeArgs a) {
    const long long c = (long long)blockIdx.x * FE_FIELD_OBS_WG + threadIdx.x;
    if (c >= (long long)a.channels * a.n_cells) return;
    const unsigned long long w = a.words[c];
    a.out[c] = (fe_real)(c < a.n_cells ? fe_dn_value(w) : fe_fo_value(w));
}

// The adjoint: a gather, one thread per slot of the frame, no atomics.  x and v are read from frame f in the frame's own order; the sums of
// fe_fo_grad are rounded to fp32 once and added once to the particle's slot of the adjoint, found through the slot_of_pid of the ADJOINT slot's
// own order (adj_slot), which across a sort boundary is not the frame's.  Only the x and v words are written: C's two words that
// share a float4 with v are stored back as read (the thread is the only writer of its slot), F's planes are not touched.
struct FieldObsGradArgs { int N; unsigned Np; float* fr; float* gr; const int* pid_of_slot; const int* grad_slot_of_pid; const float4* pinfo; FeDensitySpec sp; FeLossSel sel; int n_cells, channels; const fe_real* G; };
template <int TAIL>
__global__ __launch_bounds__(FE_FIELD_OBS_WG) void k_field_obs_grad(FieldObsGradArgs a) {
    const int s = blockIdx.x * FE_FIELD_OBS_WG + threadIdx.x;
    if (s >= a.N) return;
    const int pid = a.pid_of_slot[s];
    if ((unsigned)pid >= (unsigned)a.N) return;
    const FrameV fr = frame_view(a.fr, a.Np);
    if (!fe_tl_selected(a.sel, pid, fe_tl_mat(a.pinfo, pid), fr.used[s])) return;
    const float4 a0 = fr.A0[s];
    const float x[3] = {a0.x, a0.y, a0.z};
    FeDensityStencil st;
    if (!fe_dn_stencil(a.sp, x, st)) return;
    const float4 a1 = fr.A1[s];
    const float v[3] = {a0.w, a1.x, a1.y};
    if (!fe_fo_v_ok(v)) return;
    const int sg = a.grad_slot_of_pid[pid];
    if ((unsigned)sg >= a.Np) return;
    double gx[3], gv[3];
    fe_fo_grad(a.sp, st, a.G, (long long)a.n_cells, a.channels, v, gx, gv);
    const FrameV g = frame_view(a.gr, a.Np);
    float4 g0 = g.A0[sg];
    g0.x += (float)gx[0]; g0.y += (float)gx[1]; g0.z += (float)gx[2];
    if (a.channels == 4) {
        float4 g1 = g.A1[sg];
        g0.w += (float)gv[0]; g1.x += (float)gv[1]; g1.y += (float)gv[2];
        g.A1[sg] = g1;
    }
    g.A0[sg] = g0;
}

// ---------------------------------------------------------------------------------------------------------------- host
struct FieldObsState {
    FeDensitySpec spec[FE_FIELD_OBS_MAX] = {};                // the fields (n[0] == 0: not set)
    FeLossSel sel[FE_FIELD_OBS_MAX] = {};
    int channels[FE_FIELD_OBS_MAX] = {};
    unsigned long long* words[FE_FIELD_OBS_MAX] = {};         // per field: [channels][cells] cell words,
    fe_real* g[FE_FIELD_OBS_MAX] = {};                        // ... and the cotangent (staging of the host form of fe_field_obs_add_grad)
    size_t cap[FE_FIELD_OBS_MAX] = {};                        // values each of the two holds (grown by fe_field_obs_set)
    int lds_limit = -1;                                       // the device's LDS bytes per workgroup (asked at the first scatter)
    size_t lds_attr = 0;                                      // the largest dynamic-LDS size k_field_obs_scatter<true> has been given leave for (beyond 64 KiB; this engine's device)
};
static FieldObsState* field_obs_state(FeEngine* h) {
    if (!h->field_obs) h->field_obs = new FieldObsState();
    return h->field_obs;
}
static void field_obs_drop(FeEngine* h) {                     // fe_destroy
    FieldObsState* Q = h->field_obs;
    if (!Q) return;
    for (int k = 0; k < FE_FIELD_OBS_MAX; k++) for (void* q : {(void*)Q->words[k], (void*)Q->g[k]}) if (q) (void)hipFree(q);
    delete Q;
    h->field_obs = nullptr;
}
// The launches, defined at the end of fe_engine.hip behind every other first use of a template kernel (see the head of this file)
static int field_obs_scatter(FeEngine* h, int f, int k);                          // the words of field k from frame f (zeroed on the stream first)
static void field_obs_decode(FeEngine* h, int k, fe_real* out);                   // ... as values
static int field_obs_grad(FeEngine* h, int f, int k, const fe_real* G);          // ... and the adjoint of G into the adjoint of frame f (adj_slot, ADJ_ADD: a cleared slot takes the frame's order here)

namespace {

long long field_obs_values(const FieldObsState* Q, int k) { return (long long)Q->channels[k] * fe_dn_cells(Q->spec[k]); }
// the refusals shared by the reads and the adjoint entries: nothing has changed when one of them returns non-zero
int field_obs_check(FeEngine* h, int f, int k, const char* who) {
    CHECK_FRAME(h, f);
    if (k < 0 || k >= FE_FIELD_OBS_MAX) FAIL(h, std::string(who) + ": field id out of range");
    if (!h->field_obs || h->field_obs->spec[k].n[0] == 0) FAIL(h, std::string(who) + ": the field is not set: fe_field_obs_set first");
    return 0;
}
int field_obs_grad_check(FeEngine* h, int f, int k, const fe_real* G, const char* who) {
    if (field_obs_check(h, f, k, who)) return 1;
    if (!G) FAIL(h, std::string(who) + ": G is NULL (no adjoint word has changed)");
    return adj_slot(h, f, ADJ_READ);                          // (the refusal alone: the slot takes its order where the entry launches)
}

} // namespace

extern "C" {

int fe_field_obs_set(FeEngine* h, int k, const FeDensitySpec* spec, int spec_size, const FeLossSel* sel, int channels) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (k < 0 || k >= FE_FIELD_OBS_MAX) FAIL(h, "fe_field_obs_set: field id out of range (nothing is changed)");
    if (!spec) {                                              // remove: the buffers stay for a later field of this id
        if (!h->field_obs) return 0;
        HIPCK(h, hipStreamSynchronize(h->stream));
        h->field_obs->spec[k] = FeDensitySpec{}; h->field_obs->channels[k] = 0;
        return 0;
    }
    if (spec_size != (int)sizeof(FeDensitySpec)) FAIL(h, "fe_field_obs_set: spec_size is not sizeof(FeDensitySpec) (the field is unchanged)");
    if (h->N > (1 << 23)) FAIL(h, "fe_field_obs_set: engines with N > 2^23 particles are refused (a cell word could overflow)");
    if (channels != 1 && channels != 4) FAIL(h, "fe_field_obs_set: channels must be 1 (density) or 4 (density and momentum) (the field is unchanged)");
    long long cells = 1;
    for (int a = 0; a < 3; a++) {
        if (spec->n[a] < 1) FAIL(h, "fe_field_obs_set: n[a] must be >= 1 on every axis (the field is unchanged)");
        if (spec->n[a] > FE_DENSITY_MAX_CELLS) FAIL(h, "fe_field_obs_set: more than FE_DENSITY_MAX_CELLS cells (the field is unchanged)");
        cells *= spec->n[a];
        if (cells > FE_DENSITY_MAX_CELLS) FAIL(h, "fe_field_obs_set: more than FE_DENSITY_MAX_CELLS cells (the field is unchanged)");
        if (!(spec->cell[a] > 0.0) || !(spec->cell[a] - spec->cell[a] == 0.0)) FAIL(h, "fe_field_obs_set: cell must be finite and positive on every axis (the field is unchanged)");
        if (!(spec->origin[a] - spec->origin[a] == 0.0)) FAIL(h, "fe_field_obs_set: origin must be finite (the field is unchanged)");
    }
    const FeLossSel all = {0, h->N, -1, 1};
    const FeLossSel S = sel ? *sel : all;
    if (!tl_sel_ok(S, h->N)) FAIL(h, "fe_field_obs_set: pid range of the selection outside [0, N] (the field is unchanged)");
    FieldObsState* Q = field_obs_state(h);
    const size_t need = (size_t)channels * (size_t)cells;
    if (need > Q->cap[k]) {                                   // (buffers of their own, swapped in once both exist)
        unsigned long long* w = nullptr; fe_real* g = nullptr;
        if (dev_alloc(h, &w, need, false) || dev_alloc(h, &g, need, false)) {
            for (void* q : {(void*)w, (void*)g}) if (q) (void)hipFree(q);
            return 1;
        }
        HIPCK(h, hipStreamSynchronize(h->stream));           // (an earlier call may still use the old buffers)
        for (void* q : {(void*)Q->words[k], (void*)Q->g[k]}) if (q) (void)hipFree(q);
        Q->words[k] = w; Q->g[k] = g; Q->cap[k] = need;
    }
    Q->spec[k] = *spec; Q->spec[k].pad = 0; Q->sel[k] = S; Q->channels[k] = channels;
    return 0;
}
// the field of frame f, [channels][n0][n1][n2] in fp64, to the host; waits
int fe_field_obs_get(FeEngine* h, int f, int k, double* out, long long n_values) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (field_obs_check(h, f, k, "fe_field_obs_get")) return 1;
    FieldObsState* Q = h->field_obs;
    if (n_values != field_obs_values(Q, k)) FAIL(h, "fe_field_obs_get: n_values does not match the field (channels * cells)");
    if (!out) FAIL(h, "fe_field_obs_get: null output");
    if (field_obs_scatter(h, f, k)) return 1;
    std::vector<unsigned long long> words((size_t)n_values);
    HIPCK(h, hipMemcpyAsync(words.data(), Q->words[k], sizeof(unsigned long long) * (size_t)n_values, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    const long long cells = fe_dn_cells(Q->spec[k]);
    for (long long c = 0; c < n_values; c++) out[c] = c < cells ? fe_dn_value(words[(size_t)c]) : fe_fo_value(words[(size_t)c]);
    return check_device_errors(h);
}
// the same as fe_real values through a device pointer (waits for the engine's stream, as fe_obs_get_dev does)
int fe_field_obs_get_dev(FeEngine* h, int f, int k, fe_real* out) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (field_obs_check(h, f, k, "fe_field_obs_get_dev")) return 1;
    if (!out) FAIL(h, "fe_field_obs_get_dev: null output");
    if (field_obs_scatter(h, f, k)) return 1;
    field_obs_decode(h, k, out);
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    return check_device_errors(h);
}
// the adjoint: G [channels][n0][n1][n2] in fe_real, host pointer (staged, waits)
int fe_field_obs_add_grad(FeEngine* h, int f, int k, const fe_real* G) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (field_obs_grad_check(h, f, k, G, "fe_field_obs_add_grad")) return 1;
    FieldObsState* Q = h->field_obs;
    if (h->N == 0) return 0;
    HIPCK(h, hipMemcpyAsync(Q->g[k], G, sizeof(fe_real) * (size_t)field_obs_values(Q, k), hipMemcpyHostToDevice, h->stream));
    if (field_obs_grad(h, f, k, Q->g[k])) return 1;
    HIPCK(h, hipStreamSynchronize(h->stream));
    return check_async(h);
}
// the same from a device pointer
int fe_field_obs_add_grad_dev(FeEngine* h, int f, int k, const fe_real* G) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (field_obs_grad_check(h, f, k, G, "fe_field_obs_add_grad_dev")) return 1;
    if (h->N == 0) return 0;
    if (field_obs_grad(h, f, k, G)) return 1;
    HIPCK(h, hipStreamSynchronize(h->stream));
    return check_async(h);
}

}  // extern "C"
#endif /* FE_DENSITY_MATH_ONLY */
#endif /* FE_FIELD_OBS_H */
