// fe_task_loss.h -- the task losses evaluated in the engine: loss-term programs (include/fluidengine_ext.h: fe_task_loss_*).
// Included by fe_engine.hip behind struct FeEngine and its helpers, behind fe_summary.h: the kernels use the engine's frame views and order tables,
// the host half at the end -- the state (TaskLossState, one pointer in FeEngine), task_loss_drop for fe_destroy, the entries -- the engine itself and
// the host halves of fe_density.h and fe_nearest.h, which this header includes between its kernels.  The first part -- the selection
// test, value and gradient of the separable kinds, the pair contribution, the fixed-order merge of partial sums -- is plain
// __host__ __device__ code without any of that: tests/csrc/task_loss_test.cpp compiles it for the host with FE_TASK_LOSS_MATH_ONLY defined
// and checks it against plain fp64 loops.
//
// Every difference, product and sum is formed in fp64 from the fp32 position words.  No floating-point atomics anywhere: a workgroup leaves
// one partial sum per term, k_task_merge adds them in index order.  The forward kernels only READ the frame, the order table and pinfo.
#ifndef FE_TASK_LOSS_H
#define FE_TASK_LOSS_H

// particle `pid` of material `mat` with flag `used` is selected by s
__host__ __device__ inline bool fe_tl_selected(const FeLossSel& s, int pid, int mat, int used) {
    if (pid < s.pid_lo || pid >= s.pid_hi) return false;
    if (s.mat >= 0 && mat != s.mat) return false;
    if (s.require_used != 0 && used == 0) return false;
    return true;
}
__host__ __device__ inline bool fe_tl_separable(int kind) { return kind == FE_TERM_L1_CONST || kind == FE_TERM_SQ_CONST || kind == FE_TERM_L1_REF; }
__host__ __device__ inline double fe_tl_abs(double d) { return d < 0.0 ? -d : d; }
__host__ __device__ inline double fe_tl_sign(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0); }
// the point a separable term measures the distance to, on axis a: the constant, or the remembered position
__host__ __device__ inline double fe_tl_anchor(const FeLossTerm& t, const float* ref, int a) { return t.kind == FE_TERM_L1_REF ? (double)ref[a] : t.c[a]; }
// One selected particle's UNWEIGHTED value of a separable term: the sum over the axes in the mask.  x, ref: the particle's three fp32 words.
__host__ __device__ inline double fe_tl_sep_value(const FeLossTerm& t, const float* x, const float* ref) {
    double v = 0.0;
    for (int a = 0; a < 3; a++) {
        if (!((t.axis_mask >> a) & 1)) continue;
        const double d = (double)x[a] - fe_tl_anchor(t, ref, a);
        v += t.kind == FE_TERM_SQ_CONST ? d * d : fe_tl_abs(d);
    }
    return v;
}
// ... and its WEIGHTED derivative with respect to x_a (0 on an axis outside the mask): sign(d) w, or (2 d) w
__host__ __device__ inline double fe_tl_sep_grad(const FeLossTerm& t, const float* x, const float* ref, int a) {
    if (!((t.axis_mask >> a) & 1)) return 0.0;
    const double d = (double)x[a] - fe_tl_anchor(t, ref, a);
    return (t.kind == FE_TERM_SQ_CONST ? 2.0 * d : fe_tl_sign(d)) * t.weight;
}
// One pair on one axis: |a - b| in fp64 and the sign of a - b (0 at a tie, so i == j of a self-pair term adds nothing).
__host__ __device__ inline void fe_tl_pair(float a, float b, double& absd, int& sgn) {
    const double d = (double)a - (double)b;
    absd = fe_tl_abs(d);
    sgn = (d > 0.0) - (d < 0.0);
}
// the weighted pair gradient of one particle and axis from its integer count (#{other < x} - #{other > x}); a self-pair term counts every
// unordered pair twice
__host__ __device__ inline double fe_tl_pair_grad(const FeLossTerm& t, int count) { return t.weight * ((t.b.pid_lo < 0 ? 2.0 : 1.0) * (double)count); }

// The fixed-order merge of n partial sums: lane l of 64 adds the partials l, l + 64, ... in order, then the 64 lane sums are combined by the
// butterfly v[l] += v[l ^ o], o = 32 .. 1 (on the device: __shfl_xor).  The result depends on n and the values only.
#define FE_TL_LANES 64
__host__ __device__ inline double fe_tl_lane_sum(const double* part, int n, int lane) {
    double v = 0.0;
    for (int i = lane; i < n; i += FE_TL_LANES) v += part[i];
    return v;
}
__host__ __device__ inline double fe_tl_butterfly(double* v /* [FE_TL_LANES], overwritten */) {
    for (int o = FE_TL_LANES / 2; o > 0; o >>= 1) {
        double w[FE_TL_LANES];
        for (int l = 0; l < FE_TL_LANES; l++) w[l] = v[l] + v[l ^ o];
        for (int l = 0; l < FE_TL_LANES; l++) v[l] = w[l];
    }
    return v[0];
}
__host__ __device__ inline double fe_tl_merge(const double* part, int n) {
    double v[FE_TL_LANES];
    for (int l = 0; l < FE_TL_LANES; l++) v[l] = fe_tl_lane_sum(part, n, l);
    return fe_tl_butterfly(v);
}

#ifndef FE_TASK_LOSS_MATH_ONLY
#define FE_TL_WG 256
#define FE_TL_SEP_MAX_WGS 512
// where each term's workgroup partials sit in the partial buffer
struct TaskLayout { int off[FE_TASK_LOSS_MAX_TERMS]; int np[FE_TASK_LOSS_MAX_TERMS]; };

__device__ __forceinline__ double fe_tl_wave_sum(double v) {                 // the butterfly of fe_tl_butterfly: every lane ends with the same sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the workgroup's sum, waves in order; valid in thread 0 (all threads of the workgroup call it)
__device__ __forceinline__ double fe_tl_wg_sum(double v, double* lds /* [FE_TL_WG / 64] */) {
    v = fe_tl_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) for (int w = 0; w < FE_TL_WG / 64; w++) t += lds[w];
    return t;
}
__device__ __forceinline__ int fe_tl_mat(const float4* __restrict__ pinfo, int pid) { return (__float_as_int(pinfo[pid].w) >> 16) & 0xffff; }

// ref[pid] = x[f, pid]
__global__ __launch_bounds__(256) void k_task_set_ref(int N, size_t Np, float* fr_, const int* __restrict__ slot_of_pid, float* __restrict__ ref) {
    const int pid = blockIdx.x * blockDim.x + threadIdx.x;
    if (pid >= N) return;
    const int s = slot_of_pid[pid];
    if ((unsigned)s >= (unsigned)Np) return;
    const float4 a0 = frame_view(fr_, Np).A0[s];
    ref[3 * (size_t)pid] = a0.x; ref[3 * (size_t)pid + 1] = a0.y; ref[3 * (size_t)pid + 2] = a0.z;
}

// All separable terms in one pass over the slots of the frame, grid-stride: one fp64 accumulator per term, reduced in the wave, then over the
// waves in order; partial[L.off[t] + blockIdx.x] = the workgroup's unweighted sum of term t.
__global__ __launch_bounds__(FE_TL_WG) void k_task_sep_fwd(int N, size_t Np, float* fr_, const int* __restrict__ pid_of_slot, const float4* __restrict__ pinfo,
                                                           const float* __restrict__ ref, const FeLossTerm* __restrict__ terms, int n_terms, TaskLayout L,
                                                           double* __restrict__ partial) {
    __shared__ double lds[FE_TL_WG / 64];
    const FrameV fr = frame_view(fr_, Np);
    double acc[FE_TASK_LOSS_MAX_TERMS];
#pragma unroll
    for (int t = 0; t < FE_TASK_LOSS_MAX_TERMS; t++) acc[t] = 0.0;
    for (int base = blockIdx.x * FE_TL_WG; base < N; base += gridDim.x * FE_TL_WG) {
        const int s = base + threadIdx.x;
        if (s >= N) continue;
        const int pid = pid_of_slot[s];
        if ((unsigned)pid >= (unsigned)N) continue;
        const int used = fr.used[s], mat = fe_tl_mat(pinfo, pid);
        const float4 a0 = fr.A0[s];
        const float x[3] = {a0.x, a0.y, a0.z};
        float r[3] = {0.f, 0.f, 0.f};
        if (ref) { r[0] = ref[3 * (size_t)pid]; r[1] = ref[3 * (size_t)pid + 1]; r[2] = ref[3 * (size_t)pid + 2]; }
#pragma unroll
        for (int t = 0; t < FE_TASK_LOSS_MAX_TERMS; t++) {
            if (t >= n_terms) break;
            const FeLossTerm& T = terms[t];
            if (fe_tl_separable(T.kind) && fe_tl_selected(T.a, pid, mat, used)) acc[t] += fe_tl_sep_value(T, x, r);
        }
    }
#pragma unroll
    for (int t = 0; t < FE_TASK_LOSS_MAX_TERMS; t++) {
        if (t >= n_terms) break;                              // (uniform)
        if (!fe_tl_separable(terms[t].kind)) continue;
        const double v = fe_tl_wg_sum(acc[t], lds);
        if (threadIdx.x == 0) partial[L.off[t] + blockIdx.x] = v;
    }
}

// The tiled all-pairs kernel.  The sets are pid ranges: thread i of workgroup (bx, by) owns particle own.pid_lo + bx * 256 + i and reaches its
// row through the frame's slot_of_pid; the workgroup stages rows other.pid_lo + by * chunk ... of the other set, reached the same way, 256 at a
// time in LDS (fp64, a row that fails the selection flagged invalid), and every lane walks the tile reading the same address (LDS broadcast).
//   GRAD = false: partial[by * gridDim.x + bx] = the workgroup's sum over its pairs and the axes of the mask of |x_i - x_j| (fp64, unweighted)
//   GRAD = true:  cnt[axis * N + pid] (+)= #{other < x_i} - #{other > x_i} over the chunk: a plain store when the set is one chunk, an integer
//                 atomicAdd onto a zeroed buffer when it is several.
struct TaskPairRow { double x[3]; int valid, pad; };
template <bool GRAD>
__global__ __launch_bounds__(FE_TL_WG) void k_task_pair(int N, size_t Np, float* fr_, const int* __restrict__ slot_of_pid, const float4* __restrict__ pinfo,
                                                        FeLossSel own, FeLossSel other, int axis_mask, int chunk, double* __restrict__ partial, int* __restrict__ cnt) {
    __shared__ TaskPairRow tile[FE_TL_WG];
    __shared__ double lds[FE_TL_WG / 64];
    const FrameV fr = frame_view(fr_, Np);
    const int tid = threadIdx.x;
    const int pid = own.pid_lo + blockIdx.x * FE_TL_WG + tid;
    bool mine = false;
    double x[3] = {0.0, 0.0, 0.0};
    if (pid < own.pid_hi && (unsigned)pid < (unsigned)N) {
        const int s = slot_of_pid[pid];
        if ((unsigned)s < (unsigned)Np && fe_tl_selected(own, pid, fe_tl_mat(pinfo, pid), fr.used[s])) {
            const float4 a0 = fr.A0[s];
            x[0] = a0.x; x[1] = a0.y; x[2] = a0.z; mine = true;
        }
    }
    double acc = 0.0;
    int c[3] = {0, 0, 0};
    const int lo = other.pid_lo + blockIdx.y * chunk;
    const int hi = min(lo + chunk, other.pid_hi);
    for (int base = lo; base < hi; base += FE_TL_WG) {
        const int rows = min(FE_TL_WG, hi - base);
        __syncthreads();
        if (tid < rows) {
            const int q = base + tid;
            TaskPairRow r; r.x[0] = r.x[1] = r.x[2] = 0.0; r.valid = 0; r.pad = 0;
            if ((unsigned)q < (unsigned)N) {
                const int s = slot_of_pid[q];
                if ((unsigned)s < (unsigned)Np && fe_tl_selected(other, q, fe_tl_mat(pinfo, q), fr.used[s])) {
                    const float4 b0 = fr.A0[s];
                    r.x[0] = b0.x; r.x[1] = b0.y; r.x[2] = b0.z; r.valid = 1;
                }
            }
            tile[tid] = r;
        }
        __syncthreads();
        for (int j = 0; j < rows; j++) {
            if (!tile[j].valid) continue;                     // (uniform: every lane reads row j)
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (!((axis_mask >> a) & 1)) continue;
                const double d = x[a] - tile[j].x[a];
                if (GRAD) c[a] += (d > 0.0) - (d < 0.0);
                else acc += fe_tl_abs(d);
            }
        }
    }
    if (GRAD) {
        if (pid < own.pid_hi && (unsigned)pid < (unsigned)N) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const int v = mine ? c[a] : 0;
                if (gridDim.y == 1) cnt[(size_t)a * N + pid] = v;
                else if (v != 0) atomicAdd(&cnt[(size_t)a * N + pid], v);
            }
        }
    } else {
        const double v = fe_tl_wg_sum(mine ? acc : 0.0, lds);
        if (tid == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = v;
    }
}

// One wave: per term the fixed-order merge of its partials (fe_tl_merge), times the weight, added to term_loss[t][s]; their sum in term
// order added to step_loss[s].
__global__ __launch_bounds__(64) void k_task_merge(const double* __restrict__ partial, const FeLossTerm* __restrict__ terms, int n_terms, TaskLayout L,
                                                   int steps, int s, double* __restrict__ term_loss, double* __restrict__ step_loss) {
    const int lane = threadIdx.x;
    double total = 0.0;
    for (int t = 0; t < n_terms; t++) {
        const double v = terms[t].weight * fe_tl_wave_sum(fe_tl_lane_sum(partial + L.off[t], L.np[t], lane));
        if (lane == 0) term_loss[(size_t)t * steps + s] += v;
        total += v;
    }
    if (lane == 0) step_loss[s] += total;
}

// what every entry that takes a selection asks of its pid range (host; here because the entries of the two headers below ask it too)
static bool tl_sel_ok(const FeLossSel& s, int N) { return s.pid_lo >= 0 && s.pid_lo <= s.pid_hi && s.pid_hi <= N; }

// density fields and the density term (FE_TERM_DENSITY_SQ): its kernels use the helpers above, k_task_bwd below gathers its residual
#include "fe_density.h"
// target clouds and the Chamfer terms (FE_TERM_NEAREST_SQ, FE_TERM_COVER_SQ): the same, k_task_bwd reads what k_nn_query left
#include "fe_nearest.h"

// The adjoint: one pass over the slots of the ADJOINT frame, which may be stored in another particle order than the frame (k_loss_bwd):
// slot s of the adjoint belongs to particle pid_of_slot[s], whose state sits in slot frame_slot_of_pid[pid] of the frame (nullptr: the same
// order).  Per particle and axis the gradients of all terms are summed in fp64 in term order -- pair terms as weight x count, from the count
// buffer of k_task_pair<true>; density terms as weight x the gather of the residual k_density_resid left; NEAREST terms as weight x 2 (x - t) to
// the cloud point k_nn_query found, COVER terms as weight x 2 x the fixed-point words its cloud points left -- multiplied by scale, rounded to
// fp32 once and added to G.A0 with one read-modify-write.
__global__ __launch_bounds__(256) void k_task_bwd(int N, size_t Np, float* fr_, float* G_, const int* __restrict__ pid_of_slot, const int* __restrict__ frame_slot_of_pid,
                                                  const float4* __restrict__ pinfo, const float* __restrict__ ref, const FeLossTerm* __restrict__ terms, int n_terms,
                                                  const int* __restrict__ cnt, TaskDensity TD, TaskNearest TN, double scale) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= N) return;
    const int pid = pid_of_slot[s];
    if ((unsigned)pid >= (unsigned)N) return;
    const int sf = frame_slot_of_pid ? frame_slot_of_pid[pid] : s;
    if ((unsigned)sf >= (unsigned)Np) return;
    const FrameV fr = frame_view(fr_, Np);
    const int used = fr.used[sf], mat = fe_tl_mat(pinfo, pid);
    const float4 a0 = fr.A0[sf];
    const float x[3] = {a0.x, a0.y, a0.z};
    float r[3] = {0.f, 0.f, 0.f};
    if (ref) { r[0] = ref[3 * (size_t)pid]; r[1] = ref[3 * (size_t)pid + 1]; r[2] = ref[3 * (size_t)pid + 2]; }
    double g[3] = {0.0, 0.0, 0.0};
    bool any = false;
    int pair = 0, dens = 0, near = 0;
    for (int t = 0; t < n_terms; t++) {
        const FeLossTerm& T = terms[t];
        if (fe_tl_separable(T.kind)) {
            if (!fe_tl_selected(T.a, pid, mat, used)) continue;
            for (int a = 0; a < 3; a++) g[a] += fe_tl_sep_grad(T, x, r, a);
            any = true;
        } else if (T.kind == FE_TERM_DENSITY_SQ) {            // the 27-cell (9-cell) gather of the residual, in fixed stencil order (fe_density.h)
            const int d = dens++;
            if (d >= FE_TASK_LOSS_MAX_DENSITY_TERMS || !fe_tl_selected(T.a, pid, mat, used)) continue;
            FeDensityStencil st;
            if (!fe_dn_stencil(TD.spec[d], x, st)) continue;
            double gd[3];
            fe_dn_grad(TD.spec[d], st, TD.r[d], gd);
            for (int a = 0; a < 3; a++) g[a] += T.weight * gd[a];
            any = true;
        } else if (T.kind == FE_TERM_NEAREST_SQ || T.kind == FE_TERM_COVER_SQ) {
            const int k = near++;
            if (k >= FE_TASK_LOSS_MAX_NEAREST_TERMS || !fe_tl_selected(T.a, pid, mat, used)) continue;
            if (T.kind == FE_TERM_NEAREST_SQ) {               // a skipped particle has no nearest point (-1)
                const int j = TN.nn[k][pid];
                if (j < 0) continue;
                const float4 tj = TN.cloud[k][j];
                const float tc[3] = {tj.x, tj.y, tj.z};
                for (int a = 0; a < 3; a++) if ((T.axis_mask >> a) & 1) g[a] += (2.0 * ((double)x[a] - (double)tc[a])) * T.weight;
                any = true;
            } else {                                          // the words of a particle no cloud point chose are zero
                const long long* w = TN.acc[k] + 3 * (size_t)pid;
                if ((w[0] | w[1] | w[2]) == 0) continue;
                for (int a = 0; a < 3; a++) if ((T.axis_mask >> a) & 1) g[a] += (2.0 * fe_nn_value(w[a])) * T.weight;
                any = true;
            }
        } else {
            const int* c = cnt + (size_t)pair * 3 * N;
            pair++;
            if (fe_tl_selected(T.a, pid, mat, used) || (T.b.pid_lo >= 0 && fe_tl_selected(T.b, pid, mat, used))) {
                for (int a = 0; a < 3; a++) if ((T.axis_mask >> a) & 1) g[a] += fe_tl_pair_grad(T, c[(size_t)a * N + pid]);
                any = true;
            }
        }
    }
    if (!any) return;
    const FrameV G = frame_view(G_, Np);
    float4 g0 = G.A0[s];
    g0.x += (float)(scale * g[0]); g0.y += (float)(scale * g[1]); g0.z += (float)(scale * g[2]);
    G.A0[s] = g0;
}

// ---------------------------------------------------------------------------------------------------------------- host
// (behind the host halves of fe_density.h and fe_nearest.h, whose reserve / scatter / search functions the step calls use)
struct TaskLossState {
    int steps = 0; double *step_loss = nullptr, *term_loss = nullptr;      // fe_task_loss_alloc: [steps], [FE_TASK_LOSS_MAX_TERMS][steps] fp64 on the device
    FeLossTerm terms[FE_TASK_LOSS_MAX_TERMS]; int n = 0; FeLossTerm* terms_dev = nullptr;      // fe_task_loss_set_terms: the program, and its copy on the device
    bool has_sep = false, has_ref = false; int n_pair = 0, n_density = 0, n_nearest = 0;
    float* ref = nullptr; bool ref_set = false;               // fe_task_loss_set_ref: [3 N] by particle id
    double* partial = nullptr; size_t partial_cap = 0;        // workgroup partials of the forward kernels (grown on demand)
    int* cnt = nullptr;                                       // [FE_TASK_LOSS_MAX_PAIR_TERMS][3][N] pair counts by particle id (allocated with the first program that has a pair term)
};
// every entry starts from the state, empty at first: no program and no arrays, which is what an entry called before any set-up is told
static TaskLossState* task_loss_state(FeEngine* h) {
    if (!h->task_loss) h->task_loss = new TaskLossState();
    return h->task_loss;
}
static void task_loss_drop(FeEngine* h) {                     // fe_destroy
    TaskLossState* Q = h->task_loss;
    if (!Q) return;
    for (void* q : {(void*)Q->step_loss, (void*)Q->term_loss, (void*)Q->terms_dev, (void*)Q->ref, (void*)Q->partial, (void*)Q->cnt}) if (q) (void)hipFree(q);
    delete Q;
    h->task_loss = nullptr;
}
static bool task_loss_names_cloud(FeEngine* h, int cloud) {   // fe_cloud_set
    const TaskLossState* Q = h->task_loss;
    for (int t = 0; Q && t < Q->n; t++)
        if ((Q->terms[t].kind == FE_TERM_NEAREST_SQ || Q->terms[t].kind == FE_TERM_COVER_SQ) && Q->terms[t].b.pid_lo == cloud) return true;
    return false;
}
// the launch shape of k_task_pair for `n_own` owners against `n_other` rows: workgroups of owners, rows per chunk, chunks
struct TaskPairShape { int ablocks, chunk, nchunks; };
static TaskPairShape task_pair_shape(FeEngine* h, int n_own, int n_other) {
    TaskPairShape p;
    p.ablocks = (n_own + FE_TL_WG - 1) / FE_TL_WG;
    if (h->task_pair_chunk > 0) p.chunk = h->task_pair_chunk;
    else {                                                    // enough chunks for ~8 workgroups per CU, none shorter than 64 rows
        const int want = std::max(1, (8 * h->n_cus + p.ablocks - 1) / std::max(1, p.ablocks));
        const int per = (n_other + want - 1) / want;
        p.chunk = std::max(64, (per + 63) / 64 * 64);
    }
    p.nchunks = (n_other + p.chunk - 1) / p.chunk;
    return p;
}
// k_task_pair on frame f, `own` against `other`: cnt == nullptr -- the workgroups' sums into `partial` (<false>); else the counts into cnt (<true>).
// Defined in fe_engine.hip behind every extension header, like the launches of fe_density.h and fe_nearest.h: the first use of a template kernel
static void task_pair_launch(FeEngine* h, int f, const FeLossSel& own, const FeLossSel& other, int axis_mask, const TaskPairShape& p, double* partial, int* cnt);
static int task_loss_check_step(FeEngine* h, int s, int f) {
    TaskLossState* Q = task_loss_state(h);
    if (Q->n <= 0) FAIL(h, "no loss-term program: fe_task_loss_set_terms first");
    if (!Q->steps) FAIL(h, "no task-loss arrays: fe_task_loss_alloc first");
    if (s < 0 || s >= Q->steps) FAIL(h, "loss step out of range");
    CHECK_FRAME(h, f);
    if (Q->has_ref && !Q->ref_set) FAIL(h, "FE_TERM_L1_REF before fe_task_loss_set_ref");
    DensityState* D = density_state(h);
    for (int t = 0, d = 0; t < Q->n; t++) {
        if (Q->terms[t].kind != FE_TERM_DENSITY_SQ) continue;
        const int k = Q->terms[t].b.pid_lo;
        if (D->spec[k].n[0] == 0) FAIL(h, "a density term names a field that is not set: fe_density_set_field first");
        if (!D->has_target[k]) FAIL(h, "a density term's field has no target: fe_density_set_target first");
        if (density_reserve(h, d++, (size_t)fe_dn_cells(D->spec[k]))) return 1;
    }
    for (int t = 0, k = 0; t < Q->n; t++) {                  // (no-ops unless a cloud was replaced or "nn_cells" changed since fe_task_loss_set_terms)
        const FeLossTerm& T = Q->terms[t];
        if (T.kind != FE_TERM_NEAREST_SQ && T.kind != FE_TERM_COVER_SQ) continue;
        if (!nearest_cloud_set(h, T.b.pid_lo)) FAIL(h, "a nearest term names a cloud that is not set: fe_cloud_set first");
        if (nearest_reserve(h, k++, T.b.pid_lo, true)) return 1;
        if (T.kind == FE_TERM_NEAREST_SQ && nearest_cloud_index(h, T.b.pid_lo, T.axis_mask)) return 1;
    }
    return 0;
}

extern "C" {

// The step calls enqueue and return; only fe_task_loss_get waits.  The forward call is read-only like the frame summary.
int fe_task_loss_alloc(FeEngine* h, int max_loss_steps) {
    FE_ENTRY(h);
    TaskLossState* Q = task_loss_state(h);
    if (max_loss_steps <= 0) FAIL(h, "fe_task_loss_alloc: max_loss_steps must be positive");
    double *sl = nullptr, *tl = nullptr;
    if (dev_alloc(h, &sl, (size_t)max_loss_steps) || dev_alloc(h, &tl, (size_t)FE_TASK_LOSS_MAX_TERMS * max_loss_steps)) {
        if (sl) (void)hipFree(sl);
        return 1;
    }
    HIPCK(h, hipStreamSynchronize(h->stream));               // (an earlier step may still write the old arrays)
    if (Q->step_loss) (void)hipFree(Q->step_loss);
    if (Q->term_loss) (void)hipFree(Q->term_loss);
    Q->step_loss = sl; Q->term_loss = tl; Q->steps = max_loss_steps;
    return 0;
}
int fe_task_loss_set_terms(FeEngine* h, const FeLossTerm* terms, int n_terms, int term_size) {
    FE_ENTRY(h);
    TaskLossState* Q = task_loss_state(h);
    const DensityState* D = density_state(h);
    if (term_size != (int)sizeof(FeLossTerm)) FAIL(h, "fe_task_loss_set_terms: term_size is not sizeof(FeLossTerm) (the program is unchanged)");
    if (n_terms < 0 || n_terms > FE_TASK_LOSS_MAX_TERMS) FAIL(h, "fe_task_loss_set_terms: n_terms must be in [0, FE_TASK_LOSS_MAX_TERMS] (the program is unchanged)");
    if (n_terms > 0 && !terms) FAIL(h, "fe_task_loss_set_terms: null terms (the program is unchanged)");
    int n_pair = 0, n_density = 0, n_nearest = 0; bool has_sep = false, has_ref = false;
    for (int t = 0; t < n_terms; t++) {
        const FeLossTerm& T = terms[t];
        if (T.kind < FE_TERM_L1_CONST || T.kind > FE_TERM_COVER_SQ) FAIL(h, "fe_task_loss_set_terms: unknown term kind (the program is unchanged)");
        if ((T.axis_mask & 7) == 0 || (T.axis_mask & ~7) != 0) FAIL(h, "fe_task_loss_set_terms: axis_mask must name at least one of the axes x, y, z (bits 0..2) (the program is unchanged)");
        if (!tl_sel_ok(T.a, h->N)) FAIL(h, "fe_task_loss_set_terms: pid range of selection a outside [0, N] (the program is unchanged)");
        if (T.kind == FE_TERM_PAIR_L1) {
            n_pair++;
            if (T.b.pid_lo >= 0) {
                if (!tl_sel_ok(T.b, h->N)) FAIL(h, "fe_task_loss_set_terms: pid range of selection b outside [0, N] (the program is unchanged)");
                if (T.a.pid_lo < T.b.pid_hi && T.b.pid_lo < T.a.pid_hi) FAIL(h, "fe_task_loss_set_terms: the pid ranges of a two-set pair term overlap (the program is unchanged)");
            }
        } else if (T.kind == FE_TERM_DENSITY_SQ) {
            n_density++;
            if (T.axis_mask != 7) FAIL(h, "fe_task_loss_set_terms: a density term's axis_mask must be 7 (the program is unchanged)");
            if (T.b.pid_hi != 0 || T.b.mat != 0 || T.b.require_used != 0) FAIL(h, "fe_task_loss_set_terms: a density term carries its field id in b.pid_lo and zeros in the rest of b (the program is unchanged)");
            if (T.b.pid_lo < 0 || T.b.pid_lo >= FE_DENSITY_MAX_FIELDS) FAIL(h, "fe_task_loss_set_terms: density field id out of range (the program is unchanged)");
            if (D->spec[T.b.pid_lo].n[0] == 0) FAIL(h, "fe_task_loss_set_terms: a density term names a field that is not set: fe_density_set_field first (the program is unchanged)");
        } else if (T.kind == FE_TERM_NEAREST_SQ || T.kind == FE_TERM_COVER_SQ) {
            n_nearest++;
            if (T.b.pid_hi != 0 || T.b.mat != 0 || T.b.require_used != 0) FAIL(h, "fe_task_loss_set_terms: a nearest term carries its cloud id in b.pid_lo and zeros in the rest of b (the program is unchanged)");
            if (T.b.pid_lo < 0 || T.b.pid_lo >= FE_CLOUD_MAX) FAIL(h, "fe_task_loss_set_terms: cloud id out of range (the program is unchanged)");
            if (!nearest_cloud_set(h, T.b.pid_lo)) FAIL(h, "fe_task_loss_set_terms: a nearest term names a cloud that is not set: fe_cloud_set first (the program is unchanged)");
        } else {
            has_sep = true;
            if (T.kind == FE_TERM_L1_REF) has_ref = true;
        }
    }
    if (n_pair > FE_TASK_LOSS_MAX_PAIR_TERMS) FAIL(h, "fe_task_loss_set_terms: more than FE_TASK_LOSS_MAX_PAIR_TERMS pair terms (the program is unchanged)");
    if (n_density > FE_TASK_LOSS_MAX_DENSITY_TERMS) FAIL(h, "fe_task_loss_set_terms: more than FE_TASK_LOSS_MAX_DENSITY_TERMS density terms (the program is unchanged)");
    if (n_nearest > FE_TASK_LOSS_MAX_NEAREST_TERMS) FAIL(h, "fe_task_loss_set_terms: more than FE_TASK_LOSS_MAX_NEAREST_TERMS nearest terms (the program is unchanged)");
    HIPCK(h, hipStreamSynchronize(h->stream));               // (an earlier step may still read the old program)
    for (int t = 0, k = 0; t < n_terms; t++) {               // nearest terms: scratch, result buffers and the cloud's index for the term's mask
        if (terms[t].kind != FE_TERM_NEAREST_SQ && terms[t].kind != FE_TERM_COVER_SQ) continue;
        if (nearest_reserve(h, k++, terms[t].b.pid_lo, true)) return 1;
        if (terms[t].kind == FE_TERM_NEAREST_SQ && nearest_cloud_index(h, terms[t].b.pid_lo, terms[t].axis_mask)) return 1;
    }
    if (n_terms > 0) {
        if (!Q->terms_dev && dev_alloc(h, &Q->terms_dev, (size_t)FE_TASK_LOSS_MAX_TERMS)) return 1;
        if (n_pair > 0 && !Q->cnt && dev_alloc(h, &Q->cnt, (size_t)FE_TASK_LOSS_MAX_PAIR_TERMS * 3 * h->N)) return 1;
        if (has_ref && !Q->ref && dev_alloc(h, &Q->ref, (size_t)3 * h->N)) return 1;
        if (hipMemcpyOnStream(h, Q->terms_dev, terms, sizeof(FeLossTerm) * (size_t)n_terms, hipMemcpyHostToDevice) != hipSuccess) {
            Q->n = 0;                                         // (the device copy is undefined now)
            FAIL(h, "fe_task_loss_set_terms: hipMemcpy failed (no program is set)");
        }
        std::memcpy(Q->terms, terms, sizeof(FeLossTerm) * (size_t)n_terms);
    }
    Q->n = n_terms; Q->n_pair = n_pair; Q->n_density = n_density; Q->n_nearest = n_nearest; Q->has_sep = has_sep; Q->has_ref = has_ref;
    return 0;
}
int fe_task_loss_set_ref(FeEngine* h, int f) {
    FE_ENTRY(h);
    TaskLossState* Q = task_loss_state(h);
    CHECK_FRAME(h, f);
    if (!Q->ref && dev_alloc(h, &Q->ref, (size_t)3 * h->N)) return 1;
    if (h->N > 0)
        hipLaunchKernelGGL(k_task_set_ref, pgrid(h), dim3(256), 0, h->stream, h->N, (size_t)h->Np, h->frame(f), (const int*)h->tables[h->tbl_of_frame[f]].slot_of_pid, Q->ref);
    Q->ref_set = true;
    return check_async(h);
}
int fe_task_loss_clear(FeEngine* h) {
    FE_ENTRY(h);
    TaskLossState* Q = task_loss_state(h);
    if (!Q->steps) return 0;
    HIPCK(h, hipMemsetAsync(Q->step_loss, 0, sizeof(double) * (size_t)Q->steps, h->stream));
    HIPCK(h, hipMemsetAsync(Q->term_loss, 0, sizeof(double) * (size_t)FE_TASK_LOSS_MAX_TERMS * Q->steps, h->stream));
    return 0;
}
int fe_task_loss_step(FeEngine* h, int s, int f) {
    FE_ENTRY(h);
    if (task_loss_check_step(h, s, f)) return 1;
    TaskLossState* Q = h->task_loss;
    const DensityState* D = h->density;
    // where each term's partials go
    TaskLayout L; TaskPairShape shape[FE_TASK_LOSS_MAX_TERMS];
    int sep_wgs = std::min((h->N + FE_TL_WG - 1) / FE_TL_WG, FE_TL_SEP_MAX_WGS);
    if (sep_wgs < 1) sep_wgs = 1;
    size_t need = 0;
    for (int t = 0; t < FE_TASK_LOSS_MAX_TERMS; t++) { L.off[t] = 0; L.np[t] = 0; }
    for (int t = 0; t < Q->n; t++) {
        const FeLossTerm& T = Q->terms[t];
        size_t np = (size_t)sep_wgs;
        if (T.kind == FE_TERM_PAIR_L1) {
            const FeLossSel& B = T.b.pid_lo < 0 ? T.a : T.b;
            const int nA = T.a.pid_hi - T.a.pid_lo, nB = B.pid_hi - B.pid_lo;
            shape[t] = task_pair_shape(h, nA, nB);
            if (shape[t].nchunks > 65535) FAIL(h, "fe_task_loss_step: more than 65535 chunks (raise option task_pair_chunk)");
            np = (nA > 0 && nB > 0) ? (size_t)shape[t].ablocks * shape[t].nchunks : 0;
        } else if (T.kind == FE_TERM_DENSITY_SQ) np = (size_t)density_resid_wgs(D->spec[T.b.pid_lo]);
        else if (T.kind == FE_TERM_NEAREST_SQ || T.kind == FE_TERM_COVER_SQ) np = (size_t)nearest_sum_wgs(nearest_queries(h, T));
        if (need + np > (size_t)0x7fffffff) FAIL(h, "fe_task_loss_step: too many workgroup partials (raise option task_pair_chunk)");
        L.off[t] = (int)need; L.np[t] = (int)np;
        need += np;
    }
    if (need > Q->partial_cap) {
        HIPCK(h, hipStreamSynchronize(h->stream));
        if (Q->partial) (void)hipFree(Q->partial);
        Q->partial = nullptr; Q->partial_cap = 0;
        if (dev_alloc(h, &Q->partial, need, false)) return 1;
        Q->partial_cap = need;
    }
    if (Q->has_sep)
        hipLaunchKernelGGL(k_task_sep_fwd, dim3(sep_wgs), dim3(FE_TL_WG), 0, h->stream, h->N, (size_t)h->Np, h->frame(f), h->pid_of(f), (const float4*)h->pinfo,
                           (const float*)(Q->has_ref ? Q->ref : nullptr), (const FeLossTerm*)Q->terms_dev, Q->n, L, Q->partial);
    for (int t = 0; t < Q->n; t++) {
        const FeLossTerm& T = Q->terms[t];
        if (T.kind != FE_TERM_PAIR_L1 || L.np[t] == 0) continue;
        task_pair_launch(h, f, T.a, T.b.pid_lo < 0 ? T.a : T.b, T.axis_mask, shape[t], Q->partial + L.off[t], nullptr);
    }
    for (int t = 0, d = 0; t < Q->n; t++) {                  // density terms: the field, then the residual and its workgroup partials
        const FeLossTerm& T = Q->terms[t];
        if (T.kind != FE_TERM_DENSITY_SQ) continue;
        const FeDensitySpec& sp = D->spec[T.b.pid_lo];
        density_scatter(h, f, sp, T.a, d);
        hipLaunchKernelGGL(k_density_resid, dim3(L.np[t]), dim3(FE_DENSITY_WG), 0, h->stream, (int)fe_dn_cells(sp), (const unsigned long long*)D->words[d],
                           (const double*)D->target[T.b.pid_lo], D->r[d], Q->partial + L.off[t]);
        d++;
    }
    for (int t = 0, k = 0; t < Q->n; t++) {                  // nearest terms: the search, then the workgroup partials of d2 by query index
        const FeLossTerm& T = Q->terms[t];
        if (T.kind != FE_TERM_NEAREST_SQ && T.kind != FE_TERM_COVER_SQ) continue;
        nearest_eval(h, f, T, k, false);
        nearest_sum(h, k, nearest_queries(h, T), Q->partial + L.off[t], L.np[t]);
        k++;
    }
    hipLaunchKernelGGL(k_task_merge, dim3(1), dim3(64), 0, h->stream, (const double*)Q->partial, (const FeLossTerm*)Q->terms_dev, Q->n, L, Q->steps, s,
                       Q->term_loss, Q->step_loss);
    return check_async(h);
}
int fe_task_loss_step_grad(FeEngine* h, int s, int f, double scale) {
    FE_ENTRY(h);
    if (task_loss_check_step(h, s, f)) return 1;
    if (adj_slot(h, f, ADJ_READ)) return 1;                   // (the refusal; the slot takes its order below, behind the other ways out)
    if (h->N == 0) return 0;
    TaskLossState* Q = h->task_loss;
    const DensityState* D = h->density;
    int pair = 0;
    for (int t = 0; t < Q->n; t++) {
        const FeLossTerm& T = Q->terms[t];
        if (T.kind != FE_TERM_PAIR_L1) continue;
        int* cnt = Q->cnt + (size_t)(pair++) * 3 * h->N;
        const bool self = T.b.pid_lo < 0;
        const FeLossSel& B = self ? T.a : T.b;
        const int nA = T.a.pid_hi - T.a.pid_lo, nB = B.pid_hi - B.pid_lo;
        const TaskPairShape pa = task_pair_shape(h, nA, nB), pb = task_pair_shape(h, nB, nA);
        if (pa.nchunks > 65535 || pb.nchunks > 65535) FAIL(h, "fe_task_loss_step_grad: more than 65535 chunks (raise option task_pair_chunk)");
        // (several chunks add their counts with integer atomics onto zeros; with an empty set nothing is launched and the counts are zero)
        if (nA == 0 || nB == 0 || pa.nchunks > 1 || (!self && pb.nchunks > 1)) HIPCK(h, hipMemsetAsync(cnt, 0, sizeof(int) * 3 * (size_t)h->N, h->stream));
        if (nA == 0 || nB == 0) continue;
        task_pair_launch(h, f, T.a, B, T.axis_mask, pa, nullptr, cnt);
        if (!self) task_pair_launch(h, f, B, T.a, T.axis_mask, pb, nullptr, cnt);      // the other side: the same kernel with the roles swapped
    }
    TaskDensity TD = {};
    for (int t = 0, d = 0; t < Q->n; t++) {                  // density terms: the field of frame f again, and its residual for the gather in k_task_bwd
        const FeLossTerm& T = Q->terms[t];
        if (T.kind != FE_TERM_DENSITY_SQ) continue;
        const FeDensitySpec& sp = D->spec[T.b.pid_lo];
        density_scatter(h, f, sp, T.a, d);
        hipLaunchKernelGGL(k_density_resid, dim3(density_resid_wgs(sp)), dim3(FE_DENSITY_WG), 0, h->stream, (int)fe_dn_cells(sp), (const unsigned long long*)D->words[d],
                           (const double*)D->target[T.b.pid_lo], D->r[d], (double*)nullptr);
        TD.spec[d] = sp; TD.r[d] = D->r[d];
        d++;
    }
    TaskNearest TN = {};
    for (int t = 0, k = 0; t < Q->n; t++) {                  // nearest terms: the search on frame f again; COVER leaves its fixed-point words
        const FeLossTerm& T = Q->terms[t];
        if (T.kind != FE_TERM_NEAREST_SQ && T.kind != FE_TERM_COVER_SQ) continue;
        nearest_eval(h, f, T, k, true);
        nearest_task_view(h, T, k, TN);
        k++;
    }
    AdjSlot a; if (adj_slot(h, f, ADJ_ADD, &a)) return 1;
    hipLaunchKernelGGL(k_task_bwd, pgrid(h), dim3(256), 0, h->stream, h->N, (size_t)h->Np, h->frame(f), a.planes, a.pid, a.frame_slot_of_pid, (const float4*)h->pinfo, (const float*)(Q->has_ref ? Q->ref : nullptr),
                       (const FeLossTerm*)Q->terms_dev, Q->n, (const int*)Q->cnt, TD, TN, scale);
    return check_async(h);
}
int fe_task_loss_get(FeEngine* h, int s0, int n, double* step_loss, double* term_loss) {
    FE_ENTRY(h);
    TaskLossState* Q = task_loss_state(h);
    if (!Q->steps) FAIL(h, "no task-loss arrays: fe_task_loss_alloc first");
    if (s0 < 0 || n < 0 || s0 + n > Q->steps) FAIL(h, "fe_task_loss_get: steps out of range");
    if (n > 0 && step_loss) HIPCK(h, hipMemcpyAsync(step_loss, Q->step_loss + s0, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if (n > 0 && term_loss)
        for (int t = 0; t < Q->n; t++)
            HIPCK(h, hipMemcpyAsync(term_loss + (size_t)t * n, Q->term_loss + (size_t)t * Q->steps + s0, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    return check_device_errors(h);
}

}  // extern "C"
#endif /* FE_TASK_LOSS_MATH_ONLY */
#endif /* FE_TASK_LOSS_H */
