// fe_task_loss.h -- the task losses evaluated in the engine: loss-term programs (include/fluidengine_ext.h: fe_task_loss_*).
// Included by fe_engine.hip behind the substep kernels; the kernels use its frame views and order tables.  The first part -- the selection
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
#endif /* FE_TASK_LOSS_MATH_ONLY */
#endif /* FE_TASK_LOSS_H */
