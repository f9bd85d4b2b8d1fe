// fe_smoke_reads.h -- reads of a GPU-resident smoke frame that do not copy it: cell lists, the detector loss and the field summary
// (include/fluidengine_ext.h: fe_smoke_cells_*, fe_smoke_loss_*, fe_smoke_summary).  The smoke-side counterpart of fe_summary.h and
// fe_task_loss.h, included by fe_engine.hip behind fe_smoke.h.  The first part -- one detector's value and gradient, one cell's contribution
// to the summary with its finiteness test, the merge of partial records and the final record -- is plain __host__ __device__ code:
// tests/csrc/smoke_reads_test.cpp compiles it for the host with FE_SMOKE_READS_MATH_ONLY defined and checks it against plain fp64 loops.
//
// The reads and the forward loss only READ v and q of a frame; the backward loss adds to gq and to nothing else.  The one write of a cell
// list, fe_smoke_cells_add_grad*, adds cotangent rows to gv / gq of one frame at the listed cells and to nothing else.  No floating-point atomics.
#ifndef FE_SMOKE_READS_H
#define FE_SMOKE_READS_H

// ---- detector loss: one entry ---------------------------------------------------------------------------------------
// the weighted value of one detector: w |q - t| (FE_SMOKE_SQ: w (q - t)^2), in fp64 from the fp32 word
__host__ __device__ inline double fe_sl_value(int kind, float q, double t, double w) {
    const double d = (double)q - t;
    return w * (kind == FE_SMOKE_SQ ? d * d : fe_tl_abs(d));
}
// ... and what its gradient adds to gq, rounded to fp32 once: (float)(scale w sign(d)), sign(0) = 0 (FE_SMOKE_SQ: 2 d for sign(d)).
// `add` is false for a non-finite q: nothing is added there.
__host__ __device__ inline float fe_sl_grad(int kind, float q, double t, double w, double scale, bool& add) {
    add = fe_sum_finite(q);
    if (!add) return 0.f;
    const double d = (double)q - t;
    return (float)(scale * w * (kind == FE_SMOKE_SQ ? 2.0 * d : fe_tl_sign(d)));
}

// ---- field summary: the running record ------------------------------------------------------------------------------
// sums, not yet finished.  13 eight-byte words.
struct FeSmokeAcc {
    long long n_cells, n_nonfinite;
    double v_max, kin;                       // max |v_a|, 1/2 sum |v|^2
    double q_sum[3], q_min[3], q_max[3];
};
#define FE_SS_WORDS 13
static_assert(sizeof(FeSmokeAcc) == 8 * FE_SS_WORDS, "FeSmokeAcc is 13 eight-byte words");

__host__ __device__ inline void fe_ss_clear(FeSmokeAcc& a) {
    const double inf = __builtin_huge_val();
    a.n_cells = 0; a.n_nonfinite = 0; a.v_max = 0.0; a.kin = 0.0;
    for (int d = 0; d < 3; d++) { a.q_sum[d] = 0.0; a.q_min[d] = inf; a.q_max[d] = -inf; }
}
// One slab cell: v[3] and q[qd] are the frame's fp32 words.  A cell with a non-finite word in v or q is counted and contributes to
// nothing else.  Components beyond qd are left alone.
__host__ __device__ inline void fe_ss_cell(FeSmokeAcc& a, const float* v, const float* q, int qd) {
    a.n_cells += 1;
    bool ok = fe_sum_finite(v[0]) && fe_sum_finite(v[1]) && fe_sum_finite(v[2]);
    for (int d = 0; d < qd; d++) ok = ok && fe_sum_finite(q[d]);
    if (!ok) { a.n_nonfinite += 1; return; }
    double vv = 0.0;
    for (int d = 0; d < 3; d++) {
        const double vd = (double)v[d], av = vd < 0.0 ? -vd : vd;
        vv += vd * vd;
        if (av > a.v_max) a.v_max = av;
    }
    a.kin += 0.5 * vv;
    for (int d = 0; d < qd; d++) {
        const double qv = (double)q[d];
        a.q_sum[d] += qv;
        if (qv < a.q_min[d]) a.q_min[d] = qv;
        if (qv > a.q_max[d]) a.q_max[d] = qv;
    }
}
// a <- a merged with b (counts and sums add, extremes combine)
__host__ __device__ inline void fe_ss_merge(FeSmokeAcc& a, const FeSmokeAcc& b) {
    a.n_cells += b.n_cells; a.n_nonfinite += b.n_nonfinite;
    a.kin += b.kin;
    if (b.v_max > a.v_max) a.v_max = b.v_max;
    for (int d = 0; d < 3; d++) {
        a.q_sum[d] += b.q_sum[d];
        if (b.q_min[d] < a.q_min[d]) a.q_min[d] = b.q_min[d];
        if (b.q_max[d] > a.q_max[d]) a.q_max[d] = b.q_max[d];
    }
}
// The fixed-order merge of n partial records, by a single wave: lane l of 64 merges the records l, l + 64, ... in index order
// (fe_ss_merge_lane), then the 64 lane records are merged in lane order (fe_ss_merge_lanes).  The result depends on n and the records only.
#define FE_SS_LANES 64
__host__ __device__ inline void fe_ss_merge_lane(const FeSmokeAcc* part, int n, int lane, FeSmokeAcc& a) {
    fe_ss_clear(a);
    for (int i = lane; i < n; i += FE_SS_LANES) fe_ss_merge(a, part[i]);
}
__host__ __device__ inline void fe_ss_merge_lanes(const FeSmokeAcc* lanes /* [FE_SS_LANES] */, FeSmokeAcc& a) {
    fe_ss_clear(a);
    for (int l = 0; l < FE_SS_LANES; l++) fe_ss_merge(a, lanes[l]);
}
// The record handed out.  A slab without a finite cell is all zeros apart from its two counts; components beyond qd are zero.
__host__ __device__ inline void fe_ss_finish(const FeSmokeAcc& a, double dt, int qd, FeSmokeSummary& o) {
    o.n_cells = a.n_cells; o.n_nonfinite = a.n_nonfinite;
    const bool any = a.n_cells > a.n_nonfinite;
    o.v_max = any ? a.v_max : 0.0;
    o.courant = any ? dt * a.v_max : 0.0;
    o.kinetic = any ? a.kin : 0.0;
    for (int d = 0; d < 3; d++) {
        const bool on = any && d < qd;
        o.q_sum[d] = on ? a.q_sum[d] : 0.0;
        o.q_min[d] = on ? a.q_min[d] : 0.0;
        o.q_max[d] = on ? a.q_max[d] : 0.0;
    }
}

#ifndef FE_SMOKE_READS_MATH_ONLY
// ---- cell-list gather ------------------------------------------------------------------------------------------------
// Row i = cell idx[i] (a linear cell index, checked against res when the list was set) of the frame: one thread per list entry, two compact
// arrays out (NULL = skipped); device or staging pointers alike.
__global__ __launch_bounds__(256) void k_smoke_gather(int n, int qd, const float* __restrict__ vf, const float* __restrict__ qf, const size_t* __restrict__ idx,
                                                      float* __restrict__ v, float* __restrict__ q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t c = idx[i];
    if (v) { v[3 * (size_t)i] = vf[3 * c]; v[3 * (size_t)i + 1] = vf[3 * c + 1]; v[3 * (size_t)i + 2] = vf[3 * c + 2]; }
    if (q) for (int d = 0; d < qd; d++) q[(size_t)qd * i + d] = qf[c * qd + d];
}

// ---- cell-list scatter: the mirror image of k_smoke_gather for the adjoint of a frame ---------------------------------
// The list may name a cell several times.  The rows are grouped once per list (smoke_list_group): rows[] holds the row indices sorted by
// linear cell index, rows of one cell in list order; seg[k] .. seg[k + 1] are the rows of the k-th distinct cell.  One thread owns one
// distinct cell: it sums that cell's rows in list order in fp32, starting from 0, and adds the sum to the adjoint words once -- the result
// does not depend on the launch geometry, and it is what fe_smoke_add_grad adds for a dense field accumulated row by row from zero.
// A template instantiation with its arguments in one struct and no blockDim / gridDim, for the reasons given in fe_policy_io.h: it is
// emitted behind every plain kernel and outside the 16 KB-aligned substep group, and its metadata note is as small as a kernel's can be
// (DESIGN.md section 4 has what the sections in front of the code did all the same).
struct SmokeScatterArgs { int n_seg, qd; float *gvf, *gqf; const size_t* idx; const int *rows, *seg; const float *gv, *gq; };
template <int TAIL>
__global__ __launch_bounds__(256) void k_smoke_scatter_grad(SmokeScatterArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n_seg) return;
    const int lo = a.seg[k], hi = a.seg[k + 1];
    if (hi <= lo) return;
    const size_t c = a.idx[a.rows[lo]];                       // (checked against res when the list was set)
    const float *gv = a.gv, *gq = a.gq;
    const int qd = a.qd;
    float sv[3] = {0.f, 0.f, 0.f}, sq[3] = {0.f, 0.f, 0.f};
    for (int j = lo; j < hi; j++) {
        const size_t r = (size_t)a.rows[j];
        if (gv) { sv[0] += gv[3 * r]; sv[1] += gv[3 * r + 1]; sv[2] += gv[3 * r + 2]; }
        if (gq) for (int d = 0; d < 3; d++) if (d < qd) sq[d] += gq[(size_t)qd * r + d];
    }
    if (gv) { a.gvf[3 * c] += sv[0]; a.gvf[3 * c + 1] += sv[1]; a.gvf[3 * c + 2] += sv[2]; }
    if (gq) for (int d = 0; d < 3; d++) if (d < qd) a.gqf[c * qd + d] += sq[d];
}

// ---- Circulation's observation vector and its adjoint, one launch each (fe_smoke_obs_get*, fe_smoke_obs_add_grad*) ----------------
// The vector: the AirCon's state at local frame f (pos 3, quat 4, s, r), the v rows of the list in smoke frame s [n][3], the q rows
// [n][qd] -- FE_SMOKE_OBS_STATE + n (3 + qd) words.  Thread k copies row k; the first nine threads also copy one state word each.
// The adjoint: thread k owns the k-th distinct cell exactly as in k_smoke_scatter_grad (rows summed in list order in fp32 from 0, added
// once); the first nine threads also add one state word each to gpos / gquat / gsa / gra of frame f.  Every word has one writer.
// Template instantiations with one argument struct and no blockDim / gridDim, like k_smoke_scatter_grad above.
struct SmokeObsArgs {
    int n, n_seg, qd, f;
    const float *vf, *qf; float *gvf, *gqf;                   // frame s: fields (pack), adjoints (scatter)
    const size_t* idx; const int *rows, *seg;
    const float *pos, *quat, *sa, *ra; float *gpos, *gquat, *gsa, *gra;
    float* out; const float* g;                               // [FE_SMOKE_OBS_STATE + n (3 + qd)]
};
template <int TAIL>
__global__ __launch_bounds__(256) void k_smoke_obs_pack(SmokeObsArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < FE_SMOKE_OBS_STATE) {
        const size_t f = (size_t)a.f;
        a.out[k] = k < 3 ? a.pos[f * 3 + k] : (k < 7 ? a.quat[f * 4 + (k - 3)] : (k == 7 ? a.sa[f] : a.ra[f]));
    }
    if (k >= a.n) return;
    const size_t c = a.idx[k], n = (size_t)a.n;               // (checked against res when the list was set)
    float* v = a.out + FE_SMOKE_OBS_STATE + 3 * (size_t)k;
    v[0] = a.vf[3 * c]; v[1] = a.vf[3 * c + 1]; v[2] = a.vf[3 * c + 2];
    float* q = a.out + FE_SMOKE_OBS_STATE + 3 * n + (size_t)a.qd * k;
    for (int d = 0; d < 3; d++) if (d < a.qd) q[d] = a.qf[c * a.qd + d];
}
template <int TAIL>
__global__ __launch_bounds__(256) void k_smoke_obs_scatter_grad(SmokeObsArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < FE_SMOKE_OBS_STATE) {
        const size_t f = (size_t)a.f;
        float* w = k < 3 ? a.gpos + f * 3 + k : (k < 7 ? a.gquat + f * 4 + (k - 3) : (k == 7 ? a.gsa + f : a.gra + f));
        *w += a.g[k];
    }
    if (k >= a.n_seg) return;
    const int lo = a.seg[k], hi = a.seg[k + 1];
    if (hi <= lo) return;
    const size_t c = a.idx[a.rows[lo]];
    const int qd = a.qd;
    const float *gv = a.g + FE_SMOKE_OBS_STATE, *gq = gv + 3 * (size_t)a.n;
    float sv[3] = {0.f, 0.f, 0.f}, sq[3] = {0.f, 0.f, 0.f};
    for (int j = lo; j < hi; j++) {
        const size_t r = (size_t)a.rows[j];
        sv[0] += gv[3 * r]; sv[1] += gv[3 * r + 1]; sv[2] += gv[3 * r + 2];
        for (int d = 0; d < 3; d++) if (d < qd) sq[d] += gq[(size_t)qd * r + d];
    }
    a.gvf[3 * c] += sv[0]; a.gvf[3 * c + 1] += sv[1]; a.gvf[3 * c + 2] += sv[2];
    for (int d = 0; d < 3; d++) if (d < qd) a.gqf[c * qd + d] += sq[d];
}

// ---- detector loss ---------------------------------------------------------------------------------------------------
// One workgroup reduces the whole list: thread t adds the entries t, t + 256, ... in order, the wave sums by the butterfly of
// fe_tl_butterfly, the four wave sums are added in wave order (fe_tl_wg_sum) and thread 0 adds the result to *slot.
__global__ __launch_bounds__(FE_TL_WG) void k_smoke_loss_fwd(int n, int qd, int comp, int kind, const float* __restrict__ qf, const size_t* __restrict__ idx,
                                                             const double* __restrict__ target, const double* __restrict__ weight, double* __restrict__ slot) {
    __shared__ double lds[FE_TL_WG / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += FE_TL_WG) acc += fe_sl_value(kind, qf[idx[i] * qd + comp], target[i], weight[i]);
    const double v = fe_tl_wg_sum(acc, lds);
    if (threadIdx.x == 0) *slot += v;
}
// One thread per entry: one read-modify-write of gq at its cell (the list has no duplicate cell: checked by fe_smoke_loss_set).
__global__ __launch_bounds__(256) void k_smoke_loss_bwd(int n, int qd, int comp, int kind, const float* __restrict__ qf, float* __restrict__ gqf, const size_t* __restrict__ idx,
                                                        const double* __restrict__ target, const double* __restrict__ weight, double scale) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t at = idx[i] * qd + comp;
    bool add;
    const float g = fe_sl_grad(kind, qf[at], target[i], weight[i], scale, add);
    if (add) gqf[at] += g;
}

// ---- field summary ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fe_ss_wave_reduce(FeSmokeAcc& r) {          // butterfly: every lane ends with the merge of all 64, in one fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        FeSmokeAcc b;
        b.n_cells = __shfl_xor(r.n_cells, o, 64); b.n_nonfinite = __shfl_xor(r.n_nonfinite, o, 64);
        b.v_max = __shfl_xor(r.v_max, o, 64); b.kin = __shfl_xor(r.kin, o, 64);
#pragma unroll
        for (int d = 0; d < 3; d++) { b.q_sum[d] = __shfl_xor(r.q_sum[d], o, 64); b.q_min[d] = __shfl_xor(r.q_min[d], o, 64); b.q_max[d] = __shfl_xor(r.q_max[d], o, 64); }
        fe_ss_merge(r, b);
    }
}
#define FE_SS_WG 256
#define FE_SS_MAX_WGS 1024
// One grid-stride pass over the slab cells j0 <= j < j0 + nj (all i and k) of a frame.  Thread t of the pass is cell
// (i, j, k) = (t / (nj n), j0 + (t / n) % nj, t % n) as in sm_cell: consecutive lanes read consecutive k, the fast axis of [i][j][k].
// A lane keeps its record in registers; the wave reduces once at the end, the waves of the workgroup add their records in wave order in LDS
// and the workgroup leaves one record in partial[blockIdx.x].
__global__ __launch_bounds__(FE_SS_WG) void k_smoke_summary(int n, int qd, int j0, int nj, const float* __restrict__ vf, const float* __restrict__ qf,
                                                            FeSmokeAcc* __restrict__ partial) {
    __shared__ FeSmokeAcc rec[FE_SS_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long cells = (long long)n * nj * n;
    FeSmokeAcc acc;
    fe_ss_clear(acc);
    for (long long t = (long long)blockIdx.x * FE_SS_WG + tid; t < cells; t += (long long)gridDim.x * FE_SS_WG) {
        const int k = (int)(t % n), j = j0 + (int)((t / n) % nj), i = (int)(t / ((long long)n * nj));
        const size_t c = ((size_t)i * n + j) * n + k;
        const float v[3] = {vf[3 * c], vf[3 * c + 1], vf[3 * c + 2]};
        float q[3] = {0.f, 0.f, 0.f};
        for (int d = 0; d < qd; d++) q[d] = qf[c * qd + d];
        fe_ss_cell(acc, v, q, qd);
    }
    fe_ss_wave_reduce(acc);
    if (lane == 0) rec[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        FeSmokeAcc a;
        fe_ss_clear(a);
        for (int w = 0; w < FE_SS_WG / 64; w++) fe_ss_merge(a, rec[w]);
        partial[blockIdx.x] = a;
    }
}
// A single wave: fe_ss_merge_lane per lane, the lane records through LDS, lane 0 merges them in lane order and writes the record.
__global__ __launch_bounds__(FE_SS_LANES) void k_smoke_summary_merge(const FeSmokeAcc* __restrict__ partial, int n_partial, double dt, int qd, FeSmokeSummary* __restrict__ out) {
    __shared__ FeSmokeAcc lanes[FE_SS_LANES];
    const int lane = threadIdx.x;
    FeSmokeAcc a;
    fe_ss_merge_lane(partial, n_partial, lane, a);
    lanes[lane] = a;
    __syncthreads();
    if (lane == 0) {
        fe_ss_merge_lanes(lanes, a);
        fe_ss_finish(a, dt, qd, *out);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct SmokeCellList {
    int n = 0;
    size_t* idx = nullptr;                   // [n] linear cell indices on the device
    float* stage = nullptr;                  // [n (3 + q_dim)] on the device: v rows, then q rows
    float* hstage = nullptr;                 // the same, pinned host memory: one copy brings a gather over
    std::vector<size_t> cells;               // the host's copy of idx
    // fe_smoke_cells_add_grad*: nothing before the first call; a new fe_smoke_cells_set starts from an empty record again
    int n_seg = 0;                           // distinct cells; 0 = not grouped yet
    int *rows = nullptr, *seg = nullptr;     // [n], [n_seg + 1] on the device (smoke_list_group)
    float* gstage = nullptr;                 // [n (3 + q_dim)] on the device: staging of the host variant, gv rows, then gq rows
    // fe_smoke_obs_get / fe_smoke_obs_add_grad (host variants): nothing before the first call
    float* ostage = nullptr;                 // [FE_SMOKE_OBS_STATE + n (3 + q_dim)] on the device
    float* ohstage = nullptr;                // the same, pinned host memory
};
struct SmokeReads {
    SmokeCellList list[FE_SMOKE_MAX_LISTS];
    int loss_steps = 0; double* step_loss = nullptr;                         // fe_smoke_loss_alloc
    int loss_n = 0, loss_comp = 0, loss_kind = 0;                            // fe_smoke_loss_set: the detectors are a copy of the list's cells as they were then
    size_t* loss_idx = nullptr; double *loss_target = nullptr, *loss_weight = nullptr;
    FeSmokeAcc* partial = nullptr; FeSmokeSummary* sum_out = nullptr;        // fe_smoke_summary: [FE_SS_MAX_WGS] partial records, the result; allocated at the first call
};

static void smoke_list_free(SmokeCellList& L) {
    if (L.idx) (void)hipFree(L.idx);
    if (L.stage) (void)hipFree(L.stage);
    if (L.hstage) (void)hipHostFree(L.hstage);
    if (L.ohstage) (void)hipHostFree(L.ohstage);
    for (void* q : {(void*)L.rows, (void*)L.seg, (void*)L.gstage, (void*)L.ostage}) if (q) (void)hipFree(q);
    L = SmokeCellList();
}
// every list, the loss and all their buffers (smoke_destroy: fe_smoke_create and fe_destroy)
static void smoke_reads_drop(FeEngine* h) {
    SmokeReads* R = h->smoke_reads;
    if (!R) return;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& L : R->list) smoke_list_free(L);
    for (void* q : {(void*)R->step_loss, (void*)R->loss_idx, (void*)R->loss_target, (void*)R->loss_weight, (void*)R->partial, (void*)R->sum_out}) if (q) (void)hipFree(q);
    delete R;
    h->smoke_reads = nullptr;
}
static SmokeReads* smoke_reads(FeEngine* h) {
    if (!h->smoke_reads) h->smoke_reads = new SmokeReads();
    return h->smoke_reads;
}
// Row indices 0 .. n - 1 stably sorted by key (rows of one key keep their list order) and the segment starts, seg[n_seg] = n: the grouping
// behind every scatter of a list that may name an item twice (here, and policy_io_group of fe_policy_io.h).
template <class Key>
static void fe_group_rows(const Key* keys, int n, std::vector<int>& rows, std::vector<int>& seg) {
    rows.resize((size_t)n); seg.clear();
    for (int i = 0; i < n; i++) rows[i] = i;
    std::stable_sort(rows.begin(), rows.end(), [&](int a, int b) { return keys[a] < keys[b]; });
    for (int j = 0; j < n; j++) if (j == 0 || keys[rows[j]] != keys[rows[j - 1]]) seg.push_back(j);
    seg.push_back(n);
}
#define CHECK_SMOKE_LIST(h, list) do { if (!(h)->smoke) FAIL(h, "no smoke field"); if ((list) < 0 || (list) >= FE_SMOKE_MAX_LISTS) FAIL(h, "smoke cell list id out of range"); \
    if (!(h)->smoke_reads || (h)->smoke_reads->list[list].n == 0) FAIL(h, "smoke cell list not set: fe_smoke_cells_set first"); } while (0)

extern "C" {

int fe_smoke_cells_set(FeEngine* h, int list, const int* cells, int n) {
    FE_ENTRY(h);
    if (!h->smoke) FAIL(h, "no smoke field");
    if (list < 0 || list >= FE_SMOKE_MAX_LISTS) FAIL(h, "smoke cell list id out of range");
    if (n < 0) FAIL(h, "fe_smoke_cells_set: n < 0 (the list is unchanged)");
    if (n > FE_SMOKE_MAX_LIST_CELLS) FAIL(h, "fe_smoke_cells_set: more than FE_SMOKE_MAX_LIST_CELLS cells (the list is unchanged)");
    const SmokeP& P = h->smoke->P;
    if (!cells || n == 0) {
        if (h->smoke_reads && h->smoke_reads->list[list].n) {
            HIPCK(h, hipStreamSynchronize(h->stream));
            smoke_list_free(h->smoke_reads->list[list]);
        }
        return 0;
    }
    SmokeCellList L;                                          // (built aside and swapped in once complete: a failure leaves the old list as it was)
    L.n = n;
    L.cells.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        const int a = cells[3 * i], b = cells[3 * i + 1], c = cells[3 * i + 2];
        if (a < 0 || a >= P.n || b < 0 || b >= P.n || c < 0 || c >= P.n) FAIL(h, "fe_smoke_cells_set: cell out of range (the list is unchanged)");
        L.cells[(size_t)i] = ((size_t)a * P.n + b) * P.n + c;
    }
    const size_t words = (size_t)n * (3 + P.qd);
    if (dev_alloc(h, &L.idx, (size_t)n, false) || dev_alloc(h, &L.stage, words) || hipHostMalloc((void**)&L.hstage, sizeof(float) * words) != hipSuccess ||
        hipMemcpyOnStream(h, L.idx, L.cells.data(), sizeof(size_t) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) {
        smoke_list_free(L);
        FAIL(h, "fe_smoke_cells_set: allocation or upload failed (the list is unchanged)");
    }
    SmokeCellList& dst = smoke_reads(h)->list[list];
    smoke_list_free(dst);                                     // (the stream has drained: hipMemcpyOnStream)
    dst = std::move(L);
    return 0;
}
static void smoke_gather(FeEngine* h, const SmokeCellList& L, int s, float* v, float* q) {
    const SmokeP& P = h->smoke->P;
    hipLaunchKernelGGL(k_smoke_gather, dim3((L.n + 255) / 256), dim3(256), 0, h->stream, L.n, P.qd, (const float*)(P.v + (size_t)s * P.n3 * 3),
                       (const float*)(P.q + (size_t)s * P.n3 * P.qd), (const size_t*)L.idx, v, q);
}
int fe_smoke_cells_get(FeEngine* h, int list, int s, fe_real* v, fe_real* q) {
    FE_ENTRY(h);
    CHECK_SMOKE_LIST(h, list); CHECK_SMOKE(h, s);
    if (!v && !q) return 0;
    const SmokeCellList& L = h->smoke_reads->list[list];
    const size_t n = (size_t)L.n, qd = (size_t)h->smoke->P.qd;
    smoke_gather(h, L, s, L.stage, L.stage + 3 * n);
    HIPCK(h, hipMemcpyAsync(L.hstage, L.stage, sizeof(float) * n * (3 + qd), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    if (v) std::memcpy(v, L.hstage, sizeof(float) * 3 * n);
    if (q) std::memcpy(q, L.hstage + 3 * n, sizeof(float) * qd * n);
    return 0;
}
int fe_smoke_cells_get_dev(FeEngine* h, int list, int s, fe_real* v, fe_real* q) {
    FE_ENTRY(h);
    CHECK_SMOKE_LIST(h, list); CHECK_SMOKE(h, s);
    if (!v && !q) return 0;
    smoke_gather(h, h->smoke_reads->list[list], s, v, q);
    return check_async(h);
}

// the rows of a list grouped by cell, once per list: a failure leaves the list ungrouped and every adjoint as it was
static int smoke_list_group(FeEngine* h, SmokeCellList& L) {
    if (L.n_seg) return 0;
    std::vector<int> rows, seg;
    fe_group_rows(L.cells.data(), L.n, rows, seg);
    const size_t n = (size_t)L.n, n_seg = seg.size() - 1;
    int *d_rows = nullptr, *d_seg = nullptr; float* d_stage = nullptr;
    if (dev_alloc(h, &d_rows, n, false) || dev_alloc(h, &d_seg, n_seg + 1, false) || dev_alloc(h, &d_stage, n * (3 + (size_t)h->smoke->P.qd)) ||
        hipMemcpyAsync(d_rows, rows.data(), sizeof(int) * n, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyOnStream(h, d_seg, seg.data(), sizeof(int) * (n_seg + 1), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        for (void* q : {(void*)d_rows, (void*)d_seg, (void*)d_stage}) if (q) (void)hipFree(q);
        FAIL(h, "fe_smoke_cells_add_grad: allocation or upload of the grouping failed (nothing has changed)");
    }
    L.rows = d_rows; L.seg = d_seg; L.gstage = d_stage; L.n_seg = (int)n_seg;
    return 0;
}
// gv, gq: device pointers (or nullptr); enqueued
static void smoke_scatter(FeEngine* h, const SmokeCellList& L, int s, const float* gv, const float* gq) {
    const SmokeP& P = h->smoke->P;
    const SmokeScatterArgs a = {L.n_seg, P.qd, P.gv + (size_t)s * P.n3 * 3, P.gq + (size_t)s * P.n3 * P.qd, L.idx, L.rows, L.seg, gv, gq};
    hipLaunchKernelGGL(k_smoke_scatter_grad<0>, dim3((L.n_seg + 255) / 256), dim3(256), 0, h->stream, a);
}
// gv.grad[s][cells[i]] += gv[i], gq.grad[s][cells[i]] += gq[i] for the rows of a cell list (host pointers; staged, waits)
int fe_smoke_cells_add_grad(FeEngine* h, int list, int s, const fe_real* gv, const fe_real* gq) {
    if (!h) return 1;
    FE_ENTRY(h);
    CHECK_SMOKE_LIST(h, list); CHECK_SMOKE(h, s);
    if (!gv && !gq) return 0;
    SmokeCellList& L = h->smoke_reads->list[list];
    if (smoke_list_group(h, L)) return 1;
    const size_t n = (size_t)L.n, qd = (size_t)h->smoke->P.qd;
    if (gv) HIPCK(h, hipMemcpyAsync(L.gstage, gv, sizeof(float) * 3 * n, hipMemcpyHostToDevice, h->stream));
    if (gq) HIPCK(h, hipMemcpyAsync(L.gstage + 3 * n, gq, sizeof(float) * qd * n, hipMemcpyHostToDevice, h->stream));
    smoke_scatter(h, L, s, gv ? L.gstage : nullptr, gq ? L.gstage + 3 * n : nullptr);
    HIPCK(h, hipStreamSynchronize(h->stream));
    return check_async(h);
}
// the same from device pointers; enqueued, does not wait: the caller keeps gv and gq as they are until the engine's stream has passed
int fe_smoke_cells_add_grad_dev(FeEngine* h, int list, int s, const fe_real* gv, const fe_real* gq) {
    if (!h) return 1;
    FE_ENTRY(h);
    CHECK_SMOKE_LIST(h, list); CHECK_SMOKE(h, s);
    if (!gv && !gq) return 0;
    SmokeCellList& L = h->smoke_reads->list[list];
    if (smoke_list_group(h, L)) return 1;
    smoke_scatter(h, L, s, gv, gq);
    return check_async(h);
}

// ---- the observation vector of Circulation and its adjoint: the AirCon's state at frame f, then the list's v and q rows of frame s
// The refusals shared by the four variants; nothing has been launched or changed when one of them returns.
static int smoke_obs_check(FeEngine* h, int list, int s, int eff, int f, int n_words, const void* ptr, const char* null_msg) {
    CHECK_SMOKE_LIST(h, list); CHECK_SMOKE(h, s);
    CHECK_EFF(h, eff); CHECK_FRAME(h, f);
    if (h->effs[eff].p.type != FE_EFF_AIRCON) FAIL(h, "fe_smoke_obs: the effector is not an AirCon (nothing has changed)");
    const long long want = (long long)FE_SMOKE_OBS_STATE + (long long)h->smoke_reads->list[list].n * (3 + h->smoke->P.qd);
    if ((long long)n_words != want) FAIL(h, "fe_smoke_obs: the vector's length is not 9 + n (3 + q_dim) for this list (nothing has changed)");
    if (h->smoke->P.qd > 3) FAIL(h, "fe_smoke_obs: q_dim > 3 (nothing has changed)");
    if (!ptr) FAIL(h, null_msg);
    return 0;
}
static int smoke_obs_stage(FeEngine* h, SmokeCellList& L) {
    const size_t words = (size_t)FE_SMOKE_OBS_STATE + (size_t)L.n * (3 + (size_t)h->smoke->P.qd);
    if (!L.ostage && dev_alloc(h, &L.ostage, words)) return 1;
    if (!L.ohstage) HIPCK(h, hipHostMalloc((void**)&L.ohstage, sizeof(float) * words));
    return 0;
}
static SmokeObsArgs smoke_obs_args(FeEngine* h, const SmokeCellList& L, int s, int eff, int f) {
    const SmokeP& P = h->smoke->P;
    const EffP& p = h->effs[eff].p;
    SmokeObsArgs a;
    a.n = L.n; a.n_seg = L.n_seg; a.qd = P.qd; a.f = f;
    a.vf = P.v + (size_t)s * P.n3 * 3; a.qf = P.q + (size_t)s * P.n3 * P.qd;
    a.gvf = P.gv + (size_t)s * P.n3 * 3; a.gqf = P.gq + (size_t)s * P.n3 * P.qd;
    a.idx = L.idx; a.rows = L.rows; a.seg = L.seg;
    a.pos = p.pos; a.quat = p.quat; a.sa = p.sa; a.ra = p.ra;
    a.gpos = p.gpos; a.gquat = p.gquat; a.gsa = p.gsa; a.gra = p.gra;
    a.out = nullptr; a.g = nullptr;
    return a;
}
static unsigned smoke_obs_wgs(int rows) { return (unsigned)(((rows > FE_SMOKE_OBS_STATE ? rows : FE_SMOKE_OBS_STATE) + 255) / 256); }

// out[0..9) = pos, quat, s, r of AirCon `eff` at local frame f; then v rows [n][3] and q rows [n][q_dim] of the list in smoke frame s (host pointer; waits)
int fe_smoke_obs_get(FeEngine* h, int list, int s, int eff, int f, fe_real* out, int n_out) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (smoke_obs_check(h, list, s, eff, f, n_out, out, "fe_smoke_obs_get: out is NULL")) return 1;
    SmokeCellList& L = h->smoke_reads->list[list];
    if (smoke_obs_stage(h, L)) return 1;
    SmokeObsArgs a = smoke_obs_args(h, L, s, eff, f);
    a.out = L.ostage;
    hipLaunchKernelGGL(k_smoke_obs_pack<0>, dim3(smoke_obs_wgs(L.n)), dim3(256), 0, h->stream, a);
    HIPCK(h, hipMemcpyAsync(L.ohstage, L.ostage, sizeof(float) * (size_t)n_out, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    std::memcpy(out, L.ohstage, sizeof(float) * (size_t)n_out);
    return 0;
}
// the same into a device pointer; enqueued, does not wait
int fe_smoke_obs_get_dev(FeEngine* h, int list, int s, int eff, int f, fe_real* out, int n_out) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (smoke_obs_check(h, list, s, eff, f, n_out, out, "fe_smoke_obs_get_dev: out is NULL")) return 1;
    const SmokeCellList& L = h->smoke_reads->list[list];
    SmokeObsArgs a = smoke_obs_args(h, L, s, eff, f);
    a.out = out;
    hipLaunchKernelGGL(k_smoke_obs_pack<0>, dim3(smoke_obs_wgs(L.n)), dim3(256), 0, h->stream, a);
    return check_async(h);
}
// the adjoint: g laid out like the vector; its v / q rows are added to gv[s] / gq[s] at the list's cells, its first nine words to
// gpos[f], gquat[f], gsa[f], gra[f] of the AirCon (host pointer; staged, waits)
int fe_smoke_obs_add_grad(FeEngine* h, int list, int s, int eff, int f, const fe_real* g, int n_g) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (smoke_obs_check(h, list, s, eff, f, n_g, g, "fe_smoke_obs_add_grad: g is NULL")) return 1;
    SmokeCellList& L = h->smoke_reads->list[list];
    if (smoke_list_group(h, L) || smoke_obs_stage(h, L)) return 1;
    HIPCK(h, hipMemcpyAsync(L.ostage, g, sizeof(float) * (size_t)n_g, hipMemcpyHostToDevice, h->stream));
    SmokeObsArgs a = smoke_obs_args(h, L, s, eff, f);
    a.g = L.ostage;
    hipLaunchKernelGGL(k_smoke_obs_scatter_grad<0>, dim3(smoke_obs_wgs(L.n_seg)), dim3(256), 0, h->stream, a);
    HIPCK(h, hipStreamSynchronize(h->stream));
    return check_async(h);
}
// the same from a device pointer; enqueued, does not wait: the caller keeps g as it is until the engine's stream has passed
int fe_smoke_obs_add_grad_dev(FeEngine* h, int list, int s, int eff, int f, const fe_real* g, int n_g) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (smoke_obs_check(h, list, s, eff, f, n_g, g, "fe_smoke_obs_add_grad_dev: g is NULL")) return 1;
    SmokeCellList& L = h->smoke_reads->list[list];
    if (smoke_list_group(h, L)) return 1;
    SmokeObsArgs a = smoke_obs_args(h, L, s, eff, f);
    a.g = g;
    hipLaunchKernelGGL(k_smoke_obs_scatter_grad<0>, dim3(smoke_obs_wgs(L.n_seg)), dim3(256), 0, h->stream, a);
    return check_async(h);
}

int fe_smoke_loss_alloc(FeEngine* h, int max_loss_steps) {
    FE_ENTRY(h);
    if (!h->smoke) FAIL(h, "no smoke field");
    if (max_loss_steps <= 0) FAIL(h, "fe_smoke_loss_alloc: max_loss_steps must be positive");
    double* sl = nullptr;
    if (dev_alloc(h, &sl, (size_t)max_loss_steps)) return 1;
    HIPCK(h, hipStreamSynchronize(h->stream));               // (an earlier step may still write the old array)
    SmokeReads* R = smoke_reads(h);
    if (R->step_loss) (void)hipFree(R->step_loss);
    R->step_loss = sl; R->loss_steps = max_loss_steps;
    return 0;
}
int fe_smoke_loss_set(FeEngine* h, int list, int comp, int kind, const double* target, const double* weight) {
    FE_ENTRY(h);
    CHECK_SMOKE_LIST(h, list);
    const SmokeP& P = h->smoke->P;
    if (comp < 0 || comp >= P.qd) FAIL(h, "fe_smoke_loss_set: comp outside [0, q_dim) (the loss is unchanged)");
    if (kind != FE_SMOKE_L1 && kind != FE_SMOKE_SQ) FAIL(h, "fe_smoke_loss_set: unknown kind (the loss is unchanged)");
    if (!target) FAIL(h, "fe_smoke_loss_set: null target (the loss is unchanged)");
    SmokeReads* R = h->smoke_reads;
    const SmokeCellList& L = R->list[list];
    std::vector<size_t> sorted(L.cells);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
        FAIL(h, "fe_smoke_loss_set: the list names a cell twice (each gradient entry is one read-modify-write) (the loss is unchanged)");
    const size_t n = (size_t)L.n;
    const std::vector<double> ones(weight ? 0 : n, 1.0);
    size_t* d_i = nullptr; double *d_t = nullptr, *d_w = nullptr;
    if (dev_alloc(h, &d_i, n, false) || dev_alloc(h, &d_t, n, false) || dev_alloc(h, &d_w, n, false) ||
        hipMemcpyAsync(d_i, L.cells.data(), sizeof(size_t) * n, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(d_t, target, sizeof(double) * n, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyOnStream(h, d_w, weight ? weight : ones.data(), sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        for (void* q : {(void*)d_i, (void*)d_t, (void*)d_w}) if (q) (void)hipFree(q);
        FAIL(h, "fe_smoke_loss_set: allocation or upload failed (the loss is unchanged)");
    }
    for (void* q : {(void*)R->loss_idx, (void*)R->loss_target, (void*)R->loss_weight}) if (q) (void)hipFree(q);   // (the stream has drained)
    R->loss_idx = d_i; R->loss_target = d_t; R->loss_weight = d_w;
    R->loss_n = L.n; R->loss_comp = comp; R->loss_kind = kind;
    return 0;
}
int fe_smoke_loss_clear(FeEngine* h) {
    FE_ENTRY(h);
    if (!h->smoke) FAIL(h, "no smoke field");
    SmokeReads* R = h->smoke_reads;
    if (!R || !R->loss_steps) FAIL(h, "no smoke-loss array: fe_smoke_loss_alloc first");
    HIPCK(h, hipMemsetAsync(R->step_loss, 0, sizeof(double) * (size_t)R->loss_steps, h->stream));
    return 0;
}
static int smoke_loss_check_step(FeEngine* h, int s_loss, int s) {
    CHECK_SMOKE(h, s);
    SmokeReads* R = h->smoke_reads;
    if (!R || !R->loss_steps) FAIL(h, "no smoke-loss array: fe_smoke_loss_alloc first");
    if (R->loss_n <= 0) FAIL(h, "no smoke loss: fe_smoke_loss_set first");
    if (s_loss < 0 || s_loss >= R->loss_steps) FAIL(h, "smoke loss step out of range");
    return 0;
}
int fe_smoke_loss_step(FeEngine* h, int s_loss, int s) {
    FE_ENTRY(h);
    if (smoke_loss_check_step(h, s_loss, s)) return 1;
    const SmokeP& P = h->smoke->P;
    SmokeReads* R = h->smoke_reads;
    hipLaunchKernelGGL(k_smoke_loss_fwd, dim3(1), dim3(FE_TL_WG), 0, h->stream, R->loss_n, P.qd, R->loss_comp, R->loss_kind, (const float*)(P.q + (size_t)s * P.n3 * P.qd),
                       (const size_t*)R->loss_idx, (const double*)R->loss_target, (const double*)R->loss_weight, R->step_loss + s_loss);
    return check_async(h);
}
int fe_smoke_loss_step_grad(FeEngine* h, int s_loss, int s, double scale) {
    FE_ENTRY(h);
    if (smoke_loss_check_step(h, s_loss, s)) return 1;
    const SmokeP& P = h->smoke->P;
    SmokeReads* R = h->smoke_reads;
    hipLaunchKernelGGL(k_smoke_loss_bwd, dim3((R->loss_n + 255) / 256), dim3(256), 0, h->stream, R->loss_n, P.qd, R->loss_comp, R->loss_kind,
                       (const float*)(P.q + (size_t)s * P.n3 * P.qd), P.gq + (size_t)s * P.n3 * P.qd, (const size_t*)R->loss_idx, (const double*)R->loss_target,
                       (const double*)R->loss_weight, scale);
    return check_async(h);
}
int fe_smoke_loss_get(FeEngine* h, int s0, int n, double* step_loss) {
    FE_ENTRY(h);
    if (!h->smoke) FAIL(h, "no smoke field");
    SmokeReads* R = h->smoke_reads;
    if (!R || !R->loss_steps) FAIL(h, "no smoke-loss array: fe_smoke_loss_alloc first");
    if (s0 < 0 || n < 0 || s0 + n > R->loss_steps) FAIL(h, "fe_smoke_loss_get: steps out of range");
    if (step_loss && n > 0) HIPCK(h, hipMemcpyAsync(step_loss, R->step_loss + s0, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return check_async(h);
}

int fe_smoke_summary(FeEngine* h, int s, FeSmokeSummary* out, int record_size) {
    FE_ENTRY(h);
    CHECK_SMOKE(h, s);
    if (record_size != (int)sizeof(FeSmokeSummary)) FAIL(h, "fe_smoke_summary: record_size is not sizeof(FeSmokeSummary)");
    if (!out) return 0;
    const SmokeP& P = h->smoke->P;
    SmokeReads* R = smoke_reads(h);
    if (!R->partial && dev_alloc(h, &R->partial, (size_t)FE_SS_MAX_WGS, false)) return 1;
    if (!R->sum_out && dev_alloc(h, &R->sum_out, (size_t)1)) return 1;
    const int j0 = P.ly + 1 > 0 ? P.ly + 1 : 0, j1 = P.hy < P.n ? P.hy : P.n;     // the slab ly < j < hy, inside the grid
    const int nj = j1 > j0 ? j1 - j0 : 0;
    const long long cells = (long long)P.n * nj * P.n;
    long long wgs = (cells + FE_SS_WG - 1) / FE_SS_WG;
    if (wgs > FE_SS_MAX_WGS) wgs = FE_SS_MAX_WGS;
    if (wgs < 1) wgs = 1;                                     // (an empty slab: one workgroup leaves one cleared record)
    hipLaunchKernelGGL(k_smoke_summary, dim3((unsigned)wgs), dim3(FE_SS_WG), 0, h->stream, P.n, P.qd, j0, nj, (const float*)(P.v + (size_t)s * P.n3 * 3),
                       (const float*)(P.q + (size_t)s * P.n3 * P.qd), R->partial);
    hipLaunchKernelGGL(k_smoke_summary_merge, dim3(1), dim3(FE_SS_LANES), 0, h->stream, (const FeSmokeAcc*)R->partial, (int)wgs, (double)P.dt, P.qd, R->sum_out);
    HIPCK(h, hipMemcpyAsync(out, R->sum_out, sizeof(FeSmokeSummary), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return check_async(h);
}

}  // extern "C"
#endif /* FE_SMOKE_READS_MATH_ONLY */
#endif /* FE_SMOKE_READS_H */
