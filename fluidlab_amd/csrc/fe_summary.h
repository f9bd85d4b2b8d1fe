// fe_summary.h -- reads of a GPU-resident frame that do not copy it: the observation gather and the per-group frame summary
// (include/fluidengine_ext.h: fe_obs_*, fe_summary_set_groups, fe_frame_summary).
// Included by fe_engine.hip behind struct FeEngine and its helpers, the first of the extension headers: the kernels use the engine's frame views
// and order tables, the host half -- the state (SummaryState, one pointer in FeEngine), summary_drop for fe_destroy, the entries -- the engine itself.
// The first part -- the record, one particle's contribution, the merge of two records, the final division -- is plain __host__ __device__ code without
// any of that: tests/csrc/summary_test.cpp compiles it for the host with FE_SUMMARY_MATH_ONLY defined and checks it against an fp64 loop.
//
// Both kernels only READ the frame, the order table and pinfo: no plane, table, key or flag of the engine changes, a compact F
// (FrameV::iso) is read through load_F and stays compact.
#ifndef FE_SUMMARY_H
#define FE_SUMMARY_H

// The running record of one group: sums, not yet divided.  19 eight-byte words.
struct FeSumAcc {
    long long n_used, n_nonfinite;
    double mass, mx[3], mom[3], kin;         // sum m, sum m x, sum m v, 1/2 sum m |v|^2
    double v_max, lo[3], hi[3], J_min, J_max;
};
#define FE_SUM_WORDS 19
static_assert(sizeof(FeSumAcc) == 8 * FE_SUM_WORDS, "FeSumAcc is 19 eight-byte words");

__host__ __device__ inline void fe_sum_clear(FeSumAcc& a) {
    const double inf = __builtin_huge_val();
    a.n_used = 0; a.n_nonfinite = 0; a.mass = 0.0; a.kin = 0.0; a.v_max = 0.0; a.J_min = inf; a.J_max = -inf;
    for (int d = 0; d < 3; d++) { a.mx[d] = 0.0; a.mom[d] = 0.0; a.lo[d] = inf; a.hi[d] = -inf; }
}
// (the bit pattern, not a comparison: holds under any floating-point build flags, on the host and on the device)
__host__ __device__ inline bool fe_sum_finite(float w) {
    unsigned u;
    __builtin_memcpy(&u, &w, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}
// One USED particle: m is the engine's fp32 mass, x[3] v[3] C[9] F[9] the frame's fp32 words.  Every product and sum is formed in fp64 from
// the widened words.  A particle with a non-finite word anywhere in x, v, C or F is counted and contributes to nothing else.
__host__ __device__ inline void fe_sum_particle(FeSumAcc& a, float m, const float* x, const float* v, const float* C, const float* F) {
    a.n_used += 1;
    bool ok = true;
    for (int d = 0; d < 3; d++) ok = ok && fe_sum_finite(x[d]) && fe_sum_finite(v[d]);
    for (int d = 0; d < 9; d++) ok = ok && fe_sum_finite(C[d]) && fe_sum_finite(F[d]);
    if (!ok) { a.n_nonfinite += 1; return; }
    const double md = (double)m;
    double vv = 0.0;
    a.mass += md;
    for (int d = 0; d < 3; d++) {
        const double xd = (double)x[d], vd = (double)v[d], av = vd < 0.0 ? -vd : vd;
        a.mx[d] += md * xd;
        a.mom[d] += md * vd;
        vv += vd * vd;
        if (av > a.v_max) a.v_max = av;
        if (xd < a.lo[d]) a.lo[d] = xd;
        if (xd > a.hi[d]) a.hi[d] = xd;
    }
    a.kin += 0.5 * md * vv;
    // det F, cofactor expansion along the first row
    const double f0 = F[0], f1 = F[1], f2 = F[2], f3 = F[3], f4 = F[4], f5 = F[5], f6 = F[6], f7 = F[7], f8 = F[8];
    const double J = f0 * (f4 * f8 - f5 * f7) - f1 * (f3 * f8 - f5 * f6) + f2 * (f3 * f7 - f4 * f6);
    if (J < a.J_min) a.J_min = J;
    if (J > a.J_max) a.J_max = J;
}
// a <- a merged with b (counts and sums add, extremes combine): associative up to the rounding of the fp64 sums
__host__ __device__ inline void fe_sum_merge(FeSumAcc& a, const FeSumAcc& b) {
    a.n_used += b.n_used; a.n_nonfinite += b.n_nonfinite;
    a.mass += b.mass; a.kin += b.kin;
    if (b.v_max > a.v_max) a.v_max = b.v_max;
    if (b.J_min < a.J_min) a.J_min = b.J_min;
    if (b.J_max > a.J_max) a.J_max = b.J_max;
    for (int d = 0; d < 3; d++) {
        a.mx[d] += b.mx[d]; a.mom[d] += b.mom[d];
        if (b.lo[d] < a.lo[d]) a.lo[d] = b.lo[d];
        if (b.hi[d] > a.hi[d]) a.hi[d] = b.hi[d];
    }
}
// The record handed out.  A group without a finite used particle is all zeros apart from its two counts.
__host__ __device__ inline void fe_sum_finish(const FeSumAcc& a, double dt, double dx, FeFrameSummary& o) {
    o.n_used = a.n_used; o.n_nonfinite = a.n_nonfinite;
    const bool any = a.n_used > a.n_nonfinite;
    o.mass = any ? a.mass : 0.0;
    o.kinetic = any ? a.kin : 0.0;
    o.v_max = any ? a.v_max : 0.0;
    o.courant = any ? dt * a.v_max / dx : 0.0;
    o.J_min = any ? a.J_min : 0.0;
    o.J_max = any ? a.J_max : 0.0;
    for (int d = 0; d < 3; d++) {
        o.com[d] = (any && a.mass != 0.0) ? a.mx[d] / a.mass : 0.0;
        o.momentum[d] = any ? a.mom[d] : 0.0;
        o.lo[d] = any ? a.lo[d] : 0.0;
        o.hi[d] = any ? a.hi[d] : 0.0;
    }
}

#ifndef FE_SUMMARY_MATH_ONLY
// ---- observation gather ---------------------------------------------------------------------------------------------
// Row i = particle pids[i] of the frame: its slot comes from the slot_of_pid of the FRAME's order (frames on either side of a sort have
// different tables).  One thread per list entry, three compact arrays out (NULL = skipped); device or staging pointers alike.
__global__ __launch_bounds__(256) void k_obs_gather(int n, int N, size_t Np, float* fr_, const int* __restrict__ slot_of_pid, const int* __restrict__ pids,
                                                    float* __restrict__ x, float* __restrict__ v, int* __restrict__ used) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int pid = pids[i];
    if ((unsigned)pid >= (unsigned)N) return;                 // (checked on the host when the list was set)
    const int s = slot_of_pid[pid];
    if ((unsigned)s >= (unsigned)Np) return;
    const FrameV fr = frame_view(fr_, Np);
    const float4 a0 = fr.A0[s], a1 = fr.A1[s];
    if (x) { x[3 * (size_t)i] = a0.x; x[3 * (size_t)i + 1] = a0.y; x[3 * (size_t)i + 2] = a0.z; }
    if (v) { v[3 * (size_t)i] = a0.w; v[3 * (size_t)i + 1] = a1.x; v[3 * (size_t)i + 2] = a1.y; }
    if (used) used[i] = fr.used[s];
}

// ---- frame summary --------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fe_sum_wave_reduce(FeSumAcc& r) {          // butterfly: every lane ends with the merge of all 64, in one fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        FeSumAcc b;
        b.n_used = __shfl_xor(r.n_used, o, 64); b.n_nonfinite = __shfl_xor(r.n_nonfinite, o, 64);
        b.mass = __shfl_xor(r.mass, o, 64); b.kin = __shfl_xor(r.kin, o, 64); b.v_max = __shfl_xor(r.v_max, o, 64);
        b.J_min = __shfl_xor(r.J_min, o, 64); b.J_max = __shfl_xor(r.J_max, o, 64);
#pragma unroll
        for (int d = 0; d < 3; d++) {
            b.mx[d] = __shfl_xor(r.mx[d], o, 64); b.mom[d] = __shfl_xor(r.mom[d], o, 64);
            b.lo[d] = __shfl_xor(r.lo[d], o, 64); b.hi[d] = __shfl_xor(r.hi[d], o, 64);
        }
        fe_sum_merge(r, b);
    }
}
#define FE_SUM_WG 256
// One pass over the slots of the frame, grid-stride.  A lane forms its particle's record; the wave then reduces once per group present among
// its lanes (particles of a body sit together in a sorted order: usually one or two) and keeps the running records in registers, spread over
// its lanes: lane l holds the wave's record of group l, lane n_groups that of the whole frame (n_groups + 1 <= 33 lanes).  The waves of a
// workgroup work independently until the end, where they take turns -- once -- at adding their records to the workgroup's in LDS
// (<= 33 x 19 words).  No atomic anywhere: the result does not depend on timing.  Each workgroup leaves its records in partial[blockIdx.x][...].
__global__ __launch_bounds__(FE_SUM_WG) void k_frame_summary(int N, size_t Np, float* fr_, int iso, const int* __restrict__ pid_of_slot, const float4* __restrict__ pinfo,
                                                             const int* __restrict__ group, int n_groups, FeSumAcc* __restrict__ partial) {
    __shared__ FeSumAcc rec[FE_SUMMARY_MAX_GROUPS + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_rec = n_groups + 1;
    if (tid < n_rec) fe_sum_clear(rec[tid]);
    const FrameV fr = frame_view(fr_, Np, 0, iso);
    FeSumAcc acc;                                             // this lane's record of the wave (see above)
    fe_sum_clear(acc);
    for (int base = blockIdx.x * FE_SUM_WG; base < N; base += gridDim.x * FE_SUM_WG) {
        const int s = base + tid;
        FeSumAcc mine;
        fe_sum_clear(mine);
        int g = -2;                                           // -2: nothing to add; -1: in no group (the whole-frame record only)
        if (s < N && fr.used[s] != 0) {
            const int pid = pid_of_slot[s];
            if ((unsigned)pid < (unsigned)N) {
                g = group ? group[pid] : -1;
                if ((unsigned)g >= (unsigned)n_groups) g = -1;
                PState p;
                load_xvC(fr, s, p);
                load_F(fr, s, p.F);
                fe_sum_particle(mine, pinfo[pid].z, p.x, p.v, &p.C.a[0][0], &p.F.a[0][0]);
            }
        }
        unsigned long long todo = __ballot(g != -2);
        while (todo) {                                        // (wave-uniform)
            const int gl = __shfl(g, __builtin_ctzll(todo), 64);
            const bool in = g == gl;
            FeSumAcc r;
            fe_sum_clear(r);
            if (in) r = mine;
            fe_sum_wave_reduce(r);
            if (lane == gl || lane == n_groups) fe_sum_merge(acc, r);      // (gl == -1 is no lane's group: the whole-frame record only)
            todo &= ~__ballot(in);
        }
    }
    __syncthreads();
    for (int w = 0; w < FE_SUM_WG / 64; w++) {
        if (wave == w && lane < n_rec) fe_sum_merge(rec[lane], acc);
        __syncthreads();
    }
    if (tid < n_rec) partial[(size_t)blockIdx.x * n_rec + tid] = rec[tid];
}
// One wave per record: lane l merges the partials l, l + 64, ... in order, the wave reduces, lane 0 divides and writes the record.
__global__ __launch_bounds__(64) void k_frame_summary_merge(const FeSumAcc* __restrict__ partial, int n_partial, int n_rec, double dt, double dx, FeFrameSummary* __restrict__ out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    FeSumAcc a;
    fe_sum_clear(a);
    for (int i = lane; i < n_partial; i += 64) fe_sum_merge(a, partial[(size_t)i * n_rec + r]);
    fe_sum_wave_reduce(a);
    if (lane == 0) fe_sum_finish(a, dt, dx, out[r]);
}

// ---------------------------------------------------------------------------------------------------------------- host
#define FE_SUM_MAX_WGS 1024
struct SummaryState {
    int* obs_pids = nullptr; int obs_n = 0;                   // fe_obs_set_particles: the observation list on the device, and staging for the host variant of fe_obs_get
    float *obs_x = nullptr, *obs_v = nullptr; int* obs_u = nullptr;       // [3 n], [3 n], [n]
    int* sum_group = nullptr; int sum_n_groups = 0;           // fe_summary_set_groups: group[N] by particle id (nullptr: the whole-frame record only)
    FeSumAcc* sum_partial = nullptr; FeFrameSummary* sum_out = nullptr;   // fe_frame_summary: [FE_SUM_MAX_WGS][33] partial records, [33] results; allocated at the first call
};
// every entry starts from the state, empty at first: an entry called before any set-up meets the same checks on the same zeros as ever
static SummaryState* summary_state(FeEngine* h) {
    if (!h->summary) h->summary = new SummaryState();
    return h->summary;
}
static void summary_drop(FeEngine* h) {                       // fe_destroy
    SummaryState* Q = h->summary;
    if (!Q) return;
    for (void* q : {(void*)Q->obs_pids, (void*)Q->obs_x, (void*)Q->obs_v, (void*)Q->obs_u, (void*)Q->sum_group, (void*)Q->sum_partial, (void*)Q->sum_out}) if (q) (void)hipFree(q);
    delete Q;
    h->summary = nullptr;
}
static int obs_gather(FeEngine* h, int f, float* x, float* v, int* used) {
    const SummaryState* Q = h->summary;
    const int n = Q->obs_n;
    hipLaunchKernelGGL(k_obs_gather, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, h->N, (size_t)h->Np, h->frame(f), (const int*)h->tables[h->tbl_of_frame[f]].slot_of_pid,
                       (const int*)Q->obs_pids, x, v, used);
    return 0;
}
namespace { void policy_io_set_list(FeEngine* h, const int* pids, int n); }      // (fe_policy_io.h, which reads the list kept here)

extern "C" {

// Read-only calls: no table, key, dirty flag or fiso entry changes, a compact F stays compact.
int fe_obs_set_particles(FeEngine* h, const int* pids, int n) {
    FE_ENTRY(h);
    SummaryState* Q = summary_state(h);
    if (n < 0) FAIL(h, "fe_obs_set_particles: n < 0");
    int *d_p = nullptr, *d_u = nullptr; float *d_x = nullptr, *d_v = nullptr;
    if (pids && n > 0) {
        for (int i = 0; i < n; i++) if (pids[i] < 0 || pids[i] >= h->N) FAIL(h, "fe_obs_set_particles: particle id out of range (the list is unchanged)");
        if (dev_alloc(h, &d_p, (size_t)n, false) || dev_alloc(h, &d_x, (size_t)3 * n) || dev_alloc(h, &d_v, (size_t)3 * n) || dev_alloc(h, &d_u, (size_t)n)) {
            for (void* q : {(void*)d_p, (void*)d_x, (void*)d_v, (void*)d_u}) if (q) (void)hipFree(q);
            return 1;
        }
        if (hipMemcpyOnStream(h, d_p, pids, sizeof(int) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) {
            for (void* q : {(void*)d_p, (void*)d_x, (void*)d_v, (void*)d_u}) (void)hipFree(q);
            FAIL(h, "fe_obs_set_particles: hipMemcpy failed");
        }
    } else n = 0;
    HIPCK(h, hipStreamSynchronize(h->stream));               // (an earlier gather may still read the old list)
    for (void* q : {(void*)Q->obs_pids, (void*)Q->obs_x, (void*)Q->obs_v, (void*)Q->obs_u}) if (q) (void)hipFree(q);
    Q->obs_pids = d_p; Q->obs_x = d_x; Q->obs_v = d_v; Q->obs_u = d_u; Q->obs_n = n;
    policy_io_set_list(h, pids, n);                           // (fe_obs_add_grad groups the new list's rows at its first call)
    return 0;
}
int fe_obs_get(FeEngine* h, int f, fe_real* x, fe_real* v, int* used) {
    FE_ENTRY(h);
    SummaryState* Q = summary_state(h);
    CHECK_FRAME(h, f);
    if (!Q->obs_pids) FAIL(h, "no observation list: fe_obs_set_particles first");
    if (!x && !v && !used) return 0;
    const size_t n = (size_t)Q->obs_n;
    obs_gather(h, f, x ? Q->obs_x : nullptr, v ? Q->obs_v : nullptr, used ? Q->obs_u : nullptr);
    if (x) HIPCK(h, hipMemcpyAsync(x, Q->obs_x, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, h->stream));
    if (v) HIPCK(h, hipMemcpyAsync(v, Q->obs_v, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, h->stream));
    if (used) HIPCK(h, hipMemcpyAsync(used, Q->obs_u, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    return check_device_errors(h);
}
int fe_obs_get_dev(FeEngine* h, int f, fe_real* x, fe_real* v, int* used) {
    FE_ENTRY(h);
    SummaryState* Q = summary_state(h);
    CHECK_FRAME(h, f);
    if (!Q->obs_pids) FAIL(h, "no observation list: fe_obs_set_particles first");
    if (!x && !v && !used) return 0;
    obs_gather(h, f, x, v, used);
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    return check_device_errors(h);
}
int fe_summary_set_groups(FeEngine* h, const int* group, int n_groups) {
    FE_ENTRY(h);
    SummaryState* Q = summary_state(h);
    if (!group) n_groups = 0;
    if (n_groups < 0 || n_groups > FE_SUMMARY_MAX_GROUPS) FAIL(h, "fe_summary_set_groups: n_groups must be in [0, FE_SUMMARY_MAX_GROUPS]");
    if (group) for (int i = 0; i < h->N; i++) if (group[i] < -1 || group[i] >= n_groups) FAIL(h, "fe_summary_set_groups: group id out of range (the groups are unchanged)");
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (!group) {
        if (Q->sum_group) (void)hipFree(Q->sum_group);
        Q->sum_group = nullptr; Q->sum_n_groups = 0;
        return 0;
    }
    int* d_g = nullptr;                                       // (a buffer of its own, swapped in once it is complete: a failed upload leaves the old groups as they were)
    if (dev_alloc(h, &d_g, (size_t)h->N, false)) return 1;
    if (hipMemcpyOnStream(h, d_g, group, sizeof(int) * (size_t)h->N, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_g); FAIL(h, "fe_summary_set_groups: hipMemcpy failed (the groups are unchanged)"); }
    if (Q->sum_group) (void)hipFree(Q->sum_group);
    Q->sum_group = d_g; Q->sum_n_groups = n_groups;
    return 0;
}
int fe_frame_summary(FeEngine* h, int f, FeFrameSummary* out, int n_records, int record_size) {
    FE_ENTRY(h);
    SummaryState* Q = summary_state(h);
    CHECK_FRAME(h, f);
    if (record_size != (int)sizeof(FeFrameSummary)) FAIL(h, "fe_frame_summary: record_size is not sizeof(FeFrameSummary)");
    if (!out || n_records <= 0) return 0;
    const int n_rec = Q->sum_n_groups + 1, n_out = n_records < n_rec ? n_records : n_rec;
    if (!Q->sum_partial && dev_alloc(h, &Q->sum_partial, (size_t)FE_SUM_MAX_WGS * (FE_SUMMARY_MAX_GROUPS + 1), false)) return 1;
    if (!Q->sum_out && dev_alloc(h, &Q->sum_out, (size_t)FE_SUMMARY_MAX_GROUPS + 1)) return 1;
    int wgs = (h->N + FE_SUM_WG - 1) / FE_SUM_WG;
    if (wgs > FE_SUM_MAX_WGS) wgs = FE_SUM_MAX_WGS;
    if (wgs < 1) wgs = 1;
    hipLaunchKernelGGL(k_frame_summary, dim3(wgs), dim3(FE_SUM_WG), 0, h->stream, h->N, (size_t)h->Np, h->frame(f), h->fiso[f] ? 1 : 0, h->pid_of(f), (const float4*)h->pinfo,
                       (const int*)Q->sum_group, Q->sum_n_groups, Q->sum_partial);
    hipLaunchKernelGGL(k_frame_summary_merge, dim3(n_rec), dim3(64), 0, h->stream, (const FeSumAcc*)Q->sum_partial, wgs, n_rec, (double)h->S.dt, (double)h->S.dx, Q->sum_out);
    // (the records asked for: the first n_out; the whole-frame record is the last of n_groups + 1)
    HIPCK(h, hipMemcpyAsync(out, Q->sum_out, sizeof(FeFrameSummary) * (size_t)n_out, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    return check_device_errors(h);
}

}  // extern "C"
#endif /* FE_SUMMARY_MATH_ONLY */
#endif /* FE_SUMMARY_H */
