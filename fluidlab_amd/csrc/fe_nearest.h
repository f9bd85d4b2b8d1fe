// fe_nearest.h -- "for each query, the nearest point of an indexed set": target clouds and the Chamfer terms of the loss-term programs
// (include/fluidengine_ext.h: fe_cloud_*, FE_TERM_NEAREST_SQ, FE_TERM_COVER_SQ).  Included by fe_task_loss.h behind fe_density.h, between its
// helpers (workgroup sums, frame views), which the kernels here use, and k_task_bwd.  The first part -- the skip test, the squared distance,
// the resolution of the grid, the cell of a point, the ring bound -- is plain __host__ __device__ code: tests/csrc/nearest_math_test.hip
// compiles it for the host with FE_NEAREST_MATH_ONLY defined and checks it against numpy.  Behind the kernels: the state (NearestState, one
// pointer in FeEngine), nearest_drop for fe_destroy, what the loss-term programs call, and the fe_cloud_* entries.
//
// One code path serves both directions.  A set of points is a float4 array (x, y, z, id; id < 0: not a member): the cloud in its own order, or
// the candidates of a frame by slot (k_nn_gather).  An index over a set is a uniform grid over its bounding box (k_nn_bbox, k_nn_plan), a count
// per cell with integer atomics (k_nn_count), an exclusive scan (k_nn_scan) and a fill into a compact copy (k_nn_count<true>); k_nn_query walks
// Chebyshev rings of cells around the query's cell.  The order of the points inside a cell depends on timing; the answer does not: the nearest
// is the smallest d2, and among equal d2 the lowest id.  The kernels are template instantiations (<0>) that take one argument struct, like
// fe_contact.h's: they land at the tail of the code object and the aligned substep group keeps its place.  No floating-point atomics anywhere.
#ifndef FE_NEAREST_H
#define FE_NEAREST_H

#define FE_NN_FIX 1099511627776.0                           /* 2^40: the COVER gradient's fixed point */
#define FE_NN_AXIS_CELLS 64                                 /* at most this many cells along an axis ... */
#define FE_NN_MAX_CELLS (FE_NN_AXIS_CELLS * FE_NN_AXIS_CELLS * FE_NN_AXIS_CELLS)      /* ... and so at most this many cells */
#define FE_NN_PER_CELL 4                                    /* nn_cells = 0 aims at this many points per cell */
// The ring bound is taken this much short of (r h_min)^2 + gap^2: the cell of a point is floor((x - lo) / h) in fp64, off by at most 2^-45 h
// from the exact quotient at 64 cells, so a point of a cell r + 1 away is further than r h (1 - 2^-45); d2 and the gap carry a few 2^-53.
#define FE_NN_BOUND_SLACK (1.0 - 2e-6)

// a uniform grid: cell (i, j, k) has linear index (i n[1] + j) n[2] + k; a masked axis and an axis without extent have n = 1
struct FeNnGrid { double lo[3]; double hi[3]; double h[3]; double h_min; int n[3]; int mask; };

__host__ __device__ inline bool fe_nn_finite(float v) { return v - v == 0.0f; }
// false: the point is neither a query nor a candidate (a non-finite word, or |x_a| > FE_CLOUD_COORD_MAX on an axis of the mask)
__host__ __device__ inline bool fe_nn_point_ok(const float* x, int mask) {
    if (!fe_nn_finite(x[0]) || !fe_nn_finite(x[1]) || !fe_nn_finite(x[2])) return false;
    for (int a = 0; a < 3; a++) {
        if (!((mask >> a) & 1)) continue;
        const double v = (double)x[a];
        if (!(v >= -FE_CLOUD_COORD_MAX && v <= FE_CLOUD_COORD_MAX)) return false;
    }
    return true;
}
// d2 = (d_x d_x + d_y d_y) + d_z d_z in fp64 from the fp32 words, in that order, no fused multiply-add; a masked axis contributes 0 * 0
__host__ __device__ inline double fe_nn_d2(const float* x, const float* t, int mask) {
#pragma clang fp contract(off)
    const double d0 = (mask & 1) ? (double)x[0] - (double)t[0] : 0.0;
    const double d1 = (mask & 2) ? (double)x[1] - (double)t[1] : 0.0;
    const double d2 = (mask & 4) ? (double)x[2] - (double)t[2] : 0.0;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}
// is (d2, id) nearer than (best, best_id)?  Ties go to the lower id.
__host__ __device__ inline bool fe_nn_better(double d2, int id, double best, int best_id) { return d2 < best || (d2 == best && id < best_id); }
// the COVER gradient's deposit of one point on one axis, and a word's value
__host__ __device__ inline long long fe_nn_quant(double d) { return (long long)llrint(d * FE_NN_FIX); }
__host__ __device__ inline double fe_nn_value(long long word) { return (double)word / FE_NN_FIX; }

// The grid over `count` points with bounding box [lo, hi] (fp32 words).  nn_cells = 0: cubical cells of an edge that leaves about
// FE_NN_PER_CELL points per cell of the box; nn_cells = k > 0: at most k cells along the longest axis (k = 1: one cell, brute force).  Never
// more than FE_NN_AXIS_CELLS cells along an axis.  The box is then divided evenly: h[a] = extent[a] / n[a].
__host__ __device__ inline void fe_nn_plan(const float* lo, const float* hi, int count, int mask, int nn_cells, FeNnGrid& g) {
    g.mask = mask; g.h_min = 1.0;
    for (int a = 0; a < 3; a++) { g.lo[a] = 0.0; g.hi[a] = 0.0; g.h[a] = 1.0; g.n[a] = 1; }
    if (count <= 0) return;
    double ext[3], longest = 0.0, vol = 1.0;
    int dims = 0;
    for (int a = 0; a < 3; a++) {
        g.lo[a] = (double)lo[a]; g.hi[a] = (double)hi[a];
        ext[a] = ((mask >> a) & 1) ? (double)hi[a] - (double)lo[a] : 0.0;
        if (!(ext[a] > 0.0)) { ext[a] = 0.0; continue; }
        dims++; vol *= ext[a];
        if (ext[a] > longest) longest = ext[a];
    }
    if (dims == 0) return;
    const int kmax = nn_cells > 0 ? (nn_cells < FE_NN_AXIS_CELLS ? nn_cells : FE_NN_AXIS_CELLS) : FE_NN_AXIS_CELLS;
    double edge = longest / (double)kmax;
    if (nn_cells <= 0) {
        const double cells = (double)(count / FE_NN_PER_CELL > 1 ? count / FE_NN_PER_CELL : 1);
        const double e = pow(vol / cells, 1.0 / (double)dims);
        if (e > edge) edge = e;
    }
    bool any = false;
    for (int a = 0; a < 3; a++) {
        if (ext[a] == 0.0) continue;
        const double c = ceil(ext[a] / edge);
        g.n[a] = c >= (double)kmax ? kmax : (c > 1.0 ? (int)c : 1);
        if (g.n[a] <= 1) { g.n[a] = 1; continue; }
        g.h[a] = ext[a] / (double)g.n[a];
        if (!any || g.h[a] < g.h_min) g.h_min = g.h[a];
        any = true;
    }
}
// the cell of coordinate x on axis a, clamped into the grid (a query may lie outside the box)
__host__ __device__ inline int fe_nn_cell_axis(const FeNnGrid& g, int a, float x) {
    if (g.n[a] <= 1) return 0;
    const double u = floor(((double)x - g.lo[a]) / g.h[a]);
    if (!(u > 0.0)) return 0;
    if (u >= (double)(g.n[a] - 1)) return g.n[a] - 1;
    return (int)u;
}
__host__ __device__ inline int fe_nn_cells(const FeNnGrid& g) { return g.n[0] * g.n[1] * g.n[2]; }
__host__ __device__ inline int fe_nn_cell_index(const FeNnGrid& g, int i, int j, int k) { return (i * g.n[1] + j) * g.n[2] + k; }
__host__ __device__ inline int fe_nn_cell_of(const FeNnGrid& g, const float* x) {
    return fe_nn_cell_index(g, fe_nn_cell_axis(g, 0, x[0]), fe_nn_cell_axis(g, 1, x[1]), fe_nn_cell_axis(g, 2, x[2]));
}
// the squared distance from x to the box of the set over the axes of the mask: 0 inside; every member is at least this far
__host__ __device__ inline double fe_nn_gap2(const FeNnGrid& g, const float* x) {
    double s = 0.0;
    for (int a = 0; a < 3; a++) {
        if (!((g.mask >> a) & 1)) continue;
        const double v = (double)x[a];
        const double d = v < g.lo[a] ? g.lo[a] - v : (v > g.hi[a] ? v - g.hi[a] : 0.0);
        s += d * d;
    }
    return s;
}
// After the rings 0 .. r around the (clamped) cell of a query, every point not yet seen has d2 > this: it differs by more than r cells on an
// axis with n > 1, so it is further than r h_min on that axis -- also from a query outside the box, which is at least as far from every
// unvisited cell as its clamped image; and on every axis on which the query lies outside the box, every member is at least the gap away,
// on top of the cells between them (gap2 = fe_nn_gap2: without it a query far from the set would walk the whole grid before
// best_d2 <= (r h_min)^2).  The search stops once best_d2 <= the bound.
__host__ __device__ inline double fe_nn_ring_bound(const FeNnGrid& g, int r, double gap2) {
    const double b = (double)r * g.h_min;
    return (b * b + gap2) * FE_NN_BOUND_SLACK;
}
// has ring r around cell q left the grid on every side (the rings 0 .. r hold every cell)?
__host__ __device__ inline bool fe_nn_ring_last(const FeNnGrid& g, const int* q, int r) {
    for (int a = 0; a < 3; a++) if (q[a] - r > 0 || q[a] + r < g.n[a] - 1) return false;
    return true;
}

// The search itself, over an index: start[c] .. start[c + 1] are the places in pts (x, y, z, id) of the members of cell c.
__host__ __device__ inline int fe_nn_id(const float4& p) { return __builtin_bit_cast(int, p.w); }
__host__ __device__ inline int fe_nn_imin(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int fe_nn_imax(int a, int b) { return a > b ? a : b; }
// the cells c0 .. c1 of one (i, j): a run of consecutive k, hence one contiguous run of pts
__host__ __device__ inline void fe_nn_run(const int* start, const float4* pts, int n_pts, const float* x, int mask, int c0, int c1, double& best, int& bid, float4& bp) {
    int p = start[c0];
    int e = start[c1 + 1];
    if (e > n_pts) e = n_pts;                               // (start[] never exceeds the members; kept as a bound on the reads)
    if (p < 0) p = e;
    for (; p < e; p++) {
        const float4 P = pts[p];
        const float t[3] = {P.x, P.y, P.z};
        const double d = fe_nn_d2(x, t, mask);
        const int id = fe_nn_id(P);
        if (fe_nn_better(d, id, best, bid)) { best = d; bid = id; bp = P; }
    }
}
// The nearest member to x: best (its d2), bid (its id; -1: the index is empty), bp (the member).  Returns the last ring searched.
__host__ __device__ inline int fe_nn_search(const FeNnGrid& g, const int* start, const float4* pts, int n_pts, const float* x, int mask, double& best, int& bid, float4& bp) {
    const int q[3] = {fe_nn_cell_axis(g, 0, x[0]), fe_nn_cell_axis(g, 1, x[1]), fe_nn_cell_axis(g, 2, x[2])};
    const double gap2 = fe_nn_gap2(g, x);
    best = __builtin_huge_val();
    bid = -1;
    bp = float4{0.f, 0.f, 0.f, 0.f};
    int r = 0;
    for (; r <= FE_NN_AXIS_CELLS; r++) {
        const int i0 = fe_nn_imax(q[0] - r, 0), i1 = fe_nn_imin(q[0] + r, g.n[0] - 1);
        const int j0 = fe_nn_imax(q[1] - r, 0), j1 = fe_nn_imin(q[1] + r, g.n[1] - 1);
        const int k0 = fe_nn_imax(q[2] - r, 0), k1 = fe_nn_imin(q[2] + r, g.n[2] - 1);
        for (int ci = i0; ci <= i1; ci++) {
            for (int cj = j0; cj <= j1; cj++) {
                const int row = fe_nn_cell_index(g, ci, cj, 0);
                if (ci - q[0] == r || q[0] - ci == r || cj - q[1] == r || q[1] - cj == r) fe_nn_run(start, pts, n_pts, x, mask, row + k0, row + k1, best, bid, bp);
                else {                                       // (r > 0 here) the two ends of the k range, where they are inside the grid
                    if (q[2] - r >= 0) fe_nn_run(start, pts, n_pts, x, mask, row + q[2] - r, row + q[2] - r, best, bid, bp);
                    if (q[2] + r <= g.n[2] - 1) fe_nn_run(start, pts, n_pts, x, mask, row + q[2] + r, row + q[2] + r, best, bid, bp);
                }
            }
        }
        if (best <= fe_nn_ring_bound(g, r, gap2) || fe_nn_ring_last(g, q, r)) break;
    }
    return r;
}

#ifndef FE_NEAREST_MATH_ONLY
#define FE_NN_WG 256
static_assert(FE_NN_WG == FE_TL_WG, "k_nn_sum sums its workgroup with fe_tl_wg_sum");
#define FE_NN_MAX_WGS 512
#define FE_NN_BOX_WORDS 8
// what k_task_bwd needs of the program's nearest terms, in term order: NEAREST -- the nearest cloud point of every particle (by pid) and the
// cloud in its own order; COVER -- the three fixed-point words of every particle (by pid)
struct TaskNearest { const int* nn[FE_TASK_LOSS_MAX_NEAREST_TERMS]; const float4* cloud[FE_TASK_LOSS_MAX_NEAREST_TERMS]; const long long* acc[FE_TASK_LOSS_MAX_NEAREST_TERMS]; };

// fp32 words in an order-preserving unsigned code (for integer atomicMax)
__device__ __forceinline__ unsigned fe_nn_enc(float v) { const unsigned b = __float_as_uint(v); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float fe_nn_dec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

// The candidates of frame f by slot: set[s] = (x, y, z, pid) of a particle that `sel` selects and fe_nn_point_ok passes, id -1 otherwise.
struct NnGatherArgs { int N; size_t Np; float* fr; const int* pid_of_slot; const float4* pinfo; FeLossSel sel; int mask; float4* set; };
template <int TAIL>
__global__ __launch_bounds__(FE_NN_WG) void k_nn_gather(NnGatherArgs a) {
    const int s = blockIdx.x * FE_NN_WG + threadIdx.x;
    if (s >= a.N) return;
    float4 out = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    const int pid = a.pid_of_slot[s];
    if ((unsigned)pid < (unsigned)a.N) {
        const FrameV fr = frame_view(a.fr, a.Np);
        if (fe_tl_selected(a.sel, pid, fe_tl_mat(a.pinfo, pid), fr.used[s])) {
            const float4 a0 = fr.A0[s];
            const float x[3] = {a0.x, a0.y, a0.z};
            if (fe_nn_point_ok(x, a.mask)) out = make_float4(a0.x, a0.y, a0.z, __int_as_float(pid));
        }
    }
    a.set[s] = out;
}

// box[a] = max of the code of -x_a, box[3 + a] = max of the code of x_a, box[6] = the number of members; box was zeroed on the stream
struct NnBoxArgs { const float4* set; int n; unsigned* box; };
template <int TAIL>
__global__ __launch_bounds__(FE_NN_WG) void k_nn_bbox(NnBoxArgs a) {
    unsigned m[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    int cnt = 0;
    for (int i = blockIdx.x * FE_NN_WG + threadIdx.x; i < a.n; i += gridDim.x * FE_NN_WG) {
        const float4 p = a.set[i];
        if (__float_as_int(p.w) < 0) continue;
        const float x[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int c = 0; c < 3; c++) { m[c] = max(m[c], fe_nn_enc(-x[c])); m[3 + c] = max(m[3 + c], fe_nn_enc(x[c])); }
        cnt++;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 6; c++) m[c] = max(m[c], (unsigned)__shfl_xor((int)m[c], o, 64));
        cnt += __shfl_xor(cnt, o, 64);
    }
    if ((threadIdx.x & 63) == 0 && cnt > 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) atomicMax(&a.box[c], m[c]);
        atomicAdd(&a.box[6], (unsigned)cnt);
    }
}

// one thread: the grid of the set from its box (fe_nn_plan)
struct NnPlanArgs { const unsigned* box; int mask, nn_cells; FeNnGrid* grid; };
template <int TAIL>
__global__ __launch_bounds__(64) void k_nn_plan(NnPlanArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int cnt = (int)a.box[6];
    float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
    if (cnt > 0) for (int c = 0; c < 3; c++) { lo[c] = -fe_nn_dec(a.box[c]); hi[c] = fe_nn_dec(a.box[3 + c]); }
    FeNnGrid g;
    fe_nn_plan(lo, hi, cnt, a.mask, a.nn_cells, g);
    *a.grid = g;
}

// FILL = false: count[cell] += 1 per member (count was zeroed on the stream).  FILL = true, behind k_nn_scan: every member takes one of its
// cell's places, pts[start[cell] + (what is left of count[cell]) - 1]: count[cell] members, count[cell] places.
struct NnCountArgs { const float4* set; int n; const FeNnGrid* grid; int* count; const int* start; float4* pts; };
template <bool FILL>
__global__ __launch_bounds__(FE_NN_WG) void k_nn_count(NnCountArgs a) {
    const int i = blockIdx.x * FE_NN_WG + threadIdx.x;
    if (i >= a.n) return;
    const float4 p = a.set[i];
    if (__float_as_int(p.w) < 0) return;
    const FeNnGrid g = *a.grid;
    const float x[3] = {p.x, p.y, p.z};
    const int c = fe_nn_cell_of(g, x);                      // (in [0, cells): every axis index is clamped)
    if (!FILL) { atomicAdd(&a.count[c], 1); return; }
    const int left = atomicSub(&a.count[c], 1);              // (in [1, the cell's count])
    const int at = a.start[c] + left - 1;
    if (left >= 1 && (unsigned)at < (unsigned)a.n) a.pts[at] = p;
}

// one workgroup: start[c] = the sum of count[0 .. c), start[cells] = the number of members
struct NnScanArgs { const FeNnGrid* grid; const int* count; int* start; };
template <int TAIL>
__global__ __launch_bounds__(FE_NN_WG) void k_nn_scan(NnScanArgs a) {
    __shared__ int wsum[FE_NN_WG / 64];
    if (blockIdx.x != 0) return;
    int cells = fe_nn_cells(*a.grid);
    if (cells > FE_NN_MAX_CELLS) cells = FE_NN_MAX_CELLS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < cells; base += FE_NN_WG) {
        const int c = base + threadIdx.x;
        const int v = c < cells ? a.count[c] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
        __syncthreads();
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < FE_NN_WG / 64; w++) { if (w < wave) before += wsum[w]; total += wsum[w]; }
        if (c < cells) a.start[c] = carry + before + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) a.start[cells] = carry;
}

// One thread per query: the nearest member of the index, ring by ring (fe_nn_search).  nn[id] / d2[id] (by the query's id; preset to -1 / 0 on the stream) get the answer.
// DEPOSIT (the COVER gradient): the query, a cloud point, adds llrint((x_pa - t_ja) 2^40) to the words acc[3 p + a] of its nearest particle p
// with 64-bit integer atomics, on the axes of the mask.
struct NnQueryArgs { const float4* query; int nq; const FeNnGrid* grid; const int* start; const float4* pts; int n_pts; int mask; int* nn; double* d2; unsigned long long* acc; };
template <bool DEPOSIT>
__global__ __launch_bounds__(FE_NN_WG) void k_nn_query(NnQueryArgs a) {
    const int i = blockIdx.x * FE_NN_WG + threadIdx.x;
    if (i >= a.nq) return;
    const float4 Q = a.query[i];
    const int qid = __float_as_int(Q.w);
    if (qid < 0) return;
    const FeNnGrid g = *a.grid;
    const float x[3] = {Q.x, Q.y, Q.z};
    double best;
    int bid;
    float4 bp;
    fe_nn_search(g, a.start, a.pts, a.n_pts, x, a.mask, best, bid, bp);
    if (bid < 0) return;                                      // (an empty index: nn stays -1, d2 stays 0)
    a.nn[qid] = bid;
    a.d2[qid] = best;
    if (DEPOSIT) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (!((a.mask >> c) & 1)) continue;
            const double d = (double)(c == 0 ? bp.x : (c == 1 ? bp.y : bp.z)) - (double)x[c];
            const long long w = fe_nn_quant(d);
            if (w != 0) atomicAdd(&a.acc[3 * (size_t)bid + c], (unsigned long long)w);
        }
    }
}

// partial[blockIdx.x] = the workgroup's sum of d2[i], i = blockIdx.x 256 + t, + gridDim.x 256 ...: chunked by query index, whatever the order
// of the frame; k_task_merge adds the partials in fixed order
struct NnSumArgs { const double* d2; int n; double* partial; };
template <int TAIL>
__global__ __launch_bounds__(FE_NN_WG) void k_nn_sum(NnSumArgs a) {
    __shared__ double lds[FE_NN_WG / 64];
    double acc = 0.0;
    for (int i = blockIdx.x * FE_NN_WG + threadIdx.x; i < a.n; i += gridDim.x * FE_NN_WG) acc += a.d2[i];
    const double v = fe_tl_wg_sum(acc, lds);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = v;
}

// ---------------------------------------------------------------------------------------------------------------- host
// An index over a set of points: the grid (on the device: k_nn_plan derives it from the set's box, so building waits for nothing), the cells'
// starts and the compact copy of the set.  built_cells: the "nn_cells" it was built with (-1: not built).
struct NnIndex { FeNnGrid* grid = nullptr; int* start = nullptr; float4* pts = nullptr; int n_pts = 0; int built_cells = -1; };
struct NnCloud { int n = 0; float4* pts = nullptr; NnIndex idx[8]; };       // the points in their own order (x, y, z, index); one index per axis mask, built on demand
#define FE_NN_SLOTS (FE_TASK_LOSS_MAX_NEAREST_TERMS + 1)    /* users of the result buffers: the program's nearest terms in term order, then fe_cloud_query */
struct NearestState {
    NnCloud cloud[FE_CLOUD_MAX];
    NnIndex pidx;                                           // the particles' index, rebuilt per call
    float4* pset = nullptr;                                 // [N] the candidates of a frame by slot (k_nn_gather)
    int* count = nullptr; unsigned* box = nullptr;          // [FE_NN_MAX_CELLS], [FE_NN_BOX_WORDS]: scratch of a build
    int* nn[FE_NN_SLOTS] = {}; double* d2[FE_NN_SLOTS] = {}; size_t cap[FE_NN_SLOTS] = {};      // results by query id, max(N, the cloud's points) each
    unsigned long long* acc[FE_NN_SLOTS] = {};              // [3 N] COVER's fixed-point words by pid
};
static void nn_index_free(NnIndex& ix) {
    for (void* q : {(void*)ix.grid, (void*)ix.start, (void*)ix.pts}) if (q) (void)hipFree(q);
    ix = NnIndex{};
}
static void nn_cloud_free(NnCloud& c) {
    if (c.pts) (void)hipFree(c.pts);
    for (NnIndex& ix : c.idx) nn_index_free(ix);
    c.pts = nullptr; c.n = 0;
}
static void nearest_drop(FeEngine* h) {                     // fe_destroy
    NearestState* st = h->nearest;
    if (!st) return;
    for (NnCloud& c : st->cloud) nn_cloud_free(c);
    nn_index_free(st->pidx);
    for (void* q : {(void*)st->pset, (void*)st->count, (void*)st->box}) if (q) (void)hipFree(q);
    for (int k = 0; k < FE_NN_SLOTS; k++) for (void* q : {(void*)st->nn[k], (void*)st->d2[k], (void*)st->acc[k]}) if (q) (void)hipFree(q);
    delete st;
    h->nearest = nullptr;
}
// (before the first fe_cloud_set there is no state, and no cloud is set)
static bool nearest_cloud_set(FeEngine* h, int cloud) { return h->nearest && h->nearest->cloud[cloud].n > 0; }
// room for an index over n_pts points
static int nn_index_alloc(FeEngine* h, NnIndex& ix, int n_pts) {
    if (ix.grid && ix.n_pts >= n_pts) return 0;
    HIPCK(h, hipStreamSynchronize(h->stream));               // (an earlier step may still read the old index)
    nn_index_free(ix);
    if (dev_alloc(h, &ix.grid, 1) || dev_alloc(h, &ix.start, (size_t)FE_NN_MAX_CELLS + 1) || dev_alloc(h, &ix.pts, (size_t)std::max(1, n_pts))) return 1;
    ix.n_pts = n_pts;
    return 0;
}
// the scratch every search shares, and the result buffers of user `slot` against cloud `cloud`
static int nearest_reserve(FeEngine* h, int slot, int cloud, bool with_acc) {
    if (!h->nearest) h->nearest = new NearestState();
    NearestState* st = h->nearest;
    if (!st->pset && dev_alloc(h, &st->pset, (size_t)h->N)) return 1;
    if (!st->count && dev_alloc(h, &st->count, (size_t)FE_NN_MAX_CELLS)) return 1;
    if (!st->box && dev_alloc(h, &st->box, (size_t)FE_NN_BOX_WORDS)) return 1;
    if (nn_index_alloc(h, st->pidx, h->N)) return 1;
    const size_t need = (size_t)std::max(std::max(h->N, st->cloud[cloud].n), 1);
    if (need > st->cap[slot]) {
        HIPCK(h, hipStreamSynchronize(h->stream));           // (an earlier step may still use the old buffers)
        if (st->nn[slot]) (void)hipFree(st->nn[slot]);
        if (st->d2[slot]) (void)hipFree(st->d2[slot]);
        st->nn[slot] = nullptr; st->d2[slot] = nullptr; st->cap[slot] = 0;
        if (dev_alloc(h, &st->nn[slot], need) || dev_alloc(h, &st->d2[slot], need)) return 1;
        st->cap[slot] = need;
    }
    if (with_acc && !st->acc[slot] && dev_alloc(h, &st->acc[slot], (size_t)3 * std::max(h->N, 1))) return 1;
    return 0;
}
// The three functions that launch the kernels above are defined in fe_engine.hip behind every extension header: template kernels sit in the code
// object in the order of their first use, and these are theirs.
//   nn_build:       index `ix` (room for n points) over the members of set[n]: box, grid, counts, scan, fill -- all enqueued
//   nearest_search: one direction of frame f against a cloud into the buffers of user `slot`: to_cloud -- every selected particle's nearest cloud point
//                   (nn, d2 by pid); else every cloud point's nearest selected particle (nn, d2 by cloud index; with deposit: the fixed-point words by pid)
//   nearest_sum:    np workgroup partials of the nq values of d2 that user `slot` holds
static void nn_build(FeEngine* h, NnIndex& ix, const float4* set, int n, int mask);
static void nearest_search(FeEngine* h, int f, int cloud, const FeLossSel& sel, int mask, bool to_cloud, int slot, bool deposit);
static void nearest_sum(FeEngine* h, int slot, int nq, double* partial, int np);
// the cloud's index for `mask`: built once, and again when "nn_cells" changed
static int nearest_cloud_index(FeEngine* h, int cloud, int mask) {
    NnCloud& C = h->nearest->cloud[cloud];
    NnIndex& ix = C.idx[mask & 7];
    if (nn_index_alloc(h, ix, C.n)) return 1;
    if (ix.built_cells != h->nn_cells) nn_build(h, ix, C.pts, C.n, mask);
    return 0;
}
static int nearest_queries(FeEngine* h, const FeLossTerm& T) { return T.kind == FE_TERM_NEAREST_SQ ? h->N : h->nearest->cloud[T.b.pid_lo].n; }
static int nearest_sum_wgs(int nq) { return std::max(1, std::min((nq + FE_NN_WG - 1) / FE_NN_WG, FE_NN_MAX_WGS)); }
static void nearest_eval(FeEngine* h, int f, const FeLossTerm& T, int slot, bool grad) {
    nearest_search(h, f, T.b.pid_lo, T.a, T.axis_mask, T.kind == FE_TERM_NEAREST_SQ, slot, grad && T.kind == FE_TERM_COVER_SQ);
}
static void nearest_task_view(FeEngine* h, const FeLossTerm& T, int slot, TaskNearest& TN) {
    NearestState* st = h->nearest;
    TN.nn[slot] = st->nn[slot]; TN.cloud[slot] = st->cloud[T.b.pid_lo].pts; TN.acc[slot] = (const long long*)st->acc[slot];
}
static bool task_loss_names_cloud(FeEngine* h, int cloud);  // (fe_task_loss.h, behind this header: a nearest term of the current program names the cloud)

extern "C" {

int fe_cloud_set(FeEngine* h, int cloud, const float* xyz, int n) {
    FE_ENTRY(h);
    if (cloud < 0 || cloud >= FE_CLOUD_MAX) FAIL(h, "fe_cloud_set: cloud id out of range (nothing is changed)");
    if (n < 0) FAIL(h, "fe_cloud_set: n must not be negative (the cloud is unchanged)");
    if (n > FE_CLOUD_MAX_POINTS) FAIL(h, "fe_cloud_set: more than FE_CLOUD_MAX_POINTS points (the cloud is unchanged)");
    if (n == 0 || !xyz) {                                     // removal
        if (task_loss_names_cloud(h, cloud)) FAIL(h, "fe_cloud_set: the current loss-term program names this cloud (the cloud is unchanged)");
        if (!h->nearest) return 0;
        HIPCK(h, hipStreamSynchronize(h->stream));
        nn_cloud_free(h->nearest->cloud[cloud]);
        return 0;
    }
    std::vector<float4> pts((size_t)n);
    for (int j = 0; j < n; j++) {
        if (!fe_nn_point_ok(xyz + 3 * (size_t)j, 7)) FAIL(h, "fe_cloud_set: a coordinate is not finite or beyond FE_CLOUD_COORD_MAX (the cloud is unchanged)");
        pts[(size_t)j] = make_float4(xyz[3 * (size_t)j], xyz[3 * (size_t)j + 1], xyz[3 * (size_t)j + 2], 0.f);
        std::memcpy(&pts[(size_t)j].w, &j, sizeof(int));
    }
    if (!h->nearest) h->nearest = new NearestState();
    float4* d_p = nullptr;                                    // (a buffer of its own, swapped in once it is complete)
    if (dev_alloc(h, &d_p, (size_t)n, false)) return 1;
    if (hipMemcpyOnStream(h, d_p, pts.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_p); FAIL(h, "fe_cloud_set: hipMemcpy failed (the cloud is unchanged)"); }
    NnCloud& C = h->nearest->cloud[cloud];                    // (the stream is drained: nothing reads the old points or their indices)
    nn_cloud_free(C);
    C.pts = d_p; C.n = n;
    return 0;
}
int fe_cloud_query(FeEngine* h, int f, int cloud, const FeLossSel* sel, int axis_mask, int* nn_of_particle, double* d2_of_particle, int* nn_of_point, double* d2_of_point) {
    FE_ENTRY(h);
    CHECK_FRAME(h, f);
    if (cloud < 0 || cloud >= FE_CLOUD_MAX) FAIL(h, "fe_cloud_query: cloud id out of range");
    if (!nearest_cloud_set(h, cloud)) FAIL(h, "fe_cloud_query: the cloud is not set: fe_cloud_set first");
    if ((axis_mask & 7) == 0 || (axis_mask & ~7) != 0) FAIL(h, "fe_cloud_query: axis_mask must name at least one of the axes x, y, z (bits 0..2)");
    const FeLossSel all = {0, h->N, -1, 1};
    const FeLossSel S = sel ? *sel : all;
    if (!tl_sel_ok(S, h->N)) FAIL(h, "fe_cloud_query: pid range of the selection outside [0, N]");
    const int slot = FE_TASK_LOSS_MAX_NEAREST_TERMS;
    if (nearest_reserve(h, slot, cloud, false)) return 1;
    NearestState* st = h->nearest;
    const int n = st->cloud[cloud].n;
    if (nn_of_particle || d2_of_particle) {
        if (nearest_cloud_index(h, cloud, axis_mask)) return 1;
        nearest_search(h, f, cloud, S, axis_mask, true, slot, false);
        if (nn_of_particle && h->N > 0) HIPCK(h, hipMemcpyAsync(nn_of_particle, st->nn[slot], sizeof(int) * (size_t)h->N, hipMemcpyDeviceToHost, h->stream));
        if (d2_of_particle && h->N > 0) HIPCK(h, hipMemcpyAsync(d2_of_particle, st->d2[slot], sizeof(double) * (size_t)h->N, hipMemcpyDeviceToHost, h->stream));
    }
    if (nn_of_point || d2_of_point) {
        nearest_search(h, f, cloud, S, axis_mask, false, slot, false);
        if (nn_of_point) HIPCK(h, hipMemcpyAsync(nn_of_point, st->nn[slot], sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        if (d2_of_point) HIPCK(h, hipMemcpyAsync(d2_of_point, st->d2[slot], sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    return check_device_errors(h);
}

}  // extern "C"
#endif /* FE_NEAREST_MATH_ONLY */
#endif /* FE_NEAREST_H */
