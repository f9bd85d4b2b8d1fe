// fe_contact.h -- contact wrenches: the linear and angular impulse every SDF collider's contact law gave to the material in a substep
// (include/fluidengine_ext.h: fe_contact_count, fe_contact_wrench).  Included by fe_engine.hip ahead of fe_render.h; its three kernels are
// template instantiations (<0>) for the reason given in fe_render_scene.h: they land at the tail of the code object and the 16 KB-aligned substep group
// keeps its addresses.
//
// A replay with bookkeeping, not an adjoint: the forward pass leaves in HBM the summed (p, m) and the v_out of every stored node of frame f
// (GridStore) and the contact flag of every particle (AgentP::hit).  k_contact_nodes walks the collider chain of node_velocity again, node by
// node, and k_contact_particles the chain of agent_collide_particle<false> on the re-gathered velocity, each noting per collider what the
// contact law changed.  Everything the contact law computes is the engine's fp32 with the engine's functions (static_collide's pieces,
// t_dynamic_collide), so that the replay takes the branches the forward pass took; fp64 is used for m dv, r x J and the sums only.
//
// The first part -- the running record, one collider's step at a particle or a node, the merge of partial records, the final record -- is
// plain __host__ __device__ code: tests/csrc/contact_test.cpp compiles it for the host with FE_CONTACT_MATH_ONLY defined and
// tests/test_contact_math.py holds it against the numpy restatement tests/contact_ref.py.
//
// All three kernels only READ the frame, the order table, the store and the effectors' poses.  No floating-point atomics.
#ifndef FE_CONTACT_H
#define FE_CONTACT_H

#ifndef FE_MAX_EFF
#define FE_MAX_EFF 4
#endif
#ifndef FE_MAX_STATICS
#define FE_MAX_STATICS 4
#endif
// a partial buffer holds one slot per possible collider: effector e in slot e, static s in slot FE_MAX_EFF + s
#define FE_CT_SLOTS (FE_MAX_EFF + FE_MAX_STATICS)
#define FE_CT_LANES 64

// The running record of one collider: sums, 8 eight-byte words.
struct FeContactAcc {
    double J[3], L[3];                       // sum m dv, sum r x m dv
    long long np, nn;                        // particle-level, node-level contacts
};
static_assert(sizeof(FeContactAcc) == 64, "FeContactAcc is 8 eight-byte words");

// A moving collider as the chain sees it in substep f: the mesh and the carrier's pose words at f and f + 1 (mesh == nullptr: no mesh).
struct FeContactDyn { const SdfP* mesh; const float *p0, *q0, *p1, *q1; };

__host__ __device__ inline void fe_ct_clear(FeContactAcc& a) {
    for (int d = 0; d < 3; d++) { a.J[d] = 0.0; a.L[d] = 0.0; }
    a.np = 0; a.nn = 0;
}
// a <- a + b, word by word
__host__ __device__ inline void fe_ct_merge(FeContactAcc& a, const FeContactAcc& b) {
    for (int d = 0; d < 3; d++) { a.J[d] += b.J[d]; a.L[d] += b.L[d]; }
    a.np += b.np; a.nn += b.nn;
}
// One contact: the collider turned vin into vout at the point r, on the mass m.  Differences, products and sums in fp64 from the fp32 words.
__host__ __device__ inline void fe_ct_contact(FeContactAcc& a, float m, const float r[3], const float vin[3], const float vout[3], bool node) {
#pragma clang fp contract(off)
    const double md = (double)m;
    const double J[3] = {md * ((double)vout[0] - (double)vin[0]), md * ((double)vout[1] - (double)vin[1]), md * ((double)vout[2] - (double)vin[2])};
    const double rd[3] = {(double)r[0], (double)r[1], (double)r[2]};
    a.J[0] += J[0]; a.J[1] += J[1]; a.J[2] += J[2];
    a.L[0] += rd[1] * J[2] - rd[2] * J[1];
    a.L[1] += rd[2] * J[0] - rd[0] * J[2];
    a.L[2] += rd[0] * J[1] - rd[1] * J[0];
    if (node) a.nn += 1; else a.np += 1;
}

// One link of the moving colliders' chain (agent_collide_particle<NODE>): nv is the velocity this collider sees and, on return, the one it
// leaves.  `one` receives the contact (it is NOT cleared: the caller's running record, or a cleared one).  Returns whether the collider
// took its contact branch.  NODE: x is the node position, which does not move with the velocity.
template <bool NODE>
__host__ __device__ inline bool fe_ct_dyn_step(const FeContactDyn& c, float collide_min_y, float dt, float m, const float x[3], float nv[3], FeContactAcc& one) {
    if (!c.mesh) return false;
    const float sdt = NODE ? 0.f : dt;
    const float pos[3] = {x[0] + sdt * nv[0], x[1] + sdt * nv[1], x[2] + sdt * nv[2]};
    if (!(pos[1] > collide_min_y)) return false;                                   // agent_icecreamdynamic.py:39-43
    float out[3];
    const bool hit = t_dynamic_collide<float>(*c.mesh, c.p0, c.q0, c.p1, c.q1, pos, nv, dt, out);
    if (hit) fe_ct_contact(one, m, pos, nv, out, NODE);
    nv[0] = out[0]; nv[1] = out[1]; nv[2] = out[2];
    return hit;
}
// One static at a node: static_collide (fe_math.h) with its pieces in its order, and the note of what it changed.
__host__ __device__ inline bool fe_ct_static_step(const SdfP& s, float m, const float xn[3], float v[3], FeContactAcc& one) {
    float pv[3];
    sdf_to_voxels(s, xn, pv);
    if (sdf_sample(s, pv) > 0.f) return false;
    float n[3], out[3];
    sdf_normal(s, pv, n);
    contact_law(n, s.friction, v, out, nullptr);
    fe_ct_contact(one, m, xn, v, out, true);
    for (int d = 0; d < 3; d++) v[d] = out[d];
    return true;
}
// A stored node's velocity in front of the colliders, and its position: the head of node_velocity, its contraction spelled out as there.
__host__ __device__ inline void fe_ct_node_start(const float p[3], float m, float dt, const float g[3], float dx, int i, int j, int k, float vo[3], float xn[3]) {
    const float inv = 1.f / m;
    vo[0] = fmaf(dt, g[0], inv * p[0]);
    vo[1] = fmaf(dt, g[1], inv * p[1]);
    vo[2] = fmaf(dt, g[2], inv * p[2]);
    xn[0] = (float)i * dx; xn[1] = (float)j * dx; xn[2] = (float)k * dx;
}
// The whole chain of one used particle, as the host sees it (the kernel runs the same steps with its lanes' records): acc[e] per effector.
__host__ __device__ inline void fe_ct_particle(const FeContactDyn* cols, int n_eff, float collide_min_y, float dt, float m, const float x[3], const float nv0[3], FeContactAcc* acc) {
    float nv[3] = {nv0[0], nv0[1], nv0[2]};
    for (int e = 0; e < n_eff; e++) fe_ct_dyn_step<false>(cols[e], collide_min_y, dt, m, x, nv, acc[e]);
}
// The whole chain of one stored node (p, m) = gi: statics in order into acc_st[s], then -- dyn: the engine collides at nodes -- the effectors
// into acc_eff[e].  A node without mass (m <= FE_EPS) has no velocity and meets no collider.
__host__ __device__ inline void fe_ct_node(const SdfP* statics, int n_st, const FeContactDyn* cols, int n_eff, bool dyn, float collide_min_y, float dt, const float g[3], float dx,
                                           const float p[3], float m, int i, int j, int k, FeContactAcc* acc_eff, FeContactAcc* acc_st) {
    if (!(m > FE_EPS)) return;
    float vo[3], xn[3];
    fe_ct_node_start(p, m, dt, g, dx, i, j, k, vo, xn);
    for (int s = 0; s < n_st; s++) fe_ct_static_step(statics[s], m, xn, vo, acc_st[s]);
    if (dyn) for (int e = 0; e < n_eff; e++) fe_ct_dyn_step<true>(cols[e], collide_min_y, dt, m, xn, vo, acc_eff[e]);
}

// The fixed-order merge of n partial records `stride` apart: lane l of 64 adds the partials l, l + 64, ... in order, then the 64 lane
// records are combined by the butterfly r[l] += r[l ^ o], o = 32 .. 1 (fe_task_loss.h; on the device: __shfl_xor).  Depends on n and the values only.
__host__ __device__ inline void fe_ct_lane_sum(const FeContactAcc* part, int n, size_t stride, int lane, FeContactAcc& a) {
    fe_ct_clear(a);
    for (int i = lane; i < n; i += FE_CT_LANES) fe_ct_merge(a, part[(size_t)i * stride]);
}
inline void fe_ct_merge_partials(const FeContactAcc* part, int n, size_t stride, FeContactAcc& out) {      // host form of k_contact_merge's sum
    FeContactAcc v[FE_CT_LANES], w[FE_CT_LANES];
    for (int l = 0; l < FE_CT_LANES; l++) fe_ct_lane_sum(part, n, stride, l, v[l]);
    for (int o = FE_CT_LANES / 2; o > 0; o >>= 1) {
        for (int l = 0; l < FE_CT_LANES; l++) { w[l] = v[l]; fe_ct_merge(w[l], v[l ^ o]); }
        for (int l = 0; l < FE_CT_LANES; l++) v[l] = w[l];
    }
    out = v[0];
}
// The record handed out.  valid == 0: the frame's grid is not in the store, everything but kind is zero.  ref: an effector's position words at f.
__host__ __device__ inline void fe_ct_finish(const FeContactAcc& a, int valid, int kind, const float* ref, FeContactRecord& o) {
    for (int d = 0; d < 3; d++) {
        o.impulse[d] = valid ? a.J[d] : 0.0;
        o.ang_impulse[d] = valid ? a.L[d] : 0.0;
        o.ref[d] = (valid && ref) ? (double)ref[d] : 0.0;
    }
    o.n_particles = valid ? a.np : 0; o.n_nodes = valid ? a.nn : 0;
    o.valid = valid ? 1 : 0; o.kind = kind;
}

#ifndef FE_CONTACT_MATH_ONLY
#define FE_CT_WG 256
#define FE_CT_MAX_WGS_P 1024
#define FE_CT_MAX_WGS_N 256

__device__ __forceinline__ void fe_ct_wave_reduce(FeContactAcc& r) {          // butterfly: every lane ends with the merge of all 64, in one fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        FeContactAcc b;
#pragma unroll
        for (int d = 0; d < 3; d++) { b.J[d] = __shfl_xor(r.J[d], o, 64); b.L[d] = __shfl_xor(r.L[d], o, 64); }
        b.np = __shfl_xor(r.np, o, 64); b.nn = __shfl_xor(r.nn, o, 64);
        fe_ct_merge(r, b);
    }
}
__device__ __forceinline__ FeContactDyn fe_ct_dyn_of(const AgentP& agent, int ei, int f) {
    const EffP& e = agent.e[ei];
    FeContactDyn c;
    c.mesh = e.has_mesh ? &e.mesh : nullptr;
    c.p0 = e.pos + f * 3; c.q0 = e.quat + f * 4; c.p1 = e.pos + (f + 1) * 3; c.q1 = e.quat + (f + 1) * 4;
    return c;
}
// vout_at on the frame's store, with the slot held against the store's capacity: this call may be asked about a frame long after the sweep that
// wrote it, and must stay inside the frame's record whatever the table says by then
__device__ __forceinline__ float4 fe_ct_vout(const SimP& S, const VoutSrc& V, int cap, int i, int j, int k) {
    const int slot = V.blk_slot[(((i >> 2) * S.nb) + (j >> 2)) * S.nb + (k >> 2)];
    return (slot >= 0 && slot < cap) ? store_vout(V.store, slot, ((i & 3) << 4) | ((j & 3) << 2) | (k & 3)) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// the waves of the workgroup take turns, in order, at adding their lanes' records to the workgroup's in LDS; then slot c goes to partial[c]
__device__ __forceinline__ void fe_ct_wg_flush(FeContactAcc* rec /* LDS [FE_CT_SLOTS], cleared */, const FeContactAcc& acc /* lane c: the wave's record of slot c */, FeContactAcc* __restrict__ partial) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();
    for (int w = 0; w < FE_CT_WG / 64; w++) {
        if (wave == w && lane < FE_CT_SLOTS) fe_ct_merge(rec[lane], acc);
        __syncthreads();
    }
    if (tid < FE_CT_SLOTS) partial[tid] = rec[tid];
}

// Particle part of substep f.  Workgroup w owns the slots [w span, (w + 1) span) of the frame, in slot order, 256 at a time: the lanes whose
// slot is used and flagged are compacted into an LDS list by ballot and prefix (no global list: the order does not depend on timing), then
// every listed particle is worked by a row of 16 lanes that splits the 27-node gather as collide_grad_row does; the chain runs in every lane
// of the row and lane 0 of the row keeps the contacts, one running record per effector.  One butterfly per record at the end.
template <int TAIL>
__global__ __launch_bounds__(FE_CT_WG) void k_contact_particles(SimP S, float* fr_, TableP T, const float4* __restrict__ pinfo, GridStore GS, int f, AgentP agent, int span,
                                                                FeContactAcc* __restrict__ partial /* [gridDim.x][FE_CT_SLOTS] */) {
    __shared__ FeContactAcc rec[FE_CT_SLOTS];
    __shared__ int list[FE_CT_WG];
    __shared__ int cnt[FE_CT_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = tid & 15, row = tid >> 4;
    if (tid < FE_CT_SLOTS) fe_ct_clear(rec[tid]);
    FeContactAcc mine[FE_MAX_EFF];                            // this lane's contacts per effector (registers: every index below is unrolled)
#pragma unroll
    for (int e = 0; e < FE_MAX_EFF; e++) fe_ct_clear(mine[e]);
    const bool stored = GS.cap > 0 && GS.flag[f] != 0;        // (uniform) without the frame's grid nothing is replayed: the records stay zero
    if (stored) {
        const FrameV fr = frame_view(fr_, S.Np);
        VoutSrc V; V.g_out = nullptr; V.store = GS.data + (size_t)f * GS.cap * GS_BLK; V.blk_slot = T.blk_slot;
        const int s0 = blockIdx.x * span, s1 = min(s0 + span, S.N);
        for (int base = s0; base < s1; base += FE_CT_WG) {    // (uniform)
            const int s = base + tid;
            const bool in = s < s1 && fr.used[s] != 0 && agent.hit[(size_t)f * S.Np + s] != 0;
            const unsigned long long b = __ballot(in);
            if (lane == 0) cnt[wave] = __popcll(b);
            __syncthreads();
            int off = 0, total = 0;
#pragma unroll
            for (int w = 0; w < FE_CT_WG / 64; w++) { const int c = cnt[w]; if (w < wave) off += c; total += c; }
            if (in) list[off + __popcll(b & ((1ull << lane) - 1ull))] = s;
            __syncthreads();
            for (int it = 0; it < total; it += FE_CT_WG / 16) {
                const int idx = it + row;
                if (idx < total) {                             // whole rows enter or skip together
                    const int sl = list[idx];
                    const float4 a0 = fr.A0[sl];
                    const float x[3] = {a0.x, a0.y, a0.z};
                    Stencil st;
                    stencil_make(x, S.inv_dx, st);
                    if (stencil_inside(st, S.n)) {             // (g2p passes a particle outside the grid through untouched)
                        float nv[3] = {0.f, 0.f, 0.f};
                        for (int n = sub; n < 27; n += 16) {
                            const int i = n / 9, j = (n / 3) % 3, k = n % 3;
                            const float weight = STW(st, i, 0) * STW(st, j, 1) * STW(st, k, 2);
                            const float4 gv = fe_ct_vout(S, V, GS.cap, st.base[0] + i, st.base[1] + j, st.base[2] + k);
                            nv[0] += weight * gv.x; nv[1] += weight * gv.y; nv[2] += weight * gv.z;
                        }
                        nv[0] = row_sum(nv[0]); nv[1] = row_sum(nv[1]); nv[2] = row_sum(nv[2]);
                        const int pid = T.pid_of_slot[sl];
                        const float m = S.uni ? S.uinfo[2] : pinfo[(unsigned)pid < (unsigned)S.N ? pid : 0].z;
#pragma unroll
                        for (int e = 0; e < FE_MAX_EFF; e++) {
                            if (e < agent.n) {
                                FeContactAcc one;
                                fe_ct_clear(one);
                                fe_ct_dyn_step<false>(fe_ct_dyn_of(agent, e, f), agent.collide_min_y, S.dt, m, x, nv, one);
                                if (sub == 0) fe_ct_merge(mine[e], one);
                            }
                        }
                    }
                }
            }
            __syncthreads();                                   // (the list is rewritten by the next round)
        }
    }
    FeContactAcc acc;                                         // lane e: the wave's record of effector e
    fe_ct_clear(acc);
#pragma unroll
    for (int e = 0; e < FE_MAX_EFF; e++) {
        fe_ct_wave_reduce(mine[e]);
        if (lane == e) acc = mine[e];
    }
    fe_ct_wg_flush(rec, acc, partial + (size_t)blockIdx.x * FE_CT_SLOTS);
}

// Node part of substep f.  One wave per entry e < meta[2] of the frame's active list that the store holds, one lane per node; entries k_grid
// did not work on in this frame (live == 0) hold nothing of it and are skipped.  A lane walks node_velocity's chain for its node; where any
// lane of the wave met a collider the wave reduces that collider's contacts at once and lane `slot` keeps the wave's running record (most
// blocks meet none, and a lane holding all eight records would need 128 registers beside the ~100 of the SDF code).
template <int TAIL>
__global__ __launch_bounds__(FE_CT_WG) void k_contact_nodes(SimP S, TableP T, GridStore GS, int f, StaticsP ST, AgentP agent, int dyn,
                                                            FeContactAcc* __restrict__ partial /* [gridDim.x][FE_CT_SLOTS] */) {
    __shared__ FeContactAcc rec[FE_CT_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < FE_CT_SLOTS) fe_ct_clear(rec[tid]);
    FeContactAcc acc;                                         // lane c: the wave's record of slot c
    fe_ct_clear(acc);
    const bool stored = GS.cap > 0 && GS.flag[f] != 0;        // (uniform)
    if (stored) {
        const int n_ent = min(T.meta[2], GS.cap), nw = (int)gridDim.x * (FE_CT_WG / 64);
        const float4* __restrict__ st = GS.data + (size_t)f * GS.cap * GS_BLK;
        const unsigned char* __restrict__ live = GS.live + (size_t)f * GS.cap;
        for (int e = blockIdx.x * (FE_CT_WG / 64) + wave; e < n_ent; e += nw) {      // (uniform)
            if (live[e] == 0) continue;
            const int b = __builtin_amdgcn_readfirstlane(T.active[e]);
            const float4 gi = st[(size_t)e * GS_BLK + lane];
            const bool has = gi.w > FE_EPS;
            const int bi = b / (S.nb * S.nb), bj = (b / S.nb) % S.nb, bk = b % S.nb;
            const float p[3] = {gi.x, gi.y, gi.z};
            float vo[3] = {0.f, 0.f, 0.f}, xn[3] = {0.f, 0.f, 0.f};
            if (has) fe_ct_node_start(p, gi.w, S.dt, S.g, S.dx, bi * 4 + (lane >> 4), bj * 4 + ((lane >> 2) & 3), bk * 4 + (lane & 3), vo, xn);
#pragma unroll
            for (int si = 0; si < FE_MAX_STATICS; si++) {
                if (si < ST.n) {
                    FeContactAcc one;
                    fe_ct_clear(one);
                    const bool hit = has && fe_ct_static_step(ST.s[si], gi.w, xn, vo, one);
                    if (__any(hit)) {                          // (uniform)
                        fe_ct_wave_reduce(one);
                        if (lane == FE_MAX_EFF + si) fe_ct_merge(acc, one);
                    }
                }
            }
            if (dyn) {
#pragma unroll
                for (int ei = 0; ei < FE_MAX_EFF; ei++) {
                    if (ei < agent.n) {
                        FeContactAcc one;
                        fe_ct_clear(one);
                        const bool hit = has && fe_ct_dyn_step<true>(fe_ct_dyn_of(agent, ei, f), agent.collide_min_y, S.dt, gi.w, xn, vo, one);
                        if (__any(hit)) {
                            fe_ct_wave_reduce(one);
                            if (lane == ei) fe_ct_merge(acc, one);
                        }
                    }
                }
            }
        }
    }
    fe_ct_wg_flush(rec, acc, partial + (size_t)blockIdx.x * FE_CT_SLOTS);
}

// One wave: per collider, lane l adds the workgroups' partial records l, l + 64, ... in index order (the particle kernel's first, then the
// node kernel's), the butterfly, and lane 0 writes the substep's record.  flag == nullptr: the engine keeps no store.
template <int TAIL>
__global__ __launch_bounds__(FE_CT_LANES) void k_contact_merge(const FeContactAcc* __restrict__ partial, int n_partial, int n_eff, int n_st, const int* __restrict__ flag, int f,
                                                               const EffP* __restrict__ effs, FeContactRecord* __restrict__ out /* [n_eff + n_st] of this substep */) {
    const int lane = threadIdx.x;
    const int valid = (flag != nullptr && flag[f] != 0) ? 1 : 0;
    for (int c = 0; c < n_eff + n_st; c++) {
        const int slot = c < n_eff ? c : FE_MAX_EFF + (c - n_eff);
        FeContactAcc a;
        fe_ct_lane_sum(partial + slot, valid ? n_partial : 0, (size_t)FE_CT_SLOTS, lane, a);
        fe_ct_wave_reduce(a);
        if (lane == 0) fe_ct_finish(a, valid, c < n_eff ? 0 : 1, c < n_eff ? effs[c].pos + f * 3 : nullptr, out[c]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct ContactState {
    FeContactAcc* partial = nullptr;                          // [(FE_CT_MAX_WGS_P + FE_CT_MAX_WGS_N) * FE_CT_SLOTS]: the workgroups' records of one substep
    FeContactRecord* out = nullptr; size_t out_cap = 0;       // [n * (n_eff + n_static)] of the last call (grown on demand)
};
static void contact_drop(FeEngine* h) {                       // fe_destroy
    ContactState* Q = h->contact;
    if (!Q) return;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (Q->partial) (void)hipFree(Q->partial);
    if (Q->out) (void)hipFree(Q->out);
    delete Q;
    h->contact = nullptr;
}

extern "C" {

int fe_contact_count(FeEngine* h) { return h ? (int)h->effs.size() + (int)h->statics_host.size() : 0; }

// Read-only: no member of the engine but the buffers above changes (not even the host copy of the store flags: the kernels read the flag).
int fe_contact_wrench(FeEngine* h, int f0, int n, FeContactRecord* out, int n_records, int record_size) {
    if (!h) return 1;                                         // (no engine to keep a message: fe_last_error(NULL) speaks of fe_create)
    FE_ENTRY(h);
    if (record_size != (int)sizeof(FeContactRecord)) FAIL(h, "fe_contact_wrench: record_size is not sizeof(FeContactRecord)");
    if (f0 < 0 || n < 1 || (long long)f0 + n > (long long)h->L) FAIL(h, "fe_contact_wrench: substeps f0 .. f0 + n - 1 must lie in [0, max_substeps_local)");
    if (n_records < 1) FAIL(h, "fe_contact_wrench: n_records < 1");
    if (!out) FAIL(h, "fe_contact_wrench: out is NULL");
    const int n_eff = (int)h->effs.size(), n_st = (int)h->statics_host.size(), n_rec = n_eff + n_st;
    if (n_eff > FE_MAX_EFF || n_st > FE_MAX_STATICS) FAIL(h, "fe_contact_wrench: more colliders than FE_MAX_EFF effectors + FE_MAX_STATICS statics");
    if (n_rec == 0) {                                         // nothing to write; the call still waits for the stream, as it always does
        HIPCK(h, hipStreamSynchronize(h->stream));
        if (check_async(h)) return 1;
        return check_device_errors(h);
    }
    const int n_out = n_records < n_rec ? n_records : n_rec;
    ContactState* Q = h->contact;
    if (!Q) Q = h->contact = new ContactState();
    if (!Q->partial && dev_alloc(h, &Q->partial, (size_t)(FE_CT_MAX_WGS_P + FE_CT_MAX_WGS_N) * FE_CT_SLOTS)) return 1;
    if (Q->out_cap < (size_t)n * n_rec) {
        HIPCK(h, hipStreamSynchronize(h->stream));
        if (Q->out) (void)hipFree(Q->out);
        Q->out = nullptr; Q->out_cap = 0;
        if (dev_alloc(h, &Q->out, (size_t)n * n_rec)) return 1;
        Q->out_cap = (size_t)n * n_rec;
    }
    const bool have_store = h->gs_cap > 0;
    const bool part = have_store && particle_collide(h) && h->hit_dev != nullptr;
    const bool nodes = have_store && (n_st > 0 || grid_collide(h));
    // a workgroup of the particle kernel owns `span` slots (a multiple of 256); the node kernel's waves stride over the entries
    int wgs_p = 0, span = FE_CT_WG;
    if (part) {
        wgs_p = (h->N + FE_CT_WG - 1) / FE_CT_WG;
        if (wgs_p > FE_CT_MAX_WGS_P) wgs_p = FE_CT_MAX_WGS_P;
        if (wgs_p < 1) wgs_p = 1;
        span = (((h->N + wgs_p - 1) / wgs_p + FE_CT_WG - 1) / FE_CT_WG) * FE_CT_WG;
        if (span < FE_CT_WG) span = FE_CT_WG;
    }
    int wgs_n = 0;
    if (nodes) {
        wgs_n = (h->nb * h->nb * h->nb + 3) / 4;
        if (wgs_n > FE_CT_MAX_WGS_N) wgs_n = FE_CT_MAX_WGS_N;
    }
    const AgentP ag = agent_params(h);
    const GridStore GS = grid_store(h);
    for (int f = f0; f < f0 + n; f++) {
        const TableP T = h->tableP(h->tbl_of_frame[f]);
        if (wgs_p > 0)
            hipLaunchKernelGGL(k_contact_particles<0>, dim3(wgs_p), dim3(FE_CT_WG), 0, h->stream, h->S, h->frame(f), T, (const float4*)h->pinfo, GS, f, ag, span, Q->partial);
        if (wgs_n > 0)
            hipLaunchKernelGGL(k_contact_nodes<0>, dim3(wgs_n), dim3(FE_CT_WG), 0, h->stream, h->S, T, GS, f, statics_p(h), ag, grid_collide(h) ? 1 : 0,
                               Q->partial + (size_t)wgs_p * FE_CT_SLOTS);
        hipLaunchKernelGGL(k_contact_merge<0>, dim3(1), dim3(FE_CT_LANES), 0, h->stream, (const FeContactAcc*)Q->partial, wgs_p + wgs_n, n_eff, n_st,
                           (const int*)(have_store ? h->gs_flag : nullptr), f, (const EffP*)h->effs_dev, Q->out + (size_t)(f - f0) * n_rec);
    }
    // one copy: n rows of n_out records, n_records apart at the caller's
    HIPCK(h, hipMemcpy2DAsync(out, sizeof(FeContactRecord) * (size_t)n_records, Q->out, sizeof(FeContactRecord) * (size_t)n_rec, sizeof(FeContactRecord) * (size_t)n_out, (size_t)n,
                              hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (check_async(h)) return 1;
    return check_device_errors(h);
}

}  // extern "C"
#endif /* FE_CONTACT_MATH_ONLY */
#endif /* FE_CONTACT_H */
