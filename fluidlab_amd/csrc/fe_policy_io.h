// fe_policy_io.h -- what a closed-loop policy a_i = pi(o_i) needs from the engine besides the rollout itself (include/fluidengine_ext.h:
// fe_obs_add_grad*, fe_eff_add_state_grad*, fe_eff_get_state_grad, fe_eff_get_state_dev, fe_eff_set_action_dev, fe_eff_get_action_grad_dev):
// the cotangent of an observation goes back into the adjoint of the frame it was read from -- n rows, not two dense [N, 3] arrays -- and the
// three per-step crossings (pose out, action in, action adjoint out) have device-pointer forms.
// Included by fe_engine.hip behind fe_contact.h; its kernels are template instantiations (<0>) for the reason given in fe_render_scene.h: they
// land at the tail of the code object and the 16 KB-aligned substep group keeps its addresses.
//
// Nothing here is launched unless one of these entries is called.  No floating-point atomics, plain vector stores only.
#ifndef FE_POLICY_IO_H
#define FE_POLICY_IO_H

// ---- observation scatter: the mirror image of k_obs_gather for adjoint slots -----------------------------------------------
// The list may name a particle several times.  The rows are grouped once per list (policy_io_group): rows[] holds the row indices sorted by
// particle id, rows of one particle in list order; seg[k] .. seg[k + 1] are the rows of the k-th distinct particle.  One thread owns one
// distinct particle: it sums that particle's rows in list order in fp32, starting from 0, and adds the sum to the slot once -- the result does
// not depend on the launch geometry.  The slot comes from the slot_of_pid of the ADJOINT slot's own order (adj_slot), which
// across a sort boundary is not the frame's.  Only the x and v words are written; C's two words that share a float4 with v are stored back
// as read (the thread is the only writer of its slot), F's planes are not touched: a compact F adjoint stays compact.
// (The arguments of each kernel travel as one struct and no kernel reads blockDim / gridDim: a kernel's metadata note grows with every
// argument, hidden ones included, and the notes sit in front of the code -- the aligned substep kernels start one 16 KB notch later once the
// sections ahead of .text cross a page.)
struct ObsScatterArgs { int n_seg, N; unsigned Np; float* gr; const int *slot_of_pid, *pids, *rows, *seg; const float *gx, *gv; };
template <int TAIL>
__global__ __launch_bounds__(256) void k_obs_scatter_grad(ObsScatterArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n_seg) return;
    const int lo = a.seg[k], hi = a.seg[k + 1];
    if (hi <= lo) return;
    const int pid = a.pids[a.rows[lo]];
    if ((unsigned)pid >= (unsigned)a.N) return;               // (checked on the host when the list was set)
    const int s = a.slot_of_pid[pid];
    if ((unsigned)s >= a.Np) return;
    const float *gx = a.gx, *gv = a.gv;
    float sx[3] = {0.f, 0.f, 0.f}, sv[3] = {0.f, 0.f, 0.f};
    for (int j = lo; j < hi; j++) {
        const size_t r = 3 * (size_t)a.rows[j];
        if (gx) { sx[0] += gx[r]; sx[1] += gx[r + 1]; sx[2] += gx[r + 2]; }
        if (gv) { sv[0] += gv[r]; sv[1] += gv[r + 1]; sv[2] += gv[r + 2]; }
    }
    const FrameV g = frame_view(a.gr, a.Np);
    float4 a0 = g.A0[s];
    if (gx) { a0.x += sx[0]; a0.y += sx[1]; a0.z += sx[2]; }
    if (gv) {
        float4 a1 = g.A1[s];
        a0.w += sv[0]; a1.x += sv[1]; a1.y += sv[2];
        g.A1[s] = a1;
    }
    g.A0[s] = a0;
}

// gpos[f] += g7[0..3), gquat[f] += g7[3..7): seven lanes, one word each
struct EffStateGradArgs { float *gpos, *gquat; const float* g7; int f; };
template <int TAIL>
__global__ __launch_bounds__(64) void k_eff_add_state_grad(EffStateGradArgs a) {
    const int i = threadIdx.x;
    if (blockIdx.x != 0 || i >= 7) return;
    if (i < 3) a.gpos[(size_t)a.f * 3 + i] += a.g7[i];
    else a.gquat[(size_t)a.f * 4 + (i - 3)] += a.g7[i];
}

// gsa[f] += gs, gra[f] += gr: two lanes, one word each (an AirCon's strength and radius: what the pose adjoint above lacks for it)
struct EffSrGradArgs { float *gsa, *gra; float gs, gr; int f; };
template <int TAIL>
__global__ __launch_bounds__(64) void k_eff_add_sr_grad(EffSrGradArgs a) {
    const int i = threadIdx.x;
    if (blockIdx.x != 0 || i >= 2) return;
    if (i == 0) a.gsa[a.f] += a.gs;
    else a.gra[a.f] += a.gr;
}

// k_eff_set_action with the action read from device memory: the same body (eff_set_action_body), so the same abuf, v, w, sa, ra
struct EffActionDevArgs { EffP e; const float* action; int s, s_global, n_substeps; };
template <int TAIL>
__global__ __launch_bounds__(64) void k_eff_set_action_dev(EffActionDevArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    Act6 act;
    for (int j = 0; j < 8; j++) act.a[j] = j < a.e.action_dim ? a.action[j] : 0.f;
    eff_set_action_body(a.e, a.s, a.s_global, a.n_substeps, act);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct PolicyIOState {
    std::vector<int> pids;                                    // the observation list as given (host copy), for the grouping
    bool grouped = false;                                     // rows / seg below belong to the current list
    int n_seg = 0;
    int *rows = nullptr, *seg = nullptr;                      // [n], [n_seg + 1] on the device
    float *gx = nullptr, *gv = nullptr;                       // staging of the host variant of fe_obs_add_grad: [3 n] each
    float* g7 = nullptr;                                      // staging of the host variant of fe_eff_add_state_grad: [8]
};

namespace {

void policy_io_free_list(PolicyIOState* Q) {
    for (void* q : {(void*)Q->rows, (void*)Q->seg, (void*)Q->gx, (void*)Q->gv}) if (q) (void)hipFree(q);
    Q->rows = Q->seg = nullptr; Q->gx = Q->gv = nullptr; Q->grouped = false; Q->n_seg = 0;
}
// fe_destroy
void policy_io_drop(FeEngine* h) {
    PolicyIOState* Q = h->policy_io;
    if (!Q) return;
    policy_io_free_list(Q);
    if (Q->g7) (void)hipFree(Q->g7);
    delete Q;
    h->policy_io = nullptr;
}
// fe_obs_set_particles, after the stream has drained: the grouping of the old list goes, the new one is built at its first use
void policy_io_set_list(FeEngine* h, const int* pids, int n) {
    if (!h->policy_io) {
        if (n == 0) return;
        h->policy_io = new PolicyIOState();
    }
    PolicyIOState* Q = h->policy_io;
    policy_io_free_list(Q);
    Q->pids.assign(pids, pids + (n > 0 ? n : 0));
}
// rows sorted by particle id (stable: list order within a particle) and the segment starts -- once per list
int policy_io_group(FeEngine* h) {
    PolicyIOState* Q = h->policy_io;
    if (Q->grouped) return 0;
    const int n = (int)Q->pids.size();
    std::vector<int> rows, seg;
    fe_group_rows(Q->pids.data(), n, rows, seg);              // (fe_smoke_reads.h: shared with the smoke cell lists' scatter)
    const int n_seg = (int)seg.size() - 1;
    if (dev_alloc(h, &Q->rows, (size_t)n, false) || dev_alloc(h, &Q->seg, (size_t)n_seg + 1, false) ||
        dev_alloc(h, &Q->gx, (size_t)3 * n) || dev_alloc(h, &Q->gv, (size_t)3 * n)) { policy_io_free_list(Q); return 1; }
    if (hipMemcpyOnStream(h, Q->rows, rows.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpyOnStream(h, Q->seg, seg.data(), sizeof(int) * ((size_t)n_seg + 1), hipMemcpyHostToDevice) != hipSuccess) {
        policy_io_free_list(Q);
        FAIL(h, "fe_obs_add_grad: hipMemcpy failed");
    }
    Q->n_seg = n_seg; Q->grouped = true;
    return 0;
}
// the refusals shared by the two variants: nothing has changed when one of them returns
int policy_io_obs_check(FeEngine* h, int f) {
    CHECK_FRAME(h, f);
    const SummaryState* O = h->summary;                       // (fe_summary.h keeps the list)
    if (!O || !O->obs_pids || !h->policy_io || O->obs_n <= 0) FAIL(h, "no observation list: fe_obs_set_particles first");
    return adj_slot(h, f, ADJ_READ);                          // (the refusal alone: the slot takes its order in policy_io_obs_scatter, once there is something to add)
}
// gx, gv: device pointers (or nullptr)
int policy_io_obs_scatter(FeEngine* h, int f, const float* gx, const float* gv) {
    if (policy_io_group(h)) return 1;
    PolicyIOState* Q = h->policy_io;
    AdjSlot g; if (adj_slot(h, f, ADJ_ADD, &g)) return 1;                // (a cleared slot takes the frame's order; F's planes and gcompact stay as they are)
    const ObsScatterArgs a = {Q->n_seg, h->N, (unsigned)h->Np, g.planes, g.slot_of_pid, h->summary->obs_pids, Q->rows, Q->seg, gx, gv};
    hipLaunchKernelGGL(k_obs_scatter_grad<0>, dim3((Q->n_seg + 255) / 256), dim3(256), 0, h->stream, a);
    HIPCK(h, hipStreamSynchronize(h->stream));
    return check_async(h);
}
int policy_io_eff_check(FeEngine* h, int e, int f) {
    CHECK_EFF(h, e); CHECK_FRAME(h, f);
    return 0;
}
int policy_io_eff_add(FeEngine* h, int e, int f, const float* g7_dev) {
    EffP& p = h->effs[e].p;
    const EffStateGradArgs a = {p.gpos, p.gquat, g7_dev, f};
    hipLaunchKernelGGL(k_eff_add_state_grad<0>, dim3(1), dim3(64), 0, h->stream, a);
    HIPCK(h, hipStreamSynchronize(h->stream));
    return check_async(h);
}

} // namespace

extern "C" {

// x.grad[f][pids[i]] += gx[i], v.grad[f][pids[i]] += gv[i] for the rows of the observation list (host pointers; staged, waits)
int fe_obs_add_grad(FeEngine* h, int f, const fe_real* gx, const fe_real* gv) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (policy_io_obs_check(h, f)) return 1;
    if (!gx && !gv) return 0;
    if (policy_io_group(h)) return 1;
    PolicyIOState* Q = h->policy_io;
    const size_t n = (size_t)h->summary->obs_n;
    if (gx) HIPCK(h, hipMemcpyAsync(Q->gx, gx, sizeof(float) * 3 * n, hipMemcpyHostToDevice, h->stream));
    if (gv) HIPCK(h, hipMemcpyAsync(Q->gv, gv, sizeof(float) * 3 * n, hipMemcpyHostToDevice, h->stream));
    return policy_io_obs_scatter(h, f, gx ? Q->gx : nullptr, gv ? Q->gv : nullptr);
}
// the same from device pointers
int fe_obs_add_grad_dev(FeEngine* h, int f, const fe_real* gx, const fe_real* gv) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (policy_io_obs_check(h, f)) return 1;
    if (!gx && !gv) return 0;
    return policy_io_obs_scatter(h, f, gx, gv);
}

// gpos[f] += g7[0..3), gquat[f] += g7[3..7) of effector e
int fe_eff_add_state_grad(FeEngine* h, int e, int f, const fe_real* g7) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (policy_io_eff_check(h, e, f)) return 1;
    if (!g7) FAIL(h, "fe_eff_add_state_grad: g7 is NULL");
    if (!h->policy_io) h->policy_io = new PolicyIOState();
    PolicyIOState* Q = h->policy_io;
    if (!Q->g7 && dev_alloc(h, &Q->g7, 8)) return 1;
    HIPCK(h, hipMemcpyAsync(Q->g7, g7, sizeof(float) * 7, hipMemcpyHostToDevice, h->stream));
    return policy_io_eff_add(h, e, f, Q->g7);
}
int fe_eff_add_state_grad_dev(FeEngine* h, int e, int f, const fe_real* g7) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (policy_io_eff_check(h, e, f)) return 1;
    if (!g7) FAIL(h, "fe_eff_add_state_grad_dev: g7 is NULL");
    return policy_io_eff_add(h, e, f, g7);
}
int fe_eff_get_state_grad(FeEngine* h, int e, int f, fe_real* g7) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (policy_io_eff_check(h, e, f)) return 1;
    if (!g7) FAIL(h, "fe_eff_get_state_grad: g7 is NULL");
    const EffP& p = h->effs[e].p;
    HIPCK(h, hipMemcpyAsync(g7, p.gpos + (size_t)f * 3, sizeof(float) * 3, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(g7 + 3, p.gquat + (size_t)f * 4, sizeof(float) * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// gsa[f] += gs, gra[f] += gr of AirCon e: from there the effector move's adjoint carries them into gabuf (entries 6 and 7)
int fe_eff_add_sr_grad(FeEngine* h, int e, int f, fe_real gs, fe_real gr) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (policy_io_eff_check(h, e, f)) return 1;
    EffP& p = h->effs[e].p;
    if (p.type != FE_EFF_AIRCON) FAIL(h, "fe_eff_add_sr_grad: the effector is not an AirCon (nothing has changed)");
    const EffSrGradArgs a = {p.gsa, p.gra, gs, gr, f};
    hipLaunchKernelGGL(k_eff_add_sr_grad<0>, dim3(1), dim3(64), 0, h->stream, a);
    HIPCK(h, hipStreamSynchronize(h->stream));
    return check_async(h);
}
int fe_eff_get_sr_grad(FeEngine* h, int e, int f, fe_real* gs, fe_real* gr) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (policy_io_eff_check(h, e, f)) return 1;
    const EffP& p = h->effs[e].p;
    if (p.type != FE_EFF_AIRCON) FAIL(h, "fe_eff_get_sr_grad: the effector is not an AirCon");
    if (!gs || !gr) FAIL(h, "fe_eff_get_sr_grad: gs or gr is NULL");
    HIPCK(h, hipMemcpyAsync(gs, p.gsa + f, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(gr, p.gra + f, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// pos[f], quat[f] of effector e into 7 device floats
int fe_eff_get_state_dev(FeEngine* h, int e, int f, fe_real* s7) {
    if (!h) return 1;
    FE_ENTRY(h);
    if (policy_io_eff_check(h, e, f)) return 1;
    if (!s7) FAIL(h, "fe_eff_get_state_dev: s7 is NULL");
    const EffP& p = h->effs[e].p;
    HIPCK(h, hipMemcpyAsync(s7, p.pos + (size_t)f * 3, sizeof(float) * 3, hipMemcpyDeviceToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(s7 + 3, p.quat + (size_t)f * 4, sizeof(float) * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return 0;
}
// fe_eff_set_action with the action_dim action words in device memory
int fe_eff_set_action_dev(FeEngine* h, int e, int s, int s_global, int n_substeps, const fe_real* action) {
    if (!h) return 1;
    FE_ENTRY(h);
    CHECK_EFF(h, e);
    EffP& p = h->effs[e].p;
    if (p.action_dim == 0) return 0;
    if (!action) FAIL(h, "fe_eff_set_action_dev: action is NULL");
    if (s_global < 0 || s_global >= h->cfg.max_action_steps) FAIL(h, "s_global out of range");
    if (n_substeps < 1 || s < 0 || (s + 1) * n_substeps > h->L + 1) FAIL(h, "s out of range");
    EffActionDevArgs a; a.e = p; a.action = action; a.s = s; a.s_global = s_global; a.n_substeps = n_substeps;
    hipLaunchKernelGGL(k_eff_set_action_dev<0>, dim3(1), dim3(64), 0, h->stream, a);
    HIPCK(h, hipStreamSynchronize(h->stream));               // (the caller may overwrite `action` once this returns)
    return check_async(h);
}
// gabuf[s .. s + n) of effector e (n * action_dim words) to a device pointer
int fe_eff_get_action_grad_dev(FeEngine* h, int e, int s, int n, fe_real* grad) {
    if (!h) return 1;
    FE_ENTRY(h);
    CHECK_EFF(h, e);
    const EffP& p = h->effs[e].p;
    const int ad = p.action_dim;
    if (ad == 0 || n == 0) return 0;
    if (!grad) FAIL(h, "fe_eff_get_action_grad_dev: grad is NULL");
    if (s < 0 || n < 0 || (long long)s + n > (long long)h->cfg.max_action_steps) FAIL(h, "action grad range out of bounds");
    HIPCK(h, hipMemcpyAsync(grad, p.gabuf + (size_t)s * ad, sizeof(float) * (size_t)n * ad, hipMemcpyDeviceToDevice, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
#endif /* FE_POLICY_IO_H */
