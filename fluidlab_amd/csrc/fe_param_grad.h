// fe_param_grad.h -- adjoint of one substep with respect to the particles' material parameters (option "param_grad").
// Included by fe_engine.hip behind the substep kernels; uses its frame views, stencil and material records.
//
// substep f deposits, for every used particle p with its stencil inside the grid (mpm:339-353),
//     v_in[node] += w (mass v + affine dpos),   m[node] += w mass,   affine = scale stress(mu, lam) + mass C,   mass = p_vol rho
// and nothing else of the substep reads mu, lam or mass (F[f + 1] does not, the plastic clamp does not: constitutive_eval_t).  With the
// grid adjoint gg = (d/d v_in, d/d m) of frame f -- what k_grid_grad / k_grid_collide_grad leave in gg_in -- the three derivatives are
// node sums that used_particle_p2g_grad forms as well (Gv, M -> GA) plus Gm = sum w gg.w, contracted in constitutive_param_grad (fp64).
// The incoming adjoint of F[f + 1] is not read.
//
// A launch of its own, in front of substep f's k_p2g_grad / k_pgg_g2pg (substep_bwd): the substep kernels keep their registers.
// One thread per slot of frame f's order; the 27 nodes are a global gather (gg_in was written by the launch before: L2) with all
// loads in flight before the first is consumed.  The sums are added to three fp64 accumulators indexed by PARTICLE ID, so a sort
// between two substeps of a sweep needs no reorder; a particle has one slot, hence one writer per launch: load, add, store.
// GENERAL = false is the launch of liquid-only scenes, whose frames may hold F compactly (FrameV::iso = 1: F = c I is expanded by load_F).
template <bool GENERAL>
__global__ __launch_bounds__(256) void k_param_grad(SimP S, float* fr_cur, TableP T, const float4* __restrict__ gg_in, int fiso, float p_vol,
                                                    double* __restrict__ acc) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S.N) return;
    const FrameV cur = frame_view(fr_cur, S.Np, 0, GENERAL ? 0 : (fiso & 1));
    if (cur.used[s] == 0) return;                             // (a particle the Injector takes into use in substep f is unused in frame f: it counts from f + 1 on)
    PState p;
    load_xvC(cur, s, p);
    load_F(cur, s, p.F);
    Stencil st;
    stencil_make(p.x, S.inv_dx, st);
    if (!stencil_inside(st, S.n)) return;                     // (deposits nothing in p2g either)
    float4 g[27];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int k = 0; k < 3; k++) g[(i * 3 + j) * 3 + k] = gg_in[cell_addr(st.base[0] + i, st.base[1] + j, st.base[2] + k, S.nb)];
    float Gv[3] = {0.f, 0.f, 0.f}, Gm = 0.f;
    m3 M = m3_zero();                                         // M[a][b] = sum w gg[a] o_b, o = node offset (0, 1, 2 per axis)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float wij = st.w[i][0] * st.w[j][1];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float4 gi = g[(i * 3 + j) * 3 + k];
                const float w = wij * st.w[k][2];
                const float wg[3] = {w * gi.x, w * gi.y, w * gi.z};
                Gm += w * gi.w;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    Gv[a] += wg[a];
                    M.a[a][0] += (float)i * wg[a]; M.a[a][1] += (float)j * wg[a]; M.a[a][2] += (float)k * wg[a];
                }
            }
        }
    m3 GA;                                                    // sum w gg[a] dpos_b, dpos = (o - fx) dx: as used_particle_p2g_grad forms it
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) GA.a[a][b] = S.dx * (M.a[a][b] - st.fx[b] * Gv[a]);
    double g_mu, g_lam, g_mass;
    constitutive_param_grad(p.C, p.F, S.dt, S.stress_scale, GA, p.v, Gv, Gm, g_mu, g_lam, g_mass);
    const int pid = T.pid_of_slot[s];
    if ((unsigned)pid >= (unsigned)S.N) return;
    double* a_mu = acc + pid;
    double* a_lam = acc + (size_t)S.N + pid;
    double* a_rho = acc + 2 * (size_t)S.N + pid;
    *a_mu += g_mu;
    *a_lam += g_lam;
    *a_rho += (double)p_vol * g_mass;                         // mass = p_vol rho
}
