// fe_particles.hip -- the particle unit of the MI355X (gfx950) FluidEngine: p2g, g2p, their fused forms and their adjoints, with the batched (_b)
// and fuse_grid (_fg) entry points, as a translation unit of their own, so that these kernels -- bound by the vector instructions they issue -- get
// their own code-generation flags (__graft_entry__.py: UNITS), apart from the latency-bound grid and sort kernels of the engine unit.
// The kernels' text is fe_engine.hip's: included here up to the unit boundary (FE_PARTICLE_UNIT), where nothing has been instantiated yet.  This file
// defines the host-side launchers the engine unit calls (fe_particle_launch.h); their explicit instantiations are what emits the kernels here.
#define FE_PARTICLE_UNIT
#include "fe_engine.hip"

// host-side launchers (fe_particle_launch.h): what the engine unit launches the particle kernels through
#define PL(kernel, ...) hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel), grid, dim3(WG), 0, stream, __VA_ARGS__)
template <bool WRITE, bool GENERAL>
void launch_k_p2g(dim3 grid, hipStream_t stream, const UnitRec* h_units, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* fr_next, TableP T, const int* pool_idx, GridW G, AgentP agent, InjectP inj, int act, int f, GridStore GS, int fiso) {
    PL((k_p2g<WRITE, GENERAL>), h_units, h_meta, h_cap, S, fr_cur, fr_next, T, pool_idx, G, agent, inj, act, f, GS, fiso);
}
template <bool GENERAL>
void launch_k_g2p_p2g(dim3 grid, hipStream_t stream, const UnitRec* h_units, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* fr_next, TableP T, const int* pool_idx, GridW G, AgentP agent, InjectP inj, int act, int f, GridStore GS, int fiso, FuseP FU) {
    PL(k_g2p_p2g<GENERAL>, h_units, h_meta, h_cap, S, fr_cur, fr_next, T, pool_idx, G, agent, inj, act, f, GS, fiso, FU);
}
template <bool GENERAL> void launch_k_p2g_fg(dim3 grid, hipStream_t stream, const P2GArgs& A) { PL(k_p2g_fg<GENERAL>, A); }
template <bool GENERAL> void launch_k_g2p_p2g_fg(dim3 grid, hipStream_t stream, const P2GArgs& A) { PL(k_g2p_p2g_fg<GENERAL>, A); }
template <bool GENERAL> void launch_k_g2p_p2g_b(dim3 grid, hipStream_t stream, const Batch<P2GArgs>& B) { PL(k_g2p_p2g_b<GENERAL>, B); }
template <bool WRITE, bool GENERAL> void launch_k_p2g_b(dim3 grid, hipStream_t stream, const Batch<P2GArgs>& B) { PL((k_p2g_b<WRITE, GENERAL>), B); }
template <bool COLLIDE>
void launch_k_g2p(dim3 grid, hipStream_t stream, const UnitRec* h_units_p, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* fr_next, TableP T, const float4* g_out, int* blk_count, int* slow, AgentP agent, int f) {
    PL(k_g2p<COLLIDE>, h_units_p, h_meta, h_cap, S, fr_cur, fr_next, T, g_out, blk_count, slow, agent, f);
}
template <bool COLLIDE>
void launch_k_g2p_sortkey(dim3 grid, hipStream_t stream, const UnitRec* h_units_p, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* fr_next, TableP T, const float4* g_out, int* blk_count, int* slow, AgentP agent, int f, SortKeyP K) {
    PL(k_g2p_sortkey<COLLIDE>, h_units_p, h_meta, h_cap, S, fr_cur, fr_next, T, g_out, blk_count, slow, agent, f, K);
}
template <bool COLLIDE> void launch_k_g2p_b(dim3 grid, hipStream_t stream, const Batch<G2PArgs>& B) { PL(k_g2p_b<COLLIDE>, B); }
template <int MINW>
void launch_k_g2p_grad2(dim3 grid, hipStream_t stream, const UnitRec* h_units, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* Gn_, float* Gc_, TableP T, const float4* g_out, float* gg_out, float4* slab, int* slow, GridStore GS, int f, AgentP agent) {
    PL(k_g2p_grad2<MINW>, h_units, h_meta, h_cap, S, fr_cur, Gn_, Gc_, T, g_out, gg_out, slab, slow, GS, f, agent);
}
template <int MINW> void launch_k_g2p_grad2_b(dim3 grid, hipStream_t stream, const Batch<G2PGradArgs>& B) { PL(k_g2p_grad2_b<MINW>, B); }
template <bool GENERAL, int MINW>
void launch_k_p2g_grad(dim3 grid, hipStream_t stream, const UnitRec* h_units, const UnitRec* h_units_p, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* Gn_, float* Gc_, TableP T, const int* pool_idx, const float4* gg_in, int* blk_count, int* slow, AgentP agent, InjectP inj, int act, int f, float* Gd_, const int* to_slot, int fiso) {
    PL((k_p2g_grad<GENERAL, MINW>), h_units, h_units_p, h_meta, h_cap, S, fr_cur, Gn_, Gc_, T, pool_idx, gg_in, blk_count, slow, agent, inj, act, f, Gd_, to_slot, fiso);
}
template <bool GENERAL, int MINW> void launch_k_p2g_grad_b(dim3 grid, hipStream_t stream, const Batch<P2GGradArgs>& B) { PL((k_p2g_grad_b<GENERAL, MINW>), B); }
template <int MINW, bool GENERAL>
void launch_k_pgg_g2pg(dim3 grid, hipStream_t stream, const UnitRec* h_list, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* Gn_, float* Gc_, TableP T, const int* pool_idx, const float4* gg_in, int* blk_count, int* slow, AgentP agent, InjectP inj, int act, int f, int fiso, BwdFuseP B, GridStore GS) {
    PL((k_pgg_g2pg<MINW, GENERAL>), h_list, h_meta, h_cap, S, fr_cur, Gn_, Gc_, T, pool_idx, gg_in, blk_count, slow, agent, inj, act, f, fiso, B, GS);
}
template <int MINW> void launch_k_pgg_g2pg_b(dim3 grid, hipStream_t stream, const Batch<PggArgs>& Bt) { PL(k_pgg_g2pg_b<MINW>, Bt); }
#undef PL

// The instantiations fe_engine.hip launches (launch_fwd, launch_bwd and the batched roads); a kernel is emitted where its launcher is instantiated.
// This file is compiled twice, into two objects of the one library (__graft_entry__.py): once as it stands with PARTICLE_FLAGS -- the scatter,
// adjoint and fused kernels, which issue fewer vector instructions with the IR load/store vectoriser off --, and once with -DFE_PARTICLES_GATHER and
// the engine's flags for the plain gather kernels (k_g2p, k_g2p_sortkey, k_g2p_b), which lose a wave of occupancy without that vectoriser.
#ifdef FE_PARTICLES_GATHER
template void launch_k_g2p<true>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, TableP, const float4*, int*, int*, AgentP, int);
template void launch_k_g2p<false>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, TableP, const float4*, int*, int*, AgentP, int);
template void launch_k_g2p_sortkey<true>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, TableP, const float4*, int*, int*, AgentP, int, SortKeyP);
template void launch_k_g2p_sortkey<false>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, TableP, const float4*, int*, int*, AgentP, int, SortKeyP);
template void launch_k_g2p_b<false>(dim3, hipStream_t, const Batch<G2PArgs>&);
#else
template void launch_k_p2g<true, false>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, TableP, const int*, GridW, AgentP, InjectP, int, int, GridStore, int);
template void launch_k_p2g<true, true>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, TableP, const int*, GridW, AgentP, InjectP, int, int, GridStore, int);
template void launch_k_p2g<false, false>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, TableP, const int*, GridW, AgentP, InjectP, int, int, GridStore, int);
template void launch_k_p2g<false, true>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, TableP, const int*, GridW, AgentP, InjectP, int, int, GridStore, int);
template void launch_k_g2p_p2g<false>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, TableP, const int*, GridW, AgentP, InjectP, int, int, GridStore, int, FuseP);
template void launch_k_g2p_p2g<true>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, TableP, const int*, GridW, AgentP, InjectP, int, int, GridStore, int, FuseP);
template void launch_k_p2g_fg<false>(dim3, hipStream_t, const P2GArgs&);
template void launch_k_p2g_fg<true>(dim3, hipStream_t, const P2GArgs&);
template void launch_k_g2p_p2g_fg<false>(dim3, hipStream_t, const P2GArgs&);
template void launch_k_g2p_p2g_fg<true>(dim3, hipStream_t, const P2GArgs&);
template void launch_k_g2p_p2g_b<false>(dim3, hipStream_t, const Batch<P2GArgs>&);
template void launch_k_g2p_p2g_b<true>(dim3, hipStream_t, const Batch<P2GArgs>&);
template void launch_k_p2g_b<true, false>(dim3, hipStream_t, const Batch<P2GArgs>&);
template void launch_k_p2g_b<true, true>(dim3, hipStream_t, const Batch<P2GArgs>&);
template void launch_k_p2g_b<false, false>(dim3, hipStream_t, const Batch<P2GArgs>&);
template void launch_k_p2g_b<false, true>(dim3, hipStream_t, const Batch<P2GArgs>&);
template void launch_k_g2p_grad2<3>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, float*, TableP, const float4*, float*, float4*, int*, GridStore, int, AgentP);
template void launch_k_g2p_grad2<4>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, float*, TableP, const float4*, float*, float4*, int*, GridStore, int, AgentP);
template void launch_k_g2p_grad2_b<3>(dim3, hipStream_t, const Batch<G2PGradArgs>&);
template void launch_k_g2p_grad2_b<4>(dim3, hipStream_t, const Batch<G2PGradArgs>&);
template void launch_k_p2g_grad<false, 4>(dim3, hipStream_t, const UnitRec*, const UnitRec*, const int*, int, SimP, float*, float*, float*, TableP, const int*, const float4*, int*, int*, AgentP, InjectP, int, int, float*, const int*, int);
template void launch_k_p2g_grad<false, 3>(dim3, hipStream_t, const UnitRec*, const UnitRec*, const int*, int, SimP, float*, float*, float*, TableP, const int*, const float4*, int*, int*, AgentP, InjectP, int, int, float*, const int*, int);
template void launch_k_p2g_grad<false, 2>(dim3, hipStream_t, const UnitRec*, const UnitRec*, const int*, int, SimP, float*, float*, float*, TableP, const int*, const float4*, int*, int*, AgentP, InjectP, int, int, float*, const int*, int);
template void launch_k_p2g_grad<true, 1>(dim3, hipStream_t, const UnitRec*, const UnitRec*, const int*, int, SimP, float*, float*, float*, TableP, const int*, const float4*, int*, int*, AgentP, InjectP, int, int, float*, const int*, int);
template void launch_k_p2g_grad_b<false, 4>(dim3, hipStream_t, const Batch<P2GGradArgs>&);
template void launch_k_p2g_grad_b<false, 3>(dim3, hipStream_t, const Batch<P2GGradArgs>&);
template void launch_k_p2g_grad_b<false, 2>(dim3, hipStream_t, const Batch<P2GGradArgs>&);
template void launch_k_p2g_grad_b<true, 1>(dim3, hipStream_t, const Batch<P2GGradArgs>&);
template void launch_k_pgg_g2pg<4, false>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, float*, TableP, const int*, const float4*, int*, int*, AgentP, InjectP, int, int, int, BwdFuseP, GridStore);
template void launch_k_pgg_g2pg<3, true>(dim3, hipStream_t, const UnitRec*, const int*, int, SimP, float*, float*, float*, TableP, const int*, const float4*, int*, int*, AgentP, InjectP, int, int, int, BwdFuseP, GridStore);
template void launch_k_pgg_g2pg_b<4>(dim3, hipStream_t, const Batch<PggArgs>&);
#endif
