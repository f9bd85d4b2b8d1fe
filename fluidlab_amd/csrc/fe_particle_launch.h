// fe_particle_launch.h -- host-side launchers of the particle kernels (k_p2g*, k_g2p*, k_g2p_p2g*, k_p2g_grad*, k_g2p_grad2*, k_pgg_g2pg*).
// Included by fe_engine.hip behind the kernels and the records their launches pass, in both translation units of the library: the engine unit calls
// these functions at its launch sites, fe_particles.hip defines them -- plain host code, no relocatable device code.  launch_<kernel><...>(grid,
// stream, <the kernel's arguments>) launches <kernel><...> with WG threads per workgroup.  Every instantiation the engine uses is instantiated explicitly
// at the end of fe_particles.hip, which is where the kernel is emitted; one that is missing there fails the link of the library (-Wl,--no-undefined).
template <bool WRITE, bool GENERAL>
void launch_k_p2g(dim3 grid, hipStream_t stream, const UnitRec* h_units, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* fr_next, TableP T, const int* pool_idx, GridW G, AgentP agent, InjectP inj, int act, int f, GridStore GS, int fiso);
template <bool GENERAL>
void launch_k_g2p_p2g(dim3 grid, hipStream_t stream, const UnitRec* h_units, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* fr_next, TableP T, const int* pool_idx, GridW G, AgentP agent, InjectP inj, int act, int f, GridStore GS, int fiso, FuseP FU);
template <bool GENERAL> void launch_k_p2g_fg(dim3 grid, hipStream_t stream, const P2GArgs& A);
template <bool GENERAL> void launch_k_g2p_p2g_fg(dim3 grid, hipStream_t stream, const P2GArgs& A);
template <bool GENERAL> void launch_k_g2p_p2g_b(dim3 grid, hipStream_t stream, const Batch<P2GArgs>& B);
template <bool WRITE, bool GENERAL> void launch_k_p2g_b(dim3 grid, hipStream_t stream, const Batch<P2GArgs>& B);

template <bool COLLIDE>
void launch_k_g2p(dim3 grid, hipStream_t stream, const UnitRec* h_units_p, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* fr_next, TableP T, const float4* g_out, int* blk_count, int* slow, AgentP agent, int f);
template <bool COLLIDE>
void launch_k_g2p_sortkey(dim3 grid, hipStream_t stream, const UnitRec* h_units_p, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* fr_next, TableP T, const float4* g_out, int* blk_count, int* slow, AgentP agent, int f, SortKeyP K);
template <bool COLLIDE> void launch_k_g2p_b(dim3 grid, hipStream_t stream, const Batch<G2PArgs>& B);

template <int MINW>
void launch_k_g2p_grad2(dim3 grid, hipStream_t stream, const UnitRec* h_units, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* Gn_, float* Gc_, TableP T, const float4* g_out, float* gg_out, float4* slab, int* slow, GridStore GS, int f, AgentP agent);
template <int MINW> void launch_k_g2p_grad2_b(dim3 grid, hipStream_t stream, const Batch<G2PGradArgs>& B);

template <bool GENERAL, int MINW>
void launch_k_p2g_grad(dim3 grid, hipStream_t stream, const UnitRec* h_units, const UnitRec* h_units_p, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* Gn_, float* Gc_, TableP T, const int* pool_idx, const float4* gg_in, int* blk_count, int* slow, AgentP agent, InjectP inj, int act, int f, float* Gd_, const int* to_slot, int fiso);
template <bool GENERAL, int MINW> void launch_k_p2g_grad_b(dim3 grid, hipStream_t stream, const Batch<P2GGradArgs>& B);

template <int MINW, bool GENERAL = false>
void launch_k_pgg_g2pg(dim3 grid, hipStream_t stream, const UnitRec* h_list, const int* h_meta, int h_cap, SimP S, float* fr_cur, float* Gn_, float* Gc_, TableP T, const int* pool_idx, const float4* gg_in, int* blk_count, int* slow, AgentP agent, InjectP inj, int act, int f, int fiso, BwdFuseP B, GridStore GS);
template <int MINW> void launch_k_pgg_g2pg_b(dim3 grid, hipStream_t stream, const Batch<PggArgs>& Bt);
