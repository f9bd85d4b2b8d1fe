// Host run of the contact wrench's shared math (fluidlab_amd/csrc/fe_contact.h: fe_ct_particle, fe_ct_node, fe_ct_merge_partials,
// fe_ct_finish -- the steps k_contact_particles, k_contact_nodes and k_contact_merge run) on a case that tests/test_contact_math.py writes
// and holds against the numpy restatement tests/contact_ref.py.  No GPU.
//
//   contact_test <case file> <result file>
//
// Case file (little-endian, int32 / float32):
//   int32 n_st, n_eff, node_dyn, n_nodes, n_part, n_split;  float32 dt, dx, g[3], collide_min_y
//   per static:    int32 res;            float32 T[12], Rinv[9], friction, softness, vox[res^3]
//   per effector:  int32 has_mesh, res;  float32 T[12], Rinv[9], friction, softness, p0[3], q0[4], p1[3], q1[4], vox[res^3]
//   nodes:         int32 ijk[n_nodes][3];  float32 pm[n_nodes][4]         (summed momentum and mass)
//   particles:     float32 row[n_part][7]                                 (x[3], m, nv[3]: the gathered velocity)
// Result file: FeContactAcc node_partial[n_split][FE_CT_SLOTS], node_merged[FE_CT_SLOTS], part_partial[n_split][FE_CT_SLOTS],
//   part_merged[FE_CT_SLOTS] (nodes and particles are dealt to the n_split partial records in contiguous ranges, in order), then
//   FeContactRecord rec[FE_CT_SLOTS] = finish(node_merged + part_merged, valid 1) and rec0[FE_CT_SLOTS] = the same with valid 0.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/fluidengine_ext.h"
#include "../../fluidlab_amd/csrc/fe_math.h"
#define FE_CONTACT_MATH_ONLY
#include "../../fluidlab_amd/csrc/fe_contact.h"

static FILE* fin;
template <typename T> static void rd(T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, fin) != n) { fprintf(stderr, "contact_test: short case file\n"); exit(2); }
}
struct Col { SdfP s; std::vector<float> vox; int has_mesh = 1; float p0[3], q0[4], p1[3], q1[4]; };
static void rd_sdf(Col& c) {
    rd(&c.s.res, 1);
    rd(c.s.T, 12); rd(c.s.Rinv, 9); rd(&c.s.friction, 1); rd(&c.s.softness, 1);
}
static void rd_vox(Col& c) {
    c.vox.resize((size_t)c.s.res * c.s.res * c.s.res);
    rd(c.vox.data(), c.vox.size());
    c.s.vox = c.vox.data();
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: contact_test <case file> <result file>\n"); return 2; }
    fin = fopen(argv[1], "rb");
    if (!fin) { fprintf(stderr, "contact_test: cannot open %s\n", argv[1]); return 2; }
    int hd[6]; float fl[6];
    rd(hd, 6); rd(fl, 6);
    const int n_st = hd[0], n_eff = hd[1], node_dyn = hd[2], n_nodes = hd[3], n_part = hd[4], n_split = hd[5];
    const float dt = fl[0], dx = fl[1], g[3] = {fl[2], fl[3], fl[4]}, min_y = fl[5];
    if (n_st < 0 || n_st > FE_MAX_STATICS || n_eff < 0 || n_eff > FE_MAX_EFF || n_split < 1 || n_nodes < 0 || n_part < 0) { fprintf(stderr, "contact_test: bad header\n"); return 2; }
    std::vector<Col> st(n_st), ef(n_eff);
    for (Col& c : st) { rd_sdf(c); rd_vox(c); }
    for (Col& c : ef) { rd(&c.has_mesh, 1); rd_sdf(c); rd(c.p0, 3); rd(c.q0, 4); rd(c.p1, 3); rd(c.q1, 4); rd_vox(c); }
    std::vector<int> ijk((size_t)n_nodes * 3); std::vector<float> pm((size_t)n_nodes * 4), row((size_t)n_part * 7);
    rd(ijk.data(), ijk.size()); rd(pm.data(), pm.size()); rd(row.data(), row.size());
    fclose(fin);

    std::vector<SdfP> statics(n_st);
    for (int s = 0; s < n_st; s++) statics[s] = st[s].s;
    std::vector<FeContactDyn> cols(n_eff);
    for (int e = 0; e < n_eff; e++) { cols[e].mesh = ef[e].has_mesh ? &ef[e].s : nullptr; cols[e].p0 = ef[e].p0; cols[e].q0 = ef[e].q0; cols[e].p1 = ef[e].p1; cols[e].q1 = ef[e].q1; }

    auto chunk = [&](int n, int c) { return (int)((long long)n * c / n_split); };
    std::vector<FeContactAcc> npart((size_t)n_split * FE_CT_SLOTS), ppart((size_t)n_split * FE_CT_SLOTS);
    for (auto& a : npart) fe_ct_clear(a);
    for (auto& a : ppart) fe_ct_clear(a);
    for (int c = 0; c < n_split; c++) {
        FeContactAcc* slots = &npart[(size_t)c * FE_CT_SLOTS];
        for (int i = chunk(n_nodes, c); i < chunk(n_nodes, c + 1); i++)
            fe_ct_node(statics.data(), n_st, cols.data(), n_eff, node_dyn != 0, min_y, dt, g, dx, &pm[(size_t)i * 4], pm[(size_t)i * 4 + 3], ijk[(size_t)i * 3], ijk[(size_t)i * 3 + 1],
                       ijk[(size_t)i * 3 + 2], slots, slots + FE_MAX_EFF);
        slots = &ppart[(size_t)c * FE_CT_SLOTS];
        for (int i = chunk(n_part, c); i < chunk(n_part, c + 1); i++)
            fe_ct_particle(cols.data(), n_eff, min_y, dt, row[(size_t)i * 7 + 3], &row[(size_t)i * 7], &row[(size_t)i * 7 + 4], slots);
    }
    FeContactAcc nm[FE_CT_SLOTS], pmg[FE_CT_SLOTS];
    FeContactRecord rec[FE_CT_SLOTS], rec0[FE_CT_SLOTS];
    for (int s = 0; s < FE_CT_SLOTS; s++) {
        fe_ct_merge_partials(&npart[s], n_split, FE_CT_SLOTS, nm[s]);
        fe_ct_merge_partials(&ppart[s], n_split, FE_CT_SLOTS, pmg[s]);
        FeContactAcc both = nm[s];
        fe_ct_merge(both, pmg[s]);
        const bool eff = s < FE_MAX_EFF;
        const float* ref = (eff && s < n_eff) ? ef[s].p0 : nullptr;
        fe_ct_finish(both, 1, eff ? 0 : 1, ref, rec[s]);
        fe_ct_finish(both, 0, eff ? 0 : 1, ref, rec0[s]);
    }
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) { fprintf(stderr, "contact_test: cannot write %s\n", argv[2]); return 2; }
    fwrite(npart.data(), sizeof(FeContactAcc), npart.size(), fo);
    fwrite(nm, sizeof(FeContactAcc), FE_CT_SLOTS, fo);
    fwrite(ppart.data(), sizeof(FeContactAcc), ppart.size(), fo);
    fwrite(pmg, sizeof(FeContactAcc), FE_CT_SLOTS, fo);
    fwrite(rec, sizeof(FeContactRecord), FE_CT_SLOTS, fo);
    fwrite(rec0, sizeof(FeContactRecord), FE_CT_SLOTS, fo);
    fclose(fo);
    printf("contact_test: %d nodes, %d particles, %d statics, %d effectors, %d partial records: 0 failures\n", n_nodes, n_part, n_st, n_eff, n_split);
    return 0;
}
