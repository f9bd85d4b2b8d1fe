// Host check of the grid kernels' launch chooser (fluidlab_amd/csrc/fe_grid_launch.h: fe_grid_launch_wgs, fe_grid_launch_fixed), the function the engine
// sizes every separate k_grid / k_grid_grad launch with, over a sweep of hints x caps x grid sizes x margins, exact and lagged.  Plain C++, no GPU.
#include <algorithm>
#include <cstdio>
#include <vector>
#include "../../fluidlab_amd/csrc/fe_grid_launch.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; if (failures < 50) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

int main() {
    const int grids[] = {1, 8, 64, 512, 1000, 4096, 4097, 32768, 262144, 2097152};        // blocks: 4^3 ... 512^3 nodes, and sizes that are no multiple of anything
    const int caps[] = {0, 1, 2, 5, 16, 127, 128, 1000, 1024, 1536, 2048, 4096, 100000};   // 0 = derived; the others are option ggrid_cap set explicitly
    const int margins[] = {100, 125, 150, 400};
    std::vector<long long> hints;
    for (long long hnt = 0; hnt <= 20000; hnt += (hnt < 64 ? 1 : hnt < 4400 ? 37 : 251)) hints.push_back(hnt);
    for (long long hnt : {4LL * FE_GL_FLOOR_WGS - 1, 4LL * FE_GL_FLOOR_WGS, 4LL * FE_GL_FLOOR_WGS + 1, 4LL * FE_GL_ONE_CAP_WGS - 1, 4LL * FE_GL_ONE_CAP_WGS, 4LL * FE_GL_ONE_CAP_WGS + 1,
                          32768LL, 262144LL, 2097152LL, 2147483647LL, 1LL << 40}) hints.push_back(hnt);
    long long checked = 0;
    for (int blocks : grids)
        for (int cap : caps)
            for (int margin : margins)
                for (int exact = 0; exact < 2; exact++) {
                    const int fixed = fe_grid_launch_fixed(blocks, cap);
                    const int all = blocks > 4 ? (blocks + 3) / 4 : 1;
                    // today's launch: a wave per block, 1,024 workgroups at most, or the explicit cap
                    CHECK(fixed >= 1 && fixed <= all && fixed <= (cap > 0 ? cap : 1024), "fixed %d blocks %d cap %d", fixed, blocks, cap);
                    CHECK(fixed == all || fixed == (cap > 0 ? cap : 1024), "fixed %d is neither the grid nor the cap (blocks %d cap %d)", fixed, blocks, cap);
                    // no hint: today's launch
                    CHECK(fe_grid_launch_wgs(-1, margin, exact != 0, blocks, cap) == fixed, "no hint: %d != fixed %d", fe_grid_launch_wgs(-1, margin, exact != 0, blocks, cap), fixed);
                    if (cap == 0 && blocks >= 4096) CHECK(fe_grid_launch_wgs(-1, margin, exact != 0, blocks, cap) == 1024, "no hint, no cap: not 1,024");
                    int prev = 0; long long prev_hint = -1;
                    std::vector<long long> hs = hints;
                    std::sort(hs.begin(), hs.end());
                    for (size_t i = 0; i < hs.size(); i++) {
                        const long long hnt = hs[i];
                        const int g = fe_grid_launch_wgs(hnt, margin, exact != 0, blocks, cap);
                        checked++;
                        CHECK(g >= 1, "g %d", g);
                        CHECK(g <= all, "more workgroups (%d) than the grid has blocks for (%d)", g, all);
                        if (cap > 0) CHECK(g <= cap, "g %d above the explicit cap %d (hint %lld)", g, cap, hnt);
                        CHECK(g <= FE_GL_ONE_CAP_WGS || g == fixed, "g %d above the one-entry-per-wave cap and not the fixed launch", g);
                        const long long n = exact ? hnt : (hnt * margin + 99) / 100;
                        const bool short_reach = (n + 3) / 4 <= FE_GL_ONE_CAP_WGS;          // one entry per wave is within the cap up to which it pays
                        if (!short_reach) CHECK(g == fixed, "beyond the cap: %d != fixed %d (hint %lld)", g, fixed, hnt);
                        const bool cut = g == all || (cap > 0 && g == cap);                 // the grid or the explicit cap cut the result
                        if (short_reach) {
                            if (!cut) {
                                CHECK(g % FE_GL_QUANTUM == 0, "g %d is no multiple of %d (hint %lld blocks %d cap %d)", g, FE_GL_QUANTUM, hnt, blocks, cap);
                                CHECK(g >= FE_GL_FLOOR_WGS, "g %d below the floor (hint %lld)", g, hnt);
                                CHECK(4LL * g >= hnt && 4LL * g >= n, "4 x %d < hint %lld (n %lld)", g, hnt, n);
                                CHECK(4LL * g < n + 4LL * FE_GL_QUANTUM + 4 || g == FE_GL_FLOOR_WGS, "g %d: more than one quantum of surplus for %lld entries", g, n);
                            } else if (4LL * g < hnt) {
                                CHECK(g == all || g == cap, "short of the hint without a cut");
                            }
                            // monotone in the hint while the short road is in reach
                            if (prev_hint >= 0 && hnt >= prev_hint) CHECK(g >= prev, "not monotone: hint %lld -> %d, hint %lld -> %d (blocks %d cap %d margin %d exact %d)", prev_hint, prev, hnt, g, blocks, cap, margin, exact);
                            prev = g; prev_hint = hnt;
                        }
                        // a lagged hint never gets fewer workgroups than the same length known exactly, within the short road's reach
                        if (!exact && short_reach) CHECK(g >= fe_grid_launch_wgs(hnt, margin, true, blocks, cap), "lagged below exact (hint %lld)", hnt);
                    }
                }
    // the values the engine's defaults rest on
    CHECK(fe_grid_launch_wgs(1100, 125, true, 32768, 0) == FE_GL_FLOOR_WGS, "falling block");
    CHECK(fe_grid_launch_wgs(6025, 125, true, 32768, 0) == 1536, "layer, exact: %d", fe_grid_launch_wgs(6025, 125, true, 32768, 0));
    CHECK(fe_grid_launch_wgs(24954, 125, true, 32768, 0) == 1024, "splash: the fixed launch");
    CHECK(fe_grid_launch_wgs(5000, 125, true, 32768, 3) == 3, "explicit cap 3");
    CHECK(fe_grid_launch_wgs(1, 125, true, 32768, 0) == fe_grid_launch_wgs(0, 125, true, 32768, 0), "tiny lists");
    std::printf("%lld combinations, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
