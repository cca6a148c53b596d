// Host check of plan_columns (phiflow_amd/csrc/column_march.hpp) against the five launch-plan formulas it replaced, which stand
// below as they stood in launch_divergence, launch_diffuse, coef_plan, diff_op / diff_grid and mom_plan. Every formula is compared wherever its
// fixed parameters (target, forced chunk, single chunk, tile shape) are the tuple's. Host code only, built against the emulation's HIP header:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/hipemu/include -x c++ tools/column_plan_sweep.cpp -o sweep && ./sweep
// Prints the number of tuples and of comparisons; exit status 1 on any difference.
#include "../phiflow_amd/csrc/common.hpp"

namespace phihip {
void set_error(const char*, ...) {}
}

using phihip::ceil_div;
using phihip::ColumnPlan;

struct Old {
    int tiles1, tiles2, chunk, chunks;
};

static Old old_divergence(const int n[3], int rank, int rows, int cols) {
    const int tiles1 = ceil_div(n[1], rows), tiles2 = ceil_div(n[2], cols);
    const long long tiles = (long long)tiles1 * tiles2;
    int chunks = rank == 3 ? (int)((4096 + tiles - 1) / tiles) : 1;
    chunks = chunks > n[0] ? n[0] : (chunks < 1 ? 1 : chunks);
    const int chunk_planes = ceil_div(n[0], chunks);
    chunks = ceil_div(n[0], chunk_planes);
    return {tiles1, tiles2, chunk_planes, chunks};
}

static Old old_diffuse(const int cn[3]) {
    const int tiles1 = ceil_div(cn[1], 4), tiles2 = ceil_div(cn[2], 64);
    const long long tiles = (long long)tiles1 * tiles2;
    int chunks = (int)((4096 + tiles - 1) / tiles);
    chunks = chunks > cn[0] ? cn[0] : (chunks < 1 ? 1 : chunks);
    const int chunk = ceil_div(cn[0], chunks);
    chunks = ceil_div(cn[0], chunk);
    return {tiles1, tiles2, chunk, chunks};
}

static Old old_coef(const int n[3], int target) {
    Old op;
    op.tiles1 = (n[1] + 3) / 4;
    op.tiles2 = (n[2] + 63) / 64;
    const long long tiles = (long long)op.tiles1 * op.tiles2;
    int chunks = (int)((target + tiles - 1) / tiles);
    chunks = chunks > n[0] ? n[0] : (chunks < 1 ? 1 : chunks);
    op.chunk = (n[0] + chunks - 1) / chunks;
    chunks = (n[0] + op.chunk - 1) / op.chunk;
    op.chunks = chunks;       // nblk = tiles * chunks
    return op;
}

static Old old_diffops(const int n[3], int tuning_chunk) {
    Old op;
    op.tiles1 = ceil_div(n[1], 4);
    op.tiles2 = ceil_div(n[2], 64);
    const long long tiles = (long long)op.tiles1 * op.tiles2;
    int chunks = (int)((4096 + tiles - 1) / tiles);
    chunks = chunks > n[0] ? n[0] : (chunks < 1 ? 1 : chunks);
    op.chunk = ceil_div(n[0], chunks);
    if (tuning_chunk > 0) op.chunk = tuning_chunk < n[0] ? tuning_chunk : n[0];
    op.chunks = ceil_div(n[0], op.chunk);       // diff_grid
    return op;
}

static Old old_momentum(const int L[3], int tuning_chunk) {
    Old op;
    op.tiles1 = ceil_div(L[1], 4);
    op.tiles2 = ceil_div(L[2], 64);
    const long long tiles = (long long)op.tiles1 * op.tiles2;
    int chunks = (int)((4096 + tiles - 1) / tiles);
    chunks = chunks > L[0] ? L[0] : (chunks < 1 ? 1 : chunks);
    op.chunk = ceil_div(L[0], chunks);
    if (tuning_chunk > 0) op.chunk = tuning_chunk < L[0] ? tuning_chunk : L[0];
    op.chunks = ceil_div(L[0], op.chunk);
    return op;
}

static long long differences = 0, comparisons = 0;

static void compare(const char* which, const Old& o, const ColumnPlan& p, const int L[3], int target, int forced, bool single, int rows, int cols) {
    ++comparisons;
    if (o.tiles1 == p.tiles1 && o.tiles2 == p.tiles2 && o.chunk == p.chunk && o.chunks == p.chunks) return;
    if (++differences <= 20)
        printf("%s: L (%d, %d, %d) target %d forced %d single %d tile %d x %d: old (%d, %d, %d, %d) new (%d, %d, %d, %d)\n", which, L[0], L[1], L[2], target, forced,
               (int)single, rows, cols, o.tiles1, o.tiles2, o.chunk, o.chunks, p.tiles1, p.tiles2, p.chunk, p.chunks);
}

int main() {
    long long tuples = 0;
    const int targets[2] = {1024, 4096};
    for (int L0 = 1; L0 <= 300; ++L0)
        for (int L1 = 1; L1 <= 40; ++L1)
            for (int L2 = 1; L2 <= 200; ++L2) {
                const int L[3] = {L0, L1, L2};
                // the tile shapes: 4 x 64, and launch_divergence's vector shapes for this row length in fp32 (V = 4) and fp64 (V = 2)
                int shape[3][2] = {{4, 64}, {0, 0}, {0, 0}};
                for (int q = 1; q < 3; ++q) {
                    const int V = q == 1 ? 4 : 2;
                    int ltpr = 6;
                    while (ltpr > 0 && (1 << (ltpr - 1)) * V >= L2) --ltpr;
                    shape[q][0] = 256 >> ltpr;
                    shape[q][1] = (1 << ltpr) * V;
                }
                for (int ti = 0; ti < 2; ++ti)
                    for (int fi = 0; fi <= 6; ++fi)
                        for (int single = 0; single < 2; ++single)
                            for (int q = 0; q < 3; ++q) {
                                const int target = targets[ti], forced = fi < 6 ? fi : L0 + 3, rows = shape[q][0], cols = shape[q][1];
                                ColumnPlan p;
                                if (phihip::plan_columns(L, rows, cols, target, forced, single != 0, "sweep", p) != PHIHIP_OK) { ++differences; continue; }
                                ++tuples;
                                if (target == 4096 && forced == 0) compare("divergence", old_divergence(L, single ? 2 : 3, rows, cols), p, L, target, forced, single, rows, cols);
                                if (single || q != 0) continue;
                                if (target == 4096 && forced == 0) compare("diffuse", old_diffuse(L), p, L, target, forced, single, rows, cols);
                                if (forced == 0) compare("coef", old_coef(L, target), p, L, target, forced, single, rows, cols);
                                if (target == 4096) {
                                    compare("diffops", old_diffops(L, forced), p, L, target, forced, single, rows, cols);
                                    compare("momentum", old_momentum(L, forced), p, L, target, forced, single, rows, cols);
                                }
                            }
            }
    printf("%lld tuples planned, %lld comparisons with the old formulas, %lld differences\n", tuples, comparisons, differences);
    return differences ? 1 : 0;
}
