// column_march.hpp -- what the column-march stencil kernels share: a 256-thread workgroup owns a (kPatchRows x kPatchCols) column of one
// lattice and marches over a chunk of a0 planes with the a0 neighbours in registers (divergence*_kernel, diffuse_kernel, coef_kernel, cgrad / cdiv_kernel, the
// advect_diff_* kernels). plan_columns is their launch plan, column_tile / column_planes the way from a workgroup number to the thread's column and planes.
#pragma once

namespace phihip {

constexpr int kPatchCols = 64, kPatchRows = kBlock / kPatchCols;   // also the patches of the patch-stride kernels (project.hip decode_patch)

struct ColumnPlan { int tiles1, tiles2, chunk, chunks; };   // (rows x cols) tiles along a1 / a2, planes per workgroup, workgroups along a0

// About `target` workgroups per batch entry when L has the planes for it; forced_chunk > 0 (phihip_set_tuning_kernel): that many planes per workgroup instead;
// single_chunk: one workgroup marches over all planes. `chunks` is computed again from `chunk` (it can come out lower): it counts the partial sums of the reducing kernels.
inline int plan_columns(const int L[3], int rows, int cols, int target, int forced_chunk, bool single_chunk, const char* what, ColumnPlan& plan) {
    plan.tiles1 = ceil_div(L[1], rows);
    plan.tiles2 = ceil_div(L[2], cols);
    const long long tiles = (long long)plan.tiles1 * plan.tiles2;
    int chunks = single_chunk ? 1 : (int)((target + tiles - 1) / tiles);
    chunks = chunks > L[0] ? L[0] : (chunks < 1 ? 1 : chunks);
    plan.chunk = ceil_div(L[0], chunks);
    if (forced_chunk > 0) plan.chunk = forced_chunk < L[0] ? forced_chunk : L[0];
    plan.chunks = ceil_div(L[0], plan.chunk);
    if (tiles * plan.chunks >= (1LL << 31)) { set_error("%s: the grid is too large for one launch", what); return PHIHIP_ERR_UNSUPPORTED; }
    return PHIHIP_OK;
}

struct ColumnTile {
    int i1, i2, ch, p0, p1;     // this thread's row and (first) column, the workgroup's chunk of planes [p0, p1)
    bool inside;                // the thread has a sample in the plane
};

// Workgroup `wg` of the plan (int or unsigned, xcd_order applied or not: the caller's choice) on planes of L1 x L2 samples. Neither function returns from the
// kernel: the threads without work of a reducing kernel still take part in its block reductions. ltpr / vec: log2 of the threads along a row and the cells
// per thread (the vector form of the divergence; 6 and 1 give the 4 x 64 tile).
template <typename WG>
__device__ __forceinline__ ColumnTile column_tile(const ColumnPlan& plan, int L1, int L2, WG wg, int ltpr = 6, int vec = 1) {
    const int tx = threadIdx.x & ((1 << ltpr) - 1), ty = threadIdx.x >> ltpr;
    const int t2 = wg % plan.tiles2;
    const int t1 = (wg / plan.tiles2) % plan.tiles1;
    ColumnTile t;
    t.ch = wg / (plan.tiles2 * plan.tiles1);
    t.i1 = t1 * (kBlock >> ltpr) + ty;
    t.i2 = ((t2 << ltpr) + tx) * vec;
    t.inside = t.i1 < L1 && t.i2 < L2;
    return t;
}

// the planes of the tile's chunk out of L0; false: none. MARCH = false (kernels of 2-D grids): the one plane, `chunk` is not read
template <bool MARCH = true>
__device__ __forceinline__ bool column_planes(const ColumnPlan& plan, ColumnTile& t, int L0) {
    t.p0 = MARCH ? t.ch * plan.chunk : 0;
    t.p1 = MARCH ? (t.p0 + plan.chunk < L0 ? t.p0 + plan.chunk : L0) : 1;
    return t.p0 < t.p1;
}

}  // namespace phihip
