// diffops.hpp -- the grid differential operators of phi/field/_field_math.py, order 2:
//   laplace (:46-145)                        values through the kernels that exist: the marching kernels in MODE_APPLY with the operator
//                                            0 * I + w * L (uniform weight; project.hip lattice_view / diffuse_affine_walls) and coef_kernel
//                                            <CM_LAP> (per-axis weights and every backward pass: the operator is symmetric)
//   spatial_gradient(at='center') (:229-233) g_d = (U[i + e_d] - U[i - e_d]) / (2 dx_d)                       cgrad_kernel
//   divergence of a centred vector (:627-632) sum_d (V_d[i + e_d] - V_d[i - e_d]) / (2 dx_d)                   cdiv_kernel
//   curl, 2-D, at the cell corners (:642-673) staggered and centred                                            curl2d_kernel
// U = the field padded by one sample with its own extrapolation: PERIODIC wraps, OPEN (zero-gradient) copies the edge sample, CLOSED is the
// constant. Included by project.hip (the emulation build of the tests compiles the .hip files by name: no translation unit of its own).
//
// cgrad / cdiv: column-march kernels (column_march.hpp: launch plan and tile decode) like diffuse_kernel:
// the a0 neighbours are the values the thread read one plane earlier / reads one plane ahead (registers), the in-plane taps and their boundary
// rule are resolved once per thread. Every input array is read from HBM once, every output written once; all components and batch entries in
// one launch. curl2d: a 2-D grid has one a0 plane, so the forward kernel marches over the ROWS: every wavefront of the (4 x 64) workgroup owns 64
// columns of the (nx + 1) x (ny + 1) corners and a chunk of rows and keeps the previous row's samples in registers.
//
// Backward passes are GATHERS (no atomics) in the style of diffuse_kernel<T, true>. The transpose of a central difference
// g[i] = w (U[i + 1] - U[i - 1]) is  gs[j] = w (T[j - 1] - T[j + 1])  with the ADJOINT tap T outside the array: a wrapped tap is the wrapped
// neighbour, a clamped tap returns its weight to the edge sample (T = -G[edge]: the edge sample entered g[edge] with the opposite sign), a
// constant tap contributes nothing (T = 0). So the gradient's adjoint is cdiv_kernel<T, true> and the divergence's adjoint cgrad_kernel<T, true>:
// the same marching loops with the sign flipped and the adjoint taps -- NOT the negative divergence / gradient at walls. Gradients accumulate.
// The run_* launch sites pick the element type with with_dtype (common.hpp); the adjoint / staggered choice stays an `if` inside that lambda.
#pragma once

namespace phihip {

struct DiffOp {
    int n[3];              // cells per internal axis (n[0] == 1 for 2-D grids)
    int ax0;
    int comps;             // 3 - ax0: components of the vector side, component-major [batch][comps][cells]
    long long cells;
    int bc[3][2];          // the field's extrapolation per internal axis / side (unused axis: periodic)
    double val[3][2];
    double w[3];           // 1 / (2 dx_a), 0 on the unused axis
    ColumnPlan plan;
};

// value of a tap that falls outside the array: rule 1 = zero-gradient, 2 = constant (0 = inside / wrapped: `loaded`)
template <typename T, bool ADJ>
__device__ __forceinline__ T diff_tap(int rule, T loaded, T centre, T cval) {
    return rule == 0 ? loaded : (rule == 1 ? (ADJ ? -centre : centre) : (ADJ ? T(0) : cval));
}

// in-plane taps k = 2 * (axis - 1) + side of cell (i1, i2): offset within the plane and the rule outside the array
template <typename T>
__device__ __forceinline__ void diff_plane_taps(const DiffOp& op, int i1, int i2, int off[4], int rule[4], T cval[4]) {
    const int o_c = i1 * op.n[2] + i2;
    const int idx[2] = {i1, i2}, nn[2] = {op.n[1], op.n[2]}, st[2] = {op.n[2], 1};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int k = 2 * a + side, ax = a + 1;
            const int j = idx[a] + (side ? 1 : -1);
            off[k] = o_c + (side ? st[a] : -st[a]);
            rule[k] = 0;
            cval[k] = T(0);
            if (ax < op.ax0) { rule[k] = 2; off[k] = o_c; continue; }      // (unused axis of a 2-D grid: weight 0 anyway)
            if (j >= 0 && j < nn[a]) continue;
            const int code = op.bc[ax][side];
            if (code == PHIHIP_BC_PERIODIC) off[k] = o_c + (side ? -(nn[a] - 1) * st[a] : (nn[a] - 1) * st[a]);
            else if (code == PHIHIP_BC_OPEN) { rule[k] = 1; off[k] = o_c; }
            else { rule[k] = 2; off[k] = o_c; cval[k] = (T)op.val[ax][side]; }
        }
}

// the a0 neighbour plane `p` of this thread's column (uniform decision); `c_edge` = the edge sample of the column
template <typename T, bool ADJ>
__device__ __forceinline__ T diff_plane_nb(const DiffOp& op, const T* __restrict__ I, long long ps, int o_c, int p, T c_edge) {
    const int n0 = op.n[0];
    if (p >= 0 && p < n0) return I[(long long)p * ps + o_c];
    const int side = p < 0 ? 0 : 1;
    const int code = op.bc[0][side];
    if (code == PHIHIP_BC_PERIODIC) return I[(long long)(p < 0 ? p + n0 : p - n0) * ps + o_c];
    if (code == PHIHIP_BC_OPEN) return ADJ ? -c_edge : c_edge;
    return ADJ ? T(0) : (T)op.val[0][side];
}

#define PHIHIP_DIFF_TILE_PROLOGUE                                                                   \
    const int b = blockIdx.y;                                                                       \
    const int n0 = op.n[0], n1 = op.n[1], n2 = op.n[2];                                             \
    ColumnTile ct = column_tile(op.plan, n1, n2, xcd_order(blockIdx.x, gridDim.x));                 \
    if (!ct.inside || !column_planes(op.plan, ct, n0)) return;                                      \
    const int i1 = ct.i1, i2 = ct.i2, p0 = ct.p0, p1 = ct.p1;                                       \
    T w[3];                                                                                         \
    _Pragma("unroll") for (int ax = 0; ax < 3; ++ax) w[ax] = (T)op.w[ax];                           \
    int off[4], rule[4];                                                                            \
    T cval[4];                                                                                      \
    diff_plane_taps<T>(op, i1, i2, off, rule, cval);                                                \
    const int o_c = i1 * n2 + i2;                                                                   \
    const long long ps = (long long)n1 * n2;                                                        \
    const bool has0 = op.ax0 == 0;

// one scalar in, `comps` components out.  !ADJ: out_d = w_d (U[+e_d] - U[-e_d]) -- the centred gradient.
// ADJ: out_d += w_d (T[-e_d] - T[+e_d]) -- the adjoint of the centred DIVERGENCE (in = the divergence's output gradient).
template <typename T, bool ADJ>
__global__ __launch_bounds__(kBlock) void cgrad_kernel(DiffOp op, const T* __restrict__ in, T* __restrict__ out) {
    PHIHIP_DIFF_TILE_PROLOGUE
    const T* __restrict__ I = in + (long long)b * op.cells;
    T* __restrict__ O = out + (long long)b * op.comps * op.cells;
    T cur = I[(long long)p0 * ps + o_c];
    T prev = has0 ? diff_plane_nb<T, ADJ>(op, I, ps, o_c, p0 - 1, cur) : T(0);
    for (int p = p0; p < p1; ++p) {
        const long long po = (long long)p * ps;
        const T next = has0 ? diff_plane_nb<T, ADJ>(op, I, ps, o_c, p + 1, cur) : T(0);
        T tap[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) tap[k] = diff_tap<T, ADJ>(rule[k], I[po + off[k]], cur, cval[k]);
        T d[3] = {w[0] * (next - prev), w[1] * (tap[1] - tap[0]), w[2] * (tap[3] - tap[2])};
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (ax < op.ax0) continue;
            const long long o = (long long)(ax - op.ax0) * op.cells + po + o_c;
            if (ADJ) O[o] -= d[ax];
            else O[o] = d[ax];
        }
        prev = cur;
        cur = next;
    }
}

// `comps` components in, one scalar out.  !ADJ: out = sum_d w_d (V_d[+e_d] - V_d[-e_d]) -- the centred divergence.
// ADJ: out += sum_d w_d (T_d[-e_d] - T_d[+e_d]) -- the adjoint of the centred GRADIENT (in = the gradient's output gradient).
template <typename T, bool ADJ>
__global__ __launch_bounds__(kBlock) void cdiv_kernel(DiffOp op, const T* __restrict__ in, T* __restrict__ out) {
    PHIHIP_DIFF_TILE_PROLOGUE
    const T* __restrict__ base = in + (long long)b * op.comps * op.cells;
    const T* __restrict__ I0 = base;                                                 // component along a0 (3-D only)
    const T* __restrict__ I1 = base + (long long)(1 - op.ax0) * op.cells;            // component along a1
    const T* __restrict__ I2 = base + (long long)(2 - op.ax0) * op.cells;            // component along a2
    T* __restrict__ O = out + (long long)b * op.cells;
    const bool edge1 = rule[0] == 1 || rule[1] == 1, edge2 = rule[2] == 1 || rule[3] == 1;
    T cur = has0 ? I0[(long long)p0 * ps + o_c] : T(0);
    T prev = has0 ? diff_plane_nb<T, ADJ>(op, I0, ps, o_c, p0 - 1, cur) : T(0);
    for (int p = p0; p < p1; ++p) {
        const long long po = (long long)p * ps;
        const T next = has0 ? diff_plane_nb<T, ADJ>(op, I0, ps, o_c, p + 1, cur) : T(0);
        const T c1 = edge1 ? I1[po + o_c] : T(0), c2 = edge2 ? I2[po + o_c] : T(0);
        const T lo1 = diff_tap<T, ADJ>(rule[0], I1[po + off[0]], c1, cval[0]), hi1 = diff_tap<T, ADJ>(rule[1], I1[po + off[1]], c1, cval[1]);
        const T lo2 = diff_tap<T, ADJ>(rule[2], I2[po + off[2]], c2, cval[2]), hi2 = diff_tap<T, ADJ>(rule[3], I2[po + off[3]], c2, cval[3]);
        const T acc = w[0] * (next - prev) + w[1] * (hi1 - lo1) + w[2] * (hi2 - lo2);
        if (ADJ) O[po + o_c] -= acc;
        else O[po + o_c] = acc;
        prev = cur;
        cur = next;
    }
}

// ---- curl of a 2-D vector field at the (nx + 1) x (ny + 1) cell corners ------------------------------------------------------------------------
struct CurlOp {
    int nx, ny;            // cells
    int bc[2][2];          // rule of the padding along x / along y
    double val[2][2];      // its constants. Staggered: val[0] pads vy along x, val[1] pads vx along y (the reference takes the OTHER component of a
                           // vector-valued constant there, _field_math.py:655-656: the caller passes it). Centred: the field's constants.
    double rdx, rdy;
    int tiles1, tiles2;    // workgroups along x / along y (64 columns each)
    int chunk;             // forward: rows a wavefront marches over (a workgroup covers 4 chunks); backward: one row per wavefront
};

// index of padded position j on an axis of n samples: >= 0 inside / wrapped / clamped, -1 - side for a constant
__device__ __forceinline__ int curl_pad_index(int j, int n, const int bc[2]) {
    if (j >= 0 && j < n) return j;
    const int side = j < 0 ? 0 : 1;
    if (bc[side] == PHIHIP_BC_PERIODIC) return j < 0 ? j + n : j - n;
    if (bc[side] == PHIHIP_BC_OPEN) return j < 0 ? 0 : n - 1;
    return -1 - side;
}

// !ADJ: a, b = vx, vy -> oa = curl.  ADJ: a = the curl's output gradient C -> oa += d/d vx, ob += d/d vy.
// STAGGERED: vx (nx + 1, ny) and vy (nx, ny + 1) hold all faces; curl = (vy[i, j] - vy[i - 1, j]) / dx - (vx[i, j] - vx[i, j - 1]) / dy with vy padded
// by one along x and vx by one along y. Centred: vx, vy (nx, ny) padded by one cell (x first, then y: the later axis wins in the pad's corners);
// curl = (vx - vy)[ll] - (vx + vy)[ul] + (vx + vy)[lr] - (vx - vy)[ur] over the four cells around the corner, without 1 / dx (as the reference).
template <typename T, bool STAGGERED, bool ADJ>
__global__ __launch_bounds__(kBlock) void curl2d_kernel(CurlOp op, const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ oa, T* __restrict__ ob,
                                                        long long sa, long long sb) {
    const int nx = op.nx, ny = op.ny;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int bid = xcd_order(blockIdx.x, gridDim.x);
    const int j = (bid % op.tiles2) * 64 + tx;
    const long long bt = blockIdx.y;
    const long long sc = (long long)(nx + 1) * (ny + 1);       // batch stride of the corner array
    const T rdx = (T)op.rdx, rdy = (T)op.rdy;
    if (!ADJ) {
        // A 2-D grid has ONE a0 plane, so the ROWS (x) are what is marched here: each of the four wavefronts of the (4 x 64) workgroup owns 64 columns of
        // corners and its own chunk of rows; the samples of row i - 1 stay in registers, every row of vx / vy is loaded once per chunk.
        if (j > ny) return;
        const int r0 = ((bid / op.tiles2) * 4 + ty) * op.chunk, r1 = r0 + op.chunk < nx + 1 ? r0 + op.chunk : nx + 1;
        if (r0 >= r1) return;
        const T* __restrict__ VX = a + bt * sa;
        const T* __restrict__ VY = b + bt * sb;
        T* __restrict__ O = oa + bt * sc;
        const int jh = curl_pad_index(j, ny, op.bc[1]), jl = curl_pad_index(j - 1, ny, op.bc[1]);       // the column taps, resolved once per thread
        if (STAGGERED) {
            auto vy_row = [&](int ip) -> T {
                const int ii = curl_pad_index(ip, nx, op.bc[0]);
                return ii >= 0 ? VY[(long long)ii * (ny + 1) + j] : (T)op.val[0][-1 - ii];
            };
            const T cxh = jh >= 0 ? T(0) : (T)op.val[1][-1 - jh], cxl = jl >= 0 ? T(0) : (T)op.val[1][-1 - jl];
            T vy_lo = vy_row(r0 - 1);
            for (int i = r0; i < r1; ++i) {
                const T vy_hi = vy_row(i);
                const T vx_hi = jh >= 0 ? VX[(long long)i * ny + jh] : cxh;
                const T vx_lo = jl >= 0 ? VX[(long long)i * ny + jl] : cxl;
                O[(long long)i * (ny + 1) + j] = (vy_hi - vy_lo) * rdx - (vx_hi - vx_lo) * rdy;
                vy_lo = vy_hi;
            }
        } else {
            const int jb[2] = {jl, jh};
            // (vx + vy), (vx - vy) of the padded row ip at this corner's two columns [lower / upper]; x is padded first, then y: the later axis wins
            auto row = [&](int ip, T pos[2], T neg[2]) {
                const int ia = curl_pad_index(ip, nx, op.bc[0]);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    T vx, vy;
                    if (jb[q] < 0) vx = vy = (T)op.val[1][-1 - jb[q]];
                    else if (ia < 0) vx = vy = (T)op.val[0][-1 - ia];
                    else { vx = VX[(long long)ia * ny + jb[q]]; vy = VY[(long long)ia * ny + jb[q]]; }
                    pos[q] = vx + vy;
                    neg[q] = vx - vy;
                }
            };
            T pl[2], nl[2], pr[2], nr[2];      // left (row i - 1) and right (row i) cells
            row(r0 - 1, pl, nl);
            for (int i = r0; i < r1; ++i) {
                row(i, pr, nr);
                O[(long long)i * (ny + 1) + j] = ((nl[0] - pl[1]) + pr[0]) - nr[1];
                pl[0] = pr[0]; pl[1] = pr[1]; nl[0] = nr[0]; nl[1] = nr[1];
            }
        }
        return;
    }
    const int i = (bid / op.tiles2) * 4 + ty;
    if (i > nx || j > ny) return;
    const T* __restrict__ C = a + bt * sc;
    auto corner = [&](int ci, int cj) -> T { return (ci >= 0 && ci <= nx && cj >= 0 && cj <= ny) ? C[(long long)ci * (ny + 1) + cj] : T(0); };
    if (STAGGERED) {
        if (i < nx) {        // d/d vy[i, j]: every padded position i' that holds this face is `hi` of corner i' and `lo` of corner i' + 1
            T g = T(0);
            const int cand[3] = {i, -1, nx};
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c == 0 || curl_pad_index(cand[c], nx, op.bc[0]) == i) g += corner(cand[c], j) - corner(cand[c] + 1, j);
            ob[bt * sb + (long long)i * (ny + 1) + j] += g * rdx;
        }
        if (j < ny) {        // d/d vx[i, j]
            T g = T(0);
            const int cand[3] = {j, -1, ny};
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c == 0 || curl_pad_index(cand[c], ny, op.bc[1]) == j) g += corner(i, cand[c]) - corner(i, cand[c] + 1);
            oa[bt * sa + (long long)i * ny + j] -= g * rdy;
        }
    } else {
        if (i >= nx || j >= ny) return;
        T gx = T(0), gy = T(0);
        const int ci[3] = {i, -1, nx}, cj[3] = {j, -1, ny};
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            if (p > 0 && curl_pad_index(ci[p], nx, op.bc[0]) != i) continue;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (q > 0 && curl_pad_index(cj[q], ny, op.bc[1]) != j) continue;
                const int pa = ci[p], pb = cj[q];      // the padded cell (pa, pb) is ll of corner (pa + 1, pb + 1), ul of (pa + 1, pb), lr of (pa, pb + 1), ur of (pa, pb)
                const T c11 = corner(pa + 1, pb + 1), c10 = corner(pa + 1, pb), c01 = corner(pa, pb + 1), c00 = corner(pa, pb);
                gx += ((c11 - c10) + c01) - c00;
                gy += ((c01 - c11) - c10) + c00;
            }
        }
        oa[bt * sa + (long long)i * ny + j] += gx;
        ob[bt * sb + (long long)i * ny + j] += gy;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// planes per workgroup: phihip_set_tuning_kernel(ctx, 0, ., ., chunk) -- the family of the apply-type stencils -- wins over the plan when chunk > 0
static int diff_op(const phihip_ctx* ctx, const GridView& v, const ScalarBc& sb, DiffOp& op) {
    memset(&op, 0, sizeof(op));
    op.ax0 = v.ax0;
    op.comps = 3 - v.ax0;
    op.cells = v.cells;
    for (int a = 0; a < 3; ++a) {
        op.n[a] = v.n[a];
        op.w[a] = a < v.ax0 ? 0.0 : 0.5 / v.dx[a];
        for (int side = 0; side < 2; ++side) {
            op.bc[a][side] = a < v.ax0 ? PHIHIP_BC_PERIODIC : sb.bc[a][side];
            op.val[a][side] = a < v.ax0 ? 0.0 : sb.val[a][side];
        }
    }
    return plan_columns(op.n, kPatchRows, kPatchCols, 4096, ctx->tuning[0].chunk, false, "centred gradient / divergence", op.plan);      // ~4096 workgroups per batch entry when the grid allows
}

static inline dim3 diff_grid(const DiffOp& op, int batch) {
    return dim3((unsigned)((long long)op.plan.tiles1 * op.plan.tiles2 * op.plan.chunks), batch);
}

static int diff_check(const GridView& v, const char* what) {
    if (v.cells >= (1LL << 31) / 4) { set_error("%s: more than 2^29 cells per batch entry are not supported", what); return PHIHIP_ERR_UNSUPPORTED; }
    if (v.rank < 2) { set_error("%s: 2-D and 3-D grids only", what); return PHIHIP_ERR_UNSUPPORTED; }
    return PHIHIP_OK;
}

// one scalar -> components: the centred gradient (adjoint == 0) or the adjoint of the centred divergence (accumulated)
int run_cgrad(phihip_ctx* ctx, const GridView& v, const void* in, const int32_t s_bc[3][2], const double s_val[3][2], void* out, int adjoint, hipStream_t s) {
    PHIHIP_TRY(diff_check(v, adjoint ? "divergence_centered_backward" : "gradient_centered"));
    DiffOp op;
    PHIHIP_TRY(diff_op(ctx, v, make_scalar_bc(v, s_bc, s_val), op));
    LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
    const dim3 grid = diff_grid(op, v.batch);
    with_dtype(v, [&](auto t) {
        using T = typename decltype(t)::type;
        if (adjoint) hipLaunchKernelGGL((cgrad_kernel<T, true>), grid, dim3(kBlock), 0, s, op, (const T*)in, (T*)out);
        else hipLaunchKernelGGL((cgrad_kernel<T, false>), grid, dim3(kBlock), 0, s, op, (const T*)in, (T*)out);
    });
    PHIHIP_CHECK_HIP(hipGetLastError());
    return PHIHIP_OK;
}

// components -> one scalar: the centred divergence (adjoint == 0) or the adjoint of the centred gradient (accumulated)
int run_cdiv(phihip_ctx* ctx, const GridView& v, const void* in, const int32_t s_bc[3][2], const double s_val[3][2], void* out, int adjoint, hipStream_t s) {
    PHIHIP_TRY(diff_check(v, adjoint ? "gradient_centered_backward" : "divergence_centered"));
    DiffOp op;
    PHIHIP_TRY(diff_op(ctx, v, make_scalar_bc(v, s_bc, s_val), op));
    LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
    const dim3 grid = diff_grid(op, v.batch);
    with_dtype(v, [&](auto t) {
        using T = typename decltype(t)::type;
        if (adjoint) hipLaunchKernelGGL((cdiv_kernel<T, true>), grid, dim3(kBlock), 0, s, op, (const T*)in, (T*)out);
        else hipLaunchKernelGGL((cdiv_kernel<T, false>), grid, dim3(kBlock), 0, s, op, (const T*)in, (T*)out);
    });
    PHIHIP_CHECK_HIP(hipGetLastError());
    return PHIHIP_OK;
}

template <typename T, bool STAGGERED>
static void launch_curl(const CurlOp& op, int batch, bool adjoint, const void* a, const void* b, void* oa, void* ob, hipStream_t s) {
    const dim3 grid((unsigned)(op.tiles1 * op.tiles2), batch);
    const long long cells = (long long)op.nx * op.ny;
    const long long sa = STAGGERED ? (long long)(op.nx + 1) * op.ny : 2 * cells, sb = STAGGERED ? (long long)op.nx * (op.ny + 1) : 2 * cells;
    if (adjoint) hipLaunchKernelGGL((curl2d_kernel<T, STAGGERED, true>), grid, dim3(kBlock), 0, s, op, (const T*)a, (const T*)b, (T*)oa, (T*)ob, sa, sb);
    else hipLaunchKernelGGL((curl2d_kernel<T, STAGGERED, false>), grid, dim3(kBlock), 0, s, op, (const T*)a, (const T*)b, (T*)oa, (T*)ob, sa, sb);
}

// forward: a, b = vx, vy, oa = the corner array. adjoint: a = the corner array's gradient, oa / ob = the accumulated gradients of vx / vy.
// Centred fields are one (batch, 2, nx, ny) array: b (ob) is a (oa) + nx * ny.
int run_curl2d(phihip_ctx* ctx, const GridView& v, int staggered, const int32_t s_bc[3][2], const double s_val[3][2], int adjoint, const void* a, const void* b,
               void* oa, void* ob, hipStream_t s) {
    if (v.rank != 2) { set_error("curl_2d: 2-D grids only"); return PHIHIP_ERR_UNSUPPORTED; }
    if (v.cells >= (1LL << 29)) { set_error("curl_2d: more than 2^29 cells per batch entry are not supported"); return PHIHIP_ERR_UNSUPPORTED; }
    CurlOp op;
    memset(&op, 0, sizeof(op));
    op.nx = v.n[1];
    op.ny = v.n[2];
    for (int d = 0; d < 2; ++d)
        for (int side = 0; side < 2; ++side) {
            op.bc[d][side] = s_bc[d][side];
            op.val[d][side] = s_val ? s_val[d][side] : 0.0;
        }
    op.rdx = 1.0 / v.dx[1];
    op.rdy = 1.0 / v.dx[2];
    op.tiles2 = ceil_div(op.ny + 1, 64);
    op.chunk = 1;
    if (!adjoint) {        // ~4096 workgroups of four row chunks when the grid allows
        int chunks = 16384 / op.tiles2;
        chunks = chunks > op.nx + 1 ? op.nx + 1 : (chunks < 1 ? 1 : chunks);
        op.chunk = ceil_div(op.nx + 1, chunks);
        if (ctx->tuning[0].chunk > 0) op.chunk = ctx->tuning[0].chunk < op.nx + 1 ? ctx->tuning[0].chunk : op.nx + 1;      // (as diff_op: an explicit setting wins)
    }
    op.tiles1 = ceil_div(ceil_div(op.nx + 1, op.chunk), 4);
    LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
    with_dtype(v, [&](auto t) {
        using T = typename decltype(t)::type;
        if (staggered) launch_curl<T, true>(op, v.batch, adjoint != 0, a, b, oa, ob, s);
        else launch_curl<T, false>(op, v.batch, adjoint != 0, a, b, oa, ob, s);
    });
    PHIHIP_CHECK_HIP(hipGetLastError());
    return PHIHIP_OK;
}

// ---- laplace ---------------------------------------------------------------------------------------------------------------------------------
// coef_kernel<CM_LAP> on one lattice (a centred scalar or one staggered component, described as component `ca` of g): out = L_w in with the lattice's
// own extrapolation, or out += L_w^hom in (accumulate: the backward pass -- the operator is symmetric, the wall constants do not depend on the input)
static int laplace_coef_lattice(phihip_ctx* ctx, const GridView& v, const VelGrid& g, int ca, const double wgt[3], const void* in, void* out, int accumulate,
                                hipStream_t s) {
    CoefOp op;
    memset(&op, 0, sizeof(op));
    op.ax0 = v.ax0;
    op.cells = g.ccells[ca];
    for (int a = 0; a < 3; ++a) {
        op.n[a] = g.cn[ca][a];
        op.w[a] = a < v.ax0 ? 0.0 : wgt[a] / (v.dx[a] * v.dx[a]);
        for (int side = 0; side < 2; ++side) {
            op.ubc[a][side] = a < v.ax0 ? PHIHIP_BC_PERIODIC : g.bc[a][side];
            op.uval[a][side] = (a >= v.ax0 && g.bc[a][side] == PHIHIP_BC_CLOSED && !accumulate) ? g.bcv[a][side][ca] : 0.0;
            op.cbc[a][side] = a < v.ax0 ? PHIHIP_BC_PERIODIC : PHIHIP_BC_OPEN;       // no coefficient array: 1 everywhere, ghosts included
            op.cval[a][side] = 1.0;
        }
    }
    if (op.cells >= (1LL << 31)) { set_error("laplace: more than 2^31 samples per batch entry are not supported"); return PHIHIP_ERR_UNSUPPORTED; }
    PHIHIP_TRY(coef_plan(op, 4096, "laplace"));
    LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
    return with_dtype(v, [&](auto t) {
        using T = typename decltype(t)::type;
        CoefArgs<T> a;
        memset(&a, 0, sizeof(a));
        a.a = (const T*)in; a.o1 = (T*)out; a.accumulate = accumulate;
        return coef_launch<T, CM_LAP>(op, v.batch, a, s);
    });
}

// laplace of a centred scalar, weights per INTERNAL axis. A uniform weight runs the marching kernels (diffuse.explicit's pass with ident = 0);
// per-axis weights and the backward pass run coef_kernel<CM_LAP>.
int run_field_laplace_centered(phihip_ctx* ctx, const GridView& v, const void* sfield, const int32_t s_bc[3][2], const double s_val[3][2], const double wgt[3],
                               void* out, int adjoint, hipStream_t s) {
    const ScalarBc sb = make_scalar_bc(v, s_bc, s_val);
    const VelGrid g = scalar_as_component(v, sb);
    if (v.cells >= (1LL << 31)) { set_error("laplace: more than 2^31 cells per batch entry are not supported"); return PHIHIP_ERR_UNSUPPORTED; }
    bool uniform = true;
    for (int a = v.ax0; a < 3; ++a) uniform = uniform && wgt[a] == wgt[v.ax0];
    if (adjoint || !uniform) return laplace_coef_lattice(ctx, v, g, 2, wgt, sfield, out, adjoint ? 1 : 0, s);
    bool affine;
    const GridView w = lattice_view(v, g, 2, 0.0, wgt[v.ax0], &affine);
    PHIHIP_TRY(run_laplace_apply(ctx, w, nullptr, 1, sfield, out, s));
    if (affine) PHIHIP_TRY(diffuse_affine_walls(ctx, v, g, 2, out, wgt[v.ax0], s));
    return PHIHIP_OK;
}

// laplace of every component of a staggered field on its own face lattice with that component's wall constants (run_diffuse with ident = 0)
int run_field_laplace(phihip_ctx* ctx, const GridView& v, const void* const vin[3], void* const vout[3], double weight, int adjoint, hipStream_t s) {
    const VelGrid g = make_velgrid(v);
    if (adjoint) {
        const double wgt[3] = {weight, weight, weight};
        for (int ca = v.ax0; ca < 3; ++ca) PHIHIP_TRY(laplace_coef_lattice(ctx, v, g, ca, wgt, vin[ca], vout[ca], 1, s));
        return PHIHIP_OK;
    }
    GridView w[3];
    const void* in[3];
    void* out[3];
    bool affine[3] = {false, false, false};
    int count = 0;
    for (int ca = v.ax0; ca < 3; ++ca) {
        w[count] = lattice_view(v, g, ca, 0.0, weight, &affine[ca]);
        if (w[count].cells >= (1LL << 31)) { set_error("laplace: more than 2^31 samples per component and batch entry are not supported"); return PHIHIP_ERR_UNSUPPORTED; }
        in[count] = vin[ca];
        out[count] = vout[ca];
        ++count;
    }
    PHIHIP_TRY(run_laplace_apply_multi(ctx, w, count, in, out, s));
    for (int ca = v.ax0; ca < 3; ++ca)
        if (affine[ca]) PHIHIP_TRY(diffuse_affine_walls(ctx, v, g, ca, vout[ca], weight, s));
    return PHIHIP_OK;
}

}  // namespace phihip
