// momentum.hpp -- the finite-difference advection term -(v . grad) u of phi/physics/advect.py:78-133 (`advect.differential`), order 2:
//   staggered u, staggered velocity on the same grid and boundary (:108-116)     out_c[f] = -sum_d W_d(f) (U_c[f + e_d] - U_c[f - e_d]) / (2 dx_d)
//   centred vector u, centred vector velocity on the same grid (:117-124)         out_c[i] = -sum_d V_d[i] (U_c[i + e_d] - U_c[i - e_d]) / (2 dx_d)
// U_c = component c padded by one sample with its own extrapolation (what field.laplace pads a component with): PERIODIC wraps, OPEN (zero-gradient)
// copies the edge sample, CLOSED is that component's constant. Staggered: W_c(f) = V_c[f]; for d != c, W_d(f) is the mean of the four d-faces around
// the c-face f (`vel.at(grad)`, phi/field/_resample.py:279-287, 341-364), a missing face taken from the velocity's padding -- along d a face that is
// not stored is the wall constant or the wrapped face 0, along c the cell beyond the lattice wraps or copies the edge cell.
// Included by project.hip (the emulation build of the tests compiles the .hip files by name: no translation unit of its own).
// The run_* functions pick mom_run<T, STAG> with with_dtype (common.hpp): STAG is a constant of the entry point, mom_run picks the rank.
//
// THE ARITHMETIC, the same in the 2-D and 3-D instantiations (the rounding count K of tests/momentum_cases.py is counted from it), h_d = (T)(0.5 / dx_d):
//     g_d = U_c[f + e_d] - U_c[f - e_d]                                    1 rounding
//     W_d = V_c[f]                              (d == c, and centred)      exact
//         = ((a11 + a01) + (a10 + a00)) * 0.25  (d != c)                   3 roundings; the first index runs along the lower of the axes (c, d): the
//                                                                          reference's lerp order, hi * 0.5 + lo * 0.5 axis after axis, gives the same bits
//     t_d = W_d * h_d                                                      1 rounding (+ 1 of the constant h_d)
//     acc = t_x * g_x;  acc = fma(t_y, g_y, acc);  [acc = fma(t_z, g_z, acc)]      axis order x, y[, z]: D roundings on the first term's path
//     out = -acc                                                           exact
// A term carries at most 1 + 3 + 2 roundings in its factors (+ 1 per wall constant cast to T, at most 2) and D in the sum: (8 + D) eps / 2 of
// S = sum_d mean|V| (|U_hi| + |U_lo|) h_d.
//
// Form kept: the column march of column_march.hpp (its launch plan and tile decode) over ONE component's lattice, a chunk of a0 planes per workgroup;
// blockIdx.y = batch entry, blockIdx.z = component, so one launch covers everything and every output sample is written once by one thread. The a0
// neighbours of U_c are carried in registers (prev / cur / next, as cgrad_kernel does); the in-plane tap offsets are loop-invariant. The velocity taps
// of the four-face means are NOT carried: they are re-read per plane (the thread read them one plane earlier, they come from L1 / L2). No LDS, no atomics.
//
// Backward: two gathers (no atomics), gradients ACCUMULATE. With P_d[f] = G_c[f] W_d(f):
//     grad u_c[j]  -= sum_d h_d (T_d[j - e_d] - T_d[j + e_d])      T = P with the ADJOINT tap rule of diffops.hpp outside the lattice (wrapped: the wrapped
//                                                                   neighbour's P; clamped: -P[j]; constant: 0)
//     grad v_d[k]  -= h_d G_d[k] g_dd(k) + h_d / 4 sum over the c-faces f (c != d) whose four-face mean reads face k (every padded position that resolves to
//                     k counted) of G_c[f] g_cd(f)                  (centred: -= h_d sum_c G_c[k] g_cd(k))
#pragma once

namespace phihip {

struct MomOp {
    int ax0, comps;
    int n[3];               // cells per internal axis (n[0] == 1 for 2-D grids)
    int cn[3][3];           // [component][axis] samples of the component's lattice (centred: the cells)
    int off[3];             // physical face number of stored index 0 along the component's own axis (centred: 0)
    long long cc[3];        // samples per component lattice
    long long bs_u[3], bs_v[3], bs_o[3];   // batch strides in elements (0: a batch of 1 shared by every entry)
    int bc[3][2];           // the extrapolation per internal axis / side (staggered: of u and of the velocity; centred: of u)
    double val[3][2][3];    // [axis][side][component] constants of CLOSED sides
    double h[3];            // 0.5 / dx_a
    ColumnPlan plan;
};

template <typename T>
struct MomPtrs {
    const T* u[3];          // per internal axis (component); unused axis: nullptr
    const T* v[3];
    const T* g[3];          // backward: the output gradient
    T* o[3];                // forward: out; backward: the gradient being accumulated
};

// position j on an axis of n samples -> index inside the array (wrapped / clamped), or -1 - side for a constant. The two codes come in as values (and the
// constants below are picked by a select): a per-lane index into the by-value MomOp would make the compiler keep a copy of it in scratch.
__device__ __forceinline__ int mom_index(int j, int n, int bc_lo, int bc_hi) {
    if (j >= 0 && j < n) return j;
    const bool up = j >= n;
    const int code = up ? bc_hi : bc_lo;
    if (code == PHIHIP_BC_PERIODIC) { j %= n; return j < 0 ? j + n : j; }
    if (code == PHIHIP_BC_OPEN) return up ? n - 1 : 0;
    return up ? -2 : -1;
}

__device__ __forceinline__ long long mom_offset(const int L[3], int i0, int i1, int i2) {
    return ((long long)i0 * L[1] + i1) * L[2] + i2;
}

// sample of U_c at idx + dir * e_a on the lattice of component c, padded with the component's own rule
template <typename T>
__device__ __forceinline__ T mom_utap(const MomOp& op, const T* __restrict__ U, int c, const int idx[3], int a, int dir) {
    const T c_lo = (T)op.val[a][0][c], c_hi = (T)op.val[a][1][c];       // (both read up front: see mom_index)
    const int j = mom_index(idx[a] + dir, op.cn[c][a], op.bc[a][0], op.bc[a][1]);
    if (j < 0) return j == -1 ? c_lo : c_hi;
    return U[mom_offset(op.cn[c], a == 0 ? j : idx[0], a == 1 ? j : idx[1], a == 2 ? j : idx[2])];
}

// g_cd(f) = U_c[f + e_d] - U_c[f - e_d]
template <typename T>
__device__ __forceinline__ T mom_udiff(const MomOp& op, const T* __restrict__ U, int c, const int idx[3], int d) {
    return mom_utap<T>(op, U, c, idx, d, 1) - mom_utap<T>(op, U, c, idx, d, -1);
}

// W_d at the stored face idx of component c (d != c): mean of the four d-faces around it
template <typename T>
__device__ __forceinline__ T mom_mean4(const MomOp& op, const T* __restrict__ Vd, int c, int d, const int idx[3]) {
    const int m = idx[c] + op.off[c];               // physical face number along c
    T a[2][2];                                      // [position along d][position along c]
    // one pad per axis in spatial order: the later axis wins where both are constants
    const int hi = c > d ? c : d, lo = c > d ? d : c;
    const T ch0 = (T)op.val[hi][0][d], ch1 = (T)op.val[hi][1][d], cl0 = (T)op.val[lo][0][d], cl1 = (T)op.val[lo][1][d];
#pragma unroll
    for (int pd = 0; pd < 2; ++pd)
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {
            const int s = mom_index(idx[d] + pd - op.off[d], op.cn[d][d], op.bc[d][0], op.bc[d][1]);      // stored face along d
            const int q = mom_index(m - 1 + pc, op.cn[d][c], op.bc[c][0], op.bc[c][1]);                   // cell along c
            int pos[3] = {idx[0], idx[1], idx[2]};
            pos[d] = s;
            pos[c] = q;
            if (pos[hi] < 0) a[pd][pc] = pos[hi] == -1 ? ch0 : ch1;
            else if (pos[lo] < 0) a[pd][pc] = pos[lo] == -1 ? cl0 : cl1;
            else a[pd][pc] = Vd[mom_offset(op.cn[d], pos[0], pos[1], pos[2])];
        }
    // lerp along the lower axis first: [first index along the lower axis]
    if (d < c) return ((a[1][1] + a[0][1]) + (a[1][0] + a[0][0])) * T(0.25);
    return ((a[1][1] + a[1][0]) + (a[0][1] + a[0][0])) * T(0.25);
}

#define PHIHIP_MOM_PROLOGUE                                                                         \
    constexpr int A0 = 3 - D;                                                                       \
    constexpr int c = C;                                                                            \
    constexpr int lat = STAG ? C : 2;      /* the components of a centred field share one lattice */ \
    const long long b = blockIdx.y;                                                                 \
    ColumnTile ct = column_tile(op.plan, op.cn[lat][1], op.cn[lat][2], xcd_order(blockIdx.x, gridDim.x)); \
    if (!ct.inside || !column_planes(op.plan, ct, op.cn[lat][0])) return;                           \
    const int i1 = ct.i1, i2 = ct.i2, p0 = ct.p0, p1 = ct.p1;                                       \
    T h[3];                                                                                         \
    _Pragma("unroll") for (int ax = 0; ax < 3; ++ax) h[ax] = (T)op.h[ax];

// The component is a template parameter (the kernels branch on blockIdx.z, a uniform branch): every index into the small per-thread arrays is a
// compile-time constant after unrolling, so they stay in registers. Every tap is resolved ONCE per thread as far as it lies in the plane -- a safe offset that
// is always loaded from, and the constant that replaces the loaded value at a CLOSED side (the pattern of diff_plane_taps / diff_tap: unconditional loads and
// selects, no branch around a load) -- and per plane along a0, where the decision is uniform over the workgroup.
template <typename T, int D, bool STAG, int C>
__device__ __forceinline__ void mom_forward(const MomOp& op, const MomPtrs<T>& P) {
    PHIHIP_MOM_PROLOGUE
    const int L0 = op.cn[lat][0], L2 = op.cn[lat][2];
    const int o_c = i1 * L2 + i2;
    const long long ps = (long long)op.cn[lat][1] * L2;
    const T* __restrict__ U = P.u[c] + b * op.bs_u[c];
    T* __restrict__ O = P.o[c] + b * op.bs_o[c];
    const int ii[3] = {0, i1, i2};
    // in-plane taps of U_c: k = 2 * (axis - 1) + side
    int uoff[4];
    bool ucst[4];
    T ucv[4];
#pragma unroll
    for (int a = 1; a < 3; ++a)
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int k = 2 * (a - 1) + side;
            const T c_lo = (T)op.val[a][0][lat], c_hi = (T)op.val[a][1][lat];
            const int j = mom_index(ii[a] + (side ? 1 : -1), op.cn[lat][a], op.bc[a][0], op.bc[a][1]);
            ucst[k] = j < 0;
            ucv[k] = j == -1 ? c_lo : c_hi;
            uoff[k] = o_c + (j < 0 ? 0 : (j - ii[a]) * (a == 1 ? L2 : 1));
        }
    // the four-face means: tap t = 2 * pd + pc of W_d (pd: position along d, pc: position along c), its in-plane part
    int moff[3][4];
    bool mcst[3][4];
    T mcv[3][4];
    if (STAG) {
#pragma unroll
        for (int d = A0; d < 3; ++d) {
            if (d == c) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int pd = t >> 1, pc = t & 1;
                int pos[3] = {0, i1, i2};
                bool cst = false;
                T cv = T(0);
#pragma unroll
                for (int a = 1; a < 3; ++a) {        // (a = 2 after a = 1: the later axis wins where both are constants)
                    if (a != d && a != c) continue;
                    const int comp_of_const = d;
                    const T c_lo = (T)op.val[a][0][comp_of_const], c_hi = (T)op.val[a][1][comp_of_const];
                    const int j = a == d ? mom_index(ii[a] + pd - op.off[d], op.cn[d][d], op.bc[a][0], op.bc[a][1])
                                         : mom_index(ii[a] + op.off[c] - 1 + pc, op.cn[d][c], op.bc[a][0], op.bc[a][1]);
                    pos[a] = j < 0 ? 0 : j;
                    if (j < 0) { cst = true; cv = j == -1 ? c_lo : c_hi; }
                }
                moff[d][t] = pos[1] * op.cn[d][2] + pos[2];
                mcst[d][t] = cst;
                mcv[d][t] = cv;
            }
        }
    }
    // a0: the plane pp of U_c (a uniform decision)
    const T u0_lo = (T)op.val[0][0][lat], u0_hi = (T)op.val[0][1][lat];
    auto u_plane = [&](int pp) -> T {
        const int j = mom_index(pp, L0, op.bc[0][0], op.bc[0][1]);
        return j < 0 ? (j == -1 ? u0_lo : u0_hi) : U[(long long)j * ps + o_c];
    };
    // the a0 neighbours of U_c stay in registers (3-D only)
    T cur = U[(long long)p0 * ps + o_c];
    T prev = D == 3 ? u_plane(p0 - 1) : T(0);
    for (int p = p0; p < p1; ++p) {
        const long long po = (long long)p * ps;
        const T next = D == 3 ? u_plane(p + 1) : T(0);
        T tap[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const T loaded = U[po + uoff[k]];
            tap[k] = ucst[k] ? ucv[k] : loaded;
        }
        T acc = T(0);
#pragma unroll
        for (int d = A0; d < 3; ++d) {
            const T g = d == 0 ? next - prev : tap[2 * (d - 1) + 1] - tap[2 * (d - 1)];
            T W;
            if (!STAG || d == c) {
                W = (P.v[d] + b * op.bs_v[d])[po + o_c];
            } else {
                const T* __restrict__ Vd = P.v[d] + b * op.bs_v[d];
                const long long psd = (long long)op.cn[d][1] * op.cn[d][2];
                T a[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int pd = t >> 1, pc = t & 1;
                    // the plane of this tap: along a0 it is the face (d == 0) or the cell (c == 0) position, else the thread's plane
                    int pl = p;
                    T pcv = T(0);
                    if (d == 0 || c == 0) {
                        const T c_lo = (T)op.val[0][0][d], c_hi = (T)op.val[0][1][d];
                        pl = d == 0 ? mom_index(p + pd - op.off[0], op.cn[0][0], op.bc[0][0], op.bc[0][1])
                                    : mom_index(p + op.off[0] - 1 + pc, op.cn[d][0], op.bc[0][0], op.bc[0][1]);
                        pcv = pl == -1 ? c_lo : c_hi;
                    }
                    const T loaded = Vd[(long long)(pl < 0 ? 0 : pl) * psd + moff[d][t]];
                    a[t] = mcst[d][t] ? mcv[d][t] : (pl < 0 ? pcv : loaded);
                }
                // a[2 * pd + pc]; the lerp runs along the lower of the axes (c, d) first
                W = d < c ? ((a[3] + a[1]) + (a[2] + a[0])) * T(0.25) : ((a[3] + a[2]) + (a[1] + a[0])) * T(0.25);
            }
            const T t = W * h[d];
            acc = d == A0 ? t * g : fma(t, g, acc);
        }
        O[po + o_c] = -acc;
        prev = cur;
        cur = next;
    }
}

#define PHIHIP_MOM_PER_COMPONENT(fn)                                         \
    if (blockIdx.z == 0) fn<T, D, STAG, 3 - D>(op, P);                       \
    else if (blockIdx.z == 1) fn<T, D, STAG, 4 - D>(op, P);                  \
    else if (D == 3) fn<T, D, STAG, 2>(op, P);

template <typename T, int D>
__global__ __launch_bounds__(kBlock) void advect_diff_staggered_kernel(MomOp op, MomPtrs<T> P) {
    constexpr bool STAG = true;
    PHIHIP_MOM_PER_COMPONENT(mom_forward)
}

template <typename T, int D>
__global__ __launch_bounds__(kBlock) void advect_diff_centered_kernel(MomOp op, MomPtrs<T> P) {
    constexpr bool STAG = false;
    PHIHIP_MOM_PER_COMPONENT(mom_forward)
}

// P_d[f] = G_c[f] W_d(f) on the lattice of component c
template <typename T, bool STAG>
__device__ __forceinline__ T mom_gw(const MomOp& op, const T* __restrict__ G, const T* __restrict__ Vd, int c, int d, const int idx[3]) {
    const long long o = mom_offset(op.cn[c], idx[0], idx[1], idx[2]);
    const T W = (STAG && d != c) ? mom_mean4<T>(op, Vd, c, d, idx) : Vd[o];
    return G[o] * W;
}

// grad u: one thread per sample of u_c; o[c] += ...
template <typename T, int D, bool STAG, int C>
__device__ __forceinline__ void mom_grad_u(const MomOp& op, const MomPtrs<T>& P) {
    PHIHIP_MOM_PROLOGUE
    const T* __restrict__ G = P.g[c] + b * op.bs_o[c];
    const T* V[3];
#pragma unroll
    for (int d = A0; d < 3; ++d) V[d] = P.v[d] + b * op.bs_v[d];
    T* __restrict__ O = P.o[c] + b * op.bs_o[c];
    for (int p = p0; p < p1; ++p) {
        const int idx[3] = {p, i1, i2};
        T acc = T(0);
#pragma unroll
        for (int d = A0; d < 3; ++d) {
            T tap[2];
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const int j = idx[d] + (side ? 1 : -1), n = op.cn[c][d];
                int f[3] = {idx[0], idx[1], idx[2]};
                T sign = T(1);
                bool zero = false;
                if (j < 0 || j >= n) {
                    const int code = op.bc[d][side];
                    if (code == PHIHIP_BC_PERIODIC) f[d] = mom_index(j, n, op.bc[d][0], op.bc[d][1]);
                    else if (code == PHIHIP_BC_OPEN) sign = T(-1);           // the clamped tap returns its weight to the edge sample: f = idx
                    else zero = true;
                } else f[d] = j;
                tap[side] = zero ? T(0) : sign * mom_gw<T, STAG>(op, G, V[d], c, d, f);
            }
            acc = fma(h[d], tap[0] - tap[1], acc);
        }
        O[mom_offset(op.cn[c], p, i1, i2)] -= acc;
    }
}

// grad velocity: one thread per sample of v_c (here c names the VELOCITY component, i.e. the axis d of the header comment)
template <typename T, int D, bool STAG, int C>
__device__ __forceinline__ void mom_grad_v(const MomOp& op, const MomPtrs<T>& P) {
    PHIHIP_MOM_PROLOGUE
    constexpr int d = C;
    const T* U[3];
    const T* G[3];
#pragma unroll
    for (int e = A0; e < 3; ++e) { U[e] = P.u[e] + b * op.bs_u[e]; G[e] = P.g[e] + b * op.bs_o[e]; }
    T* __restrict__ O = P.o[d] + b * op.bs_o[d];
    for (int p = p0; p < p1; ++p) {
        const int k[3] = {p, i1, i2};
        const long long o = mom_offset(op.cn[d], p, i1, i2);
        T acc = T(0);
        if (!STAG) {
#pragma unroll
            for (int e = A0; e < 3; ++e) acc = fma(G[e][o], mom_udiff<T>(op, U[e], e, k, d), acc);
            O[o] -= h[d] * acc;
            continue;
        }
        acc = G[d][o] * mom_udiff<T>(op, U[d], d, k, d);
        T sum = T(0);
#pragma unroll
        for (int e = A0; e < 3; ++e) {
            if (e == d) continue;
            // padded positions (face jp along d, cell qp along e) of the velocity's padding that resolve to the stored sample k
            const int jd = k[d] + op.off[d];
            for (int a = 0; a < 2; ++a) {
                const int jp = a == 0 ? jd : jd + op.n[d];
                if (a == 1 && (jp > op.n[d] || mom_index(jp - op.off[d], op.cn[d][d], op.bc[d][0], op.bc[d][1]) != k[d])) continue;
                for (int q = 0; q < 3; ++q) {
                    const int qp = q == 0 ? k[e] : (q == 1 ? -1 : op.n[e]);
                    if (q > 0 && mom_index(qp, op.n[e], op.bc[e][0], op.bc[e][1]) != k[e]) continue;
                    // the e-faces whose mean reads (jp, qp): cell fd along d with the face in {fd, fd + 1}, physical face m along e with the cell in {m - 1, m}
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int fd = jp - 1 + s;
                        if (fd < 0 || fd >= op.n[d]) continue;
#pragma unroll
                        for (int r = 0; r < 2; ++r) {
                            const int fe = qp + r - op.off[e];
                            if (fe < 0 || fe >= op.cn[e][e]) continue;
                            int f[3] = {k[0], k[1], k[2]};
                            f[d] = fd;
                            f[e] = fe;
                            sum = fma(G[e][mom_offset(op.cn[e], f[0], f[1], f[2])], mom_udiff<T>(op, U[e], e, f, d), sum);
                        }
                    }
                }
            }
        }
        acc = fma(T(0.25), sum, acc);
        O[o] -= h[d] * acc;
    }
}

template <typename T, int D, bool STAG>
__global__ __launch_bounds__(kBlock) void advect_diff_grad_u_kernel(MomOp op, MomPtrs<T> P) { PHIHIP_MOM_PER_COMPONENT(mom_grad_u) }

template <typename T, int D, bool STAG>
__global__ __launch_bounds__(kBlock) void advect_diff_grad_v_kernel(MomOp op, MomPtrs<T> P) { PHIHIP_MOM_PER_COMPONENT(mom_grad_v) }

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
static int mom_plan(const phihip_ctx* ctx, MomOp& op, const char* what) {
    int L[3] = {1, 1, 1};
    for (int c = op.ax0; c < 3; ++c) {
        if (op.cc[c] >= (1LL << 31)) { set_error("%s: more than 2^31 samples per component and batch entry are not supported", what); return PHIHIP_ERR_UNSUPPORTED; }
        for (int a = 0; a < 3; ++a) L[a] = op.cn[c][a] > L[a] ? op.cn[c][a] : L[a];
    }
    return plan_columns(L, kPatchRows, kPatchCols, 4096, ctx->tuning[0].chunk, false, what, op.plan);      // ~4096 workgroups per batch entry and component; an explicit setting wins
}

static MomOp mom_op_staggered(const GridView& v) {
    MomOp op;
    memset(&op, 0, sizeof(op));
    op.ax0 = v.ax0;
    op.comps = v.rank;
    for (int a = 0; a < 3; ++a) {
        op.n[a] = v.n[a];
        op.off[a] = a < v.ax0 ? 0 : v.off[a];
        op.cc[a] = v.ccells[a];
        op.h[a] = a < v.ax0 ? 0.0 : 0.5 / v.dx[a];
        for (int e = 0; e < 3; ++e) op.cn[a][e] = v.cn[a][e];
        for (int side = 0; side < 2; ++side) {
            op.bc[a][side] = v.bc[a][side];
            for (int e = 0; e < 3; ++e) op.val[a][side][e] = v.bcv[a][side][e];
        }
    }
    return op;
}

static MomOp mom_op_centered(const GridView& v, const ScalarBc& sb) {
    MomOp op;
    memset(&op, 0, sizeof(op));
    op.ax0 = v.ax0;
    op.comps = v.rank;
    for (int a = 0; a < 3; ++a) {
        op.n[a] = v.n[a];
        op.cc[a] = v.cells;
        op.h[a] = a < v.ax0 ? 0.0 : 0.5 / v.dx[a];
        for (int e = 0; e < 3; ++e) op.cn[a][e] = v.n[e];
        for (int side = 0; side < 2; ++side) {
            op.bc[a][side] = a < v.ax0 ? PHIHIP_BC_PERIODIC : sb.bc[a][side];
            for (int e = 0; e < 3; ++e) op.val[a][side][e] = a < v.ax0 ? 0.0 : sb.val[a][side];
        }
    }
    return op;
}

// which: 0 forward, 1 grad u, 2 grad velocity
template <typename T, int D, bool STAG>
static void mom_launch(const MomOp& op, int batch, int which, const MomPtrs<T>& P, hipStream_t s) {
    const dim3 grid((unsigned)((long long)op.plan.tiles1 * op.plan.tiles2 * op.plan.chunks), (unsigned)batch, (unsigned)D);
    if (which == 1) hipLaunchKernelGGL((advect_diff_grad_u_kernel<T, D, STAG>), grid, dim3(kBlock), 0, s, op, P);
    else if (which == 2) hipLaunchKernelGGL((advect_diff_grad_v_kernel<T, D, STAG>), grid, dim3(kBlock), 0, s, op, P);
    else if (STAG) hipLaunchKernelGGL((advect_diff_staggered_kernel<T, D>), grid, dim3(kBlock), 0, s, op, P);
    else hipLaunchKernelGGL((advect_diff_centered_kernel<T, D>), grid, dim3(kBlock), 0, s, op, P);
}

template <typename T, bool STAG>
static int mom_run(phihip_ctx* ctx, const GridView& v, const MomOp& op, int which, const void* const u[3], const void* const vel[3], const void* const g[3],
                   void* const o[3], hipStream_t s) {
    MomPtrs<T> P;
    for (int a = 0; a < 3; ++a) {
        P.u[a] = u ? (const T*)u[a] : nullptr;
        P.v[a] = vel ? (const T*)vel[a] : nullptr;
        P.g[a] = g ? (const T*)g[a] : nullptr;
        P.o[a] = (T*)o[a];
    }
    LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
    if (v.rank == 3) mom_launch<T, 3, STAG>(op, v.batch, which, P, s);
    else mom_launch<T, 2, STAG>(op, v.batch, which, P, s);
    PHIHIP_CHECK_HIP(hipGetLastError());
    return PHIHIP_OK;
}

// staggered: u / vel / out per internal axis; a batch of 1 on either input side is shared (u_batch / vel_batch: 1 or v.batch)
int run_advect_differential(phihip_ctx* ctx, const GridView& v, const void* const u[3], int u_batch, const void* const vel[3], int vel_batch, void* const out[3],
                            hipStream_t s) {
    MomOp op = mom_op_staggered(v);
    PHIHIP_TRY(mom_plan(ctx, op, "advect_differential"));
    for (int c = 0; c < 3; ++c) {
        op.bs_u[c] = u_batch == 1 ? 0 : op.cc[c];
        op.bs_v[c] = vel_batch == 1 ? 0 : op.cc[c];
        op.bs_o[c] = op.cc[c];
    }
    return with_dtype(v, [&](auto t) { return mom_run<typename decltype(t)::type, true>(ctx, v, op, 0, u, vel, nullptr, out, s); });
}

// gradients accumulate; gu / gv may be NULL (that gradient is not wanted). Every array has v.batch entries.
int run_advect_differential_bwd(phihip_ctx* ctx, const GridView& v, const void* const u[3], const void* const vel[3], const void* const gout[3], void* const gu[3],
                                void* const gv[3], hipStream_t s) {
    MomOp op = mom_op_staggered(v);
    PHIHIP_TRY(mom_plan(ctx, op, "advect_differential_backward"));
    for (int c = 0; c < 3; ++c) op.bs_u[c] = op.bs_v[c] = op.bs_o[c] = op.cc[c];
    for (int which = 1; which <= 2; ++which) {
        void* const* o = which == 1 ? gu : gv;
        if (!o) continue;
        PHIHIP_TRY(with_dtype(v, [&](auto t) { return mom_run<typename decltype(t)::type, true>(ctx, v, op, which, u, vel, gout, o, s); }));
    }
    return PHIHIP_OK;
}

static void mom_split(const GridView& v, const void* base, const void* out[3]) {
    const size_t es = elem_bytes(v);
    for (int a = 0; a < 3; ++a) out[a] = (a < v.ax0 || !base) ? nullptr : (const void*)((const char*)base + (size_t)(a - v.ax0) * (size_t)v.cells * es);
}

// centred vector fields [batch][rank][cells]; s_bc / s_val: u's extrapolation
int run_advect_differential_centered(phihip_ctx* ctx, const GridView& v, const void* u, int u_batch, const int32_t s_bc[3][2], const double s_val[3][2],
                                     const void* vel, int vel_batch, void* out, hipStream_t s) {
    if (v.cells >= (1LL << 31) / 4) { set_error("advect_differential_centered: more than 2^29 cells per batch entry are not supported"); return PHIHIP_ERR_UNSUPPORTED; }
    MomOp op = mom_op_centered(v, make_scalar_bc(v, s_bc, s_val));
    PHIHIP_TRY(mom_plan(ctx, op, "advect_differential_centered"));
    for (int c = 0; c < 3; ++c) {
        op.bs_u[c] = u_batch == 1 ? 0 : v.rank * v.cells;
        op.bs_v[c] = vel_batch == 1 ? 0 : v.rank * v.cells;
        op.bs_o[c] = v.rank * v.cells;
    }
    const void *pu[3], *pv[3], *po[3];
    mom_split(v, u, pu);
    mom_split(v, vel, pv);
    mom_split(v, out, po);
    void* o[3] = {(void*)po[0], (void*)po[1], (void*)po[2]};
    return with_dtype(v, [&](auto t) { return mom_run<typename decltype(t)::type, false>(ctx, v, op, 0, pu, pv, nullptr, o, s); });
}

int run_advect_differential_centered_bwd(phihip_ctx* ctx, const GridView& v, const void* u, const int32_t s_bc[3][2], const double s_val[3][2], const void* vel,
                                         const void* gout, void* gu, void* gv, hipStream_t s) {
    if (v.cells >= (1LL << 31) / 4) { set_error("advect_differential_centered_backward: more than 2^29 cells per batch entry are not supported"); return PHIHIP_ERR_UNSUPPORTED; }
    MomOp op = mom_op_centered(v, make_scalar_bc(v, s_bc, s_val));
    PHIHIP_TRY(mom_plan(ctx, op, "advect_differential_centered_backward"));
    for (int c = 0; c < 3; ++c) op.bs_u[c] = op.bs_v[c] = op.bs_o[c] = v.rank * v.cells;
    const void *pu[3], *pv[3], *pg[3], *po[3];
    mom_split(v, u, pu);
    mom_split(v, vel, pv);
    mom_split(v, gout, pg);
    for (int which = 1; which <= 2; ++which) {
        void* dst = which == 1 ? gu : gv;
        if (!dst) continue;
        mom_split(v, dst, po);
        void* o[3] = {(void*)po[0], (void*)po[1], (void*)po[2]};
        PHIHIP_TRY(with_dtype(v, [&](auto t) { return mom_run<typename decltype(t)::type, false>(ctx, v, op, which, pu, pv, pg, o, s); }));
    }
    return PHIHIP_OK;
}

}  // namespace phihip
