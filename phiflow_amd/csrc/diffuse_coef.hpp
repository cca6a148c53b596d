// diffuse_coef.hpp -- diffusion with a spatially varying and / or per-axis diffusivity on a CenteredGrid (phi/physics/diffuse.py:13-60,
// :98-141): the explicit flux-form stencil and the device-driven CG on  sharpen = I + L_a  (implicit, diffuse.py:90-95).
// Included by project.hip (the emulation build of the tests compiles the .hip files by name: no translation unit of its own).
//
// The reference (differential, diffuse.py:129-141) for an amount with spatial dimensions, centred grids only:
//     face_a = stagger(amount, math.minimum, NONE)        per axis d: a_f = min(a_L, a_R), ghost cells from AMOUNT's own extrapolation
//     du     = u.gradient(boundary=NONE, at='face')       (u_R - u_L) / dx_d, ghost cells from u's extrapolation
//     lap    = (face_a * du).divergence()                 sum_d (F_{i+1/2} - F_{i-1/2}) / dx_d
// and u += lap, `substeps` times. Here amount_d = w_d * a with w_d = k_d * dt' / dx_d^2 (k_d: the per-axis factor of a lazy `field * (k_x, k_y)`
// or of `vec(...)`, 1 for a plain field; a == 1 without a coefficient array), so on axis d
//     L_a u (i) = sum_d  f_{i+1/2} (u_{i+1} - u_i) - f_{i-1/2} (u_i - u_{i-1}),     f = min(w_d a_L, w_d a_R)
// 1. ALL n + 1 faces per axis carry flux: otherwise divergence would return n - 1 cells and `u += lap` could not be formed (Heat_Flow's
//    `x-: 1` wall would pass no heat). u's ghost: PERIODIC wraps, ZERO_GRADIENT copies the edge cell (that face carries nothing), a constant c
//    is c (0 for the homogeneous operator: the adjoint and the CG's linear part). The coefficient's ghost: PERIODIC wraps, ZERO_GRADIENT is
//    the edge cell, a constant c is c (the amount's extrapolation is the diffusivity's times dt / substeps: w_d c). On an axis where u itself
//    is PERIODIC there is no wall: the faces at both ends are ONE face between cell n - 1 and cell 0 and its coefficient is formed from those two
//    cells (what leaves through one end enters through the other: sum u is conserved and the operator stays symmetric).
// 2. The minimum is that of the SIGNED amount: min(w a_L, w a_R) = w * max(a_L, a_R) for w < 0 -- implicit (explicit with -dt) takes the
//    larger neighbour, explicit with dt > 0 the smaller; a coefficient with a ZERO extrapolation insulates the wall in explicit (min(w a, 0) = 0)
//    but not in implicit (min(-|w| a, 0) = -|w| a). Read from the reference's code, not run against PhiML.
// Without a coefficient array (a == 1) the operator is the per-axis weighted Laplacian of laplace(u, weights=k) (diffuse.py:140-141).
//
// Kernels: a column march (column_march.hpp: plan and tile decode; the tap block below resolves u's rule and the coefficient's in one pass and
// is this kernel's own) like diffuse_kernel (project.hip): the a0 neighbours of u and of the coefficient are the values the thread read one plane earlier / reads one plane ahead
// (registers), the in-plane neighbours are the neighbouring lanes' loads of the same plane (L1 / L2 hits). Every array is read from HBM once
// per launch: explicit = u + a in, out written, 12 B per cell in fp32.
// CG (same semantics as cg.hip cg_t: 'CG' and 'CG-adaptive', rtol / atol, max_iterations, refresh every `refresh_every` like PhiML, tolerance
// mode polling the host-mapped flags): two launches per iteration, each reducing its predecessor's per-workgroup partial sums in a fixed
// order in its prologue (stencil_march.hpp cg_prologue / cg_advance), no host synchronisation per iteration.
//   MATVEC  S = r + beta d_old  ->  d_new = S ; sum S (A S) [ + sum S r ]                (r, d_old, a in; d_new out)
//   UPDATE  S = d               ->  x += alpha S ; r -= alpha A S ; sum r^2 [ + r.AS ]  (d, a, x, r in; x, r out)
#pragma once

namespace phihip {

enum CoefMode {
    CM_APPLY = 0,    // o1 = S + L S  (accumulate: o1 += ...), S = a
    CM_RHS = 1,      // o1 = a - L(0): the right-hand side y - sharpen(0) of the affine walls (S = 0, u's wall constants as ghosts)
    CM_RESID = 2,    // o1 = r = b - (S + L S), S = a ; part1 = sum r^2, part2 = sum b^2
    CM_MATVEC = 3,   // S = a + beta b ; o1 = S ; part1 = sum S (S + L S), part2 = sum S a ('CG-adaptive': d.r)
    CM_UPDATE = 4,   // S = a ; q = S + L S ; o1 += alpha S ; o2 -= alpha q ; part1 = sum o2^2, part2 = sum o2 q
    CM_AXPY = 5,     // o1 += alpha a (the true-residual refresh step: x only)
    CM_DOTQ = 6,     // S = a ; part1 = sum b (S + L S)  ('CG-adaptive' refresh: r_new . A d)
    CM_LAP = 7       // o1 = L S without the identity term (accumulate: o1 += ...), S = a: field.laplace (diffops.hpp) -- an instantiation of its own
};

struct CoefOp {
    int n[3];              // cells per internal axis (n[0] == 1 for 2-D grids)
    int ax0;
    long long cells;
    int ubc[3][2];         // u's extrapolation per internal axis / side: PHIHIP_BC_PERIODIC / OPEN (zero-gradient) / CLOSED (constant uval)
    double uval[3][2];
    int cbc[3][2];         // the coefficient's extrapolation (ignored where u is PERIODIC, see 1. above)
    double cval[3][2];
    double w[3];           // signed k_d dt' / dx_d^2 (0 on unused axes)
    int has_c;             // 0: no coefficient array (a == 1)
    int c_per_batch;       // 1: the coefficient has u's batch, 0: one array for every batch entry
    ColumnPlan plan;
    int nblk;              // workgroups = partial sums per batch entry
};

template <typename T>
struct CoefArgs {
    const T* a;
    const T* b;
    T* o1;
    T* o2;
    const T* coef;
    const CgState* st_in;
    CgState* st_out;
    const double* pin1;
    const double* pin2;
    double* part1;
    double* part2;
    CgParams prm;
    int prologue;
    int accumulate;
    unsigned long long* host_flags;
    unsigned int seq;
};

template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void coef_kernel(CoefOp op, CoefArgs<T> p) {
    __shared__ double red[kBlock / kWave];
    __shared__ CgState sh_state;
    const int b = blockIdx.y;
    const int n0 = op.n[0], n1 = op.n[1], n2 = op.n[2];
    const long long bb = (long long)b * op.cells;
    T alpha = T(0), beta = T(0);
    if (p.prologue != PRO_NONE) {
        const CgState S = cg_prologue(p.prologue, p.st_in, p.st_out, p.pin1, p.pin2, op.nblk, p.prm, b, blockIdx.x == 0, red, &sh_state);
        if (MODE == CM_MATVEC && p.host_flags && blockIdx.x == 0 && threadIdx.x == 0)   // the host stops enqueueing once every entry reports 0
            publish_flag(p.host_flags + b, ((unsigned long long)p.seq << 32) | (unsigned long long)(S.cont != 0));
        if (S.cont == 0) return;   // frozen batch entry (uniform per workgroup)
        alpha = (T)S.alpha;
        beta = (T)S.beta;
    }
    // (neighbouring columns share an XCD's L2: their halo rows / columns; inactive threads still take part in the block reductions)
    ColumnTile t = column_tile(op.plan, n1, n2, xcd_order(blockIdx.x, gridDim.x));
    const bool active = column_planes(op.plan, t, n0) && t.inside;
    const int i1 = t.i1, i2 = t.i2, p0 = t.p0, p1 = t.p1;
    const T* __restrict__ A = p.a + bb;
    const T* __restrict__ B = p.b ? p.b + bb : nullptr;
    const T* __restrict__ C = op.has_c ? p.coef + (op.c_per_batch ? bb : 0) : nullptr;
    T w[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) w[ax] = (T)op.w[ax];
    // the source S at a stored index of this batch entry (CM_RHS: zero everywhere -- only the wall constants remain)
    auto src = [&](long long i) -> T {
        if (MODE == CM_RHS) return T(0);
        if (MODE == CM_MATVEC) return A[i] + beta * B[i];
        return A[i];
    };
    auto coef = [&](long long i) -> T { return C ? C[i] : T(1); };
    // face coefficient between a cell and its neighbour on axis ax: the minimum of the SIGNED amounts (see 2. above)
    auto face = [&](int ax, T ac, T an) -> T {
        const T fc = w[ax] * ac, fn = w[ax] * an;
        return fn < fc ? fn : fc;
    };
    // in-plane taps k = 2 * (axis - 1) + side: offset of the neighbour, u's rule outside the array (0: inside / wrapped, 1: zero-gradient =
    // no flux, 2: constant), the coefficient's rule (0: load at coff, 1: the centre's, 2: constant cv)
    int off[4], coff[4], urule[4], crule[4];
    T uv[4], cv[4];
    const int o_c = i1 * n2 + i2;
    {
        const int idx[2] = {i1, i2}, nn[2] = {n1, n2}, st[2] = {n2, 1};
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const int k = 2 * a + side, ax = a + 1;
                const int j = idx[a] + (side ? 1 : -1);
                off[k] = o_c + (side ? st[a] : -st[a]);
                coff[k] = off[k];
                urule[k] = 0; crule[k] = 0;
                uv[k] = T(0); cv[k] = T(0);
                if (ax < op.ax0) { urule[k] = 1; off[k] = coff[k] = o_c; continue; }     // (unused axis of a 2-D grid)
                if (j >= 0 && j < nn[a]) continue;
                const int wrapped = o_c + (side ? -(nn[a] - 1) * st[a] : (nn[a] - 1) * st[a]);
                const int ucode = op.ubc[ax][side];
                if (ucode == PHIHIP_BC_PERIODIC) { off[k] = coff[k] = wrapped; continue; }
                off[k] = o_c;
                if (ucode == PHIHIP_BC_OPEN) { urule[k] = 1; coff[k] = o_c; continue; }
                urule[k] = 2; uv[k] = (T)op.uval[ax][side];
                const int ccode = op.cbc[ax][side];
                if (ccode == PHIHIP_BC_PERIODIC) coff[k] = wrapped;
                else if (ccode == PHIHIP_BC_OPEN) { crule[k] = 1; coff[k] = o_c; }
                else { crule[k] = 2; coff[k] = o_c; cv[k] = (T)op.cval[ax][side]; }
            }
    }
    const long long ps = (long long)n1 * n2;
    const bool has0 = op.ax0 == 0;
    // the a0 neighbour plane `pl` of this thread's column: u value, coefficient value and u's rule (as for the in-plane taps)
    auto plane_nb = [&](int pl, T s_c, T a_c, T& s_out, T& a_out) -> int {
        if (pl >= 0 && pl < n0) { const long long i = (long long)pl * ps + o_c; s_out = src(i); a_out = coef(i); return 0; }
        const int side = pl < 0 ? 0 : 1;
        const int wrapped = pl < 0 ? pl + n0 : pl - n0;
        const int ucode = op.ubc[0][side];
        if (ucode == PHIHIP_BC_PERIODIC) { const long long i = (long long)wrapped * ps + o_c; s_out = src(i); a_out = coef(i); return 0; }
        if (ucode == PHIHIP_BC_OPEN) { s_out = s_c; a_out = a_c; return 1; }
        s_out = (T)op.uval[0][side];
        const int ccode = op.cbc[0][side];
        a_out = ccode == PHIHIP_BC_PERIODIC ? coef((long long)wrapped * ps + o_c) : (ccode == PHIHIP_BC_OPEN ? a_c : (T)op.cval[0][side]);
        return 2;
    };
    T acc1 = T(0), acc2 = T(0);
    if (active) {
        T s_cur = src((long long)p0 * ps + o_c), a_cur = coef((long long)p0 * ps + o_c);
        T s_prev = T(0), a_prev = T(0), s_next = T(0), a_next = T(0);
        int r_prev = 1, r_next = 1;
        if (has0) r_prev = plane_nb(p0 - 1, s_cur, a_cur, s_prev, a_prev);
        for (int pl = p0; pl < p1; ++pl) {
            const long long po = (long long)pl * ps;
            const long long ic = po + o_c;
            if (has0) r_next = plane_nb(pl + 1, s_cur, a_cur, s_next, a_next);
            T lap = T(0);
            if (MODE != CM_AXPY) {
                // flux form (differences of neighbours first, like stencil_march.hpp): F_hi - F_lo per axis, zero-gradient faces carry nothing
                if (has0) {
                    const T fh = r_next == 1 ? T(0) : face(0, a_cur, a_next) * (s_next - s_cur);
                    const T fl = r_prev == 1 ? T(0) : face(0, a_cur, a_prev) * (s_cur - s_prev);
                    lap = fh - fl;
                }
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int ax = a + 1;
                    T fx[2];
#pragma unroll
                    for (int side = 0; side < 2; ++side) {
                        const int k = 2 * a + side;
                        if (urule[k] == 1) { fx[side] = T(0); continue; }
                        const T sn = urule[k] == 2 ? uv[k] : src(po + off[k]);
                        const T an = crule[k] == 0 ? coef(po + coff[k]) : (crule[k] == 1 ? a_cur : cv[k]);
                        fx[side] = face(ax, a_cur, an) * (side ? sn - s_cur : s_cur - sn);
                    }
                    lap += fx[1] - fx[0];
                }
            }
            if (MODE == CM_APPLY) {
                const T q = s_cur + lap;
                if (p.accumulate) p.o1[bb + ic] += q;
                else p.o1[bb + ic] = q;
            } else if (MODE == CM_LAP) {
                if (p.accumulate) p.o1[bb + ic] += lap;
                else p.o1[bb + ic] = lap;
            } else if (MODE == CM_RHS) {
                p.o1[bb + ic] = A[ic] - lap;
            } else if (MODE == CM_RESID) {
                const T y = B[ic];
                const T r = y - (s_cur + lap);
                p.o1[bb + ic] = r;
                acc1 += r * r;
                acc2 += y * y;
            } else if (MODE == CM_MATVEC) {
                const T q = s_cur + lap;
                p.o1[bb + ic] = s_cur;
                acc1 += s_cur * q;
                acc2 += s_cur * A[ic];
            } else if (MODE == CM_UPDATE) {
                const T q = s_cur + lap;
                p.o1[bb + ic] = fma(alpha, s_cur, p.o1[bb + ic]);
                const T r = fma(-alpha, q, p.o2[bb + ic]);
                p.o2[bb + ic] = r;
                acc1 += r * r;
                acc2 += r * q;
            } else if (MODE == CM_AXPY) {
                p.o1[bb + ic] = fma(alpha, s_cur, p.o1[bb + ic]);
            } else if (MODE == CM_DOTQ) {
                acc1 += B[ic] * (s_cur + lap);
            }
            s_prev = s_cur; a_prev = a_cur; r_prev = 0;
            s_cur = s_next; a_cur = a_next;
        }
    }
    if (MODE == CM_RESID || MODE == CM_MATVEC || MODE == CM_UPDATE || MODE == CM_DOTQ) {
        double t[2] = {(double)acc1, (double)acc2};
        block_sum_n<2>(t, red);
        if (threadIdx.x == 0) {
            const long long o = (long long)b * op.nblk + blockIdx.x;
            p.part1[o] = t[0];
            if (p.part2) p.part2[o] = t[1];
        }
    }
}

// control block after the loop (fold the last reduction) -- cg.hip's cg_state_kernel for this solver's partials
__global__ __launch_bounds__(kBlock) void coef_state_kernel(int kind, const CgState* st_in, CgState* st_out, const double* pin1, const double* pin2,
                                                             int nblk, CgParams prm) {
    __shared__ double red[kBlock / kWave];
    __shared__ CgState sh;
    cg_prologue(kind, st_in, st_out, pin1, pin2, nblk, prm, blockIdx.x, true, red, &sh);
}

// launch geometry: about `target` workgroups per batch entry (column_march.hpp)
static inline int coef_plan(CoefOp& op, int target, const char* what) {
    PHIHIP_TRY(plan_columns(op.n, kPatchRows, kPatchCols, target, 0, false, what, op.plan));
    op.nblk = op.plan.tiles1 * op.plan.tiles2 * op.plan.chunks;
    return PHIHIP_OK;
}

template <typename T, int MODE>
static int coef_launch(const CoefOp& op, int batch, const CoefArgs<T>& a, hipStream_t s) {
    hipLaunchKernelGGL((coef_kernel<T, MODE>), dim3((unsigned)op.nblk, batch), dim3(kBlock), 0, s, op, a);
    PHIHIP_CHECK_HIP(hipGetLastError());
    return PHIHIP_OK;
}

// the operator of one call: u's and the coefficient's extrapolation per internal axis, w_d = sign * kdt_d / dx_d^2
static CoefOp coef_op(const GridView& v, const ScalarBc& ub, const void* coef, int c_batch, const ScalarBc& cb, const double kdt[3], double sign) {
    CoefOp op;
    memset(&op, 0, sizeof(op));
    op.ax0 = v.ax0;
    op.cells = v.cells;
    for (int a = 0; a < 3; ++a) {
        op.n[a] = v.n[a];
        op.w[a] = a < v.ax0 ? 0.0 : sign * kdt[a] / (v.dx[a] * v.dx[a]);
        for (int side = 0; side < 2; ++side) {
            op.ubc[a][side] = a < v.ax0 ? PHIHIP_BC_PERIODIC : ub.bc[a][side];
            op.uval[a][side] = ub.bc[a][side] == PHIHIP_BC_CLOSED ? ub.val[a][side] : 0.0;
            // no coefficient array: 1 everywhere, ghosts included -- the ghost is the cell's own 1 (zero-gradient), never u's wall constant
            op.cbc[a][side] = a < v.ax0 ? PHIHIP_BC_PERIODIC : (coef != nullptr ? cb.bc[a][side] : PHIHIP_BC_OPEN);
            op.cval[a][side] = coef != nullptr ? cb.val[a][side] : 1.0;
        }
    }
    op.has_c = coef != nullptr;
    op.c_per_batch = coef != nullptr && c_batch > 1;
    return op;
}

// diffuse.explicit substep: out = u + L_a u (adjoint: out += (I + L_a)^T u = the same stencil with homogeneous walls -- the operator is symmetric)
int run_diffuse_coef_explicit(phihip_ctx* ctx, const GridView& v, const void* u, const int32_t s_bc[3][2], const double s_val[3][2], const void* coef,
                              int c_batch, const int32_t c_bc[3][2], const double c_val[3][2], const double kdt[3], int adjoint, void* out, hipStream_t s) {
    if (v.cells >= (1LL << 31)) { set_error("diffuse: more than 2^31 cells per batch entry are not supported"); return PHIHIP_ERR_UNSUPPORTED; }
    const ScalarBc ub = make_scalar_bc(v, s_bc, s_val), cb = make_scalar_bc(v, c_bc, c_val);
    CoefOp op = coef_op(v, ub, coef, c_batch, cb, kdt, 1.0);
    if (adjoint)
        for (int a = 0; a < 3; ++a) op.uval[a][0] = op.uval[a][1] = 0.0;
    PHIHIP_TRY(coef_plan(op, 4096, "diffuse"));
    LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
    return with_dtype(v, [&](auto t) {
        using T = typename decltype(t)::type;
        CoefArgs<T> a;
        memset(&a, 0, sizeof(a));
        a.a = (const T*)u; a.o1 = (T*)out; a.coef = (const T*)coef; a.accumulate = adjoint ? 1 : 0;
        return coef_launch<T, CM_APPLY>(op, v.batch, a, s);
    });
}

// CG on (I + L_a) x = rhs with homogeneous walls, x holds x0 on entry (cg.hip cg_t's two-launch form without the deferred x update)
template <typename T>
static int coef_cg_t(phihip_ctx* ctx, const CoefOp& op0, int batch, const T* coef, const T* rhs, T* x, const phihip_solve* solve,
                     phihip_solve_info* info, hipStream_t s) {
    CoefOp op = op0;
    PHIHIP_TRY(coef_plan(op, 1024, "diffuse_implicit"));      // (fewer workgroups than the explicit pass: every workgroup of the next launch re-reduces all partials)
    const size_t vec_bytes = (size_t)batch * op.cells * sizeof(T);
    const size_t part_n = (size_t)batch * op.nblk;
    PHIHIP_TRY(ensure_buffer(ctx->ws_coef_r, vec_bytes));
    PHIHIP_TRY(ensure_buffer(ctx->ws_coef_d0, vec_bytes));
    PHIHIP_TRY(ensure_buffer(ctx->ws_coef_d1, vec_bytes));
    PHIHIP_TRY(ensure_buffer(ctx->ws_coef_part, 5 * part_n * sizeof(double)));
    PHIHIP_TRY(ensure_buffer(ctx->ws_coef_state, (size_t)2 * batch * sizeof(CgState)));
    unsigned int seq;
    PHIHIP_TRY(cg_host_prepare(ctx, batch, &seq));
    int checks = 0;
    T* r = (T*)ctx->ws_coef_r.ptr;
    T* d[2] = {(T*)ctx->ws_coef_d0.ptr, (T*)ctx->ws_coef_d1.ptr};
    double* part_rr = (double*)ctx->ws_coef_part.ptr;
    double* part_dq = part_rr + part_n;
    double* part_yy = part_dq + part_n;
    double* part_rq = part_yy + part_n;   // 'CG-adaptive': sum r_new . A d (UPDATE / DOTQ) and sum d . r (MATVEC)
    double* part_dr = part_rq + part_n;
    const bool ad = solve->method == PHIHIP_METHOD_CG_ADAPTIVE;
    const int pro_alpha = ad ? PRO_ALPHA_AD : PRO_ALPHA, pro_beta = ad ? PRO_BETA_AD : PRO_BETA;
    CgState* st[2] = {(CgState*)ctx->ws_coef_state.ptr, (CgState*)ctx->ws_coef_state.ptr + batch};
    int cur = 0;
    const CgParams prm = cg_params(solve);
    CoefArgs<T> base;
    memset(&base, 0, sizeof(base));
    base.coef = coef;
    base.prm = prm;
    {   // r0 = y - A x0 ; sum r^2, sum y^2
        CoefArgs<T> a = base;
        a.a = x; a.b = rhs; a.o1 = r; a.part1 = part_rr; a.part2 = part_yy;
        a.prologue = PRO_NONE;
        LaunchScope ls(ctx, PHIHIP_K_CG_RESIDUAL, s);
        PHIHIP_TRY((coef_launch<T, CM_RESID>(op, batch, a, s)));
    }
    bool first = true;
    for (int k = 1; k <= solve->max_iterations; ++k) {
        T* d_old = d[(k - 1) & 1];
        T* d_new = d[k & 1];
        {   // d_new = r + beta d_old (the first one reads r in place of d_old with beta = 0)
            CoefArgs<T> a = base;
            a.a = r; a.b = first ? r : d_old; a.o1 = d_new; a.part1 = part_dq; a.part2 = ad ? part_dr : nullptr;
            if (solve->check_every > 0) { a.host_flags = ctx->cg.host_flags_dev; a.seq = seq; }
            a.prologue = first ? PRO_FIRST : pro_beta;
            a.st_in = st[cur]; a.st_out = st[cur ^ 1]; a.pin1 = part_rr; a.pin2 = (first || !ad) ? part_yy : part_rq;
            LaunchScope ls(ctx, PHIHIP_K_CG_MATVEC_DOT, s);
            PHIHIP_TRY((coef_launch<T, CM_MATVEC>(op, batch, a, s)));
            cur ^= 1;
            first = false;
        }
        if (solve->refresh_every > 0 && k % solve->refresh_every == 0) {
            {   // x += alpha d ; then the true residual r = y - A x (PhiML every refresh_every-th iteration)
                CoefArgs<T> a = base;
                a.a = d_new; a.o1 = x;
                a.prologue = pro_alpha;
                a.st_in = st[cur]; a.st_out = st[cur ^ 1]; a.pin1 = part_dq; a.pin2 = part_dr;
                LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
                PHIHIP_TRY((coef_launch<T, CM_AXPY>(op, batch, a, s)));
                cur ^= 1;
            }
            {
                CoefArgs<T> a = base;
                a.a = x; a.b = rhs; a.o1 = r; a.part1 = part_rr; a.part2 = part_yy;   // (sum y^2 is not needed again: scratch)
                a.prologue = PRO_CONT;
                a.st_in = st[cur];
                LaunchScope ls(ctx, PHIHIP_K_CG_RESIDUAL, s);
                PHIHIP_TRY((coef_launch<T, CM_RESID>(op, batch, a, s)));
            }
            if (ad) {
                CoefArgs<T> a = base;
                a.a = d_new; a.b = r; a.part1 = part_rq;
                a.prologue = PRO_CONT;
                a.st_in = st[cur];
                LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
                PHIHIP_TRY((coef_launch<T, CM_DOTQ>(op, batch, a, s)));
            }
        } else {
            CoefArgs<T> a = base;
            a.a = d_new; a.o1 = x; a.o2 = r; a.part1 = part_rr; a.part2 = ad ? part_rq : nullptr;
            a.prologue = pro_alpha;
            a.st_in = st[cur]; a.st_out = st[cur ^ 1]; a.pin1 = part_dq; a.pin2 = part_dr;
            LaunchScope ls(ctx, PHIHIP_K_CG_UPDATE, s);
            PHIHIP_TRY((coef_launch<T, CM_UPDATE>(op, batch, a, s)));
            cur ^= 1;
        }
        bool stop = false;
        PHIHIP_TRY(cg_poll(ctx, solve, k, seq, batch, &checks, s, &stop));
        if (stop) break;
    }
    {
        LaunchScope ls(ctx, PHIHIP_K_CG_SCALAR, s);
        hipLaunchKernelGGL(coef_state_kernel, dim3(batch), dim3(kBlock), 0, s, (int)(first ? PRO_FIRST : pro_beta), (const CgState*)st[cur],
                           st[cur ^ 1], (const double*)part_rr, (const double*)((first || !ad) ? part_yy : part_rq), op.nblk, prm);
        cur ^= 1;
    }
    PHIHIP_CHECK_HIP(hipGetLastError());
    return cg_report(ctx, st[cur], batch, info, s);
}

// diffuse.implicit: solve_linear(sharpen, y = field, x0 = field) with sharpen(x) = explicit(x, a, -dt) = x + L_a x (w_d = -kdt_d / dx_d^2).
// sharpen is affine when u has constant walls: (I + L_a^hom) x = field - L_a(0) -- the constants' share moves to the right-hand side like the
// scalar path (project.hip implicit_rhs_kernel); tolerances are relative to that right-hand side.
template <typename T>
static int diffuse_coef_implicit_t(phihip_ctx* ctx, const GridView& v, const void* u, const ScalarBc& ub, const void* coef, int c_batch, const ScalarBc& cb,
                                   const double kdt[3], const phihip_solve* solve, phihip_solve_info* info, void* out, hipStream_t s) {
    CoefOp op = coef_op(v, ub, coef, c_batch, cb, kdt, -1.0);
    bool affine = false;
    for (int a = v.ax0; a < 3; ++a)
        for (int side = 0; side < 2; ++side) affine = affine || (op.ubc[a][side] == PHIHIP_BC_CLOSED && op.uval[a][side] != 0.0);
    const size_t bytes = (size_t)v.batch * v.cells * sizeof(T);
    const T* rhs = (const T*)u;
    if (affine) {
        PHIHIP_TRY(ensure_buffer(ctx->ws_coef_rhs, bytes));
        CoefOp o = op;
        PHIHIP_TRY(coef_plan(o, 4096, "diffuse_implicit"));
        CoefArgs<T> a;
        memset(&a, 0, sizeof(a));
        a.a = (const T*)u; a.o1 = (T*)ctx->ws_coef_rhs.ptr; a.coef = (const T*)coef;
        LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
        PHIHIP_TRY((coef_launch<T, CM_RHS>(o, v.batch, a, s)));
        rhs = (const T*)ctx->ws_coef_rhs.ptr;
    }
    for (int a = 0; a < 3; ++a) op.uval[a][0] = op.uval[a][1] = 0.0;
    PHIHIP_CHECK_HIP(hipMemcpyAsync(out, u, bytes, hipMemcpyDeviceToDevice, s));      // x0 = field (diffuse.py:90-91)
    return coef_cg_t<T>(ctx, op, v.batch, (const T*)coef, rhs, (T*)out, solve, info, s);
}

int run_diffuse_coef_implicit(phihip_ctx* ctx, const GridView& v, const void* u, const int32_t s_bc[3][2], const double s_val[3][2], const void* coef,
                              int c_batch, const int32_t c_bc[3][2], const double c_val[3][2], const double kdt[3], const phihip_solve* solve,
                              phihip_solve_info* info, void* out, hipStream_t s) {
    if (v.cells >= (1LL << 31)) { set_error("diffuse_implicit: more than 2^31 cells per batch entry are not supported"); return PHIHIP_ERR_UNSUPPORTED; }
    if (solve->method == PHIHIP_METHOD_CG_MULTIGRID) { set_error("diffuse_implicit: the multigrid preconditioner covers the pressure solve only"); return PHIHIP_ERR_UNSUPPORTED; }
    const ScalarBc ub = make_scalar_bc(v, s_bc, s_val), cb = make_scalar_bc(v, c_bc, c_val);
    return with_dtype(v, [&](auto t) { return diffuse_coef_implicit_t<typename decltype(t)::type>(ctx, v, u, ub, coef, c_batch, cb, kdt, solve, info, out, s); });
}

}  // namespace phihip
