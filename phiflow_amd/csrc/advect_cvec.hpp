// advect_cvec.hpp -- centred vector fields (included at the end of advect.hip; uses its decode_sample / sample_blocks launch geometry).
//
// Layout of a centred field with C components: one dense array (batch, C, n0, n1, n2), component-major; component c of batch entry b is a
// contiguous centred scalar grid of `cells` values. A centred velocity is such an array with C = D (component d along grid axis d).
//
//   advect_cvec_kernel       semi-Lagrangian advection of a C-component centred field by a D-component centred velocity on the same grid,
//                            euler back-trace (phi/physics/advect.py:20-24, 156-179): the velocity sampled at the cell itself is the stored
//                            value (_resample.py `sample`: shallow_equals), lookup = x - dt u, one grid_sample of the whole vector field with
//                            the field's extrapolation (_resample.py:257-259). The taps are resolved once per cell and shared by all C
//                            components.
//   staggered_to_cvec_kernel staggered -> cell centres (sample_grid_at_centers, _resample.py:241-259, 341-364): component d at a cell = mean of
//                            its two d-faces, faces that are not stored from the velocity's boundary rule (center_velocity).
//   cvec_to_faces_kernel     centred vector -> the stored faces of a staggered grid (the dot_face_normal branch of `sample`,
//                            _resample.py:148-153): component d at a d-face = mean of component d in the two adjacent cells, outside cells
//                            from the centred field's extrapolation.
// All three are gather kernels, one launch each for every component and batch entry; index math is 32-bit inside one batch entry.
// The run_* functions pick <T, DIM> with with_dtype_rank / with_dtype (common.hpp); the component count NC is chosen inside that lambda.
#pragma once

namespace phihip {

template <typename T>
struct WComp3 {
    T* p[3];
};

// NC > 0: the component count as a compile-time constant (1 = a scalar, DIM = a vector): the component loop unrolls and the 2^DIM * NC tap
// loads of a cell are all in flight together; NC = 0 reads it from C
template <typename T, int DIM, int NC>
__global__ __launch_bounds__(kBlock) void advect_cvec_kernel(VelGrid g, ScalarBc sb, const T* __restrict__ field, long long fstride, int C_,
                                                             const T* __restrict__ vel, long long vstride, T* __restrict__ out, T dt) {
    const int C = NC > 0 ? NC : C_;
    constexpr int A0 = 3 - DIM;
    const int b = blockIdx.y;
    const int total = (int)g.cells;
    const int n[3] = {g.n[0], g.n[1], g.n[2]};
    const T* __restrict__ F = field + (long long)b * fstride;
    const T* __restrict__ U = vel + (long long)b * vstride;
    T* __restrict__ O = out + (long long)b * C * total;
    int bc[3][2];
    T cv[3][2];
    scalar_rule<T>(sb, bc, cv);
    int idx[3], f;
    if (!decode_sample(n[1], n[2], idx, f)) return;
    T disp[3] = {T(0), T(0), T(0)};     // back-trace displacement in index units (same arithmetic as advect_centered_kernel)
#pragma unroll
    for (int a = A0; a < 3; ++a) disp[a] = -(U[(a - A0) * total + f] * (dt * (T)g.rdx[a]));
    AxisPair<T> ax[3];
    T fr[3];
    lookup_pairs_rel<T, DIM>(idx, disp, n, bc, cv, ax, fr);
#pragma unroll
    for (int c = 0; c < (NC > 0 ? NC : 16); ++c) {
        if (NC == 0 && c >= C) break;
        O[c * total + f] = gather_multilinear<T, DIM>(F + (long long)c * total, ax, fr);
    }
}

template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void staggered_to_cvec_kernel(VelGrid g, CComp3a<T> vel, T* __restrict__ out) {
    constexpr int A0 = 3 - DIM;
    const int b = blockIdx.y;
    const int total = (int)g.cells;
    int idx[3], f;
    if (!decode_sample(g.n[1], g.n[2], idx, f)) return;
    T u[3];
    center_velocity<T, DIM>(g, vel, b, idx, u);
    T* __restrict__ O = out + (long long)b * DIM * total;
#pragma unroll
    for (int a = A0; a < 3; ++a) O[(a - A0) * total + f] = u[a];
}

// blockIdx.z = component (ca = ax0 + z); the faces of that component are strided over blockIdx.x
template <typename T>
__global__ __launch_bounds__(kBlock) void cvec_to_faces_kernel(VelGrid g, ScalarBc sb, const T* __restrict__ field, long long fstride,
                                                               WComp3<T> out) {
    const int b = blockIdx.y;
    const int ca = g.ax0 + (int)blockIdx.z;
    const int total = (int)g.ccells[ca];
    const int c1 = g.cn[ca][1], c2 = g.cn[ca][2];
    const int n = g.n[ca];
    const int pstride = ca == 0 ? g.n[1] * g.n[2] : (ca == 1 ? g.n[2] : 1);
    const T* __restrict__ S = field + (long long)b * fstride + (long long)(ca - g.ax0) * g.cells;
    T* __restrict__ O = out.p[ca] + (long long)b * total;
    for (int f = blockIdx.x * kBlock + threadIdx.x; f < total; f += gridDim.x * kBlock) {
        int idx[3];
        idx[2] = f % c2;
        const int t = f / c2;
        idx[1] = t % c1;
        idx[0] = t / c1;
        const int phys = idx[ca] + g.off[ca];
        int l = phys - 1, r = phys;
        bool cl = false, cr = false;
        if (l < 0) { if (sb.bc[ca][0] == PHIHIP_BC_PERIODIC) l += n; else { cl = sb.bc[ca][0] == PHIHIP_BC_CLOSED; l = 0; } }
        if (r >= n) { if (sb.bc[ca][1] == PHIHIP_BC_PERIODIC) r -= n; else { cr = sb.bc[ca][1] == PHIHIP_BC_CLOSED; r = n - 1; } }
        const int rest = (idx[0] * g.n[1] + idx[1]) * g.n[2] + idx[2] - idx[ca] * pstride;
        const T sl = cl ? (T)sb.val[ca][0] : S[rest + l * pstride];
        const T sr = cr ? (T)sb.val[ca][1] : S[rest + r * pstride];
        O[f] = sl * T(0.5) + sr * T(0.5);
    }
}

static int check_cvec_sizes(const GridView& v, int C, const char* what) {
    bool big = v.cells * (C > v.rank ? C : v.rank) >= (1LL << 31);
    for (int ca = v.ax0; ca < 3; ++ca) big = big || v.ccells[ca] >= (1LL << 31);
    if (big) {
        set_error("%s: more than 2^31 values per batch entry are not supported", what);
        return PHIHIP_ERR_UNSUPPORTED;
    }
    return PHIHIP_OK;
}

// field (field_batch, C, *res), velocity (velocity_batch, D, *res), out (v.batch, C, *res); batches of 1 are shared by every entry
int run_advect_cvec(phihip_ctx* ctx, const GridView& v, const void* field, int field_batch, int C, const int32_t s_bc[3][2], const double s_val[3][2],
                    const void* vel, int vel_batch, void* out, double dt, hipStream_t s) {
    PHIHIP_TRY(check_cvec_sizes(v, C, "advect_centered_vector"));
    const VelGrid g = make_velgrid(v);
    const ScalarBc sb = make_scalar_bc(v, s_bc, s_val);
    const long long fstride = field_batch > 1 ? (long long)C * v.cells : 0, vstride = vel_batch > 1 ? (long long)v.rank * v.cells : 0;
    LaunchScope ls(ctx, PHIHIP_K_ADVECT, s);
    const dim3 grid((unsigned)sample_blocks(v.n), v.batch);
    with_dtype_rank(v, [&](auto t, auto d) {
        using T = typename decltype(t)::type;
        constexpr int DIM = decltype(d)::value;
        const T *f = (const T*)field, *u = (const T*)vel;
        if (C == 1) hipLaunchKernelGGL((advect_cvec_kernel<T, DIM, 1>), grid, dim3(kBlock), 0, s, g, sb, f, fstride, C, u, vstride, (T*)out, (T)dt);
        else if (C == DIM) hipLaunchKernelGGL((advect_cvec_kernel<T, DIM, DIM>), grid, dim3(kBlock), 0, s, g, sb, f, fstride, C, u, vstride, (T*)out, (T)dt);
        else hipLaunchKernelGGL((advect_cvec_kernel<T, DIM, 0>), grid, dim3(kBlock), 0, s, g, sb, f, fstride, C, u, vstride, (T*)out, (T)dt);
    });
    PHIHIP_CHECK_HIP(hipGetLastError());
    return PHIHIP_OK;
}

// vel[ca] (v.batch, stored faces of ca), out (v.batch, D, *res)
int run_staggered_to_cvec(phihip_ctx* ctx, const GridView& v, const void* const vel[3], void* out, hipStream_t s) {
    PHIHIP_TRY(check_cvec_sizes(v, v.rank, "staggered_to_centered"));
    const VelGrid g = make_velgrid(v);
    LaunchScope ls(ctx, PHIHIP_K_ADVECT, s);
    const dim3 grid((unsigned)sample_blocks(v.n), v.batch);
    with_dtype_rank(v, [&](auto t, auto d) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((staggered_to_cvec_kernel<T, decltype(d)::value>), grid, dim3(kBlock), 0, s, g,
                           (CComp3a<T>{{(const T*)vel[0], (const T*)vel[1], (const T*)vel[2]}}), (T*)out);
    });
    PHIHIP_CHECK_HIP(hipGetLastError());
    return PHIHIP_OK;
}

// field (field_batch, D, *res) with its own extrapolation (s_bc / s_val), out[ca] (v.batch, stored faces of ca under the grid's rule)
int run_cvec_to_faces(phihip_ctx* ctx, const GridView& v, const void* field, int field_batch, const int32_t s_bc[3][2], const double s_val[3][2],
                      void* const out[3], hipStream_t s) {
    PHIHIP_TRY(check_cvec_sizes(v, v.rank, "centered_vector_to_staggered"));
    const VelGrid g = make_velgrid(v);
    const ScalarBc sb = make_scalar_bc(v, s_bc, s_val);
    const long long fstride = field_batch > 1 ? (long long)v.rank * v.cells : 0;
    long long most = 0;
    for (int ca = v.ax0; ca < 3; ++ca) most = v.ccells[ca] > most ? v.ccells[ca] : most;
    const int nblk = ceil_div(most, kBlock) < 16384 ? ceil_div(most, kBlock) : 16384;
    LaunchScope ls(ctx, PHIHIP_K_ADVECT, s);
    const dim3 grid((unsigned)nblk, v.batch, v.rank);
    with_dtype(v, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(cvec_to_faces_kernel<T>, grid, dim3(kBlock), 0, s, g, sb, (const T*)field, fstride, (WComp3<T>{{(T*)out[0], (T*)out[1], (T*)out[2]}}));
    });
    PHIHIP_CHECK_HIP(hipGetLastError());
    return PHIHIP_OK;
}

}  // namespace phihip
