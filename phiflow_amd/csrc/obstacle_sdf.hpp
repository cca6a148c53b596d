// f13: obstacles of arbitrary shape from a signed-distance grid -- phi.geom.SDFGrid (phi/geom/_sdf_grid.py:13-243), sample_sdf (:245-298).
// Included by project.hip inside namespace phihip, after the analytic obstacle kernels: it reuses their (4 x 64) patches, PatchBox,
// decode_box_patch, ObstacleSet and obstacle_sdf. The analytic kernels and their launches are not touched: the dispatchers at the end of
// this file cut the host obstacle list into maximal runs of analytic entries (sent through the existing code) and single SDF entries (one
// launch each); the application is sequential per obstacle (fluid.py:226-240), so the cut reproduces the reference's loop.
//
// Restated semantics, res = the array's resolution, size = upper - lower of its bounds:
//   sdf_val(x)  = multilinear(sdf, (x - lower) / size * res - 0.5)           _sdf_grid.py:150-151, :184-185
//                 math.grid_sample(values, idx, ZERO_GRADIENT): every tap index clamped to [0, res - 1]  [PHIML-RECALL] (as advect_common.hpp
//                 and oracle.grid_sample restate it)
//   lies_inside = approximate_outside ? lower <= x <= upper (inclusive, Box.lies_inside _box.py:174-185) && sdf_val <= 0 : sdf_val <= 0      :149-156
//   distance    = approximate_outside ? (within bounds ? sdf_val : |x - center| - bounding_radius) : sdf_val                               :183-191
// Positions, the float index, the weights and the interpolation are computed in double, as the analytic path does; the 2^D taps are plain
// clamped loads of the array (fp32 or fp64, its own dtype code) converted to double. Neighbouring threads read neighbouring taps: no LDS.
#pragma once

struct SdfView {
    const void* data;
    int f64;                 // element type of the array
    int n[3];                // values per internal axis (unused leading axis: 1)
    int approx;
    int moving;
    double lower[3], upper[3], size[3], center[3], vel[3];   // internal axis order
    double bounding_radius;
};

static SdfView make_sdf_view(const GridView& v, const phihip_sdf_grid& d, const phihip_obstacle& o) {
    SdfView w;
    memset(&w, 0, sizeof(w));
    w.data = d.sdf;
    w.f64 = d.dtype == PHIHIP_F64;
    w.approx = d.approximate_outside != 0;
    w.bounding_radius = d.bounding_radius;
    for (int a = 0; a < 3; ++a) { w.n[a] = 1; w.size[a] = 1.0; }
    for (int k = 0; k < v.rank; ++k) {
        const int a = k + v.ax0;
        w.n[a] = d.res[k];
        w.lower[a] = d.lower[k];
        w.upper[a] = d.upper[k];
        w.size[a] = d.upper[k] - d.lower[k];
        w.center[a] = d.center[k];
        w.vel[a] = o.velocity[k];
        w.moving = w.moving || o.velocity[k] != 0.0;
    }
    return w;
}

__device__ __forceinline__ double sdf_tap(const SdfView& w, long long i) {
    return w.f64 ? ((const double*)w.data)[i] : (double)((const float*)w.data)[i];
}

// sdf_val(x); *within = lower <= x <= upper on every axis
__device__ __forceinline__ double sdf_sample(const SdfView& w, const double (&x)[3], int ax0, bool* within) {
    // one rounding per operation, as written (no fused multiply-add): where positions, bounds and values are dyadic the index, the weights
    // and the sample are then exact, and the inclusive `<= 0` on a tap or half-way between two decides as the reference's does
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int i0[3] = {0, 0, 0}, i1[3] = {0, 0, 0};
    double f[3] = {0, 0, 0};
    bool in = true;
    for (int a = ax0; a < 3; ++a) {
        in = in && x[a] >= w.lower[a] && x[a] <= w.upper[a];
        const double idx = (x[a] - w.lower[a]) / w.size[a] * (double)w.n[a] - 0.5;
        // (a wild coordinate must not overflow the conversion: everything below / above the array clamps to its edge value anyway)
        const double c = idx < -1.0 ? -1.0 : (idx > (double)w.n[a] ? (double)w.n[a] : idx);
        const double fl = floor(c);
        f[a] = c - fl;
        const int lo = (int)fl, hi = lo + 1;
        i0[a] = lo < 0 ? 0 : (lo > w.n[a] - 1 ? w.n[a] - 1 : lo);
        i1[a] = hi < 0 ? 0 : (hi > w.n[a] - 1 ? w.n[a] - 1 : hi);
    }
    *within = in;
    double val = 0;
    // lerp along a2 first (neighbouring threads: neighbouring columns), then a1, then a0
    double p[2] = {0, 0};
    const int planes = ax0 == 0 ? 2 : 1;
    for (int s0 = 0; s0 < planes; ++s0) {
        const long long b0 = (long long)(s0 ? i1[0] : i0[0]) * w.n[1];
        double r[2];
        for (int s1 = 0; s1 < 2; ++s1) {
            const long long b1 = (b0 + (s1 ? i1[1] : i0[1])) * w.n[2];
            const double t0 = sdf_tap(w, b1 + i0[2]), t1 = sdf_tap(w, b1 + i1[2]);
            r[s1] = t0 * (1.0 - f[2]) + t1 * f[2];
        }
        p[s0] = r[0] * (1.0 - f[1]) + r[1] * f[1];
    }
    val = planes == 2 ? p[0] * (1.0 - f[0]) + p[1] * f[0] : p[0];
    return val;
}

__device__ __forceinline__ double sdf_distance(const SdfView& w, const double (&x)[3], int ax0) {
    bool within;
    const double val = sdf_sample(w, x, ax0, &within);
    if (!w.approx || within) return val;
    double d2 = 0;
    for (int a = ax0; a < 3; ++a) d2 += (x[a] - w.center[a]) * (x[a] - w.center[a]);
    return sqrt(d2) - w.bounding_radius;
}

// The patches an SDF obstacle can touch on lattice `ca` (faces of component ca, ca < 0: cell centres), written into slot l.
// approximate_outside: the bounding box of bounds U ball(center, bounding_radius), grown by `margin` as the analytic kernels grow theirs
// (patch_box_slot with a box of that extent); otherwise every patch of the lattice -- the clamped sample has no bounding box.
static void sdf_patch_slot(const GridView& v, const SdfView& w, int ca, double margin, int l, PatchBox* pb) {
    if (!w.approx) {
        const int n0 = ca >= 0 ? v.cn[ca][0] : v.n[0], n1 = ca >= 0 ? v.cn[ca][1] : v.n[1], n2 = ca >= 0 ? v.cn[ca][2] : v.n[2];
        pb->i0[l] = 0; pb->n0[l] = n0;
        pb->p1[l] = 0; pb->np1[l] = ceil_div(n1, kPatchRows);
        pb->p2[l] = 0; pb->np2[l] = ceil_div(n2, kPatchCols);
        return;
    }
    ObstacleSet box;
    memset(&box, 0, sizeof(box));
    box.count = 1;
    box.kind[0] = PHIHIP_OBSTACLE_BOX;
    const double r = w.bounding_radius > 0 ? w.bounding_radius : 0.0;
    for (int a = v.ax0; a < 3; ++a) {
        const double lo = fmin(w.lower[a], w.center[a] - r), hi = fmax(w.upper[a], w.center[a] + r);
        box.center[0][a] = 0.5 * (lo + hi);
        box.half[0][a] = 0.5 * (hi - lo) * (1.0 + 1e-12) + 1e-300;
    }
    patch_box_slot(v, box, ca, margin, l, pb);
}

// accessible = ~lies_inside at the cell centres (fluid.py:130-133): clears the cells inside; the array starts as all ones (or as what
// the obstacles before this one left)
__global__ __launch_bounds__(kBlock) void sdf_accessible_kernel(VelGrid g, double lower0, double lower1, double lower2, SdfView w, PatchBox pb,
                                                                uint8_t* accessible) {
    const double lower[3] = {lower0, lower1, lower2};
    const int tx = threadIdx.x & (kPatchCols - 1), ty = threadIdx.x / kPatchCols;
    const int npatch = pb.first[3];
    for (int patch = blockIdx.x; patch < npatch; patch += gridDim.x) {
        int l, i0, r0, c0;
        decode_box_patch(pb, patch, l, i0, r0, c0);
        const int idx[3] = {i0, r0 + ty, c0 + tx};
        if (idx[0] >= g.n[0] || idx[1] >= g.n[1] || idx[2] >= g.n[2]) continue;
        double x[3] = {0, 0, 0};
        for (int a = g.ax0; a < 3; ++a) x[a] = lower[a] + (idx[a] + 0.5) * g.dx[a];
        bool within;
        const double val = sdf_sample(w, x, g.ax0, &within);
        if ((!w.approx || within) && val <= 0.0) accessible[((long long)i0 * g.n[1] + idx[1]) * g.n[2] + idx[2]] = (uint8_t)0;
    }
}

// apply_boundary_conditions for ONE SDF obstacle (fluid.py:226-240), every component and batch entry in one launch:
//   m = clip(1 - distance(x_face) / |half a cell's diagonal|, 0, 1);  v = safe_mul(1 - m, v) [+ safe_mul(m, velocity)]
// -- the arithmetic in the element type is that of apply_obstacles_kernel
template <typename T>
__global__ __launch_bounds__(kBlock) void sdf_apply_kernel(VelGrid g, double lower0, double lower1, double lower2, SdfView w, PatchBox pb, Comp3<T> vel) {
    const double lower[3] = {lower0, lower1, lower2};
    const int b = blockIdx.y;
    double r2 = 0;   // bounding radius of a face cell: |half size of a grid cell|
    for (int a = g.ax0; a < 3; ++a) r2 += 0.25 * g.dx[a] * g.dx[a];
    const double radius = sqrt(r2);
    const int tx = threadIdx.x & (kPatchCols - 1), ty = threadIdx.x / kPatchCols;
    const int npatch = pb.first[3];
    for (int patch = blockIdx.x; patch < npatch; patch += gridDim.x) {
        int ca, i0, r0, cc0;
        decode_box_patch(pb, patch, ca, i0, r0, cc0);          // slot = component (uniform)
        const int c0n = g.cn[ca][0], c1 = g.cn[ca][1], c2 = g.cn[ca][2];
        const int idx[3] = {i0, r0 + ty, cc0 + tx};
        if (idx[0] >= c0n || idx[1] >= c1 || idx[2] >= c2) continue;
        T* __restrict__ V = (ca == 0 ? vel.p[0] : (ca == 1 ? vel.p[1] : vel.p[2])) + (long long)b * g.ccells[ca];
        double x[3] = {0, 0, 0};
        for (int a = g.ax0; a < 3; ++a) x[a] = a == ca ? lower[a] + (double)(idx[a] + g.off[a]) * g.dx[a] : lower[a] + (idx[a] + 0.5) * g.dx[a];
        double m = 1.0 - sdf_distance(w, x, g.ax0) / radius;
        m = m < 0.0 ? 0.0 : (m > 1.0 ? 1.0 : m);
        if (m == 0.0) continue;                                 // keep = 1, nothing added: the sample keeps its bits
        const long long f = ((long long)i0 * c1 + idx[1]) * c2 + idx[2];
        T val = V[f];
        const T mt = (T)m, keep = T(1) - mt;
        val = keep == T(0) ? T(0) : keep * val;                 // safe_mul(1 - mask, velocity)
        if (w.moving && mt != T(0)) val += mt * (T)w.vel[ca];   // safe_mul(mask, obstacle.velocity)
        V[f] = val;
    }
}

// sample_sdf (:279, :295): out = min over the members of approximate_signed_distance at the cell centres of the SDF grid `w`
template <typename T>
__global__ __launch_bounds__(kBlock) void sdf_from_analytic_kernel(SdfView w, int ax0, ObstacleSet s, int first_chunk, T* out) {
    const long long cells = (long long)w.n[0] * w.n[1] * w.n[2];
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < cells; i += (long long)gridDim.x * kBlock) {
        const long long row = i / w.n[2];
        const int idx[3] = {(int)(row / w.n[1]), (int)(row % w.n[1]), (int)(i - row * w.n[2])};
        double x[3] = {0, 0, 0};
        for (int a = ax0; a < 3; ++a) x[a] = w.lower[a] + (idx[a] + 0.5) * (w.size[a] / (double)w.n[a]);
        double d = first_chunk ? 1e300 : (double)out[i];
        for (int k = 0; k < s.count; ++k) {
            const double dk = obstacle_sdf(s, k, x, ax0);
            d = dk < d ? dk : d;
        }
        out[i] = (T)d;
    }
}

static bool sdf_lookup(phihip_ctx* ctx, const phihip_obstacle& o, const phihip_sdf_grid** out) {
    if (o.reserved < 0 || o.reserved >= PHIHIP_SDF_SLOTS || !ctx->sdf_bound[o.reserved]) return false;
    *out = &ctx->sdf_slots[o.reserved];
    return true;
}

// end of the maximal run of analytic entries starting at `first`
static int analytic_run_end(const phihip_obstacle* obs, int first, int count) {
    int e = first;
    while (e < count && obs[e].kind != PHIHIP_OBSTACLE_SDF) ++e;
    return e;
}

static int run_sdf_accessible(phihip_ctx* ctx, const GridView& v, const phihip_obstacle& o, uint8_t* accessible, hipStream_t s) {
    const phihip_sdf_grid* d = nullptr;
    PHIHIP_REQUIRE(sdf_lookup(ctx, o, &d), "obstacle_accessible: SDF slot %d is not bound", o.reserved);
    PHIHIP_REQUIRE(d->rank == v.rank, "obstacle_accessible: SDF grid of rank %d on a grid of rank %d", d->rank, v.rank);
    const VelGrid g = make_velgrid(v);
    const SdfView w = make_sdf_view(v, *d, o);
    PatchBox pb;
    memset(&pb, 0, sizeof(pb));
    sdf_patch_slot(v, w, -1, 1e-6 * (v.dx[2] + v.dx[1]), 2, &pb);
    const long long np = (long long)pb.n0[2] * pb.np1[2] * pb.np2[2];
    PHIHIP_REQUIRE(np < (1LL << 31), "obstacle_accessible: grid too large");
    pb.first[3] = (int)np;
    if (np > 0) {
        const int nblk = np < 4096 ? (int)np : 4096;
        hipLaunchKernelGGL(sdf_accessible_kernel, dim3(nblk), dim3(kBlock), 0, s, g, v.lower[0], v.lower[1], v.lower[2], w, pb, accessible);
    }
    return PHIHIP_OK;
}

static int run_sdf_apply(phihip_ctx* ctx, const GridView& v, const phihip_obstacle& o, void* const vel[3], hipStream_t s) {
    const phihip_sdf_grid* d = nullptr;
    PHIHIP_REQUIRE(sdf_lookup(ctx, o, &d), "apply_obstacles: SDF slot %d is not bound", o.reserved);
    PHIHIP_REQUIRE(d->rank == v.rank, "apply_obstacles: SDF grid of rank %d on a grid of rank %d", d->rank, v.rank);
    const VelGrid g = make_velgrid(v);
    const SdfView w = make_sdf_view(v, *d, o);
    double r2 = 0;
    for (int a = v.ax0; a < 3; ++a) r2 += 0.25 * v.dx[a] * v.dx[a];
    const double radius = sqrt(r2);
    PatchBox pb;
    memset(&pb, 0, sizeof(pb));
    long long total = 0;
    for (int ca = 0; ca < 3; ++ca) {
        pb.first[ca] = (int)total;
        if (ca >= v.ax0) {
            sdf_patch_slot(v, w, ca, radius * 1.00001, ca, &pb);
            total += (long long)pb.n0[ca] * pb.np1[ca] * pb.np2[ca];
        }
        PHIHIP_REQUIRE(total < (1LL << 31), "apply_obstacles: grid too large");
    }
    pb.first[3] = (int)total;
    if (total == 0) return PHIHIP_OK;
    const int nblk = total < 4096 ? (int)total : 4096;
    with_dtype(v, [&](auto t) {
        using T = typename decltype(t)::type;
        Comp3<T> c{{(T*)vel[0], (T*)vel[1], (T*)vel[2]}};
        hipLaunchKernelGGL(sdf_apply_kernel<T>, dim3(nblk, v.batch), dim3(kBlock), 0, s, g, v.lower[0], v.lower[1], v.lower[2], w, pb, c);
    });
    return PHIHIP_OK;
}

int run_sdf_from_analytic(phihip_ctx* ctx, const GridView& v, const phihip_sdf_grid& d, const phihip_obstacle* obs, int count, void* out, hipStream_t s) {
    LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
    phihip_obstacle still;
    memset(&still, 0, sizeof(still));
    const SdfView w = make_sdf_view(v, d, still);
    const long long cells = (long long)w.n[0] * w.n[1] * w.n[2];
    const int nblk = ceil_div(cells, kBlock) < 8192 ? ceil_div(cells, kBlock) : 8192;
    for (int first = 0; first < count; first += kObstaclesPerLaunch) {
        const int n = count - first < kObstaclesPerLaunch ? count - first : kObstaclesPerLaunch;
        const ObstacleSet set = make_obstacle_set(v, obs, first, n);
        if (w.f64)
            hipLaunchKernelGGL(sdf_from_analytic_kernel<double>, dim3(nblk), dim3(kBlock), 0, s, w, v.ax0, set, first == 0 ? 1 : 0, (double*)out);
        else
            hipLaunchKernelGGL(sdf_from_analytic_kernel<float>, dim3(nblk), dim3(kBlock), 0, s, w, v.ax0, set, first == 0 ? 1 : 0, (float*)out);
    }
    PHIHIP_CHECK_HIP(hipGetLastError());
    return PHIHIP_OK;
}
