// multigrid.hpp -- Solve(..., preconditioner='multigrid'): CG on the masked pressure operator, preconditioned by ONE geometric multigrid
// V-cycle per iteration (PHIHIP_METHOD_CG_MULTIGRID). Included by cg.hip (the emulation build of the tests compiles the .hip files by name:
// no translation unit of its own).
//
// The operator. A = fluid.masked_laplace (phi/physics/fluid.py:165-202) is negative semidefinite on the active cells and the identity on
// inactive ones. The cycle works on P = -A restricted to the active cells (symmetric positive semidefinite, inactive neighbours and OPEN
// walls act as zero ghosts) and returns z = M r with M ~ A^-1: z = -(V-cycle of P)(r) on active cells, z = r on inactive cells. M is a fixed
// symmetric linear operator with the sign of A, so CG's alpha = r.z / d.Ad and beta = r'.z' / r.z keep their signs.
//
// The recipe (prototyped in NumPy on this operator; DESIGN.md "f6"):
//   levels      cell-centred coarsening n -> ceil(n / 2) per axis until the smallest axis has <= coarsest_cells (4) cells. Coarse operators are
//               the GALERKIN operators of piecewise-constant prolongation: coupling of a coarse face = sum of the fine couplings on it, diagonal =
//               sum of the children's diagonals - 2 x the couplings inside the coarse cell. A coarse level stores the diagonal and one coupling
//               array per axis (towards the upper neighbour; both include 1 / dx^2), i.e. it is symmetric by construction; a cell with a zero
//               diagonal is inactive. The fine level reads the flag byte (or the boundary rules when there are no flags).
//   transfer    restriction = sum over the children (P^T), prolongation = copy to the children TIMES 2 (over-correction: without it the
//               iteration count grows with the resolution).
//   smoother    damped Jacobi, omega = 0.8, `sweeps` (2) before and after the coarse correction -- equal counts keep the cycle symmetric; the
//               first pre-sweep starts from zero (x = omega b / diag, no stencil). Coarsest level: 2 x 30 sweeps by ONE workgroup per entry.
//   hierarchy   rebuilt by nlevels - 1 small kernels at the start of every solve (moving obstacles change the flags every step), no read-back.
// Kernels: one generic set used on every level, one thread per cell, every workgroup owning one contiguous chunk of cells, at most kMgBlocks workgroups per batch entry
// (bounded so that the next kernel's prologue re-reduces at most that many partial sums). The plain form: residual + restriction are one pass
// (a thread per COARSE cell sums the residuals of its children, r is never stored), prolongation is a pass of its own.
//
// The PCG loop is device-driven like cg_t / coef_cg_t: alpha, beta and the continue flags never reach the host, partial sums are re-reduced
// in a fixed order in the next kernel's prologue (deterministic, no atomics). Per iteration:
//   V-cycle   z = M r ; sum r.z          (first kernel folds sum r^2 of the last UPDATE: PhiML's convergence / divergence tests on the PLAIN residual)
//   MATVEC    d_new = z + beta d_old ; sum d.Ad        beta = r.z / (r.z)_old
//   UPDATE    x += alpha d ; r -= alpha A d ; sum r^2  alpha = r.z / d.Ad      (every refresh_every-th iteration: x += alpha d ; r = y - A x)
// CgState::sigma carries r.z between the iterations.
#pragma once

namespace phihip {

constexpr int kMgMaxLevels = 16;
constexpr int kMgLdsCells = 2048;   // coarsest levels up to this size are smoothed in LDS
constexpr int kMgBlocks = 2048;      // workgroups per batch entry at most (8 per CU)

enum MgPrologue { PRO_MG_BETA = 100, PRO_MG_ALPHA = 101 };

struct MgLevel {
    int n[3];              // cells per internal axis (n[0] == 1 for 2-D grids)
    int nb[3][2];          // NeighbourRule of the pressure per internal axis / side (NB_WRAP / NB_CLAMP / NB_ZERO), the same on every level
    int ax0;
    int coef_batch;        // 1: the flags / coefficient arrays have a batch dimension
    int cells;
    double w[3];           // 1 / dx^2 of the FINE level (0 on unused axes)
};

template <typename T>
struct MgCoef {
    const uint8_t* flags;  // fine level: flag bytes or nullptr (no obstacles: bits from the boundary rules)
    const T* D;            // coarse level: diagonal of P (>= 0; 0 = inactive cell)
    const T* C[3];         // coarse level: coupling with the UPPER neighbour per axis (wraps on periodic axes)
};

__device__ __forceinline__ void mg_coords(const MgLevel& L, int c, int (&i)[3]) {
    i[2] = c % L.n[2];
    const int t = c / L.n[2];
    i[1] = t % L.n[1];
    i[0] = t / L.n[1];
}
__device__ __forceinline__ int mg_stride(const MgLevel& L, int a) { return a == 2 ? 1 : (a == 1 ? L.n[2] : L.n[1] * L.n[2]); }

// The cells a workgroup owns: one CONTIGUOUS chunk (a multiple of the block size), chunks dealt to the XCDs in contiguous ranges (xcd_order) so that the
// rows and planes a chunk's stencil reaches into are fetched by workgroups of the same XCD at about the same time and meet in its L2.
struct MgRange {
    int begin, end;
};
__device__ __forceinline__ MgRange mg_range(int cells) {
    const int nblk = (int)gridDim.x;
    const int chunk = ((cells + nblk - 1) / nblk + kBlock - 1) / kBlock * kBlock;
    const long long begin = (long long)xcd_order((int)blockIdx.x, nblk) * chunk;
    MgRange r;
    r.begin = begin < cells ? (int)begin : cells;
    r.end = begin + chunk < cells ? (int)(begin + chunk) : cells;
    return r;
}

// the fine level's flag byte: bit 2 * axis + side = the face carries flux, bit 6 = active (include/phihip.h phihip_build_cellflags)
__device__ __forceinline__ unsigned mg_fine_bits(const MgLevel& L, const uint8_t* flags, long long fb, int c, const int (&i)[3]) {
    if (flags) {
        unsigned f = flags[fb + c];
        if (L.ax0 > 0) f &= ~3u;
        return f;
    }
    unsigned f = 64u;
    for (int a = L.ax0; a < 3; ++a) {
        if (i[a] > 0 || L.nb[a][0] != NB_CLAMP) f |= 1u << (2 * a);
        if (i[a] < L.n[a] - 1 || L.nb[a][1] != NB_CLAMP) f |= 2u << (2 * a);
    }
    return f;
}

// index of the neighbour of cell c on (axis a, side): >= 0 stored cell (wrapped on periodic axes), -1 zero ghost, -2 no neighbour (closed wall)
__device__ __forceinline__ int mg_neighbour(const MgLevel& L, int a, int side, int ia, int c) {
    const int s = mg_stride(L, a), n = L.n[a];
    const int j = ia + (side ? 1 : -1);
    if (j >= 0 && j < n) return c + (side ? s : -s);
    const int rule = L.nb[a][side];
    if (rule == NB_WRAP) return c + (side ? -(n - 1) * s : (n - 1) * s);
    return rule == NB_ZERO ? -1 : -2;
}

// diagonal of P at a fine cell from its flag byte (0: inactive)
template <typename T>
__device__ __forceinline__ T mg_fine_diag(const MgLevel& L, const T (&w)[3], unsigned f, const int (&i)[3]) {
    if (!(f & 64u)) return T(0);
    T d = T(0);
    for (int a = L.ax0; a < 3; ++a)
        for (int side = 0; side < 2; ++side) {
            if (!(f & (1u << (2 * a + side)))) continue;
            const int j = i[a] + (side ? 1 : -1);
            if ((j < 0 || j >= L.n[a]) && L.nb[a][side] == NB_CLAMP) continue;
            d += w[a];
        }
    return d;
}

// (P x)(c) and the diagonal on either kind of level. X = this batch entry's vector, ZERO on inactive cells; cb = offset of the entry's coefficients.
template <typename T, bool FINE>
__device__ __forceinline__ T mg_row(const MgLevel& L, const MgCoef<T>& A, const T (&w)[3], long long cb, int c, const int (&i)[3], const T* __restrict__ X, T xi, T& diag) {
    if (FINE) {
        // every neighbour load is issued before the flag byte is looked at (no load waits for a branch on another load's result)
        int nbi[3][2];
        T xn[3][2];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                nbi[a][side] = a < L.ax0 ? -2 : mg_neighbour(L, a, side, i[a], c);
                xn[a][side] = X[nbi[a][side] >= 0 ? nbi[a][side] : c];
            }
        const unsigned f = mg_fine_bits(L, A.flags, cb, c, i);
        const bool act = (f & 64u) != 0;
        T acc = T(0);
        diag = T(0);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const bool on = act && (f & (1u << (2 * a + side))) && nbi[a][side] != -2;
                const T v = nbi[a][side] >= 0 ? xn[a][side] : T(0);
                diag += on ? w[a] : T(0);
                acc += on ? w[a] * (xi - v) : T(0);
            }
        return acc;
    }
    diag = A.D[cb + c];
    T acc = diag * xi;
    for (int a = L.ax0; a < 3; ++a) {
        const int hi = mg_neighbour(L, a, 1, i[a], c), lo = mg_neighbour(L, a, 0, i[a], c);
        if (hi >= 0) acc -= A.C[a][cb + c] * X[hi];
        if (lo >= 0) acc -= A.C[a][cb + lo] * X[lo];
    }
    return acc;
}

template <typename T, bool FINE>
__device__ __forceinline__ T mg_diag(const MgLevel& L, const MgCoef<T>& A, const T (&w)[3], long long cb, int c, const int (&i)[3]) {
    if (FINE) return mg_fine_diag<T>(L, w, mg_fine_bits(L, A.flags, cb, c, i), i);
    return A.D[cb + c];
}

// ---- hierarchy: Galerkin coarsening of level `Lf` into the arrays of the next level --------------------------------------------------------------
template <typename T, bool FINE>
__global__ __launch_bounds__(kBlock) void mg_coarsen_kernel(MgLevel Lf, MgCoef<T> Af, MgLevel Lc, T* Dc, T* Cc0, T* Cc1, T* Cc2) {
    const int b = blockIdx.y;
    const long long fb = (long long)b * Lf.cells, cb = (long long)b * Lc.cells;
    T w[3];
    for (int a = 0; a < 3; ++a) w[a] = (T)Lf.w[a];
    T* Cc[3] = {Cc0, Cc1, Cc2};
    const MgRange rg = mg_range(Lc.cells);
    for (int c = rg.begin + threadIdx.x; c < rg.end; c += kBlock) {
        int I[3];
        mg_coords(Lc, c, I);
        T dsum = T(0), dpos = T(0), csum[3] = {T(0), T(0), T(0)};
        const int k0n = Lf.ax0 <= 0 ? 2 : 1, k1n = Lf.ax0 <= 1 ? 2 : 1;
        for (int k0 = 0; k0 < k0n; ++k0)
            for (int k1 = 0; k1 < k1n; ++k1)
                for (int k2 = 0; k2 < 2; ++k2) {
                    const int k[3] = {k0, k1, k2};
                    int j[3];
                    bool inside = true;
                    for (int a = 0; a < 3; ++a) {
                        j[a] = a < Lf.ax0 ? 0 : 2 * I[a] + k[a];
                        inside = inside && j[a] < Lf.n[a];
                    }
                    if (!inside) continue;
                    const int cf = (j[0] * Lf.n[1] + j[1]) * Lf.n[2] + j[2];
                    unsigned f = 0u;
                    T dj;
                    if (FINE) {
                        f = mg_fine_bits(Lf, Af.flags, fb, cf, j);
                        dj = mg_fine_diag<T>(Lf, w, f, j);
                    } else {
                        dj = Af.D[fb + cf];
                    }
                    if (!(dj > T(0))) continue;
                    dsum += dj;
                    dpos += dj;
                    for (int a = Lf.ax0; a < 3; ++a) {
                        // coupling of child j with its upper neighbour on axis a
                        T ch = T(0);
                        if (FINE) {
                            const int nbi = mg_neighbour(Lf, a, 1, j[a], cf);
                            if ((f & (2u << (2 * a))) && nbi >= 0) {
                                int jn[3] = {j[0], j[1], j[2]};
                                jn[a] = j[a] + 1 < Lf.n[a] ? j[a] + 1 : 0;
                                const unsigned fn = mg_fine_bits(Lf, Af.flags, fb, nbi, jn);
                                if (fn & 64u) ch = w[a];      // (an inactive neighbour is a zero ghost: it stays in the diagonal only)
                            }
                        } else {
                            ch = Af.C[a][fb + cf];
                        }
                        if (k[a] == 0 && j[a] + 1 < Lf.n[a]) dsum -= T(2) * ch;     // a face inside the coarse cell
                        else csum[a] += ch;                                          // the last child on this axis: a face of the coarse cell
                    }
                }
        // a periodic axis with ONE coarse cell couples the cell with itself
        for (int a = Lf.ax0; a < 3; ++a)
            if (Lc.n[a] == 1) { dsum -= T(2) * csum[a]; csum[a] = T(0); }
        // a coarse cell without any coupling to the outside (an enclosed pocket) has a zero diagonal in exact arithmetic: what the cancellation leaves
        // of it must not pass for an active cell
        Dc[cb + c] = dsum > T(1e-4) * dpos ? dsum : T(0);
        for (int a = Lf.ax0; a < 3; ++a) Cc[a][cb + c] = csum[a];
    }
}

// ---- smoother -----------------------------------------------------------------------------------------------------------------------------------------
enum MgSmoothMode {
    MG_FIRST = 0,      // xout = omega b / diag (the sweep that starts from zero)
    MG_JACOBI = 1,     // xout = xin + omega (b - P xin) / diag
    MG_FINAL = 2       // fine level, last sweep: z = -(Jacobi result) on active cells, z = b on inactive cells ; part = sum b z
};

template <typename T>
struct MgArgs {
    const T* b;
    const T* xin;
    T* xout;
    T omega;
    int prologue;              // CgPrologue: PRO_NONE (stand-alone cycle), PRO_CONT, or PRO_FIRST / PRO_BETA in the first kernel of a cycle
    const CgState* st_in;
    CgState* st_out;
    const double* pin1;
    const double* pin2;
    int nblk_in;
    CgParams prm;
    double* part;              // MG_FINAL: [batch][gridDim.x] partial sums of r.z
    int sweeps;                // coarsest-level kernel: number of sweeps
};

// prologue of every kernel of a cycle: returns false for a frozen batch entry
template <typename T>
__device__ __forceinline__ bool mg_enter(const MgArgs<T>& p, int b, bool writer, double* red, CgState* sh) {
    if (p.prologue == PRO_NONE) return true;
    const CgState S = cg_prologue(p.prologue, p.st_in, p.st_out, p.pin1, p.pin2, p.nblk_in, p.prm, b, writer, red, sh);
    return S.cont != 0;
}

template <typename T, bool FINE, int MODE>
__global__ __launch_bounds__(kBlock) void mg_smooth_kernel(MgLevel L, MgCoef<T> A, MgArgs<T> p) {
    __shared__ double red[kBlock / kWave];
    __shared__ CgState sh_state;
    const int b = blockIdx.y;
    if (!mg_enter(p, b, blockIdx.x == 0, red, &sh_state)) return;
    const long long vb = (long long)b * L.cells, cb = L.coef_batch ? vb : 0;
    const T* __restrict__ B = p.b + vb;
    const T* __restrict__ X = MODE == MG_FIRST ? nullptr : p.xin + vb;
    T* __restrict__ O = p.xout + vb;
    T w[3];
    for (int a = 0; a < 3; ++a) w[a] = (T)L.w[a];
    double acc = 0;
    const MgRange rg = mg_range(L.cells);
    for (int c = rg.begin + threadIdx.x; c < rg.end; c += kBlock) {
        int i[3];
        mg_coords(L, c, i);
        const T bi = B[c];
        T xn;
        bool active;
        if (MODE == MG_FIRST) {
            const T d = mg_diag<T, FINE>(L, A, w, cb, c, i);
            active = d > T(0);
            xn = active ? p.omega * bi / d : T(0);
        } else {
            const T xi = X[c];
            T d;
            const T q = mg_row<T, FINE>(L, A, w, cb, c, i, X, xi, d);
            active = d > T(0);
            xn = active ? xi + p.omega * (bi - q) / d : T(0);
        }
        if (MODE == MG_FINAL) {
            const T z = active ? -xn : bi;
            O[c] = z;
            acc += (double)bi * (double)z;
        } else {
            O[c] = xn;
        }
    }
    if (MODE == MG_FINAL) {
        const double t = block_sum(acc, red);
        if (threadIdx.x == 0) p.part[(long long)b * gridDim.x + blockIdx.x] = t;
    }
}

// coarsest level: `sweeps` Jacobi sweeps from zero by ONE workgroup per batch entry (the level lives in L2; a barrier per sweep instead of a launch).
// The iterate alternates between xa and xb; the LAST sweep writes xa.
template <typename T, bool FINE>
__global__ __launch_bounds__(kBlock) void mg_coarsest_kernel(MgLevel L, MgCoef<T> A, MgArgs<T> p, T* xa, T* xb) {
    __shared__ double red[kBlock / kWave];
    __shared__ CgState sh_state;
    const int b = blockIdx.x;
    if (!mg_enter(p, b, true, red, &sh_state)) return;
    const long long vb = (long long)b * L.cells, cb = L.coef_batch ? vb : 0;
    const T* __restrict__ B = p.b + vb;
    T w[3];
    for (int a = 0; a < 3; ++a) w[a] = (T)L.w[a];
    // a level of at most kMgLdsCells cells keeps both iterates in LDS (a sweep then costs an LDS round trip instead of one through L2)
    __shared__ T lds[2 * kMgLdsCells];
    const bool in_lds = L.cells <= kMgLdsCells;
    T* const pa = in_lds ? lds : xa + vb;
    T* const pb = in_lds ? lds + kMgLdsCells : xb + vb;
    for (int sweep = 0; sweep < p.sweeps; ++sweep) {
        const bool to_a = ((p.sweeps - 1 - sweep) & 1) == 0;
        const T* X = to_a ? pb : pa;
        T* O = to_a ? pa : pb;
        for (int c = threadIdx.x; c < L.cells; c += kBlock) {
            int i[3];
            mg_coords(L, c, i);
            const T bi = B[c];
            T xn;
            if (sweep == 0) {
                const T d = mg_diag<T, FINE>(L, A, w, cb, c, i);
                xn = d > T(0) ? p.omega * bi / d : T(0);
            } else {
                const T xi = X[c];
                T d;
                const T q = mg_row<T, FINE>(L, A, w, cb, c, i, X, xi, d);
                xn = d > T(0) ? xi + p.omega * (bi - q) / d : T(0);
            }
            O[c] = xn;
        }
        __threadfence();
        __syncthreads();
    }
    if (in_lds)
        for (int c = threadIdx.x; c < L.cells; c += kBlock) xa[vb + c] = pa[c];
}

// ---- transfer -----------------------------------------------------------------------------------------------------------------------------------------
// residual + restriction in one pass: bc(I) = sum over the active children j of I of (b - P x)(j)
template <typename T, bool FINE>
__global__ __launch_bounds__(kBlock) void mg_restrict_kernel(MgLevel Lf, MgCoef<T> Af, MgArgs<T> p, MgLevel Lc, T* bc) {
    __shared__ double red[kBlock / kWave];
    __shared__ CgState sh_state;
    const int b = blockIdx.y;
    if (!mg_enter(p, b, false, red, &sh_state)) return;
    const long long vb = (long long)b * Lf.cells, cb = Lf.coef_batch ? vb : 0;
    const T* __restrict__ B = p.b + vb;
    const T* __restrict__ X = p.xin + vb;
    T w[3];
    for (int a = 0; a < 3; ++a) w[a] = (T)Lf.w[a];
    const int k0n = Lf.ax0 <= 0 ? 2 : 1, k1n = Lf.ax0 <= 1 ? 2 : 1;
    const MgRange rg = mg_range(Lc.cells);
    for (int c = rg.begin + threadIdx.x; c < rg.end; c += kBlock) {
        int I[3];
        mg_coords(Lc, c, I);
        T sum = T(0);
        for (int k0 = 0; k0 < k0n; ++k0)
            for (int k1 = 0; k1 < k1n; ++k1)
                for (int k2 = 0; k2 < 2; ++k2) {
                    const int k[3] = {k0, k1, k2};
                    int j[3];
                    bool inside = true;
                    for (int a = 0; a < 3; ++a) {
                        j[a] = a < Lf.ax0 ? 0 : 2 * I[a] + k[a];
                        inside = inside && j[a] < Lf.n[a];
                    }
                    if (!inside) continue;
                    const int cf = (j[0] * Lf.n[1] + j[1]) * Lf.n[2] + j[2];
                    T d;
                    const T q = mg_row<T, FINE>(Lf, Af, w, cb, cf, j, X, X[cf], d);
                    if (d > T(0)) sum += B[cf] - q;
                }
        bc[(long long)b * Lc.cells + c] = sum;
    }
}

// x += 2 * (coarse correction of the parent) on active cells
template <typename T, bool FINE>
__global__ __launch_bounds__(kBlock) void mg_prolong_kernel(MgLevel Lf, MgCoef<T> Af, MgArgs<T> p, MgLevel Lc, const T* ec) {
    __shared__ double red[kBlock / kWave];
    __shared__ CgState sh_state;
    const int b = blockIdx.y;
    if (!mg_enter(p, b, false, red, &sh_state)) return;
    const long long vb = (long long)b * Lf.cells, cb = Lf.coef_batch ? vb : 0;
    T* __restrict__ X = p.xout + vb;
    const T* __restrict__ E = ec + (long long)b * Lc.cells;
    T w[3];
    for (int a = 0; a < 3; ++a) w[a] = (T)Lf.w[a];
    const MgRange rg = mg_range(Lf.cells);
    for (int c = rg.begin + threadIdx.x; c < rg.end; c += kBlock) {
        int i[3];
        mg_coords(Lf, c, i);
        const T d = mg_diag<T, FINE>(Lf, Af, w, cb, c, i);
        if (!(d > T(0))) continue;
        const int cc = ((i[0] >> (Lf.ax0 <= 0 ? 1 : 0)) * Lc.n[1] + (i[1] >> (Lf.ax0 <= 1 ? 1 : 0))) * Lc.n[2] + (i[2] >> 1);
        X[c] += T(2) * E[cc];
    }
}

// ---- the PCG phases on the fine level: the operator A itself (identity on inactive cells, true neighbour values) -----------------------------------
enum MgCgMode {
    MGC_RESID = 0,     // o1 = r = b - A a ; part1 = sum r^2, part2 = sum b^2 (optional)
    MGC_MATVEC = 1,    // S = a + beta b ; o1 = S ; part1 = sum S (A S)
    MGC_UPDATE = 2,    // S = a ; o1 += alpha S ; o2 -= alpha A S ; part1 = sum o2^2
    MGC_AXPY = 3       // o1 += alpha a (the true-residual refresh step: x only)
};

template <typename T>
struct MgCgArgs {
    const T* a;
    const T* b;
    T* o1;
    T* o2;
    const uint8_t* flags;
    const CgState* st_in;
    CgState* st_out;
    const double* pin1;
    const double* pin2;
    int nblk_in;
    double* part1;
    double* part2;
    CgParams prm;
    int prologue;          // CgPrologue or MgPrologue
    unsigned long long* host_flags;
    unsigned int seq;
};

// control block of the preconditioned recurrence: PRO_MG_BETA folds sum r.z (beta = r.z / (r.z)_old, kept in sigma), PRO_MG_ALPHA folds sum d.Ad
// (alpha = r.z / d.Ad, iteration count); everything else is cg_prologue
__device__ __forceinline__ CgState mg_prologue(int kind, const CgState* st_in, CgState* st_out, const double* pin1, const double* pin2, int nblk,
                                              const CgParams& prm, int b, bool writer, double* red, CgState* sh) {
    if (kind != PRO_MG_BETA && kind != PRO_MG_ALPHA) return cg_prologue(kind, st_in, st_out, pin1, pin2, nblk, prm, b, writer, red, sh);
    CgState s = CgState();
    if (threadIdx.x == 0) s = st_in[b];
    const double s1 = reduce_partials(pin1 + (long long)b * nblk, nblk, red);
    if (threadIdx.x == 0) {
        if (s.cont) {
            if (kind == PRO_MG_BETA) {
                s.beta = (s.iterations > 0 && s.sigma != 0) ? s1 / s.sigma : 0;
                s.sigma = s1;
            } else {
                s.iterations += 1;
                s.dq = s1;
                s.alpha_prev = s.alpha;
                s.alpha = s1 != 0 ? s.sigma / s1 : 0;
            }
        }
        *sh = s;
        if (writer) st_out[b] = s;
    }
    __syncthreads();
    return *sh;
}

template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void mg_cg_kernel(MgLevel L, MgCgArgs<T> p) {
    __shared__ double red[2 * kBlock / kWave];
    __shared__ CgState sh_state;
    const int b = blockIdx.y;
    T alpha = T(0), beta = T(0);
    if (p.prologue != PRO_NONE) {
        const CgState S = mg_prologue(p.prologue, p.st_in, p.st_out, p.pin1, p.pin2, p.nblk_in, p.prm, b, blockIdx.x == 0, red, &sh_state);
        if (MODE == MGC_MATVEC && p.host_flags && blockIdx.x == 0 && threadIdx.x == 0)   // the host stops enqueueing once every entry reports 0
            publish_flag(p.host_flags + b, ((unsigned long long)p.seq << 32) | (unsigned long long)(S.cont != 0));
        if (S.cont == 0) return;   // frozen batch entry (uniform per workgroup)
        alpha = (T)S.alpha;
        beta = (T)S.beta;
    }
    const long long vb = (long long)b * L.cells, fb = L.coef_batch ? vb : 0;
    const T* __restrict__ A = p.a + vb;
    const T* __restrict__ B = p.b ? p.b + vb : nullptr;
    T w[3];
    for (int a = 0; a < 3; ++a) w[a] = (T)L.w[a];
    auto src = [&](int c) -> T { return MODE == MGC_MATVEC ? A[c] + beta * B[c] : A[c]; };
    double acc1 = 0, acc2 = 0;
    const MgRange rg = mg_range(L.cells);
    for (int c = rg.begin + threadIdx.x; c < rg.end; c += kBlock) {
        const T sc = src(c);
        if (MODE == MGC_AXPY) {
            p.o1[vb + c] = fma(alpha, sc, p.o1[vb + c]);
            continue;
        }
        int i[3];
        mg_coords(L, c, i);
        int nbi[3][2];
        T sn[3][2];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                nbi[a][side] = a < L.ax0 ? -2 : mg_neighbour(L, a, side, i[a], c);
                sn[a][side] = src(nbi[a][side] >= 0 ? nbi[a][side] : c);
            }
        const unsigned f = mg_fine_bits(L, p.flags, fb, c, i);
        T q = T(0);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const bool on = (f & (1u << (2 * a + side))) && nbi[a][side] != -2;
                const T v = nbi[a][side] >= 0 ? sn[a][side] : T(0);
                q += on ? (v - sc) * w[a] : T(0);
            }
        if (!(f & 64u)) q = sc;   // inactive cell: identity row (fluid.py:202)
        if (MODE == MGC_RESID) {
            const T y = B[c];
            const T r = y - q;
            p.o1[vb + c] = r;
            acc1 += (double)r * (double)r;
            acc2 += (double)y * (double)y;
        } else if (MODE == MGC_MATVEC) {
            p.o1[vb + c] = sc;
            acc1 += (double)sc * (double)q;
        } else if (MODE == MGC_UPDATE) {
            p.o1[vb + c] = fma(alpha, sc, p.o1[vb + c]);
            const T r = fma(-alpha, q, p.o2[vb + c]);
            p.o2[vb + c] = r;
            acc1 += (double)r * (double)r;
        }
    }
    if (MODE != MGC_AXPY) {
        double t[2] = {acc1, acc2};
        block_sum_n<2>(t, red);
        if (threadIdx.x == 0) {
            const long long o = (long long)b * gridDim.x + blockIdx.x;
            p.part1[o] = t[0];
            if (p.part2) p.part2[o] = t[1];
        }
    }
}

// control block after the loop (fold the last reduction)
__global__ __launch_bounds__(kBlock) void mg_state_kernel(int kind, const CgState* st_in, CgState* st_out, const double* pin1, const double* pin2, int nblk,
                                                          CgParams prm) {
    __shared__ double red[kBlock / kWave];
    __shared__ CgState sh;
    cg_prologue(kind, st_in, st_out, pin1, pin2, nblk, prm, blockIdx.x, true, red, &sh);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
static inline int mg_blocks(int cells) {
    const int n = ceil_div(cells, kBlock);
    return n < kMgBlocks ? (n < 1 ? 1 : n) : kMgBlocks;
}

template <typename T>
struct MgHierarchy {
    int nlev;
    int batch, coef_batch;
    MgLevel L[kMgMaxLevels];
    MgCoef<T> A[kMgMaxLevels];
    T* D[kMgMaxLevels];
    T* C[kMgMaxLevels][3];
    T* X[kMgMaxLevels];      // the level's result (level 0: z)
    T* Tm[kMgMaxLevels];     // smoothing temporary
    T* B[kMgMaxLevels];      // right-hand side (level 0: r)
};

// level geometry + workspace (grown on demand BEFORE the loop), then the nlev - 1 coarsening launches
template <typename T>
static int mg_build(phihip_ctx* ctx, const GridView& v, const uint8_t* flags, int mask_batch, MgHierarchy<T>* H, hipStream_t s) {
    if (v.cells > (1LL << 30)) { set_error("multigrid: more than 2^30 cells per batch entry are not supported"); return PHIHIP_ERR_UNSUPPORTED; }      // (int cell indices + the grid stride)
    memset(H, 0, sizeof(*H));
    H->batch = v.batch;
    H->coef_batch = (flags && mask_batch > 1) ? v.batch : 1;
    MgLevel& L0 = H->L[0];
    L0.ax0 = v.ax0;
    L0.coef_batch = H->coef_batch > 1 ? 1 : 0;
    L0.cells = (int)v.cells;
    for (int a = 0; a < 3; ++a) {
        L0.n[a] = v.n[a];
        L0.w[a] = a < v.ax0 ? 0.0 : 1.0 / (v.dx[a] * v.dx[a]);
        for (int side = 0; side < 2; ++side) {
            const int code = v.bc[a][side];
            L0.nb[a][side] = code == PHIHIP_BC_PERIODIC ? NB_WRAP : (code == PHIHIP_BC_CLOSED ? NB_CLAMP : NB_ZERO);
        }
    }
    const int stop = ctx->mg_coarsest > 1 ? ctx->mg_coarsest : 1;
    int nlev = 1;
    while (nlev < kMgMaxLevels) {
        const MgLevel& P = H->L[nlev - 1];
        int mn = P.n[2];
        for (int a = P.ax0; a < 3; ++a) mn = P.n[a] < mn ? P.n[a] : mn;
        if (mn <= stop) break;
        MgLevel& C = H->L[nlev];
        C = P;
        long long cells = 1;
        for (int a = 0; a < 3; ++a) {
            C.n[a] = a < P.ax0 ? 1 : (P.n[a] + 1) / 2;
            cells *= C.n[a];
        }
        C.cells = (int)cells;
        ++nlev;
    }
    H->nlev = nlev;
    // one buffer for every coarse level: D, C[3] per coefficient batch entry; X, Tm, B per batch entry (256-byte aligned pieces)
    auto al = [](size_t n) { return (n + 255) / 256 * 256; };
    size_t total = 0;
    for (int l = 1; l < nlev; ++l) total += 4 * al((size_t)H->coef_batch * H->L[l].cells * sizeof(T)) + 3 * al((size_t)v.batch * H->L[l].cells * sizeof(T));
    PHIHIP_TRY(ensure_buffer(ctx->ws_mg_levels, total > 0 ? total : 256));
    PHIHIP_TRY(ensure_buffer(ctx->ws_mg_t, (size_t)v.batch * v.cells * sizeof(T)));
    unsigned char* base = (unsigned char*)ctx->ws_mg_levels.ptr;
    size_t off = 0;
    auto take = [&](size_t bytes) { T* q = (T*)(base + off); off += al(bytes); return q; };
    H->A[0].flags = flags;
    H->Tm[0] = (T*)ctx->ws_mg_t.ptr;
    for (int l = 1; l < nlev; ++l) {
        const size_t cbytes = (size_t)H->coef_batch * H->L[l].cells * sizeof(T), vbytes = (size_t)v.batch * H->L[l].cells * sizeof(T);
        H->D[l] = take(cbytes);
        for (int a = 0; a < 3; ++a) H->C[l][a] = take(cbytes);
        H->X[l] = take(vbytes);
        H->Tm[l] = take(vbytes);
        H->B[l] = take(vbytes);
        H->A[l].flags = nullptr;
        H->A[l].D = H->D[l];
        for (int a = 0; a < 3; ++a) H->A[l].C[a] = H->C[l][a];
    }
    for (int l = 0; l + 1 < nlev; ++l) {
        LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
        const dim3 grid((unsigned)mg_blocks(H->L[l + 1].cells), (unsigned)H->coef_batch);
        if (l == 0)
            hipLaunchKernelGGL((mg_coarsen_kernel<T, true>), grid, dim3(kBlock), 0, s, H->L[0], H->A[0], H->L[1], H->D[1], H->C[1][0], H->C[1][1], H->C[1][2]);
        else
            hipLaunchKernelGGL((mg_coarsen_kernel<T, false>), grid, dim3(kBlock), 0, s, H->L[l], H->A[l], H->L[l + 1], H->D[l + 1], H->C[l + 1][0], H->C[l + 1][1],
                               H->C[l + 1][2]);
        PHIHIP_CHECK_HIP(hipGetLastError());
    }
    ctx->mg_last_levels = nlev;
    return PHIHIP_OK;
}

template <typename T, bool FINE>
static int mg_smooth_launch(phihip_ctx* ctx, const MgHierarchy<T>& H, int l, int mode, MgArgs<T> a, hipStream_t s, int* launches) {
    LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
    const dim3 grid((unsigned)mg_blocks(H.L[l].cells), (unsigned)H.batch);
    if (mode == MG_FIRST) hipLaunchKernelGGL((mg_smooth_kernel<T, FINE, MG_FIRST>), grid, dim3(kBlock), 0, s, H.L[l], H.A[l], a);
    else if (mode == MG_JACOBI) hipLaunchKernelGGL((mg_smooth_kernel<T, FINE, MG_JACOBI>), grid, dim3(kBlock), 0, s, H.L[l], H.A[l], a);
    else hipLaunchKernelGGL((mg_smooth_kernel<T, FINE, MG_FINAL>), grid, dim3(kBlock), 0, s, H.L[l], H.A[l], a);
    PHIHIP_CHECK_HIP(hipGetLastError());
    ++*launches;
    return PHIHIP_OK;
}

// One V-cycle: H.X[0] (z) = M H.B[0] (r), partial sums of r.z into `part_rz` (mg_blocks(fine cells) per batch entry). `first` describes the prologue of
// the cycle's first kernel (PRO_NONE: stand-alone, else PRO_FIRST / PRO_BETA with its partial sums: it advances the control block st_in -> st_out);
// the other kernels only read the continue flag of st_out.
template <typename T>
static int mg_vcycle(phihip_ctx* ctx, const MgHierarchy<T>& H, const MgArgs<T>& first, double* part_rz, hipStream_t s) {
    const int nu = ctx->mg_sweeps, last = H.nlev - 1;
    int launches = 0;
    MgArgs<T> cont;
    memset(&cont, 0, sizeof(cont));
    cont.omega = (T)ctx->mg_omega;
    cont.prologue = first.prologue == PRO_NONE ? PRO_NONE : PRO_CONT;
    cont.st_in = first.st_out;
    cont.prm = first.prm;
    bool used_first = false;
    auto args = [&]() {
        if (used_first) return cont;
        used_first = true;
        MgArgs<T> a = first;
        a.omega = (T)ctx->mg_omega;
        return a;
    };
    T* cur[kMgMaxLevels];
    // down: pre-smoothing, residual + restriction
    for (int l = 0; l < last; ++l) {
        // 2 nu sweeps alternate between Tm and X so that the last one writes X
        T* out = H.Tm[l];
        const T* in = nullptr;
        for (int k = 0; k < nu; ++k) {
            MgArgs<T> a = args();
            a.b = H.B[l]; a.xin = in; a.xout = out;
            if (l == 0) PHIHIP_TRY((mg_smooth_launch<T, true>(ctx, H, l, k == 0 ? MG_FIRST : MG_JACOBI, a, s, &launches)));
            else PHIHIP_TRY((mg_smooth_launch<T, false>(ctx, H, l, k == 0 ? MG_FIRST : MG_JACOBI, a, s, &launches)));
            in = out;
            out = out == H.Tm[l] ? H.X[l] : H.Tm[l];
        }
        cur[l] = (T*)in;
        MgArgs<T> a = args();
        a.b = H.B[l]; a.xin = cur[l];
        LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
        const dim3 grid((unsigned)mg_blocks(H.L[l + 1].cells), (unsigned)H.batch);
        if (l == 0) hipLaunchKernelGGL((mg_restrict_kernel<T, true>), grid, dim3(kBlock), 0, s, H.L[l], H.A[l], a, H.L[l + 1], H.B[l + 1]);
        else hipLaunchKernelGGL((mg_restrict_kernel<T, false>), grid, dim3(kBlock), 0, s, H.L[l], H.A[l], a, H.L[l + 1], H.B[l + 1]);
        PHIHIP_CHECK_HIP(hipGetLastError());
        ++launches;
    }
    // coarsest level
    {
        MgArgs<T> a = args();
        a.b = H.B[last];
        LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
        if (last == 0) {
            // a single level: all but the last sweep here, the last one is the MG_FINAL sweep below
            a.sweeps = 2 * ctx->mg_bottom - 1;
            hipLaunchKernelGGL((mg_coarsest_kernel<T, true>), dim3((unsigned)H.batch), dim3(kBlock), 0, s, H.L[0], H.A[0], a, H.Tm[0], H.X[0]);
        } else {
            a.sweeps = 2 * ctx->mg_bottom;
            hipLaunchKernelGGL((mg_coarsest_kernel<T, false>), dim3((unsigned)H.batch), dim3(kBlock), 0, s, H.L[last], H.A[last], a, H.X[last], H.Tm[last]);
        }
        PHIHIP_CHECK_HIP(hipGetLastError());
        ++launches;
    }
    if (last == 0) {
        MgArgs<T> a = args();
        a.b = H.B[0]; a.xin = H.Tm[0]; a.xout = H.X[0]; a.part = part_rz;
        PHIHIP_TRY((mg_smooth_launch<T, true>(ctx, H, 0, MG_FINAL, a, s, &launches)));
    }
    // up: prolongation (x 2) and add, post-smoothing
    for (int l = last - 1; l >= 0; --l) {
        {
            MgArgs<T> a = args();
            a.xout = cur[l];
            LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
            const dim3 grid((unsigned)mg_blocks(H.L[l].cells), (unsigned)H.batch);
            if (l == 0) hipLaunchKernelGGL((mg_prolong_kernel<T, true>), grid, dim3(kBlock), 0, s, H.L[l], H.A[l], a, H.L[l + 1], (const T*)H.X[l + 1]);
            else hipLaunchKernelGGL((mg_prolong_kernel<T, false>), grid, dim3(kBlock), 0, s, H.L[l], H.A[l], a, H.L[l + 1], (const T*)H.X[l + 1]);
            PHIHIP_CHECK_HIP(hipGetLastError());
            ++launches;
        }
        const T* in = cur[l];
        for (int k = 0; k < nu; ++k) {
            T* out = in == H.Tm[l] ? H.X[l] : H.Tm[l];
            MgArgs<T> a = args();
            a.b = H.B[l]; a.xin = in; a.xout = out;
            const bool fin = l == 0 && k == nu - 1;
            if (fin) a.part = part_rz;
            if (l == 0) PHIHIP_TRY((mg_smooth_launch<T, true>(ctx, H, l, fin ? MG_FINAL : MG_JACOBI, a, s, &launches)));
            else PHIHIP_TRY((mg_smooth_launch<T, false>(ctx, H, l, MG_JACOBI, a, s, &launches)));
            in = out;
        }
    }
    ctx->mg_last_launches = launches;
    return PHIHIP_OK;
}

template <typename T>
static int mg_apply_t(phihip_ctx* ctx, const GridView& v, const uint8_t* flags, int mask_batch, const void* r, void* z, hipStream_t s) {
    MgHierarchy<T> H;
    PHIHIP_TRY(ensure_buffer(ctx->ws_mg_part, (size_t)4 * v.batch * kMgBlocks * sizeof(double)));
    PHIHIP_TRY(mg_build<T>(ctx, v, flags, mask_batch, &H, s));
    H.B[0] = (T*)r;
    H.X[0] = (T*)z;
    MgArgs<T> first;
    memset(&first, 0, sizeof(first));
    first.prologue = PRO_NONE;
    return mg_vcycle<T>(ctx, H, first, (double*)ctx->ws_mg_part.ptr, s);
}

int run_multigrid_apply(phihip_ctx* ctx, const GridView& v, const uint8_t* flags, int mask_batch, const void* r, void* z, hipStream_t s) {
    if (v.op_custom || v.halo[0] || v.halo[1]) { set_error("multigrid: only the pressure operator of an undivided grid is covered"); return PHIHIP_ERR_UNSUPPORTED; }
    return with_dtype(v, [&](auto t) { return mg_apply_t<typename decltype(t)::type>(ctx, v, flags, mask_batch, r, z, s); });
}

template <typename T, int MODE>
static int mg_cg_launch(const MgLevel& L, int batch, int nblk, const MgCgArgs<T>& a, hipStream_t s) {
    hipLaunchKernelGGL((mg_cg_kernel<T, MODE>), dim3((unsigned)nblk, (unsigned)batch), dim3(kBlock), 0, s, L, a);
    PHIHIP_CHECK_HIP(hipGetLastError());
    return PHIHIP_OK;
}

// CG on A x = rhs preconditioned by one V-cycle per iteration; x holds x0 on entry. Same semantics as cg_t ('CG'): tolerances on the plain residual,
// max_iterations, refresh every `refresh_every`, tolerance mode polling the host-mapped flags, check_every = 0 = run max_iterations iterations.
template <typename T>
static int mg_cg_t(phihip_ctx* ctx, const GridView& v, const uint8_t* flags, int mask_batch, const T* rhs, T* x, const phihip_solve* solve,
                   phihip_solve_info* info, hipStream_t s) {
    const int batch = v.batch;
    const size_t vec_bytes = (size_t)batch * v.cells * sizeof(T);
    PHIHIP_TRY(ensure_buffer(ctx->ws_mg_r, vec_bytes));
    PHIHIP_TRY(ensure_buffer(ctx->ws_mg_d0, vec_bytes));
    PHIHIP_TRY(ensure_buffer(ctx->ws_mg_d1, vec_bytes));
    PHIHIP_TRY(ensure_buffer(ctx->ws_mg_z, vec_bytes));
    PHIHIP_TRY(ensure_buffer(ctx->ws_mg_part, (size_t)4 * batch * kMgBlocks * sizeof(double)));
    PHIHIP_TRY(ensure_buffer(ctx->ws_mg_state, (size_t)2 * batch * sizeof(CgState)));
    MgHierarchy<T> H;
    PHIHIP_TRY(mg_build<T>(ctx, v, flags, mask_batch, &H, s));
    unsigned int seq;
    PHIHIP_TRY(cg_host_prepare(ctx, batch, &seq));
    int checks = 0;
    T* r = (T*)ctx->ws_mg_r.ptr;
    T* z = (T*)ctx->ws_mg_z.ptr;
    T* d[2] = {(T*)ctx->ws_mg_d0.ptr, (T*)ctx->ws_mg_d1.ptr};
    H.B[0] = r;
    H.X[0] = z;
    const MgLevel& L = H.L[0];
    const int nblk = mg_blocks(L.cells);
    const size_t part_n = (size_t)batch * kMgBlocks;
    double* part_rr = (double*)ctx->ws_mg_part.ptr;
    double* part_yy = part_rr + part_n;
    double* part_rz = part_yy + part_n;
    double* part_dq = part_rz + part_n;
    CgState* st[2] = {(CgState*)ctx->ws_mg_state.ptr, (CgState*)ctx->ws_mg_state.ptr + batch};
    int cur = 0;
    const CgParams prm = cg_params(solve);
    MgCgArgs<T> base;
    memset(&base, 0, sizeof(base));
    base.flags = flags;
    base.prm = prm;
    base.nblk_in = nblk;
    {   // r0 = y - A x0 ; sum r^2, sum y^2
        MgCgArgs<T> a = base;
        a.a = x; a.b = rhs; a.o1 = r; a.part1 = part_rr; a.part2 = part_yy;
        a.prologue = PRO_NONE;
        LaunchScope ls(ctx, PHIHIP_K_CG_RESIDUAL, s);
        PHIHIP_TRY((mg_cg_launch<T, MGC_RESID>(L, batch, nblk, a, s)));
    }
    bool first = true;
    for (int k = 1; k <= solve->max_iterations; ++k) {
        T* d_old = d[(k - 1) & 1];
        T* d_new = d[k & 1];
        {   // z = M r ; sum r.z -- the cycle's first kernel judges the residual of the previous update
            MgArgs<T> f;
            memset(&f, 0, sizeof(f));
            f.prologue = first ? PRO_FIRST : PRO_BETA;
            f.st_in = st[cur]; f.st_out = st[cur ^ 1]; f.pin1 = part_rr; f.pin2 = part_yy; f.nblk_in = nblk; f.prm = prm;
            PHIHIP_TRY(mg_vcycle<T>(ctx, H, f, part_rz, s));
            cur ^= 1;
        }
        {   // d_new = z + beta d_old (the first one reads z in place of d_old with beta = 0)
            MgCgArgs<T> a = base;
            a.a = z; a.b = first ? z : d_old; a.o1 = d_new; a.part1 = part_dq;
            if (solve->check_every > 0) { a.host_flags = ctx->cg.host_flags_dev; a.seq = seq; }
            a.prologue = PRO_MG_BETA;
            a.st_in = st[cur]; a.st_out = st[cur ^ 1]; a.pin1 = part_rz;
            LaunchScope ls(ctx, PHIHIP_K_CG_MATVEC_DOT, s);
            PHIHIP_TRY((mg_cg_launch<T, MGC_MATVEC>(L, batch, nblk, a, s)));
            cur ^= 1;
            first = false;
        }
        if (solve->refresh_every > 0 && k % solve->refresh_every == 0) {
            {   // x += alpha d ; then the true residual r = y - A x (PhiML every refresh_every-th iteration)
                MgCgArgs<T> a = base;
                a.a = d_new; a.o1 = x;
                a.prologue = PRO_MG_ALPHA;
                a.st_in = st[cur]; a.st_out = st[cur ^ 1]; a.pin1 = part_dq;
                LaunchScope ls(ctx, PHIHIP_K_OTHER, s);
                PHIHIP_TRY((mg_cg_launch<T, MGC_AXPY>(L, batch, nblk, a, s)));
                cur ^= 1;
            }
            {
                MgCgArgs<T> a = base;
                a.a = x; a.b = rhs; a.o1 = r; a.part1 = part_rr;
                a.prologue = PRO_CONT;
                a.st_in = st[cur];
                LaunchScope ls(ctx, PHIHIP_K_CG_RESIDUAL, s);
                PHIHIP_TRY((mg_cg_launch<T, MGC_RESID>(L, batch, nblk, a, s)));
            }
        } else {
            MgCgArgs<T> a = base;
            a.a = d_new; a.o1 = x; a.o2 = r; a.part1 = part_rr;
            a.prologue = PRO_MG_ALPHA;
            a.st_in = st[cur]; a.st_out = st[cur ^ 1]; a.pin1 = part_dq;
            LaunchScope ls(ctx, PHIHIP_K_CG_UPDATE, s);
            PHIHIP_TRY((mg_cg_launch<T, MGC_UPDATE>(L, batch, nblk, a, s)));
            cur ^= 1;
        }
        bool stop = false;
        PHIHIP_TRY(cg_poll(ctx, solve, k, seq, batch, &checks, s, &stop));
        if (stop) break;
    }
    {
        LaunchScope ls(ctx, PHIHIP_K_CG_SCALAR, s);
        hipLaunchKernelGGL(mg_state_kernel, dim3(batch), dim3(kBlock), 0, s, (int)(first ? PRO_FIRST : PRO_BETA), (const CgState*)st[cur], st[cur ^ 1],
                           (const double*)part_rr, (const double*)part_yy, nblk, prm);
        cur ^= 1;
    }
    PHIHIP_CHECK_HIP(hipGetLastError());
    return cg_report(ctx, st[cur], batch, info, s);
}

int run_cg_multigrid(phihip_ctx* ctx, const GridView& v, const uint8_t* flags, int mask_batch, const void* rhs, void* x, const phihip_solve* solve,
                     phihip_solve_info* info, hipStream_t s) {
    if (v.op_custom || v.halo[0] || v.halo[1]) {
        set_error("the multigrid preconditioner covers the pressure solve only (not diffuse.implicit, shifted operators or slab-decomposed solves)");
        return PHIHIP_ERR_UNSUPPORTED;
    }
    return with_dtype(v, [&](auto t) {
        using T = typename decltype(t)::type;
        return mg_cg_t<T>(ctx, v, flags, mask_batch, (const T*)rhs, (T*)x, solve, info, s);
    });
}

}  // namespace phihip
