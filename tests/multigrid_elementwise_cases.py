"""
Element-wise parity of the multigrid V-cycle and of the preconditioned CG loop around it (csrc/multigrid.hpp) with the float64 restatement of the
documented recipe (tests/multigrid_ref.py), driven through the C ABI with a (ctx, mem) pair like tests/multigrid_cases.py. Used by
tests/test_multigrid_elementwise_emu.py (emulation) and tests/test_gpu_multigrid_elementwise.py (MI355X). Where tests/multigrid_cases.py asks what the
cycle ACHIEVES (convergence, iteration counts, symmetry), these checks compare every array it RETURNS.

Inputs: seeded white noise that is NON-ZERO on inactive cells (the z = r branch and the identity rows of the CG kernels see data); where no side is
open its active part is made mean-zero as multigrid_cases.Case.noise does. No element of a compared array is masked or skipped.

Bounds. fp64: 1e-12 of max |reference| for z and x (the fp64 parity bound of tests/adjoint_cases.py), 1e-10 relative for sum r^2 and sum y^2.
fp32: no constant -- the yardstick is the reference itself run in float32 on the same inputs. Kernel and float32 reference evaluate the same operator and differ
in summation order and contraction only, so the kernel's distance from the float64 reference may be at most 4 x the float32 reference's + 16 eps (the form of
parity_cases.truth_check, with 4 for 1.5: 60 coarsest sweeps and up to 7 levels accumulate order-dependent rounding). The fp32 sum r^2 is ONE number: its
rounding error has a sign and can cancel in either evaluation, so a ratio of two such errors is no yardstick. Its bound comes from the residual VECTOR of the
float32 reference instead: |delta sum r^2| / sum r^2 <= 2 |delta r|_2 / |r|_2 to first order, with |delta r|_2 / |r|_2 <= 4 e_r32 + 16 eps by the rule above.
Every check prints its figures (lines starting with "MGEW") before it asserts.
"""
import functools

import numpy as np

import multigrid_ref as R
from parity_cases import CLO, OPN, PER, C, O, make_case

DEFAULTS = (2, 4, 30, 0.8)       # phihip_set_multigrid: sweeps, coarsest_cells, coarsest_sweeps, omega
EPS32 = float(np.finfo(np.float32).eps)
FACTOR32 = 4.0
TOL64, TOL64_SUMS = 1e-12, 1e-10


def _sphere(centre, radius):
    return lambda shift: [O.SphereObstacle(tuple(float(c) + s for c, s in zip(centre, shift)), float(radius))]


def _frame(solid, fluid):
    """ a square frame of four boxes: solid (s0..s1)^2 around an enclosed fluid pocket (f0..f1)^2 (cell size 1: no cell centre lies on an edge) """
    (s0, s1), (f0, f1) = solid, fluid
    boxes = [((s0, s0), (f0, s1)), ((f1, s0), (s1, s1)), ((f0, s0), (f1, f0)), ((f0, f1), (f1, s1))]
    return lambda shift: [O.BoxObstacle(tuple(map(float, lo)), tuple(map(float, hi))) for lo, hi in boxes]


def _user_mask(res):
    """ inactive cells in the interior, behind the OPEN lower x side and in the corner of two OPEN sides: active neighbours see them through open faces """
    a = np.ones(res, np.uint8)
    a[20:26, 14:19] = 0
    a[0:3, 5:9] = 0
    a[47:50, 30:36] = 0
    a[30, 0:4] = 0
    return a


_BOX = ((CLO, CLO), (CLO, CLO))
_BOX_OPEN = ((CLO, OPN), (CLO, CLO))
_THIN_WALLS = {'closed': _BOX, 'open': ((OPN, CLO), (CLO, OPN)), 'periodic': ((PER, PER), (PER, PER))}

# name -> res, bc, box (upper corner; default: cell size 1), obstacles(shift), user (active mask), pocket (a cell inside the enclosed pocket)
CASES = {
    'A': dict(res=(64, 48), bc=_BOX, obstacles=_sphere((20, 24), 7)),                                                   # four coarse levels
    'B': dict(res=(50, 36), bc=((OPN, OPN), (CLO, OPN))),
    'C': dict(res=(33, 17), bc=((PER, PER), (CLO, CLO)), obstacles=_sphere((10, 8), 3)),                                  # odd axes
    'D': dict(res=(24, 20, 16), bc=((PER, PER), (CLO, OPN), (OPN, OPN)), obstacles=_sphere((12, 10, 8), 4)),             # mixed walls in 3-D
    'F': dict(res=(48, 48), bc=((PER, PER), (PER, PER))),                                                                # singular operator
    'aniso': dict(res=(40, 36), box=(10.0, 27.0), bc=((OPN, CLO), (PER, PER)), obstacles=_sphere((4.1, 12.2), 2.3)),      # unequal w[a] with flags
    'aniso_noflags': dict(res=(40, 36), box=(10.0, 27.0), bc=((OPN, CLO), (CLO, OPN))),                                   # ... without flags
    'aniso3d': dict(res=(12, 10, 9), box=(6.0, 15.0, 3.0), bc=((CLO, OPN), (PER, PER), (CLO, CLO)), obstacles=_sphere((3.2, 7.0, 1.4), 1.3)),
    'user_mask': dict(res=(50, 36), bc=((OPN, OPN), (CLO, OPN)), user=_user_mask),                                        # zero-ghost coupling
    'pocket2': dict(res=(32, 32), bc=_BOX, obstacles=_frame((8, 16), (10, 12)), pocket=(10, 11)),                         # the coarse cell must come out inactive
    'pocket4': dict(res=(32, 32), bc=_BOX, obstacles=_frame((6, 18), (8, 12)), pocket=(9, 10)),                           # larger aligned pocket
    'pocket3': dict(res=(32, 32), bc=_BOX_OPEN, obstacles=_frame((9, 16), (11, 14)), pocket=(12, 13)),                    # misaligned pocket
    'pocket1': dict(res=(32, 32), bc=_BOX_OPEN, obstacles=_frame((9, 14), (11, 12)), pocket=(11, 11)),                    # fine diagonal 0
    'global_2d': dict(res=(6, 3000), bc=((CLO, CLO), (OPN, CLO))),                                                        # coarsest level of 4500 cells
    'global_3d': dict(res=(6, 48, 64), bc=((CLO, OPN), (PER, PER), (CLO, CLO)), obstacles=_sphere((3, 20, 30), 2.2)),    # ... of 2304 cells
    # more than kMgBlocks * kBlock = 524 288 cells: mg_range chunks larger than a workgroup, xcd_order (GPU; the reference stays sparse)
    'large_3d': dict(res=(96, 80, 72), bc=((CLO, OPN), (CLO, CLO), (PER, PER)), obstacles=_sphere((40, 38, 30), 11)),
    'large_2d': dict(res=(724, 726), bc=((PER, PER), (CLO, CLO))),
}
for _res in ((5, 300), (6, 301), (3, 40)):                     # two levels with a long coarsest level; (3, 40): a single level, LDS branch
    for _w, _bc in _THIN_WALLS.items():
        CASES[f"thin_{_res[0]}x{_res[1]}_{_w}"] = dict(res=_res, bc=_bc)
THIN = [n for n in CASES if n.startswith('thin_')]
POCKETS = ['pocket2', 'pocket4', 'pocket3', 'pocket1']
SMALL = ['A', 'B', 'C', 'D', 'F', 'aniso', 'aniso_noflags', 'aniso3d', 'user_mask'] + POCKETS + THIN + ['global_2d', 'global_3d']
LARGE = ['large_3d', 'large_2d']

# (case, set_multigrid tuple): sweeps other than 2 + 2, a single level of 3072 cells (global-memory branch with FINE), two levels with bottom = 1,
# another omega and coarsest sweep count, 7 levels down to axes of 2 and 1 cells. The other grids with coarsest_cells = 1 add what grid A (closed walls)
# cannot reach: a PERIODIC axis coarsened to ONE cell, whose coupling with itself is folded into the diagonal. On F and C that coarsest cell sees a
# right-hand side of zero (singular operators, mean-zero input), so the fold only decides whether the cell is active; aniso has an OPEN side, and there the
# folded diagonal sets the coarsest level's Jacobi step. The row itself is the same with and without the fold, so 60 sweeps on one cell converge to the same
# value either way: bottom = 1 (two sweeps) is what shows the step.
PARAMETERS = [('A', (1, 4, 30, 0.8)), ('A', (3, 4, 30, 0.8)), ('A', (2, 64, 30, 0.8)), ('A', (2, 40, 1, 0.8)), ('A', (2, 4, 5, 0.6)), ('A', (2, 1, 30, 0.8)),
              ('F', (2, 1, 30, 0.8)), ('C', (2, 1, 30, 0.8)), ('aniso', (2, 1, 1, 0.8))]
TRAJECTORY_CASES = ['A', 'B', 'aniso', 'pocket3', 'D']
TRAJECTORIES = [(1, 50), (4, 50), (5, 2)]        # (K, refresh_every); the last takes the AXPY + true-residual branch twice
BATCH_CASES = {'A': [(0, 0), (5, -3), (-8, 6)], 'D': [(0, 0, 0), (3, -2, 1), (-4, 2, -2)]}       # obstacle shifts per batch entry
IMPULSE_CASES = ['C', 'user_mask'] + POCKETS


# ---- geometry and references (computed once per process, never modified) -------------------------------------------------------------------------------
class Geometry:
    def __init__(self, name, shift=None):
        spec = CASES[name]
        self.name, self.spec, self.shift = name, spec, shift
        self.res, self.bc = tuple(spec['res']), spec['bc']
        self.upper = tuple(float(v) for v in spec.get('box', self.res))
        self.dom = O.Domain(self.res, (0.0,) * len(self.res), self.upper, self.bc)
        self.hard = self.active = self.accessible = self.user = None
        if 'obstacles' in spec:
            obstacles = spec['obstacles'](shift or (0,) * len(self.res))
            self.active, self.hard, _ = O.obstacle_masks(obstacles, self.dom, np.float64)
            self.accessible = (self.active[0] > 0).astype(np.uint8)
        if 'user' in spec:
            self.user = spec['user'](self.res)
            self.active = self.user[None].astype(np.float64) * (self.active if self.active is not None else 1.0)
        self.singular = not self.dom.flexible()


@functools.lru_cache(maxsize=None)
def _geometry(name, shift):
    return Geometry(name, shift)


def geometry(name, shift=None):
    return _geometry(name, tuple(shift) if shift is not None and any(shift) else None)


@functools.lru_cache(maxsize=None)
def _reference(name, coarsest, dtype_name, shift):
    g = _geometry(name, shift)
    H = R.Hierarchy(g.dom, g.hard, g.active, coarsest, np.dtype(dtype_name))
    if dtype_name == 'float64':
        print(f"MGEW pin {name} shift {shift} coarsest {coarsest}: -P x vs O.masked_laplace {H.pin():.2e}, {H.nlevels} levels", flush=True)
    return H


def reference(name, coarsest=4, dtype_name='float64', shift=None):
    """ the hierarchy of one case; the float64 one is pinned to the oracle's operator when it is built """
    return _reference(name, int(coarsest), dtype_name, geometry(name, shift).shift)


def noise(g, seed, batch=1):
    """ standard-normal noise on EVERY cell; where no side is open, mean-zero over the active cells (float64) """
    b = np.random.default_rng(seed).standard_normal((batch,) + g.res)
    if g.singular:
        act = reference(g.name, shift=g.shift).active[None]
        mean = (b * act).sum(axis=tuple(range(1, b.ndim)), keepdims=True) / act.sum()
        b = np.where(act, b - mean, b)
    return b


class System:
    """ one geometry on the 'device': grid struct and flag bytes (from phihip_build_cellflags, accessible and / or the user's active mask) """

    def __init__(self, ctx, mem, g, dtype, batch=1):
        self.g, self.dtype, self.batch = g, np.dtype(dtype), batch
        _, self.grid = make_case(g.res, g.bc, dtype, batch, upper=g.upper)
        self.dflags = None
        if g.accessible is not None or g.user is not None:
            self.dflags = build_flags(ctx, mem, g, [g])

    def flags_ptr(self, mem):
        return mem.ptr(self.dflags) if self.dflags is not None else 0


def build_flags(ctx, mem, g, geometries):
    """ flag bytes [len(geometries)][res] (one entry: [res]) of geometries that share g's grid """
    n = len(geometries)
    lead = (n,) if n > 1 else ()
    stack = lambda arrays: np.ascontiguousarray(np.stack(arrays).reshape(lead + g.res))
    dacc = mem.to_dev(stack([q.accessible for q in geometries])) if g.accessible is not None else None
    dusr = mem.to_dev(stack([q.user for q in geometries])) if g.user is not None else None
    dflags = mem.empty(lead + g.res, np.uint8)
    grid = C.make_grid(len(g.res), C.PHIHIP_F64, n, g.res, (0.0,) * len(g.res), g.upper, g.bc)
    ctx.build_cellflags(grid, mem.ptr(dacc) if dacc is not None else 0, mem.ptr(dusr) if dusr is not None else 0, n, mem.ptr(dflags))
    mem.sync()
    return dflags


def apply_M(ctx, mem, grid, flags, mask_batch, r):
    dr, dz = mem.to_dev(r), mem.empty(r.shape, r.dtype)
    ctx.precondition_apply(grid, flags, mask_batch, mem.ptr(dr), mem.ptr(dz))
    mem.sync()
    return mem.to_host(dz)


class tuned:
    """ with tuned(ctx, params): the V-cycle's parameters for the block, the defaults again afterwards (contexts are shared on the GPU) """

    def __init__(self, ctx, params):
        self.ctx, self.params = ctx, params

    def __enter__(self):
        if self.params is not None:
            self.ctx.set_multigrid(*self.params)

    def __exit__(self, *exc):
        if self.params is not None:
            self.ctx.set_multigrid(*DEFAULTS)
        return False


def _dist(a, ref):
    """ max |a - ref| / max |ref|, every element """
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-300)


def compare(tag, got, ref64, ref32_fn, dtype):
    """ fp64: got within 1e-12 of max |ref64|. fp32: got no further from ref64 than 4 x the float32 reference + 16 eps. Returns the printed figures """
    assert np.isfinite(got).all(), f"{tag}: non-finite values"
    e = _dist(got, ref64)
    if np.dtype(dtype) == np.float64:
        print(f"MGEW {tag} float64 e_kernel {e:.2e} (bound {TOL64:.0e})", flush=True)
        assert e <= TOL64, f"{tag}: {e:.2e} of max|reference| from the float64 reference"
        return e, None
    e32 = _dist(ref32_fn(), ref64)
    print(f"MGEW {tag} float32 e_kernel {e:.2e} e_ref32 {e32:.2e} ratio {e / max(e32, 1e-300):.2f} (bound {FACTOR32:g} x e_ref32 + 16 eps = {FACTOR32 * e32 + 16 * EPS32:.2e})",
          flush=True)
    assert e <= FACTOR32 * e32 + 16 * EPS32, f"{tag}: kernel {e:.2e} vs float32 reference {e32:.2e} from the float64 reference"
    return e, e32


# ---- (a) one cycle on white noise ------------------------------------------------------------------------------------------------------------------------
def check_cycle(ctx, mem, name, dtype, params=None, seed=31):
    sweeps, coarsest, bottom, omega = params or DEFAULTS
    g = geometry(name)
    H = reference(name, coarsest)
    sys_ = System(ctx, mem, g, dtype)
    r = noise(g, seed).astype(dtype)
    with tuned(ctx, params):
        z = apply_M(ctx, mem, sys_.grid, sys_.flags_ptr(mem), 1, r)
        levels = ctx.query_multigrid()["levels"]
    r64 = r.astype(np.float64)
    z64 = H.apply(r64, sweeps, bottom, omega)
    tag = f"cycle {name}{'' if params is None else ' ' + str(tuple(params))}"
    out = compare(tag, z, z64, lambda: reference(name, coarsest, 'float32').apply(r, sweeps, bottom, omega), dtype)
    assert levels == H.nlevels, f"{tag}: the library built {levels} levels, the reference {H.nlevels}"
    return out


def check_cycle_random(ctx, mem, res, bc, upper, sphere, seed, dtype=np.float64):
    """ tests/fuzz_parity.py: check_cycle on a grid, walls, cell sizes and solid sphere (centre, radius in physical units, or None) of the caller's """
    name = f"random_{seed}"
    CASES[name] = dict(res=tuple(res), bc=tuple(bc), box=tuple(upper), **({'obstacles': _sphere(*sphere)} if sphere else {}))
    return check_cycle(ctx, mem, name, dtype, seed=seed)


# ---- (b) columns of M ------------------------------------------------------------------------------------------------------------------------------------------
def impulse_cells(g, H, limit=12):
    """ a corner, the middle of every wall (each kind of wall of the case), the last cell of every axis (odd axes: the child without a sibling), a cell
    touching an inactive one, a cell inside the pocket, an inactive cell """
    res, act = g.res, H.active
    cells = [tuple(0 for _ in res), tuple(n - 1 for n in res)]
    for a in range(len(res)):
        for side in (0, 1):
            c = [n // 2 for n in res]
            c[a] = 0 if side == 0 else res[a] - 1
            cells.append(tuple(c))
    inactive = np.argwhere(~act)
    if len(inactive):
        cells.append(tuple(int(v) for v in inactive[len(inactive) // 2]))
        touching = act.copy()
        near = np.zeros_like(act)
        for a in range(len(res)):
            for step in (1, -1):
                sh = np.roll(~act, step, axis=a)
                idx = [slice(None)] * len(res)
                idx[a] = 0 if step == 1 else -1
                sh[tuple(idx)] = False
                near |= sh
        touching &= near
        found = np.argwhere(touching)
        if len(found):
            cells += [tuple(int(v) for v in found[0]), tuple(int(v) for v in found[-1])]
    if 'pocket' in g.spec:
        cells.append(tuple(g.spec['pocket']))
    unique = []
    for c in cells:
        if c not in unique:
            unique.append(c)
    return unique[:limit]


def check_impulses(ctx, mem, name):
    """ fp64: M e_j for unit impulses on the hierarchy's edges, each compared with the reference's column """
    g = geometry(name)
    H = reference(name)
    sys_ = System(ctx, mem, g, np.float64, batch=1)
    cells = impulse_cells(g, H)
    assert 0 < len(cells) <= 12
    worst = 0.0
    for cell in cells:
        e = np.zeros((1,) + g.res)
        e[(0,) + cell] = 1.0
        z = apply_M(ctx, mem, sys_.grid, sys_.flags_ptr(mem), 1, e)
        err, _ = compare(f"impulse {name} {cell} ({'active' if H.active[cell] else 'inactive'})", z, H.apply(e), None, np.float64)
        worst = max(worst, err)
    return worst


# ---- (c) batches and geometry batches ----------------------------------------------------------------------------------------------------------------------
def check_batch(ctx, mem, name, dtype, seed=41):
    shifts = BATCH_CASES[name]
    gs = [geometry(name, tuple(s)) for s in shifts]
    g = gs[0]
    grid3 = make_case(g.res, g.bc, dtype, 3, upper=g.upper)[1]
    grid1 = make_case(g.res, g.bc, dtype, 1, upper=g.upper)[1]
    r = noise(g, seed, 3).astype(dtype)          # (case A: singular -- mean-zero over entry 0's active cells; M is linear, any r serves)
    flags3 = build_flags(ctx, mem, g, gs)
    z3 = apply_M(ctx, mem, grid3, mem.ptr(flags3), 3, r)
    for b, q in enumerate(gs):
        H = reference(name, 4, 'float64', tuple(shifts[b]))
        z64 = H.apply(r[b:b + 1].astype(np.float64))
        compare(f"batch {name} entry {b} shift {shifts[b]}", z3[b:b + 1], z64,
                lambda b=b: reference(name, 4, 'float32', tuple(shifts[b])).apply(r[b:b + 1]), dtype)
        flags1 = build_flags(ctx, mem, q, [q])
        z1 = apply_M(ctx, mem, grid1, mem.ptr(flags1), 1, np.ascontiguousarray(r[b:b + 1]))
        assert np.array_equal(z1, z3[b:b + 1]), f"batch {name}: entry {b} of the batch-3 call differs from the batch-1 call on its geometry"
    shared = build_flags(ctx, mem, g, [g])
    replicated = build_flags(ctx, mem, g, [g, g, g])
    za = apply_M(ctx, mem, grid3, mem.ptr(shared), 1, r)
    zb = apply_M(ctx, mem, grid3, mem.ptr(replicated), 3, r)
    assert np.array_equal(za, zb), f"batch {name}: shared flags (mask_batch 1) and the same flags three times (mask_batch 3) give different bits"


# ---- (d) the first iterations of the preconditioned CG ---------------------------------------------------------------------------------------------------
def check_pcg_trajectory(ctx, mem, name, dtype, K, refresh_every, seed=51):
    g = geometry(name)
    H = reference(name)
    sys_ = System(ctx, mem, g, dtype)
    y = noise(g, seed).astype(dtype)
    x0 = np.random.default_rng(seed + 1).standard_normal((1,) + g.res).astype(dtype)      # non-zero on inactive cells
    solve = C.Solve(1e-30, 0.0, K, refresh_every, 0, 2)
    drhs, dx = mem.to_dev(y), mem.to_dev(x0)
    info = ctx.cg_solve(sys_.grid, sys_.flags_ptr(mem), 1, mem.ptr(drhs), mem.ptr(dx), solve)
    mem.sync()
    x = mem.to_host(dx)
    ref = R.pcg(H, y.astype(np.float64), x0.astype(np.float64), K, refresh_every)
    tag = f"pcg {name} K {K} refresh {refresh_every}"
    ref32 = R.pcg(reference(name, 4, 'float32'), y, x0, K, refresh_every) if np.dtype(dtype) == np.float32 else None
    # (no constant is removed from x: the reference's own distance shows none is needed for K <= 5, on the singular operator too)
    compare(tag + " x", x, ref.x, lambda: ref32.x, dtype)
    rs, ys = float(info[0].residual_sq), float(info[0].rhs_sq)
    e_rs, e_ys = abs(rs - ref.residual_sq) / ref.residual_sq, abs(ys - ref.rhs_sq) / ref.rhs_sq
    if np.dtype(dtype) == np.float64:
        bound_rs = TOL64_SUMS
    else:
        e_r32 = float(np.linalg.norm((ref32.r.astype(np.float64) - ref.r).ravel()) / np.linalg.norm(ref.r.ravel()))
        bound_rs = 2 * (FACTOR32 * e_r32 + 16 * EPS32)
    print(f"MGEW {tag} {np.dtype(dtype).name} sums: residual_sq {rs:.15e} reference {ref.residual_sq:.15e} rel {e_rs:.2e} (bound {bound_rs:.2e}); "
          f"rhs_sq {ys:.15e} reference {ref.rhs_sq:.15e} rel {e_ys:.2e} (bound {TOL64_SUMS:.0e}); iterations {info[0].iterations}", flush=True)
    assert info[0].iterations == K, (info[0].iterations, K)
    assert e_ys <= TOL64_SUMS, f"{tag}: rhs_sq {ys} vs {ref.rhs_sq}"
    assert e_rs <= bound_rs, f"{tag}: residual_sq {rs} vs {ref.residual_sq} ({e_rs:.2e} > {bound_rs:.2e})"
