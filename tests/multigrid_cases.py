"""
Shared cases of the multigrid-preconditioned CG (Solve(preconditioner='multigrid'), phihip_method 2), driven through the C ABI like
tests/parity_cases.py. Used by tests/test_multigrid_emu.py (emulation) and tests/test_gpu_multigrid.py (MI355X).
Yardsticks: the oracle's operator (masked_laplace, obstacle_masks) in float64 and the PLAIN CG path of the library, never the multigrid path itself.
"""
import numpy as np

from parity_cases import CLO, OPN, PER, TOL32, TOL64, C, O, make_case, rel_l2

METHOD_CG, METHOD_MG = 0, 2

# name -> (res, bc, obstacle (centre in cells, radius in cells) or None); cell size 1
CASES = {
    'A': ((64, 48), ((CLO, CLO), (CLO, CLO)), ((20, 24), 7)),
    'B': ((50, 36), ((OPN, OPN), (CLO, OPN)), None),
    'C': ((33, 17), ((PER, PER), (CLO, CLO)), ((10, 8), 3)),
    'D': ((24, 20, 16), ((PER, PER), (CLO, OPN), (OPN, OPN)), ((12, 10, 8), 4)),
    'E': ((32, 32, 32), ((CLO, CLO),) * 3, ((10, 16, 16), 5)),
    'F': ((48, 48), ((PER, PER), (PER, PER)), None),
}
# iterations(multigrid) <= iterations(plain) / RATIO
RATIO = {'A': 4, 'B': 4, 'C': 3, 'D': 3, 'E': 4, 'F': 4}


class Case:
    """ one system: domain, grid struct, oracle masks, flag bytes on the 'device' """

    def __init__(self, ctx, mem, name, dtype, batch=1, res=None, obstacle='default'):
        shape, bc, ob = CASES[name]
        if res is not None:
            shape = res
        if obstacle != 'default':
            ob = obstacle
        self.name, self.dtype, self.batch = name, np.dtype(dtype), batch
        self.dom, self.grid = make_case(tuple(shape), bc, dtype, batch)
        self.obstacles = [O.SphereObstacle(tuple(float(c) for c in ob[0]), float(ob[1]))] if ob else []
        self.hard = self.active = None
        self.dflags = None
        if self.obstacles:
            self.active, self.hard, _ = O.obstacle_masks(self.obstacles, self.dom, np.float64)
            dacc = mem.to_dev((self.active[0] > 0).astype(np.uint8))
            self.dflags = mem.empty(self.dom.res, np.uint8)
            g1 = C.make_grid(self.dom.rank, self.grid.dtype, 1, self.dom.res, self.dom.lower, self.dom.upper, self.dom.bc, self.dom.bc_val)
            ctx.build_cellflags(g1, mem.ptr(dacc), 0, 1, mem.ptr(self.dflags))
            self._keep = dacc
        self.singular = not self.dom.flexible()
        self.mask = np.ones((1,) + tuple(self.dom.res)) if self.active is None else (self.active > 0).astype(np.float64)

    def flags_ptr(self, mem):
        return mem.ptr(self.dflags) if self.dflags is not None else 0

    def noise(self, seed):
        """ seeded standard-normal noise on the active cells, zero elsewhere, mean-zero over the active cells where no side is open (float64) """
        rng = np.random.default_rng(seed)
        b = rng.standard_normal((self.batch,) + tuple(self.dom.res)) * self.mask
        if self.singular:
            ax = tuple(range(1, b.ndim))
            b = (b - b.sum(axis=ax, keepdims=True) / self.mask.sum() * self.mask) * self.mask
        return b

    def A64(self, x):
        return O.masked_laplace(np.asarray(x, np.float64), self.dom, self.hard, self.active)

    def true_rel_residual(self, x, rhs):
        r = np.asarray(rhs, np.float64) - self.A64(x)
        ax = tuple(range(1, r.ndim))
        return np.sqrt((r ** 2).sum(axis=ax) / (np.asarray(rhs, np.float64) ** 2).sum(axis=ax))


def solve(ctx, mem, case, rhs, method, rel_tol=1e-5, max_iter=5000, x0=None, check=10, refresh=50):
    """ phihip_cg_solve on the case; returns (x, infos) """
    s = C.Solve(rel_tol, 0.0, max_iter, refresh, check, method)
    drhs = mem.to_dev(np.asarray(rhs, case.dtype))
    dx = mem.to_dev(np.zeros(rhs.shape, case.dtype) if x0 is None else np.asarray(x0, case.dtype))
    info = ctx.cg_solve(case.grid, case.flags_ptr(mem), 1, mem.ptr(drhs), mem.ptr(dx), s)
    mem.sync()
    return mem.to_host(dx), info


def plain_iterations(ctx, mem, case, rhs, rel_tol=1e-5):
    """ the plain CG's count; should its fp32 solve stagnate (parity_cases.py records one closed box with a disc), the float64 count """
    _, info = solve(ctx, mem, case, rhs, METHOD_CG, rel_tol)
    if all(i.converged for i in info) or case.dtype == np.float64:
        return [i.iterations for i in info], info
    c64 = Case(ctx, mem, case.name, np.float64, case.batch, res=case.dom.res)
    _, info64 = solve(ctx, mem, c64, rhs, METHOD_CG, rel_tol)
    return [i.iterations for i in info64], info64


def check_converged_and_fewer(ctx, mem, name, dtype, rel_tol=1e-5, compare=True, seed=0):
    """ tests 1 and 2 of the issue: converged means converged (true residual in float64 by the oracle's operator <= 4 rel_tol), and
    iterations(multigrid) <= iterations(plain) / RATIO on the same inputs """
    case = Case(ctx, mem, name, dtype)
    rhs = case.noise(seed).astype(dtype)
    x, info = solve(ctx, mem, case, rhs, METHOD_MG, rel_tol)
    res = case.true_rel_residual(x, rhs)
    its = [i.iterations for i in info]
    print(f"case {name} {np.dtype(dtype).name} rel_tol {rel_tol:g}: multigrid CG {its} iterations, true relative residual {res}", flush=True)
    assert all(i.converged and not i.diverged for i in info), [(i.iterations, i.residual_sq, i.rhs_sq) for i in info]
    assert float(res.max()) <= 4 * rel_tol, (res, rel_tol)
    if compare:
        plain, _ = plain_iterations(ctx, mem, case, rhs, rel_tol)
        print(f"case {name} {np.dtype(dtype).name}: plain CG {plain} iterations (bound: / {RATIO[name]})", flush=True)
        assert all(k <= kp / RATIO[name] for k, kp in zip(its, plain)), (its, plain)
    return its


def check_symmetric_operator(ctx, mem, name):
    """ test 3: <u, M v> = <v, M u> to 1e-10 relative and <u, M u> non-zero with the sign of <u, A u> (fp64, through phihip_precondition_apply) """
    case = Case(ctx, mem, name, np.float64)
    u, v = case.noise(11)[0:1], case.noise(12)[0:1]

    def M(r):
        dr, dz = mem.to_dev(r), mem.empty(r.shape, np.float64)
        ctx.precondition_apply(case.grid, case.flags_ptr(mem), 1, mem.ptr(dr), mem.ptr(dz))
        mem.sync()
        return mem.to_host(dz)

    Mu, Mv = M(u), M(v)
    uMv, vMu, uMu, uAu = float((u * Mv).sum()), float((v * Mu).sum()), float((u * Mu).sum()), float((u * case.A64(u)).sum())
    print(f"case {name}: <u,Mv> {uMv:.15e} <v,Mu> {vMu:.15e} asymmetry {abs(uMv - vMu) / abs(uMv):.2e}; <u,Mu> {uMu:.6e}, <u,Au> {uAu:.6e}", flush=True)
    assert np.isfinite(Mu).all() and np.isfinite(Mv).all()
    assert abs(uMv - vMu) <= 1e-10 * abs(uMv)
    assert uMu != 0 and np.sign(uMu) == np.sign(uAu)
    assert np.array_equal(Mu, M(u))      # a fixed operator: the same bits on a second application


# ---- through the Python layer (fluid.make_incompressible, jit_compile) ----------------------------------------------------------------------------------
def _ext(bc):
    names = 'xyz'
    from phiflow_amd.flow import BOUNDARY, PERIODIC, ZERO, combine_sides
    one = lambda c: PERIODIC if c == PER else (ZERO if c == CLO else BOUNDARY)
    return combine_sides(**{names[d]: (one(lo), one(hi)) if lo != hi else one(lo) for d, (lo, hi) in enumerate(bc)})


def check_projection(backend, name, dtype, batched_geometry=False, user_active=False, seed=7):
    """ test 4 of the issue: (a) max |div| <= 5e-5 or <= 1.25 x the plain-CG result's; (b) against the oracle's float64 CG to 1e-12 on the same right-hand
    side, velocity and mean-removed pressure are no further than 1.5 x the plain-CG result's distance + cg_rel_l2 (tests/parity_cases.py) """
    from phiflow_amd.flow import Box, CenteredGrid, Obstacle, Solve, Sphere, StaggeredGrid, fluid
    res, bc, ob = CASES[name]
    D = len(res)
    dims = 'xyz'[:D]
    kw = dict(zip(dims, res))
    bounds = Box(**{d: float(n) for d, n in zip(dims, res)})
    ext = _ext(bc)
    dom = O.Domain(res, (0.0,) * D, tuple(float(r) for r in res), bc)
    rng = np.random.default_rng(seed)
    B = 2 if batched_geometry else 1
    centres = [[float(c) for c in ob[0]] for _ in range(B)]
    if batched_geometry:
        centres[1][0] -= 2.0
    sphere = Sphere(radius=float(ob[1]), **{d: ([c[k] for c in centres] if batched_geometry else centres[0][k]) for k, d in enumerate(dims)})
    obstacles = [Obstacle(sphere)]
    shapes = StaggeredGrid(0, ext, bounds, backend=backend, **kw).component_shapes
    vals = [(0.1 * rng.standard_normal((B,) + tuple(s))).astype(dtype) for s in shapes]
    v = StaggeredGrid(vals if B > 1 else [a[0] for a in vals], ext, bounds, backend=backend, **kw)
    act_np = None
    active = None
    if user_active:
        act_np = np.ones(res)
        act_np[tuple(slice(n // 2, n // 2 + 3) for n in res)] = 0
        active = CenteredGrid(act_np, 0, bounds, backend=backend, **kw)
    tol = 1e-5 if np.dtype(dtype) == np.float32 else 1e-10
    out = {}
    for key, solve in (('mg', Solve('CG', tol, 0, preconditioner='multigrid')), ('cg', Solve('CG', tol, 0, max_iterations=5000))):
        vo, po = fluid.make_incompressible(v, obstacles, solve, active=active)
        assert all(po.solve_info.converged), (key, po.solve_info)
        vn = vo.numpy()
        out[key] = ([np.asarray(a, np.float64).reshape((B,) + a.shape[-D:]) for a in vn], np.asarray(po.numpy(), np.float64).reshape((B,) + tuple(res)),
                    po.solve_info.iterations)
    print(f"projection {name} {np.dtype(dtype).name}: iterations multigrid {out['mg'][2]}, plain {out['cg'][2]}", flush=True)
    bound = (TOL32 if np.dtype(dtype) == np.float32 else TOL64)['cg_rel_l2']
    for b in range(B):
        obs_o = [O.SphereObstacle(tuple(centres[b]), float(ob[1]))]
        v64 = [a[b:b + 1].astype(np.float64) for a in vals]
        vt, pt, it, _ = O.make_incompressible(v64, dom, obs_o, rtol=1e-12, atol=0.0, max_iter=20000, active_user=act_np)
        active_o, _, _ = O.obstacle_masks(obs_o, dom, np.float64)
        if act_np is not None:
            active_o = active_o * act_np
        div = {k: np.abs(O.divergence([a[b:b + 1] for a in out[k][0]], dom) * active_o).max() for k in out}
        cat = lambda vs: np.concatenate([a.ravel() for a in vs])
        dv = {k: rel_l2(cat([a[b:b + 1] for a in out[k][0]]), cat(vt)) for k in out}
        dm = lambda p: (p - (p * active_o).sum() / active_o.sum()) * active_o
        dp = {k: rel_l2(dm(out[k][1][b:b + 1]), dm(pt)) for k in out}
        print(f"  entry {b}: max|div| {div}, velocity distance from the float64 truth {dv}, pressure distance {dp}", flush=True)
        assert div['mg'] <= 5e-5 or div['mg'] <= 1.25 * div['cg'], div
        assert dv['mg'] <= 1.5 * dv['cg'] + bound, dv
        assert dp['mg'] <= 1.5 * dp['cg'] + bound, dp
    assert all(k <= kp / RATIO[name] for k, kp in zip(out['mg'][2], out['cg'][2])), (out['mg'][2], out['cg'][2])


def jit_step_matches_eager(backend, n, dims, replays=5):
    """ advect.semi_lagrangian + make_incompressible(Solve('CG', 1e-5, x0=p, max_iterations=6, preconditioner='multigrid')): the jit_compile'd step replayed
    equals the eager steps bit for bit (the form of test_heat_flow_direct_solve_and_jit_replay) """
    import torch
    from phiflow_amd.flow import Box, NotConverged, Obstacle, Solve, Sphere, StaggeredGrid, advect, fluid, jit_compile
    kw = {d: n for d in dims}
    bounds = Box(**{d: 1.0 for d in dims})
    rng = np.random.default_rng(9)
    shapes = StaggeredGrid(0, 0, bounds, backend=backend, **kw).component_shapes
    v0 = StaggeredGrid([(0.05 * rng.standard_normal(s)).astype(np.float32) for s in shapes], 0, bounds, backend=backend, **kw)
    ball = Obstacle(Sphere(radius=0.15, **{d: 0.4 for d in dims}))

    def step(v, p, dt):
        v = advect.semi_lagrangian(v, v, dt)
        return fluid.make_incompressible(v, [ball], Solve('CG', 1e-5, x0=p, max_iterations=6, preconditioner='multigrid', suppress=[NotConverged]))
    jstep = jit_compile(step)
    eager, traced = (v0, None), (v0, None)
    for _ in range(replays):
        eager = step(*eager, 0.1)
        traced = jstep(*traced, 0.1)
        for fe, ft in zip(eager, traced):
            for a, b in zip(fe.values if fe.is_staggered else [fe.values], ft.values if ft.is_staggered else [ft.values]):
                assert torch.equal(a, b)
    assert float(eager[1].values.abs().max()) > 0


# ---- large grids (GPU) -------------------------------------------------------------------------------------------------------------------------------------
def closed_box_with_ball(ctx, mem, n, rank, dtype):
    """ closed box of n cells per axis with a solid disc / sphere of radius 0.1 n at (0.3, 0.5[, 0.5]) n """
    name = 'E' if rank == 3 else 'A'
    centre = (0.3 * n,) + (0.5 * n,) * (rank - 1)
    return Case(ctx, mem, name, dtype, 1, res=(n,) * rank, obstacle=(centre, 0.1 * n))


def check_size_independence(ctx, mem, sizes, rank, dtype, rel_tol=1e-5, plain_ratio=None):
    """ test 10: iterations(largest) <= 1.5 x iterations(smallest) + 2; with `plain_ratio`: at the largest size also iterations <= iterations(plain) / ratio,
    plain CG given max_iterations = 5000 """
    its = []
    for n in sizes:
        case = closed_box_with_ball(ctx, mem, n, rank, dtype)
        rhs = case.noise(n).astype(dtype)
        _, info = solve(ctx, mem, case, rhs, METHOD_MG, rel_tol)
        print(f"closed box {n}^{rank} {np.dtype(dtype).name}: multigrid CG {info[0].iterations} iterations, converged {info[0].converged}, V-cycle {ctx.query_multigrid()}", flush=True)
        assert info[0].converged and not info[0].diverged, (n, info[0].iterations, info[0].residual_sq, info[0].rhs_sq)
        its.append(info[0].iterations)
        if plain_ratio and n == sizes[-1]:
            _, pinfo = solve(ctx, mem, case, rhs, METHOD_CG, rel_tol, max_iter=5000)
            print(f"closed box {n}^{rank}: plain CG {pinfo[0].iterations} iterations, converged {pinfo[0].converged}", flush=True)
            assert info[0].iterations <= pinfo[0].iterations / plain_ratio, (info[0].iterations, pinfo[0].iterations)
    assert its[-1] <= 1.5 * its[0] + 2, its
    return its
