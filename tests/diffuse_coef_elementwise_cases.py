"""
Element-wise parity of diffusion with a varying / per-axis diffusivity (phiflow_amd/csrc/diffuse_coef.hpp: coef_kernel's seven modes, the two-launch CG driver
coef_cg_t and the affine-wall shift) with the float64 restatement of tests/diffuse_coef_ref.py, driven through the C ABI with a (ctx, mem) pair like
tests/multigrid_elementwise_cases.py. Used by tests/test_diffuse_coef_elementwise_emu.py (emulation) and tests/test_gpu_diffuse_coef_elementwise.py (MI355X).
Where the older diffuse-coef tests ask what the solver ACHIEVES (converged, true residual), these compare every array and every sum it RETURNS:
  (a) check_explicit        one explicit step (CM_APPLY), coefficient shared / per entry / absent, kdt > 0 and kdt < 0 (sharpen's `max` branch)
  (b) check_cg_trajectory   x, sum r^2 and sum y^2 after K iterations of 'CG' / 'CG-adaptive' with refresh steps inside (CM_RHS, CM_RESID, CM_MATVEC, CM_UPDATE,
                            CM_AXPY, CM_DOTQ and every prologue)
  (c) check_batch_freeze    batch entries that stop at different iterations, one of them with r0 == 0 exactly
  (d) check_python_walls    diffuse.explicit / diffuse.implicit on CenteredGrids with the reference's codes and constants written out as literals

Inputs: u is white noise, the coefficient 0.25 + U(0, 1); every CLOSED side of u carries a non-zero constant (CM_RHS runs); the cells are (1, 1.25, 0.8)
wide and kdt_d / dx_d^2 = 0.3 / 0.45 / 0.6 (2-D: 0.35 / 0.55), so a mixed-up axis shows. fp32: the inputs are rounded to fp32 first and the float64 reference
evaluates those numbers. No element is masked, no constant removed.

Bounds (the project's own). (a): TOL64['stencil'] / TOL32['stencil'] of max |reference|; the float32 reference's error is printed next to the kernel's.
(b), fp64: 1e-12 of max |reference| for x, 1e-10 relative for the two sums. (b), fp32, x: kernel and float32 reference evaluate the same recurrence and differ in
summation order and contraction only, so the kernel's distance from the float64 reference may be at most 4 x the float32 reference's + 16 eps. (b), fp32, sums:
one number's rounding error has a sign and can cancel, so the yardstick is the VECTOR of the float32 reference: |delta sum r^2| / sum r^2 <= 2 |delta r|_2 / |r|_2
to first order, with |delta r|_2 / |r|_2 <= 4 e_r32 + 16 eps; the same for sum y^2 with the right-hand-side vector (the kernel accumulates y^2 in the element
type). Every check prints its figures (lines starting with "DCEW") before it asserts.

Each case asserts the launch plan it is there for (`plan` restates plan_columns of csrc/column_march.hpp as coef_plan calls it; PLANS holds the expected figures as literals): a later change to the plan makes the
case complain, not silently stop covering.
"""
import functools

import numpy as np

import diffuse_coef_ref as R
from parity_cases import CLO, OPN, PER, TOL32, TOL64, C, O

assert (PER, CLO, OPN) == (R.PERIODIC, R.CLOSED, R.OPEN)

EPS32 = float(np.finfo(np.float32).eps)
FACTOR32 = 4.0
TOL64_X, TOL64_SUMS = 1e-12, 1e-10
METHOD_CODE = {'CG': 0, 'CG-adaptive': 1}          # phihip.h PHIHIP_METHOD_*
TARGET_CG, TARGET_EXPLICIT = 1024, 4096              # coef_cg_t / run_diffuse_coef_explicit: workgroups per batch entry that coef_plan aims at
TRAJECTORIES = [(1, 50, 'CG'), (4, 50, 'CG'), (5, 2, 'CG'), (4, 4, 'CG-adaptive'), (5, 2, 'CG-adaptive')]      # (K, refresh_every, method)
FORMS = ('shared', 'per_entry', 'absent')            # the coefficient: one array for every batch entry, one per entry, none (per-axis factors only)

DX = (1.0, 1.25, 0.8)
WEIGHTS = {2: (0.35, 0.55), 3: (0.3, 0.45, 0.6)}     # kdt_d / dx_d^2

U_KINDS = [(PER, PER), (CLO, CLO), (OPN, OPN), (CLO, OPN), (OPN, CLO)]
C_KINDS = {'P': (PER, 0.0), 'Z': (OPN, 0.0), 'K': (CLO, 0.75), '0': (CLO, 0.0)}      # one side of the coefficient's extrapolation: (code, constant)
PAIRS = [(p % 5, 'PZK0'[p % 4]) for p in range(20)]                                   # every (u kind, coefficient kind) once


def plan(res, target):
    """ plan_columns (csrc/column_march.hpp) as coef_plan calls it: (4 x 64)-cell tiles in the plane, a0 split into chunks so that a batch entry has about `target` workgroups.
    Returns (tiles1, tiles2, chunk, chunks, planes in the last chunk) """
    n = (1,) * (3 - len(res)) + tuple(res)
    tiles1, tiles2 = (n[1] + 3) // 4, (n[2] + 63) // 64
    tiles = tiles1 * tiles2
    chunks = min(max(-(-target // tiles), 1), n[0])
    chunk = -(-n[0] // chunks)
    chunks = -(-n[0] // chunk)
    return tiles1, tiles2, chunk, chunks, n[0] - (chunks - 1) * chunk


# (res, target) -> (tiles1, tiles2, chunk, chunks, planes in the last chunk): what each shape is in the table FOR, as literals
PLANS = {
    # in-plane edges: one below, at and one above the 4 x 64 tile on both axes; several tiles with a ragged last one
    ((3, 63), 1024): (1, 1, 1, 1, 1), ((4, 64), 1024): (1, 1, 1, 1, 1), ((5, 65), 1024): (2, 2, 1, 1, 1), ((9, 70), 1024): (3, 2, 1, 1, 1),
    ((37, 130), 1024): (10, 3, 1, 1, 1),
    # thin axes
    ((1, 5), 1024): (1, 1, 1, 1, 1), ((6, 1), 1024): (2, 1, 1, 1, 1), ((2, 2), 1024): (1, 1, 1, 1, 1), ((2, 3, 1), 1024): (1, 1, 1, 2, 1),
    ((1, 6, 5), 1024): (2, 1, 1, 1, 1), ((5, 1, 66), 1024): (1, 2, 1, 5, 1),
    # 3-D, one plane per chunk
    ((7, 9, 70), 1024): (3, 2, 1, 7, 1), ((3, 5, 65), 1024): (2, 2, 1, 3, 1), ((4, 4, 64), 1024): (1, 1, 1, 4, 1),
    # chunked: 18 tiles, 3 planes per workgroup, 39 chunks, ONE plane in the last; explicit: 2 planes per workgroup, 116 chunks, one plane in the last
    ((115, 33, 65), 1024): (9, 2, 3, 39, 1), ((231, 33, 65), 4096): (9, 2, 2, 116, 1),
    ((115, 33, 65), 4096): (9, 2, 1, 115, 1),        # (CM_RHS of the chunked CG case runs under the explicit target: one plane per workgroup)
    # mid-size: 51 tiles, ragged on both in-plane axes; CG marches 4 planes per workgroup, explicit 1
    ((64, 66, 130), 1024): (17, 3, 4, 16, 4), ((64, 66, 130), 4096): (17, 3, 1, 64, 1),
}
for (_res, _target), _p in list(PLANS.items()):       # the small shapes have the same plan under the explicit target
    if _target == 1024 and _p[2] == 1 and (_res, 4096) not in PLANS:
        PLANS[(_res, 4096)] = _p


class Case:
    """ a grid, u's walls (kind per axis) and the coefficient's (kind per axis: one letter of C_KINDS for both sides or a (lower, upper) pair) """

    def __init__(self, res, u_kinds, c_kinds, batch=1, seed=0, form='shared', trajectory=None, check_plan=True):
        self.res, self.batch, self.seed, self.form, self.check_plan = tuple(res), int(batch), int(seed), form, check_plan
        D = self.rank = len(res)
        self.u_codes = [tuple(k) for k in u_kinds]
        # non-zero, pairwise different constants on every CLOSED side of u
        self.u_vals = [[(0.5 + 0.25 * d) if lo == CLO else 0.0, (-0.75 + 0.125 * d) if hi == CLO else 0.0] for d, (lo, hi) in enumerate(self.u_codes)]
        sides = [(k, k) if isinstance(k, str) else tuple(k) for k in c_kinds]
        self.c_letters = ["".join(s) for s in sides]
        self.a_codes = [[C_KINDS[lo][0], C_KINDS[hi][0]] for lo, hi in sides]
        self.a_vals = [[C_KINDS[lo][1], C_KINDS[hi][1]] for lo, hi in sides]
        self.dx = DX[:D]
        self.upper = tuple(n * h for n, h in zip(self.res, self.dx))
        self.kdt = [w * h * h for w, h in zip(WEIGHTS[D], self.dx)]
        self.cells = int(np.prod(self.res))
        self.affine = any(c == CLO for pair in self.u_codes for c in pair)
        # grids of a handful of cells: CG is exact after as many iterations as the operator has distinct eigenvalues, the trajectory beyond is rounding noise
        self.trajectory = TRAJECTORIES[0] if self.cells < 16 else (trajectory or TRAJECTORIES[1])

    @property
    def id(self):
        return "x".join(map(str, self.res)) + "-" + "".join("pco"[lo] + "pco"[hi] for lo, hi in self.u_codes) + "-" + ".".join(self.c_letters) + f"-b{self.batch}"

    def grid(self, dtype, batch=None):
        code = C.PHIHIP_F64 if np.dtype(dtype) == np.float64 else C.PHIHIP_F32
        bc = [[PER if c == PER else OPN for c in pair] for pair in self.u_codes]       # the grid carries the cells; periodicity must match the scalar's
        return C.make_grid(self.rank, code, self.batch if batch is None else batch, self.res, (0.0,) * self.rank, self.upper, bc)

    def assert_plan(self, target):
        if self.check_plan:
            got, want = plan(self.res, target), PLANS[(self.res, target)]
            assert got == want, f"{self.id}: coef_plan(target {target}) gives (tiles1, tiles2, chunk, chunks, last) = {got}, the case is there for {want}"

    def inputs(self, dtype, form=None, seed_shift=0):
        """ u [B, *res] white noise, a [1 or B, *res] = 0.25 + U(0, 1) or None, both rounded to the element type """
        form = form or self.form
        rng = np.random.default_rng(1000 * self.seed + seed_shift)
        u = rng.standard_normal((self.batch,) + self.res).astype(dtype)
        a = None if form == 'absent' else (0.25 + rng.random(((self.batch if form == 'per_entry' else 1),) + self.res)).astype(dtype)
        return u, a


def _walls_table():
    """ the case table. Across it every internal axis (a0 included) meets every (u kind, coefficient kind) pair -- asserted by `wall_coverage` --, axes of one
    and two cells sit under every u kind, batch 1, 2 and 3 and the three coefficient forms appear, and the five trajectory settings take turns """
    edge2 = [(3, 63), (4, 64), (5, 65), (9, 70), (37, 130)]
    thin = [(1, 5), (6, 1), (2, 2), (2, 3, 1), (1, 6, 5), (5, 1, 66)]
    planes3 = [(7, 9, 70), (3, 5, 65), (4, 4, 64)]
    cases = []
    for shapes in (edge2, planes3):
        for i in range(20):
            res = shapes[(i + i // 5) % len(shapes)]
            pairs = [PAIRS[(i + 7 * d) % 20] for d in range(len(res))]
            batch = 1 + i % 3 if np.prod(res) < 4000 else 1 + i % 2          # (batch 3 on the smaller grids: the emulation's time goes with the threads)
            cases.append(Case(res, [U_KINDS[u] for u, _ in pairs], [c for _, c in pairs], batch=batch, seed=len(cases), form=FORMS[(i // 3) % 3],
                              trajectory=TRAJECTORIES[i % 5]))
    for s, res in enumerate(thin):
        for k in range(5):
            u_kinds = [U_KINDS[k] if n <= 2 else U_KINDS[(k + 1 + d) % 5] for d, n in enumerate(res)]
            cases.append(Case(res, u_kinds, ['PZK0'[(k + s + d) % 4] for d in range(len(res))], batch=1 + (k + s) % 3, seed=len(cases), form=FORMS[(k + s) % 3],
                              trajectory=TRAJECTORIES[(k + s) % 5]))
    return cases


TABLE = _walls_table()
# the non-affine path (every u wall OPEN or PERIODIC): CM_RHS does not run and u itself is the right-hand side
NON_AFFINE = [Case((9, 70), [(OPN, OPN), (PER, PER)], ['K', 'Z'], batch=2, seed=101, form='per_entry'),
              Case((7, 9, 70), [(PER, PER), (OPN, OPN), (PER, PER)], ['Z', '0', 'P'], batch=1, seed=102)]
# every trajectory setting, both methods with refresh steps inside, on the grids of the prototype
FULL = [Case((9, 70), [(CLO, OPN), (OPN, CLO)], [('K', 'Z'), ('Z', '0')], batch=2, seed=111),
        Case((37, 130), [(PER, PER), (CLO, CLO)], ['Z', ('0', 'K')], batch=1, seed=112, form='absent'),
        Case((7, 9, 70), [(OPN, CLO), (CLO, OPN), (PER, PER)], ['P', ('Z', 'K'), 'Z'], batch=1, seed=113, form='per_entry')]


def _chunked(res, seed):
    """ a0 PERIODIC: the wrap plane belongs to another workgroup's chunk; a0 (CLOSED, OPEN) with a constant / ZERO_GRADIENT coefficient and a0 (OPEN, CLOSED)
    with a PERIODIC one (`coff = wrapped` across the chunks): plane_nb's three coefficient rules """
    return {'periodic': Case(res, [(PER, PER), (CLO, OPN), (OPN, CLO)], ['Z', 'K', 'P'], batch=1, seed=seed),
            'walls': Case(res, [(CLO, OPN), (OPN, OPN), (CLO, CLO)], [('K', 'Z'), 'Z', '0'], batch=2, seed=seed + 1),
            'wrapped': Case(res, [(OPN, CLO), (PER, PER), (CLO, OPN)], ['P', 'K', 'Z'], batch=1, seed=seed + 2, form='per_entry')}


CHUNKED_CG = _chunked((115, 33, 65), 121)
CHUNKED_EXPLICIT = _chunked((231, 33, 65), 131)
CHUNKED_TRAJECTORIES = [(3, 2, 'CG'), (3, 2, 'CG-adaptive')]
MID = Case((64, 66, 130), [(CLO, OPN), (PER, PER), (OPN, CLO)], [('Z', 'K'), 'P', '0'], batch=1, seed=141)


def wall_coverage(cases):
    """ internal axis (0, 1, 2) -> the set of (u kind, coefficient kind) pairs with both sides of the coefficient alike that the cases put on it """
    seen = {0: set(), 1: set(), 2: set()}
    for c in cases:
        for d in range(c.rank):
            if c.c_letters[d][0] == c.c_letters[d][1]:
                seen[d + 3 - c.rank].add((U_KINDS.index(c.u_codes[d]), c.c_letters[d][0]))
    return seen


def thin_coverage(cases):
    """ (cells, internal axis) -> the u kinds that axes of one and two cells sit under """
    seen = {}
    for c in cases:
        for d, n in enumerate(c.res):
            if n <= 2:
                seen.setdefault((n, d + 3 - c.rank), set()).add(U_KINDS.index(c.u_codes[d]))
    return seen


# ---- comparison ------------------------------------------------------------------------------------------------------------------------------------------------
def _dist(a, ref):
    """ max |a - ref| / max |ref|, every element """
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-300)


def _rel_l2(a, ref):
    return float(np.linalg.norm((np.asarray(a, np.float64) - ref).ravel())) / max(float(np.linalg.norm(np.asarray(ref).ravel())), 1e-300)


RECORDS = []          # (check, dtype name, e_kernel, e_ref32 or None): the source of the table in DESIGN.md


def _device(mem, a):
    return None if a is None else mem.to_dev(a)


def _ptr(mem, h):
    return 0 if h is None else mem.ptr(h)


def _f64(a):
    return None if a is None else a.astype(np.float64)


# ---- (a) one explicit step ----------------------------------------------------------------------------------------------------------------------------------
def check_explicit(ctx, mem, case, dtype, forms=FORMS, signs=(1.0, -1.0)):
    """ diffuse_explicit_centered_coef (forward) against R.explicit, every element; kdt < 0 takes the larger neighbour (sharpen) """
    case.assert_plan(TARGET_EXPLICIT)
    f32 = np.dtype(dtype) == np.float32
    tol = (TOL32 if f32 else TOL64)['stencil']
    grid = case.grid(dtype)
    worst = 0.0
    for k, form in enumerate(forms):
        u, a = case.inputs(dtype, form, seed_shift=k)
        du, da = mem.to_dev(u), _device(mem, a)
        for sign in signs:
            kdt = [sign * v for v in case.kdt]
            dout = mem.empty(u.shape, dtype)           # (NaN everywhere: an element the kernel does not write shows)
            ctx.diffuse_explicit_centered_coef(grid, mem.ptr(du), case.u_codes, case.u_vals, _ptr(mem, da), 1 if a is None else a.shape[0], case.a_codes, case.a_vals,
                                               kdt, mem.ptr(dout))
            mem.sync()
            out = mem.to_host(dout)
            ref = R.explicit(_f64(u), _f64(a), kdt, case.dx, case.u_codes, case.u_vals, case.a_codes, case.a_vals)
            assert np.isfinite(out).all(), f"explicit {case.id} {form}: non-finite or unwritten elements"
            e = _dist(out, ref)
            e32 = _dist(R.explicit(u, a, kdt, case.dx, case.u_codes, case.u_vals, case.a_codes, case.a_vals, dtype=np.float32), ref) if f32 else None
            print(f"DCEW explicit {case.id} {form} sign {sign:+.0f} {np.dtype(dtype).name} e_kernel {e:.2e}" + (f" e_ref32 {e32:.2e}" if f32 else "") + f" (bound {tol:.0e})",
                  flush=True)
            RECORDS.append(('explicit', np.dtype(dtype).name, e, e32))
            if e > tol:
                diff = np.abs(out.astype(np.float64) - ref)
                where = np.unravel_index(int(diff.argmax()), diff.shape)
                raise AssertionError(f"explicit {case.id} {form} sign {sign:+.0f}: element {where} is {out[where]!r}, the reference {ref[where]!r} ({e:.2e} of max|reference|; "
                                     f"bound {tol:.0e}; {int((diff > tol * np.abs(ref).max()).sum())} elements beyond it)")
            worst = max(worst, e)
    return worst


# ---- (b) the first K iterations of the CG -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pin_recurrence(method):
    """ R.cg_trajectory's recurrences against the oracle's cg / cg_adaptive (which are pinned to the reference project) on one small system, with refresh """
    case = FULL[0]
    u, a = (_f64(v) for v in case.inputs(np.float64))
    w = [-k / (h * h) for k, h in zip(case.kdt, case.dx)]
    zero = [[0.0, 0.0]] * case.rank
    A = lambda x: x + R.lap(x, a, w, case.u_codes, zero, case.a_codes, case.a_vals)
    y = u - R.lap(np.zeros_like(u), a, w, case.u_codes, case.u_vals, case.a_codes, case.a_vals)
    worst = 0.0
    for K, refresh in ((3, 50), (5, 2)):
        x, info = (O.cg if method == 'CG' else O.cg_adaptive)(A, y, u, 1e-30, 0.0, K, refresh)
        t = R.cg_trajectory(u, a, case.kdt, case.dx, case.u_codes, case.u_vals, case.a_codes, case.a_vals, K, refresh, method)
        worst = max(worst, _dist(t.x, x), float(np.abs(t.residual_sq / info.residual_sq - 1).max()), float(np.abs(t.rhs_sq / info.rhs_sq - 1).max()))
        assert list(info.iterations) == [K] * case.batch
    print(f"DCEW pin {method}: cg_trajectory vs the oracle's recurrence {worst:.2e}", flush=True)
    assert worst <= 1e-13, f"tests/diffuse_coef_ref.py cg_trajectory('{method}') is {worst:.2e} from the oracle's recurrence"
    return worst


def check_cg_trajectory(ctx, mem, case, dtype, K=None, refresh_every=None, method=None, form=None):
    """ diffuse_implicit_centered_coef stopped after K iterations: x element by element, sum r^2 and sum y^2 per batch entry, iterations == K """
    if K is None:
        K, refresh_every, method = case.trajectory
    _pin_recurrence(method)
    case.assert_plan(TARGET_CG)
    if case.affine:
        case.assert_plan(TARGET_EXPLICIT)        # (CM_RHS runs under the explicit pass's plan)
    f32 = np.dtype(dtype) == np.float32
    name = np.dtype(dtype).name
    u, a = case.inputs(dtype, form)
    grid = case.grid(dtype)
    du, da, dout = mem.to_dev(u), _device(mem, a), mem.empty(u.shape, dtype)
    solve = C.Solve(1e-30, 0.0, int(K), int(refresh_every), 0, METHOD_CODE[method])
    info = ctx.diffuse_implicit_centered_coef(grid, mem.ptr(du), case.u_codes, case.u_vals, _ptr(mem, da), 1 if a is None else a.shape[0], case.a_codes, case.a_vals,
                                              case.kdt, mem.ptr(dout), solve)
    mem.sync()
    x = mem.to_host(dout)
    args = (case.kdt, case.dx, case.u_codes, case.u_vals, case.a_codes, case.a_vals, K, refresh_every, method)
    ref = R.cg_trajectory(_f64(u), _f64(a), *args)
    ref32 = R.cg_trajectory(u, a, *args, dtype=np.float32) if f32 else None
    tag = f"trajectory {case.id} {form or case.form} K {K} refresh {refresh_every} {method} {name}"
    assert np.isfinite(x).all(), f"{tag}: non-finite or unwritten elements"
    # the trajectory must not have collapsed into rounding noise (decided by the reference alone): r is then known to ~ eps |y| / |r| <= 1e-12 of itself
    assert (ref.residual_sq >= 1e-8 * ref.rhs_sq).all(), f"{tag}: the reference's residual is {ref.residual_sq} of {ref.rhs_sq}: choose fewer iterations for this grid"
    failures = []
    for b in range(case.batch):
        e = _dist(x[b], ref.x[b])
        rs, ys = float(info[b].residual_sq), float(info[b].rhs_sq)
        e_rs, e_ys = abs(rs - ref.residual_sq[b]) / ref.residual_sq[b], abs(ys - ref.rhs_sq[b]) / ref.rhs_sq[b]
        if f32:
            e32 = _dist(ref32.x[b], ref.x[b])
            bound_x = FACTOR32 * e32 + 16 * EPS32
            bound_rs = 2 * (FACTOR32 * _rel_l2(ref32.r[b], ref.r[b]) + 16 * EPS32)
            bound_ys = 2 * (FACTOR32 * _rel_l2(ref32.y[b], ref.y[b]) + 16 * EPS32)
            print(f"DCEW {tag} entry {b}: x e_kernel {e:.2e} e_ref32 {e32:.2e} ratio {e / max(e32, 1e-300):.2f} (bound {bound_x:.2e}); residual_sq rel {e_rs:.2e} "
                  f"(bound {bound_rs:.2e}); rhs_sq rel {e_ys:.2e} (bound {bound_ys:.2e}); iterations {info[b].iterations}", flush=True)
        else:
            e32, bound_x, bound_rs, bound_ys = None, TOL64_X, TOL64_SUMS, TOL64_SUMS
            print(f"DCEW {tag} entry {b}: x e_kernel {e:.2e} (bound {bound_x:.0e}); residual_sq rel {e_rs:.2e}; rhs_sq rel {e_ys:.2e} (bound {bound_rs:.0e}); "
                  f"iterations {info[b].iterations}", flush=True)
        RECORDS.append(('trajectory', name, e, e32))
        if info[b].iterations != K:
            failures.append(f"entry {b}: {info[b].iterations} iterations, not {K}")
        if e > bound_x:
            failures.append(f"entry {b}: x is {e:.2e} of max|reference| from the float64 reference (bound {bound_x:.2e})")
        if e_rs > bound_rs:
            failures.append(f"entry {b}: residual_sq {rs!r} vs {ref.residual_sq[b]!r} ({e_rs:.2e} > {bound_rs:.2e})")
        if e_ys > bound_ys:
            failures.append(f"entry {b}: rhs_sq {ys!r} vs {ref.rhs_sq[b]!r} ({e_ys:.2e} > {bound_ys:.2e})")
    assert not failures, f"{tag}: " + "; ".join(failures)


def check_cg_trajectory_random(ctx, mem, res, u_codes, seed):
    """ tests/fuzz_parity.py: check (b) in fp64 with K = 3 and a refresh inside on a grid and u walls of the caller's; the coefficient's walls, its form and the
    method follow the seed """
    r = np.random.default_rng(seed)
    c_kinds = [tuple(str(r.choice(list('PZK0'))) for _ in range(2)) for _ in res]
    c_kinds = [('P', 'P') if 'P' in k else k for k in c_kinds]
    case = Case(res, u_codes, c_kinds, batch=int(r.integers(1, 4)), seed=seed, form=FORMS[int(r.integers(0, 3))], check_plan=False)
    K, refresh = (3, 2) if case.cells >= 16 else (1, 50)
    check_cg_trajectory(ctx, mem, case, np.float64, K, refresh, 'CG' if seed % 2 == 0 else 'CG-adaptive')


# ---- (c) batch entries that stop at different iterations ---------------------------------------------------------------------------------------------------------
FREEZE_RES, FREEZE_KDT = (9, 70), (2.0, 3.0)
FREEZE_U_CODES, FREEZE_U_VALS = [(OPN, OPN), (PER, PER)], [[0.0, 0.0], [0.0, 0.0]]
FREEZE_A_CODES, FREEZE_A_VALS = [[OPN, OPN], [PER, PER]], [[0.0, 0.0], [0.0, 0.0]]
FREEZE_RTOL = {'float64': 1e-12, 'float32': 1e-5}
FREEZE_REFRESH = {'CG': 50, 'CG-adaptive': 20}        # PhiML's periods


def _freeze_inputs(dtype):
    """ three entries: a smooth field, white noise, a constant (under OPEN / PERIODIC walls A u = u: r0 == 0 exactly); one shared coefficient """
    rng = np.random.default_rng(77)
    i, j = np.meshgrid(np.arange(FREEZE_RES[0]), np.arange(FREEZE_RES[1]), indexing='ij')
    smooth = 1.0 + 0.5 * np.cos(np.pi * (i + 0.5) / FREEZE_RES[0]) * np.sin(2 * np.pi * j / FREEZE_RES[1])
    u = np.stack([smooth, rng.standard_normal(FREEZE_RES), np.full(FREEZE_RES, 1.5)]).astype(dtype)
    a = (0.25 + rng.random((1,) + FREEZE_RES)).astype(dtype)
    return u, a


@functools.lru_cache(maxsize=None)
def _freeze_reference(dtype_name, method):
    """ the oracle's iteration counts (float64, on the inputs rounded to the element type) and the direct solve; computed once, never modified """
    u, a = (_f64(v) for v in _freeze_inputs(np.dtype(dtype_name)))
    w = [-k for k in FREEZE_KDT]
    A = lambda x: x + R.lap(x, a, w, FREEZE_U_CODES, FREEZE_U_VALS, FREEZE_A_CODES, FREEZE_A_VALS)
    _, info = (O.cg if method == 'CG' else O.cg_adaptive)(A, u, u, FREEZE_RTOL[dtype_name], 0.0, 1000, FREEZE_REFRESH[method])
    counts = [int(n) for n in info.iterations]
    direct = R.implicit(u, a, FREEZE_KDT, (1.0, 1.0), FREEZE_U_CODES, FREEZE_U_VALS, FREEZE_A_CODES, FREEZE_A_VALS)
    return counts, direct


def _freeze_solve(ctx, mem, dtype, u, a, solve):
    code = C.PHIHIP_F64 if np.dtype(dtype) == np.float64 else C.PHIHIP_F32
    grid = C.make_grid(2, code, u.shape[0], FREEZE_RES, (0.0, 0.0), tuple(float(n) for n in FREEZE_RES), [[OPN, OPN], [PER, PER]])
    du, da, dout = mem.to_dev(u), mem.to_dev(a), mem.empty(u.shape, dtype)
    info = ctx.diffuse_implicit_centered_coef(grid, mem.ptr(du), FREEZE_U_CODES, FREEZE_U_VALS, mem.ptr(da), 1, FREEZE_A_CODES, FREEZE_A_VALS, FREEZE_KDT,
                                              mem.ptr(dout), solve)
    mem.sync()
    return mem.to_host(dout), [(i.residual_sq, i.rhs_sq, i.iterations, i.converged, i.diverged) for i in info]


def check_batch_freeze(ctx, mem, dtype, method, check_every=1):
    """ tolerance mode. Each entry of the batch-3 call equals its own batch-1 call bit for bit (x and every SolveInfo field); the constant entry reports 0
    iterations, converged, and keeps x0 bit for bit; the counts equal the oracle's within the project's rule max(2, 5 %); x is the direct solve's """
    name = np.dtype(dtype).name
    rtol = FREEZE_RTOL[name]
    u, a = _freeze_inputs(dtype)
    counts, direct = _freeze_reference(name, method)
    tag = f"freeze {method} {name} check_every {check_every}"
    print(f"DCEW {tag}: the oracle's iteration counts {counts}", flush=True)
    assert counts[2] == 0 and all(abs(p - q) >= 3 for k, p in enumerate(counts) for q in counts[k + 1:]), f"{tag}: the reference's counts {counts} do not differ by >= 3"
    solve = C.Solve(rtol, 0.0, 1000, FREEZE_REFRESH[method], int(check_every), METHOD_CODE[method])
    x3, info3 = _freeze_solve(ctx, mem, dtype, u, a, solve)
    print(f"DCEW {tag}: iterations {[i[2] for i in info3]} converged {[i[3] for i in info3]}", flush=True)
    for b in range(3):
        x1, info1 = _freeze_solve(ctx, mem, dtype, np.ascontiguousarray(u[b:b + 1]), a, solve)
        assert np.array_equal(x1[0], x3[b]), f"{tag}: x of entry {b} of the batch-3 call differs from its batch-1 call in {int((x1[0] != x3[b]).sum())} elements"
        assert info1[0] == info3[b], f"{tag}: SolveInfo of entry {b}: batch-3 {info3[b]}, batch-1 {info1[0]}"
    if check_every != 1:         # every entry freezes itself on the device: how often the host looks must not change a bit
        x_1, info_1 = _freeze_solve(ctx, mem, dtype, u, a, C.Solve(rtol, 0.0, 1000, FREEZE_REFRESH[method], 1, METHOD_CODE[method]))
        assert np.array_equal(x_1, x3) and info_1 == info3, f"{tag}: the result depends on check_every"
    assert info3[2][2] == 0 and info3[2][3] == 1 and info3[2][4] == 0 and info3[2][0] == 0.0, f"{tag}: the constant entry reports {info3[2]}"
    assert np.array_equal(x3[2], u[2]), f"{tag}: the constant entry (r0 == 0) does not keep x0 bit for bit"
    for b in range(3):
        assert info3[b][3] == 1 and info3[b][4] == 0, f"{tag}: entry {b} reports {info3[b]}"
        assert abs(info3[b][2] - counts[b]) <= max(2, 0.05 * counts[b]), f"{tag}: entry {b} took {info3[b][2]} iterations, the oracle {counts[b]}"
    # |x - x*|_max <= |A^-1|_2 |r|_2 <= |r|_2 (A = I + L_a >= I) <= 2 rtol |y|_2 (the project's rule for the true residual of a converged solve);
    # fp64, rtol 1e-12: |y|_2 ~ 40, within the 1e-9 of the other implicit tests
    bound = 1e-9 if name == 'float64' else 2 * rtol * float(np.sqrt((u.astype(np.float64) ** 2).sum(axis=(1, 2)).max()))
    e = float(np.abs(x3.astype(np.float64) - direct).max())
    print(f"DCEW {tag}: max |x - direct solve| {e:.2e} (bound {bound:.2e})", flush=True)
    assert e <= bound, f"{tag}: x is {e:.2e} from the direct solve (bound {bound:.2e})"
    return counts, [i[2] for i in info3]


# ---- (d) the Python level: extrapolations to codes and constants -------------------------------------------------------------------------------------------------
def python_wall_cases():
    """ name -> (resolution, box, u's extrapolation, its codes and constants AS LITERALS, the coefficient's extrapolation, codes, constants, per-axis factors).
    Every axis of every table is asymmetric (a lower / upper swap shows) and every constant differs from the others """
    from phiflow_amd.flow import PERIODIC, ZERO_GRADIENT, combine_sides
    return {
        'mixed3d': dict(res=dict(x=6, y=5, z=7), box=((0, 3.0), (0, 2.0), (0, 1.75)), factors=(1, 2, 0.5),
                        u_ext=combine_sides(x=(1.0, ZERO_GRADIENT), y=PERIODIC, z=(ZERO_GRADIENT, -0.5)),
                        u_codes=[[1, 2], [0, 0], [2, 1]], u_vals=[[1.0, 0.0], [0.0, 0.0], [0.0, -0.5]],
                        a_ext=combine_sides(x=(ZERO_GRADIENT, 2.5), y=PERIODIC, z=(0.0, ZERO_GRADIENT)),
                        a_codes=[[2, 1], [0, 0], [1, 2]], a_vals=[[0.0, 2.5], [0.0, 0.0], [0.0, 0.0]]),
        'heat_flow': dict(res=dict(x=12, y=10), box=((0, 10.0), (0, 5.0)), factors=None,
                          u_ext={'x-': 1, 'x+': ZERO_GRADIENT, 'y': PERIODIC},
                          u_codes=[[1, 2], [0, 0]], u_vals=[[1.0, 0.0], [0.0, 0.0]],
                          a_ext=ZERO_GRADIENT, a_codes=[[2, 2], [2, 2]], a_vals=[[0.0, 0.0], [0.0, 0.0]]),
        # the coefficient's constants meet CLOSED sides of u: 2.5 at x+, 0 at y-
        'constants2d': dict(res=dict(x=9, y=11), box=((0, 3.0), (0, 5.5)), factors=(1, 2),
                            u_ext=combine_sides(x=(ZERO_GRADIENT, 1.0), y=(-0.25, 0.5)),
                            u_codes=[[2, 1], [1, 1]], u_vals=[[0.0, 1.0], [-0.25, 0.5]],
                            a_ext=combine_sides(x=(ZERO_GRADIENT, 2.5), y=(0.0, ZERO_GRADIENT)),
                            a_codes=[[2, 1], [1, 2]], a_vals=[[0.0, 2.5], [0.0, 0.0]]),
    }


def check_python_walls(backend, name, bits):
    """ diffuse.explicit (dt > 0) and diffuse.implicit on CenteredGrids against the reference fed from the literal tables """
    from phiflow_amd.flow import Box, CenteredGrid, Solve, diffuse, precision
    spec = python_wall_cases()[name]
    dims = list(spec['res'])
    shape = tuple(spec['res'].values())
    dtype = np.float64 if bits == 64 else np.float32
    rng = np.random.default_rng(len(name))
    u_np = rng.standard_normal((1,) + shape).astype(dtype)
    a_np = (0.25 + rng.random((1,) + shape)).astype(dtype)
    with precision(bits):
        box = Box(**{d: (lo, hi) for d, (lo, hi) in zip(dims, spec['box'])})
        u = CenteredGrid(u_np, spec['u_ext'], box, backend=backend, **spec['res'])
        a = CenteredGrid(a_np, spec['a_ext'], box, backend=backend, **spec['res'])
        dx = [(hi - lo) / n for (lo, hi), n in zip(spec['box'], shape)]
        factors = spec['factors'] or (1,) * len(shape)
        amount = a * spec['factors'] if spec['factors'] else a
        tol = (TOL64 if bits == 64 else TOL32)['stencil']
        dt = 0.3 * min(dx) ** 2
        out = diffuse.explicit(u, amount, dt).numpy()
        walls = (spec['u_codes'], spec['u_vals'], spec['a_codes'], spec['a_vals'])
        ref = R.explicit(_f64(u_np), _f64(a_np), [f * dt for f in factors], dx, *walls)
        e = _dist(out, ref)
        print(f"DCEW python {name} fp{bits} explicit e_kernel {e:.2e} (bound {tol:.0e})", flush=True)
        assert e <= tol, f"diffuse.explicit {name}: {e:.2e} of max|reference| from the reference fed from the literal wall table"
        rtol = 1e-12 if bits == 64 else 1e-6
        dt = 1.5 * min(dx) ** 2
        sol = diffuse.implicit(u, amount, dt, Solve('CG', rtol, 0, max_iterations=1000))
        assert all(sol.solve_info.converged)
        ref = R.implicit(_f64(u_np), _f64(a_np), [f * dt for f in factors], dx, *walls)
        # fp64: the 1e-9 of the other implicit tests; fp32: |x - x*|_max <= |r|_2 <= 2 rtol |y|_2 as in check_batch_freeze, y = u - L(0) from the reference
        y = _f64(u_np) - R.lap(np.zeros(u_np.shape), _f64(a_np), [-f * dt / (h * h) for f, h in zip(factors, dx)], *walls)
        bound = 1e-9 if bits == 64 else 2 * rtol * float(np.sqrt((y ** 2).sum(axis=tuple(range(1, y.ndim))).max()))
        e = float(np.abs(sol.numpy().astype(np.float64) - ref).max())
        print(f"DCEW python {name} fp{bits} implicit max |x - direct solve| {e:.2e} (bound {bound:.2e})", flush=True)
        assert e <= bound, f"diffuse.implicit {name}: {e:.2e} from the direct solve fed from the literal wall table (bound {bound:.2e})"
