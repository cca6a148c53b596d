"""
Element-wise parity of the SDF obstacle kernels (phiflow_amd/csrc/obstacle_sdf.hpp) through the C ABI, in the layout of tests/project_elementwise_cases.py (f12).
Used by tests/test_sdf_obstacle_emu.py (emulation) and tests/test_gpu_sdf_obstacle.py (MI355X). DESIGN.md "f13" holds the derivation.

Reference: tests/sdf_obstacle_ref.py (float64, from the reference's text) on the SDF values AFTER rounding to the array's element type and the velocity AFTER
rounding to its own; the obstacle loop, the flags and the bound are tests/project_ref.py's (accessible, cell_flags, apply_obstacles, surface_clearance), which
take the SDF obstacle through the same duck-typed interface as Box and Sphere. Rule per sample, no sample dropped:
    phihip_obstacle_accessible, phihip_build_cellflags of it      equal
    phihip_apply_obstacles                                         |kernel - ref| <= eps(T) E + eps64 (K_REF scale + K_GEO G)          (f12's constants)
G covers the rounding of the sampled distance through `reach` (sdf_obstacle_ref.SdfObstacle.reach): the scenes are scaled to a Lipschitz constant <= 1.
Discrete decisions are kept safe by the reference alone: |sampled sdf| at every centre and face, and with approximate_outside every sample coordinate's
distance to each bounds face, exceed f12's CLEARANCE (in units of the smallest cell); the first of 8 seeds that qualifies is taken and asserted.
"""
import itertools
import math

import numpy as np

import project_elementwise_cases as P
import project_ref as R
import sdf_obstacle_ref as S
from parity_cases import CLO, OPN, PER, C, obstacle_items

CLEARANCE = P.CLEARANCE
EPS64 = P.EPS64

# simulation grids: the smallest that cross every edge of the (4 x 64) patches, with the boundary mixes of f12's OBSTACLE_GRIDS; batch 1 and 3
GRIDS = [((5, 7), ((OPN, CLO), (PER, PER)), 3), ((9, 70), ((PER, PER), (OPN, CLO)), 1), ((24, 20), ((CLO, CLO), (OPN, OPN)), 3),
         ((5, 6, 134), ((OPN, OPN), (CLO, CLO), (PER, PER)), 1), ((12, 10, 16), ((CLO, OPN), (PER, PER), (CLO, CLO)), 3)]
# SDF resolutions: 1 and 2 along an axis (every clamp), a coarse grid, a fine one not aligned with the simulation grid
SDF_RES = {2: [(1, 5), (6, 2), (3, 4), (40, 33)], 3: [(1, 5, 2), (2, 1, 6), (3, 4, 5), (21, 17, 13)]}
SCENES = ("star", "two blobs", "mixed", "partly outside", "outside", "covering")
OPTIONS = ("approximate_outside", "sdf64", "moving", "explicit")


def case_id(case):
    return P.case_id(case)


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------------------------------
def blob_values(sres, lower, upper, centre, r_f, lobes, amp, phase):
    """ a star-shaped blob at the cell centres of the SDF grid, in coordinates q = (x - c) / size of the bounds: (|q| - r_f (1 + amp cos(lobes * angle + phase)))
    * min(size), divided by its own Lipschitz constant where that exceeds 1 (the zero level set stays): neighbouring values then differ by less than the cell size
    along the axis -- by a margin of 1e-3 that the rounding to fp32 cannot use up """
    pts = S.cell_centres(sres, lower, upper)
    q = [(p - c) / (u - l) for p, c, l, u in zip(pts, centre, lower, upper)]
    rad = np.sqrt(sum(x * x for x in q))
    ang = np.arctan2(q[-1], q[-2]) + (0.0 if len(sres) == 2 else 0.7 * np.arctan2(q[0], np.sqrt(q[1] ** 2 + q[2] ** 2)))
    vals = (rad - r_f * (1.0 + amp * np.cos(lobes * ang + phase))) * min(u - l for l, u in zip(lower, upper))
    vals = np.broadcast_to(vals, tuple(sres)).astype(np.float64)
    lip = 0.0
    for a, n in enumerate(sres):
        if n > 1:
            lip = max(lip, float(np.abs(np.diff(vals, axis=a)).max()) / ((upper[a] - lower[a]) / n))
    return vals / (max(lip, 1.0) * (1.0 + 1e-3))


def make_sdf(rng, L, sres, lo_f, hi_f, opts, sdf_dtype, velocity=None, r_f=0.22):
    """ a blob on bounds [lo_f L, hi_f L] (jittered by the seed); opts: approximate_outside, explicit center / bounding_radius """
    D = len(L)
    j = lambda: rng.uniform(-0.02, 0.02)
    lower = [(lo_f[a] + j()) * L[a] for a in range(D)]
    upper = [(hi_f[a] + j()) * L[a] for a in range(D)]
    centre = [0.5 * (l + u) + j() * (u - l) for l, u in zip(lower, upper)]
    r0 = r_f + j()
    vals = blob_values(sres, lower, upper, centre, r0, 5, 0.3, rng.uniform(0, 6.0)).astype(sdf_dtype)
    explicit = {}
    if opts["explicit"]:
        explicit = dict(center=[c + 0.01 * (u - l) for c, l, u in zip(centre, lower, upper)], bounding_radius=1.35 * r0 * max(u - l for l, u in zip(lower, upper)))
    return S.SdfObstacle(vals, lower, upper, opts["approximate_outside"], velocity=velocity, **explicit)


def scene(name, res, dx, rng, sres, opts, sdf_dtype):
    """ obstacles of one named scene on the domain [0, res * dx] """
    D = len(res)
    L = [n * h for n, h in zip(res, dx)]
    lin = (0.4, -0.7, 0.25)[:D]
    lin2 = (-0.3, 0.5, 0.6)[:D]
    moving = lin if opts["moving"] else None
    sdf = lambda lo, hi, vel, **kw: make_sdf(rng, L, sres, [lo] * D if np.isscalar(lo) else lo, [hi] * D if np.isscalar(hi) else hi, opts, sdf_dtype, vel, **kw)
    j = lambda: rng.uniform(-0.03, 0.03)
    pt = lambda *f: tuple((f[a] + j()) * L[a] for a in range(D))
    if name == "star":
        return [sdf(0.15, 0.85, moving)]
    if name == "two blobs":         # overlapping, different velocities: the order matters
        return [sdf((0.1, 0.15, 0.1)[:D], (0.7, 0.75, 0.8)[:D], lin), sdf((0.3, 0.25, 0.2)[:D], (0.9, 0.85, 0.9)[:D], lin2 if opts["moving"] else None)]
    if name == "mixed":             # [Box, SDF, moving Sphere, moving SDF, Box], overlapping: the cut into runs must keep the order
        return [R.Box(pt(0.2, 0.3, 0.25), pt(0.55, 0.6, 0.6)), sdf(0.25, 0.8, None), R.Sphere(pt(0.5, 0.5, 0.5), (0.2 + j()) * min(L), velocity=lin2),
                sdf((0.35, 0.1, 0.3)[:D], (0.95, 0.7, 0.9)[:D], lin), R.Box(pt(0.45, 0.4, 0.5), pt(0.7, 0.8, 0.75), velocity=lin if opts["moving"] else None)]
    if name == "partly outside":
        return [sdf((-0.4, 0.3, -0.3)[:D], (0.5, 1.3, 0.6)[:D], moving, r_f=0.3)]
    if name == "outside":
        return [sdf(1.6, 2.1, lin, r_f=0.12)]
    if name == "covering":
        return [sdf(-0.13, 1.17, moving, r_f=0.25)]
    if name == "margin":        # as f12's `margin`: the ball (center, bounding_radius) ends 0.95 cell radii below the cell centres of column 64, the first column of the
        radius = math.sqrt(sum((0.5 * h) ** 2 for h in dx))      # next 4 x 64 patch, and the bounds end well before: the mask 0.05 there comes from the distance to the ball
        big = 0.3 * L[-1]                                        # and is reached only through the margin of the patch box
        centre = [(int(0.5 * n) + 0.5) * h for n, h in zip(res[:-1], dx[:-1])] + [64.5 * dx[-1] - (0.95 + 0.01 * j()) * radius - big]
        lower = [(0.2 + j()) * l for l in L[:-1]] + [centre[-1] - 0.5 * big]
        upper = [(0.8 + j()) * l for l in L[:-1]] + [centre[-1] + 0.6 * big]
        vals = blob_values(sres, lower, upper, [0.5 * (l + u) for l, u in zip(lower, upper)], 0.25, 5, 0.3, 1.0).astype(sdf_dtype)
        return [S.SdfObstacle(vals, lower, upper, True, center=centre, bounding_radius=big, velocity=lin)]
    raise ValueError(name)


def pick_scene(name, res, bc, dx, seed, sres, opts, sdf_dtype, tries=8):
    """ the first seed (seed + 1000 k) of 8 whose geometry keeps every sample CLEARANCE cells off every discrete decision: decided by the reference alone """
    lower = (0.0,) * len(res)
    for k in range(tries):
        obs = scene(name, res, dx, np.random.default_rng(seed + 1000 * k), sres, opts, sdf_dtype)
        if R.surface_clearance(obs, res, bc, lower, dx) > CLEARANCE:
            return obs
    raise AssertionError(f"scene {name!r} on {res} (SDF {sres}): no seed of {tries} keeps the samples {CLEARANCE} cells off the surfaces and bounds faces")


def option_table(n):
    """ n option sets: the 4 options run through all 16 combinations, neighbours in the list differing in several options (a grid runs 24 sets: every combination) """
    combos = [dict(zip(OPTIONS, bits)) for bits in itertools.product((True, False), repeat=len(OPTIONS))]
    order = [0, 15, 5, 10, 3, 12, 6, 9, 1, 14, 2, 13, 4, 11, 7, 8]
    return [combos[order[k % 16]] for k in range(n)]


# ---- the check ---------------------------------------------------------------------------------------------------------------------------------------------------
def bind_items(ctx, mem, obstacles, D, keep):
    """ the obstacle list for the C ABI, in order: analytic entries as f12 builds them, SDF entries bound to a slot (handles and slots appended to `keep`) """
    items = []
    for ob in obstacles:
        if isinstance(ob, S.SdfObstacle):
            h = mem.to_dev(np.ascontiguousarray(ob.values))
            code = C.PHIHIP_F64 if ob.values.dtype == np.float64 else C.PHIHIP_F32
            slot = ctx.sdf_bind(C.make_sdf_grid(mem.ptr(h), code, ob.values.shape, ob.lower, ob.upper, ob.center, ob.bounding_radius, ob.approximate_outside))
            keep.append((h, slot))
            items.append(dict(kind=C.OBSTACLE_SDF, slot=slot, velocity=list(ob.velocity) if ob.velocity is not None else [0.0] * D))
        else:
            items += obstacle_items([P.to_oracle(ob)], D)
    return items


def check_sdf_obstacles(ctx, mem, res, bc, dtype, batch, obstacles, kind="random", seed=0, exact=False, what="scene", unchanged=False):
    """ phihip_obstacle_accessible (equality), phihip_build_cellflags of it (equality), phihip_apply_obstacles (in place, the bound project_ref.apply_obstacles
    returns). exact: the dyadic case, no clearance asked. unchanged: nothing may change (bounds entirely outside) """
    x = P.make_inputs(res, bc, dtype, batch, kind, seed)
    if exact:      # dx = 1, lower = 0
        x.dom, x.grid = P.make_case(tuple(res), bc, dtype, batch, bc_val=x.bcv)
        x.dx = x.dom.dx
    D = len(res)
    lower = (0.0,) * D
    if kind == "nonfinite":      # NaN and Inf where the first obstacle's mask is exactly 1
        planted = 0
        for d in range(D):
            inside = np.argwhere(np.broadcast_to(obstacles[0].sdf(R.face_points(d, x.res, x.bc, lower, x.dx)) <= 0, x.v[d].shape[1:]))
            for i, bad in zip(inside[:3], (np.nan, np.inf, -np.inf)):
                x.v[d][(slice(None),) + tuple(i)] = bad
                planted += 1
        assert planted, f"{what}: no sample inside the first obstacle"
    if not exact:
        c = R.surface_clearance(obstacles, x.res, x.bc, lower, x.dx)
        assert c > CLEARANCE, f"{what}: a sample lies {c:.2e} cells from a surface or a bounds face"
    keep = []
    try:
        items = bind_items(ctx, mem, obstacles, D, keep)
        arr = C.make_obstacles(items)
        g1 = C.make_grid(D, x.grid.dtype, 1, x.res, x.dom.lower, x.dom.upper, x.bc, x.bcv)
        dacc = P.empty(mem, x.res, np.uint8)
        ctx.obstacle_accessible(g1, arr, len(items), mem.ptr(dacc))
        mem.sync()
        acc = R.accessible(obstacles, x.res, lower, x.dx)
        got = mem.to_host(dacc)
        assert np.array_equal(got, acc), f"obstacle_accessible [{what}] res {res}: differs at {np.argwhere(got != acc)[:4].tolist()}"
        dfl = P.empty(mem, x.res, np.uint8)
        ctx.build_cellflags(g1, mem.ptr(dacc), 0, 1, mem.ptr(dfl))
        mem.sync()
        assert np.array_equal(mem.to_host(dfl), R.cell_flags(acc, None, x.res, x.bc, False)), f"build_cellflags of the accessible mask [{what}]"
        P.RECORDS.append(dict(entry="obstacle_accessible", path=what, dtype="uint8", res="x".join(map(str, x.res)), ratio=0.0, inside=int((acc == 0).sum())))
        v64 = P._to64(x.v)
        with np.errstate(invalid='ignore', over='ignore'):
            ref, E, G = R.apply_obstacles(v64, obstacles, x.res, x.bc, lower, x.dx)
            r32 = R.apply_obstacles(x.v, obstacles, x.res, x.bc, lower, x.dx, dtype)[0]
        dv = [P.to_dev(mem, a) for a in x.v]
        ctx.apply_obstacles(x.grid, arr, len(items), P._P(mem, dv))
        mem.sync()
        eps = P.eps_of(dtype)
        worst = 0.0
        for d in range(D):
            got = mem.to_host(dv[d])
            if unchanged:
                assert acc.all() and np.array_equal(P._bits(got), P._bits(x.v[d])), f"{what}: bounds entirely outside the domain, yet component {d} changed"
            scale = np.abs(ref[d]) + E[d]
            worst = max(worst, P.compare(f"apply_obstacles[{d}]", what, x, kind, got, ref[d], eps * E[d] + EPS64 * (P.K_REF * scale + P.K_GEO * G[d]),
                                         None, None if kind == "nonfinite" else r32[d]))
        return worst, int((acc == 0).sum())
    finally:
        for h, slot in keep:
            ctx.sdf_release(slot)


def dyadic_obstacles(res):
    """ dx = 1, lower = 0, the SDF grid identical to the cell grid: cell centres sit ON taps and faces half-way between two. Integer values (the L1 distance to a
    cell minus 2, and the distance to a plane minus 1: neighbours differ by exactly 1) with zeros: sampled values are integers or half-integers, exact on both
    sides, and the inclusive `<= 0` decides on the zeros themselves. One grid with approximate_outside (bounds faces ON the outer faces: inclusive too), one
    without, one in fp32 """
    idx = np.indices(res)
    c = [min(n - 2, 3) for n in res]
    l1 = sum(np.abs(i - k) for i, k in zip(idx, c)) - 2.0
    plane = np.abs(idx[-1] - (res[-1] - 2)) - 1.0 + 0.0 * idx[0]
    up = [float(n) for n in res]
    zero = [0.0] * len(res)
    obs = [S.SdfObstacle(l1.astype(np.float64), zero, up, True, center=[k + 0.5 for k in c], bounding_radius=2.0),
           S.SdfObstacle(plane.astype(np.float32), zero, up, False, velocity=(0.5, -0.25, 0.75)[:len(res)])]
    if min(res) >= 5:      # a block of -1 on the cells [1, n - 1): its bounds faces lie ON faces of the simulation grid, well inside the domain. Inclusive bounds give those
        inner = tuple(n - 2 for n in res)      # faces the mask 1; with a bounding radius of 0 anything outside the bounds is more than a cell radius from the "ball"
        obs.append(S.SdfObstacle(-np.ones(inner, np.float32), [1.0] * len(res), [float(n - 1) for n in res], True, center=[0.5 * n for n in res], bounding_radius=0.0))
    return obs


def run_sdf_obstacles(ctx, mem, res, bc, dtype, batch, seed=0, scenes=SCENES):
    """ every scene x every SDF resolution of the rank on one simulation grid; the options (approximate_outside, SDF dtype, moving, explicit center / radius) run
    through option_table along the way; a `nonfinite` and a `graded` input on the first scene; the dyadic case. Prints the figures (also when a check fails) """
    del P.RECORDS[:]
    D = len(res)
    worst = 0.0
    try:
        dx = P.make_inputs(res, bc, dtype, batch, "random", seed).dx
        table = option_table(len(scenes) * len(SDF_RES[D]))
        for k, (name, sres) in enumerate(itertools.product(scenes, SDF_RES[D])):
            opts = table[(k + seed) % len(table)]
            sdf_dtype = np.float64 if opts["sdf64"] else np.float32
            what = f"{name} sdf{'x'.join(map(str, sres))} " + "".join(o[0] if opts[o] else "-" for o in OPTIONS)
            obs = pick_scene(name, res, bc, dx, seed + k, sres, opts, sdf_dtype)
            w, inside = check_sdf_obstacles(ctx, mem, res, bc, dtype, batch, obs, "random", seed + k, what=what,
                                            unchanged=(name == "outside" and opts["approximate_outside"]))
            worst = max(worst, w)
            if name == "star" and min(sres) > 2:
                assert inside > 0, f"{what}: no cell inside the blob"
                for kind in ("nonfinite", "graded"):
                    worst = max(worst, check_sdf_obstacles(ctx, mem, res, bc, dtype, batch, obs, kind, seed + k, what=what)[0])
        if res[-1] > 64:
            opts = dict(approximate_outside=True, sdf64=False, moving=True, explicit=True)
            obs = pick_scene("margin", res, bc, dx, seed, SDF_RES[D][2], opts, np.float32)
            col = [p[..., 64:65] if p.shape[-1] > 1 else p for p in R.face_points(0, res, bc, (0.0,) * D, dx)]
            m = np.clip(1.0 - obs[0].sdf(col) / math.sqrt(sum((0.5 * h) ** 2 for h in dx)), 0, 1)
            assert 0.0 < m.max() < 0.1, f"margin: the mask in column 64 is {m.max()}"
            worst = max(worst, check_sdf_obstacles(ctx, mem, res, bc, dtype, batch, obs, "random", seed, what="margin")[0])
        check_sdf_obstacles(ctx, mem, res, bc, dtype, batch, dyadic_obstacles(res), "random", seed, exact=True, what="dyadic")
    finally:
        P.report()
    return worst
