"""
Element-wise parity of the cylinder branch of the obstacle kernels (phiflow_amd/csrc/project.hip: cylinder_coords, cylinder_extent; kind PHIHIP_OBSTACLE_CYLINDER)
through the C ABI, in the scheme of tests/project_elementwise_cases.check_obstacles (f12). Used by tests/test_cylinder_emu.py (emulation) and
tests/test_gpu_cylinder.py (MI355X). DESIGN.md "f16" holds the derivation.

Reference: tests/cylinder_ref.Cylinder (float64, from the reference's text); the obstacle loop, the flags and the bound are tests/project_ref.py's (accessible,
cell_flags, apply_obstacles, surface_clearance), which take the cylinder through the duck-typed interface of Box and Sphere. Rule per sample, no sample dropped:
    phihip_obstacle_accessible, phihip_build_cellflags of it      equal
    phihip_apply_obstacles                                         |kernel - ref| <= eps(T) E + eps64 (K_REF scale + K_CYL G)
K_CYL is counted, per side, in u = eps64 / 2: position (i + off) dx + lower 2, x - c 1, the rotation 5, two squares and their sum 3, the root 1, - R 1, / radius 1,
1 - . 1 = 15 u; both sides 30 u = 15 eps64, K_CYL = 16 (the old kinds have either the rotation or the root: K_GEO = 12). The cap |h| - depth / 2 has fewer.
Scene seeds are chosen by the reference alone: the first of 8 whose surface_clearance (mantle AND caps) exceeds CLEARANCE cells; asserted otherwise.
"""
import math

import numpy as np

import cylinder_ref as CR
import project_elementwise_cases as P
import project_ref as R
import sdf_obstacle_cases as SC
import sdf_obstacle_ref as S
from parity_cases import C, obstacle_items

CLEARANCE = P.CLEARANCE
EPS64 = P.EPS64
K_CYL = 16.0
GRIDS = [g for g in P.OBSTACLE_GRIDS if len(g[0]) == 3]       # (12, 10, 16) batch 2 and (5, 6, 134) batch 3: rows cross the 64-column tile
SCENES = ("along x", "along y", "along z", "generic rotation", "thin disc", "long rod", "linear velocity", "spinning", "tumbling", "union with a box",
          "cylinder sdf box", "outside", "covering", "16 cylinders")
LIN = (0.4, -0.7, 0.25)


def case_id(case):
    return P.case_id(case)


def _across(L, axis):
    return min(l for a, l in enumerate(L) if a != axis)


def scene(name, res, dx, rng):
    """ obstacles of one named scene on the domain [0, res * dx], positions jittered by the seed """
    L = [n * h for n, h in zip(res, dx)]
    j = lambda: rng.uniform(-0.03, 0.03)
    pt = lambda *f: tuple((f[a] + j()) * L[a] for a in range(3))
    cyl = lambda axis, r_f=0.22, d_f=0.5, c=(0.5, 0.45, 0.55), **kw: CR.Cylinder(pt(*c), (r_f + j()) * _across(L, axis), (d_f + j()) * L[axis], axis, **kw)
    if name in ("along x", "along y", "along z"):      # a wrong axis index (ax0, the dimension order) shows here
        return [cyl("xyz".index(name[-1]))]
    if name == "generic rotation":
        return [cyl(1, rotation=P._rot(3, rng))]
    if name == "thin disc":                             # thinner than a cell: no cell centre need lie inside, the soft mask still sees it
        disc = cyl(2, r_f=0.3)
        disc.depth = (0.3 + j()) * min(dx)
        return [disc, CR.Cylinder(pt(0.4, 0.6, 0.35), 0.25 * _across(L, 0), (0.4 + j()) * min(dx), 0, rotation=P._rot(3, rng))]
    if name == "long rod":                              # longer than the domain, thin: the culling box must not become the bounding sphere
        return [cyl(2, r_f=0.12, d_f=2.5), cyl(0, r_f=0.1, d_f=3.0, c=(0.5, 0.6, 0.4), rotation=P._rot(3, rng))]
    if name == "linear velocity":
        return [cyl(0, velocity=LIN)]
    if name == "spinning":                              # about its own axis, the axis turned
        M = P._rot(3, rng)
        return [cyl(1, rotation=M, angular_velocity=tuple(0.8 * M[:, 1]))]
    if name == "tumbling":                              # an angular velocity perpendicular to the axis, and a linear one
        return [cyl(2, velocity=LIN, angular_velocity=(0.7, -0.4, 0.0))]
    if name == "union with a box":
        return [R.Union([cyl(0, r_f=0.18, c=(0.45, 0.4, 0.5)), R.Box(pt(0.4, 0.45, 0.5), pt(0.8, 0.7, 0.9))], velocity=LIN)]
    if name == "cylinder sdf box":                      # in that order in one call: the cut into runs keeps the order
        opts = dict(approximate_outside=True, explicit=False)
        sdf = SC.make_sdf(rng, L, SC.SDF_RES[3][2], [0.25] * 3, [0.8] * 3, opts, np.float32, (-0.3, 0.5, 0.6))
        return [cyl(1, velocity=LIN), sdf, R.Box(pt(0.45, 0.4, 0.5), pt(0.7, 0.8, 0.75), velocity=LIN)]
    if name == "outside":
        return [CR.Cylinder(tuple(1.7 * l for l in L), 0.1 * min(L), 0.2 * min(L), 1, rotation=P._rot(3, rng), velocity=LIN)]
    if name == "covering":
        return [CR.Cylinder(pt(0.5, 0.5, 0.5), 2.0 * max(L), 4.0 * max(L), 0, rotation=P._rot(3, rng), velocity=LIN)]
    if name == "16 cylinders":                          # one full launch
        out = []
        for k in range(16):
            axis = k % 3
            out.append(CR.Cylinder(pt(*(0.1 + 0.8 * rng.random(3))), (0.05 + 0.08 * rng.random()) * _across(L, axis), (0.1 + 0.3 * rng.random()) * L[axis], axis,
                                   rotation=P._rot(3, rng) if k % 2 else None, velocity=LIN if k % 4 == 0 else None,
                                   angular_velocity=(0.5, -0.3, 0.9) if k % 5 == 0 else None))
        return out
    if name == "margin":
        return [margin_cylinder(res, dx, rng)[0]]
    raise ValueError(name)


def margin_cylinder(res, dx, rng):
    """ A cylinder turned 45 degrees about x whose upper rim points at a sample of component x in column 64, the first column of the next 4 x 64 patch: that sample
    has sdf = 0.85 cell radii (mask 0.15) and lies beyond |up| depth / 2 + R sqrt(1 - up^2) + margin along z, i.e. it is reached only through the margin terms of
    the culling box (cylinder_extent in project.hip). Returns (cylinder, the sample's index in component x, its position) """
    m = math.sqrt(sum((0.5 * h) ** 2 for h in dx))
    t = -math.pi / 4
    M = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(t), -math.sin(t)], [0.0, math.sin(t), math.cos(t)]])
    Rad, hd = 0.6 + 0.01 * rng.uniform(-1, 1), 1.0
    idx = (2, 3, 64)
    sample = np.array([idx[0] * dx[0], (idx[1] + 0.5) * dx[1], (idx[2] + 0.5) * dx[2]])      # (both grids' x sides store face 0: offset 0 -- asserted by the caller)
    local = np.array([0.0, -(Rad + 0.85 * m), hd + 0.85 * m])
    return CR.Cylinder(tuple(sample - M @ local), Rad, 2 * hd, 2, rotation=M, velocity=LIN), idx, sample


def pick_scene(name, res, bc, dx, seed, tries=8):
    """ the first seed (seed + 1000 k) whose geometry leaves every sample position farther than CLEARANCE cells from every surface: decided by the reference alone """
    for k in range(tries):
        obs = scene(name, res, dx, np.random.default_rng(seed + 1000 * k))
        if R.surface_clearance(obs, res, bc, (0.0,) * 3, dx) > CLEARANCE:
            return obs
    raise AssertionError(f"scene {name!r} on {res}: no seed of {tries} keeps the samples {CLEARANCE} cells off the surfaces")


def dyadic_obstacles(res):
    """ dx = 1, lower = 0: cell centres at half-integers, faces at integers. Centres on the half-grid; radius 5 puts cell centres (offsets (3, 4), (0, 5)) ON the
    mantle and depth 4 puts cell centres ON the caps; radius 2.5 puts faces (offsets (1.5, 2)) ON the mantle and depth 3 puts faces of the axis' own component
    ON the caps: `<=` is inclusive, and every coordinate, square, sum and root is exact in float64 on both sides """
    big = CR.Cylinder((min(res[0] // 2, 5) + 0.5, min(res[1] // 2 - 1, 4) + 0.5, 6.5), 5.0, 4.0, 0)
    small = CR.Cylinder((2.5, 2.5, 8.5), 2.5, 3.0, 2, velocity=(0.5, -0.25, 0.75))
    return [big, small]


def cylinder_item(ob, group=0, velocity=None):
    lin = velocity if velocity is not None else ob.velocity
    return dict(kind=C.OBSTACLE_CYLINDER, center=ob.center, half_size=[ob.radius, 0.5 * ob.depth, 0.0], axis=ob.axis, rotation=ob.rotation, group=group,
                velocity=list(lin) if lin is not None else [0.0] * 3, angular_velocity=list(ob.angular_velocity) if ob.angular_velocity is not None else [0.0] * 3)


def bind_items(ctx, mem, obstacles, keep):
    """ the obstacle list for the C ABI, in order: cylinders, unions with cylinders as one group, SDF entries bound to a slot (appended to `keep`), the rest as f12 """
    items, group = [], 0
    for ob in obstacles:
        if isinstance(ob, CR.Cylinder):
            items.append(cylinder_item(ob))
        elif isinstance(ob, R.Union):
            group += 1
            for m in ob.members:
                if isinstance(m, CR.Cylinder):
                    items.append(cylinder_item(m, group, ob.velocity))
                else:
                    it = obstacle_items([P.to_oracle(m)], 3)[0]
                    items.append(dict(it, group=group, velocity=list(ob.velocity) if ob.velocity is not None else [0.0] * 3))
        elif isinstance(ob, S.SdfObstacle):
            items += SC.bind_items(ctx, mem, [ob], 3, keep)
        else:
            items += obstacle_items([P.to_oracle(ob)], 3)
    return items


def check_cylinder_obstacles(ctx, mem, res, bc, dtype, batch, obstacles, kind="random", seed=0, exact=False, what="scene", unchanged=False):
    """ phihip_obstacle_accessible (equality), phihip_build_cellflags of it (equality), phihip_apply_obstacles (in place, the bound above with E, G from
    project_ref.apply_obstacles). exact: the dyadic case, no clearance asked. unchanged: the velocity must come back bit-identical. Returns (worst ratio, cells inside) """
    x = P.make_inputs(res, bc, dtype, batch, kind, seed)
    if exact:      # dx = 1, lower = 0
        x.dom, x.grid = P.make_case(tuple(res), bc, dtype, batch, bc_val=x.bcv)
        x.dx = x.dom.dx
    lower = (0.0,) * 3
    if kind == "nonfinite":      # NaN and Inf where the first obstacle's mask is exactly 1: safe_mul makes them 0, a moving obstacle then adds its velocity
        planted = 0
        for d in range(3):
            inside = np.argwhere(np.broadcast_to(obstacles[0].sdf(R.face_points(d, x.res, x.bc, lower, x.dx)) <= 0, x.v[d].shape[1:]))
            for i, bad in zip(inside[:3], (np.nan, np.inf, -np.inf)):
                x.v[d][(slice(None),) + tuple(i)] = bad
                planted += 1
        assert planted, f"{what}: no sample inside the first obstacle"
    if not exact:
        c = R.surface_clearance(obstacles, x.res, x.bc, lower, x.dx)
        assert c > CLEARANCE, f"{what}: a sample lies {c:.2e} cells from a surface"
    keep = []
    try:
        items = bind_items(ctx, mem, obstacles, keep)
        arr = C.make_obstacles(items)
        g1 = C.make_grid(3, x.grid.dtype, 1, x.res, x.dom.lower, x.dom.upper, x.bc, x.bcv)
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
        for d in range(3):
            got = mem.to_host(dv[d])
            if unchanged:
                assert acc.all() and np.array_equal(P._bits(got), P._bits(x.v[d])), f"{what}: the obstacle lies entirely outside, yet component {d} changed"
            scale = np.abs(ref[d]) + E[d]
            worst = max(worst, P.compare(f"apply_obstacles[{d}]", what, x, kind, got, ref[d], eps * E[d] + EPS64 * (P.K_REF * scale + K_CYL * G[d]),
                                         None, None if kind == "nonfinite" else r32[d]))
        return worst, int((acc == 0).sum())
    finally:
        for h, slot in keep:
            ctx.sdf_release(slot)


def check_margin(ctx, mem, res, bc, dtype, batch, seed):
    """ the `margin` scene: the reference alone shows that the sample is reached through the margin terms only, then the usual comparison """
    dx = P.make_inputs(res, bc, dtype, batch, "random", seed).dx
    assert res[-1] > 64 and R.face_offset(bc, 0) == 0
    for k in range(8):
        ob, idx, sample = margin_cylinder(res, dx, np.random.default_rng(seed + 1000 * k))
        if R.surface_clearance([ob], res, bc, (0.0,) * 3, dx) > CLEARANCE:
            break
    else:
        raise AssertionError("margin: no seed of 8 keeps the samples off the surfaces")
    m = math.sqrt(sum((0.5 * h) ** 2 for h in dx))
    pts = R.face_points(0, res, bc, (0.0,) * 3, dx)
    assert np.allclose([p.reshape(-1)[i] for p, i in zip(pts, idx)], sample, rtol=0, atol=1e-12)
    mask = np.clip(1.0 - ob.sdf(pts) / m, 0, 1)
    assert abs(mask[idx] - 0.15) < 1e-9, mask[idx]
    dz = sample[2] - ob.center[2]
    assert ob.culling_extent(0.0)[2] + 1.000001 * m < dz <= ob.culling_extent(m)[2], "the sample must lie beyond the box without margin terms and within the one with them"
    # every sample of the first 64 columns lies farther than the cell radius from the cylinder: whoever sets column 64 went through the next patch
    return check_cylinder_obstacles(ctx, mem, res, bc, dtype, batch, [ob], "random", seed, what="margin")[0]


def run_cylinder_obstacles(ctx, mem, res, bc, dtype, batch, seed=0, scenes=SCENES):
    """ every scene on one grid; a `nonfinite` input under a stationary and under a moving cylinder, a `graded` one; the margin scene where rows cross a patch; the
    dyadic scene. Prints the figures (also when a check fails). Returns the worst error / bound """
    del P.RECORDS[:]
    worst = 0.0
    try:
        dx = P.make_inputs(res, bc, dtype, batch, "random", seed).dx
        for k, name in enumerate(scenes):
            obs = pick_scene(name, res, bc, dx, seed + k)
            w, inside = check_cylinder_obstacles(ctx, mem, res, bc, dtype, batch, obs, "random", seed + k, what=name, unchanged=(name == "outside"))
            worst = max(worst, w)
            if name.startswith("along") or name in ("generic rotation", "covering"):
                assert inside > 0, f"{name}: no cell inside the cylinder"
            if name in ("along z", "linear velocity"):      # NaN under a mask of 1: 0 (stationary) or the obstacle's velocity (moving), as safe_mul gives
                worst = max(worst, check_cylinder_obstacles(ctx, mem, res, bc, dtype, batch, obs, "nonfinite", seed + k, what=name)[0])
            if name == "generic rotation":
                worst = max(worst, check_cylinder_obstacles(ctx, mem, res, bc, dtype, batch, obs, "graded", seed + k, what=name)[0])
        if res[-1] > 64:
            worst = max(worst, check_margin(ctx, mem, res, bc, dtype, batch, seed))
        worst = max(worst, check_cylinder_obstacles(ctx, mem, res, bc, dtype, batch, dyadic_obstacles(res), "random", seed, exact=True, what="dyadic")[0])
    finally:
        P.report()
    return worst
