"""
Finite, rotated and moving cylinders (Cylinder / cylinder) under the CPU emulation (tests/hipemu): the cylinder branch of the obstacle kernels
element by element through the C ABI (tests/cylinder_cases.py: the rule, the scenes, the grids), the refusals of the C ABI, the Python class against the
restatement tests/cylinder_ref.py, the mapping in fluid.py against the composed C calls, the mask cache, jit_compile, the backward pass, sample_sdf and the
example. tests/test_gpu_cylinder.py repeats the device side on the MI355X. Every case prints its figures.
"""
import ast
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import cylinder_cases as CC
import cylinder_ref as CR
import parity_cases as pc
import project_elementwise_cases as P
import project_ref as R
from phiflow_amd import _capi, autodiff
from phiflow_amd.flow import (BOUNDARY, ZERO, Box, Cylinder, Obstacle, SDFGrid, Solve, Sphere, StaggeredGrid, combine_sides, cylinder, fluid, geom, jit_compile, l2_loss,
                              sample_sdf, union, vec)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEM = pc.NumpyMem()
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


def _rx(t):
    return np.array([[1.0, 0.0, 0.0], [0.0, math.cos(t), -math.sin(t)], [0.0, math.sin(t), math.cos(t)]])


def _rz(t):
    return np.array([[math.cos(t), -math.sin(t), 0.0], [math.sin(t), math.cos(t), 0.0], [0.0, 0.0, 1.0]])


# ---- the reference stands alone; the tables cover what they claim (NumPy only) ----------------------------------------------------------------------------------
def test_reference_imports_nothing_under_test():
    tree = ast.parse(open(os.path.join(os.path.dirname(__file__), "cylinder_ref.py")).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names == {"numpy"}, names


def test_reference_is_the_embedded_disc_cut_by_a_slab():
    """ an unrotated cylinder along z = project_ref.Embedded(Sphere) intersected with |z - c_z| <= depth / 2; sdf = the maximum of the two; and by hand """
    rng = np.random.default_rng(0)
    c, Rad, depth = (1.25, -0.5, 2.0), 1.5, 3.0
    cyl = CR.Cylinder(c, Rad, depth, 2)
    disc = R.Embedded(R.Sphere(c[:2], Rad), (0, 1))
    pts = [rng.uniform(-3, 5, 4000) for _ in range(3)]
    pts[2][:3] = (c[2] + 1.5, c[2] - 1.5, c[2])                     # on the caps
    pts[0][:3], pts[1][:3] = c[0], c[1]
    slab = np.abs(pts[2] - c[2]) - 0.5 * depth
    assert np.array_equal(cyl.lies_inside(pts), disc.lies_inside(pts) & (slab <= 0)) and cyl.lies_inside(pts)[:3].all()
    assert np.array_equal(cyl.sdf(pts), np.maximum(disc.sdf(pts), slab))
    at = lambda x, y, z, ob=cyl: float(ob.sdf([np.array([x]), np.array([y]), np.array([z])])[0])
    assert at(1.25, -0.5, 2.0) == -1.5 and at(1.25 + 3.0, -0.5, 2.0) == 1.5 and at(1.25, -0.5, 6.0) == 2.5 and at(1.25 + 1.5, -0.5, 3.5) == 0.0
    # axis x, turned a quarter about z: the axis then points along y
    turned = CR.Cylinder((0, 0, 0), 1.0, 4.0, 0, rotation=_rz(math.pi / 2))
    assert abs(at(0.0, 1.9, 0.0, turned) + 0.1) < 1e-15 and abs(at(1.5, 0.0, 0.0, turned) - 0.5) < 1e-15 and np.allclose(turned.up, (0, 1, 0), atol=1e-16)
    assert cyl.bounding_half_extent() == (1.5, 1.5, 1.5) and CR.Cylinder(c, 1.0, 4.0, 2).bounding_half_extent() == (1.0, 1.0, 2.0)
    assert cyl.bounding_radius() == math.sqrt(1.5 ** 2 + 1.5 ** 2) and cyl.reach == 1.25 + 0.5 + 2.0 + 1.5 + 1.5


def test_tables_cover_the_listed_grids_and_scenes():
    assert [(g[0], g[2]) for g in CC.GRIDS] == [((12, 10, 16), 2), ((5, 6, 134), 3)]
    assert CC.GRIDS[0][1] == ((pc.CLO, pc.OPN), (pc.PER, pc.PER), (pc.CLO, pc.CLO)) and CC.GRIDS[1][1] == ((pc.OPN, pc.OPN), (pc.CLO, pc.CLO), (pc.PER, pc.PER))
    assert CC.SCENES == ("along x", "along y", "along z", "generic rotation", "thin disc", "long rod", "linear velocity", "spinning", "tumbling", "union with a box",
                         "cylinder sdf box", "outside", "covering", "16 cylinders")
    assert CC.K_CYL == 16.0 and P.K_GEO == 12.0 and CC.CLEARANCE == 1e-9 and P.DX_FACTORS == (1.0, 1.25, 0.8)


@pytest.mark.parametrize("case", CC.GRIDS, ids=CC.case_id)
def test_every_listed_scene_finds_a_seed(case):
    """ decided by the reference alone; and the scenes are what their names say """
    res, bc, batch = case
    dx = P.make_inputs(res, bc, np.float32, batch, "random", 5).dx
    L = [n * h for n, h in zip(res, dx)]
    for k, name in enumerate(CC.SCENES):
        obs = CC.pick_scene(name, res, bc, dx, 5 + k)
        assert R.surface_clearance(obs, res, bc, (0.0,) * 3, dx) > CC.CLEARANCE
        first = obs[0].members[0] if isinstance(obs[0], R.Union) else obs[0]
        assert isinstance(first, CR.Cylinder)
        if name.startswith("along"):
            assert first.axis == "xyz".index(name[-1]) and first.rotation is None
        if name == "thin disc":
            assert all(o.depth < min(dx) for o in obs)
        if name == "long rod":
            assert all(o.depth > 2 * L[o.axis] for o in obs) and obs[0].radius < 0.2 * min(L)
        if name == "spinning":
            assert np.allclose(np.cross(first.angular_velocity, first.up), 0, atol=1e-15) and first.rotation is not None
        if name == "tumbling":
            assert abs(float(np.dot(first.angular_velocity, first.up))) < 1e-15 and any(first.angular_velocity)
        if name == "union with a box":
            assert [type(m).__name__ for m in obs[0].members] == ["Cylinder", "Box"]
        if name == "cylinder sdf box":
            assert [type(o).__name__ for o in obs] == ["Cylinder", "SdfObstacle", "Box"]
        if name == "outside":
            assert R.accessible(obs, res, (0.0,) * 3, dx).all()
        if name == "covering":
            assert not R.accessible(obs, res, (0.0,) * 3, dx).any()
        if name == "16 cylinders":
            assert len(obs) == 16 and {o.axis for o in obs} == {0, 1, 2}
    # the dyadic scene: cell centres ON a cap plane and ON the mantle, faces likewise -- exactly
    unit = (1.0, 1.0, 1.0)
    big, small = CC.dyadic_obstacles(res)
    mantle, caps = big.surfaces(R.cell_points(res, (0.0,) * 3, unit))
    assert ((mantle == 0) & (caps <= 0)).any() and ((caps == 0) & (mantle <= 0)).any()
    mantle, caps = small.surfaces(R.face_points(0, res, bc, (0.0,) * 3, unit))
    assert ((mantle == 0) & (caps <= 0)).any()
    mantle, caps = small.surfaces(R.face_points(2, res, bc, (0.0,) * 3, unit))
    assert ((caps == 0) & (mantle <= 0)).any()


def test_culling_box_is_conservative():
    """ the bound the kernels cull with (cylinder_extent in project.hip, cylinder_ref.culling_extent): on 200 random cylinders on a (9, 8, 7) grid, cell centres and
    all three face lattices, margin = half a cell diagonal, no sample with sdf <= margin lies outside the box -- and without the margin terms some do """
    res, bc, dx = (9, 8, 7), ((pc.OPN, pc.OPN), (pc.CLO, pc.CLO), (pc.PER, pc.PER)), (0.37, 0.4625, 0.296)
    margin = math.sqrt(sum((0.5 * h) ** 2 for h in dx))
    L = [n * h for n, h in zip(res, dx)]
    rng = np.random.default_rng(16)
    lattices = [R.cell_points(res, (0.0,) * 3, dx)] + [R.face_points(d, res, bc, (0.0,) * 3, dx) for d in range(3)]
    missed_without = 0
    for k in range(200):
        c = CR.Cylinder([rng.uniform(-0.2, 1.2) * l for l in L], rng.uniform(0.05, 0.6) * min(L), rng.uniform(0.02, 1.5) * max(L), k % 3,
                        rotation=None if k % 4 == 0 else P._rot(3, rng))
        ext, bare = c.culling_extent(margin), c.culling_extent(0.0) + margin
        for pts in lattices:
            near = c.sdf(pts) <= margin
            off = [np.abs(p - cc) + np.zeros(near.shape) for p, cc in zip(pts, c.center)]
            assert all((o[near] <= e * (1 + 1e-12)).all() for o, e in zip(off, ext)), f"cylinder {k}: a sample within the margin lies outside the culling box"
            missed_without += sum(int((o[near] > e).sum()) for o, e in zip(off, bare))
    assert missed_without > 0


# ---- the kernels, element by element -----------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("case", CC.GRIDS, ids=CC.case_id)
def test_cylinder_kernels(emu_ctx, case, dtype):
    worst = CC.run_cylinder_obstacles(emu_ctx, MEM, case[0], case[1], dtype, case[2], seed=5)
    print(f"cylinder worst error / bound {worst:.3g} ({CC.case_id(case)}, {np.dtype(dtype).name})")
    assert worst <= 1.0


def test_c_abi_refusals(emu_ctx):
    check_c_abi_refusals(emu_ctx, MEM)


def check_c_abi_refusals(ctx, mem):
    """ every refusal is decided on the host before anything is launched: PHIHIP_ERR_UNSUPPORTED (-3) and a message; the accepted calls run on buffers of `mem` """
    g3 = _capi.make_grid(3, _capi.PHIHIP_F32, 1, (5, 7, 3), (0, 0, 0), (5, 7, 3), ((1, 1),) * 3)
    g2 = _capi.make_grid(2, _capi.PHIHIP_F32, 1, (5, 7), (0, 0), (5, 7), ((1, 1), (1, 1)))
    acc = mem.to_dev(np.zeros((5, 7, 3), np.uint8))
    v = [mem.to_dev(np.zeros((5, 7, 3), np.float32)) for _ in range(3)]
    out = mem.to_dev(np.zeros((4, 4, 4), np.float32))
    desc3 = _capi.make_sdf_grid(0, _capi.PHIHIP_F32, (4, 4, 4), (0, 0, 0), (4, 4, 4), (2, 2, 2), 0.0, False)
    desc2 = _capi.make_sdf_grid(0, _capi.PHIHIP_F32, (4, 4), (0, 0), (4, 4), (2, 2), 0.0, False)
    ok = dict(kind=_capi.OBSTACLE_CYLINDER, center=[2.5, 3.5, 1.5], half_size=[1.5, 1.0, 0.0], axis=1, velocity=[0.5, 0, 0], angular_velocity=[0, 0.1, 0])

    def refused(item, word, grid=g3, desc=desc3):
        arr = _capi.make_obstacles([item])
        for call in (lambda: ctx.obstacle_accessible(grid, arr, 1, mem.ptr(acc)), lambda: ctx.apply_obstacles(grid, arr, 1, [mem.ptr(a) for a in v]),
                     lambda: ctx.sdf_from_analytic(desc, arr, 1, mem.ptr(out))):
            with pytest.raises(_capi.PhiHipError) as e:
                call()
            assert e.value.status == -3 and word in str(e.value), str(e.value)
    arr = _capi.make_obstacles([ok])
    ctx.obstacle_accessible(g3, arr, 1, mem.ptr(acc))
    ctx.apply_obstacles(g3, arr, 1, [mem.ptr(a) for a in v])
    ctx.sdf_from_analytic(desc3, arr, 1, mem.ptr(out))
    mem.sync()
    assert (mem.to_host(acc) == 0).sum() > 0
    refused(ok, "rank 3", grid=g2, desc=desc2)
    refused(dict(ok, embed_mask=1), "embedded")
    refused(dict(ok, axis=3), "axis")
    refused(dict(ok, axis=-1), "axis")
    refused(dict(ok, half_size=[-1.0, 1.0, 0.0]), "negative")
    refused(dict(ok, half_size=[1.0, -0.5, 0.0]), "negative")
    with pytest.raises(_capi.PhiHipError, match="unknown kind"):
        ctx.obstacle_accessible(g3, _capi.make_obstacles([dict(ok, kind=4)]), 1, mem.ptr(acc))
    assert ctypes.sizeof(_capi.ObstacleStruct) == 184 and ctx.lib.version() == 102 and _capi.OBSTACLE_CYLINDER == 3


# ---- the Python class --------------------------------------------------------------------------------------------------------------------------------------------
def _cloud(rng, n=600):
    pts = [rng.uniform(-4, 6, n) for _ in range(3)]
    return pts


def _same_samples(made, want, rng):
    """ host queries of `made` (phiflow_amd Cylinder) against the restatement `want`: the same float64 steps, at most K_CYL eps64 of the coordinates' magnitude """
    pts = _cloud(rng)
    d = np.abs(made.approximate_signed_distance(pts) - want.sdf(pts))
    X = sum(np.abs(p) for p in pts) + want.reach
    assert (d <= CC.K_CYL * P.EPS64 * X).all(), float((d / X).max())
    safe = np.minimum(*[np.abs(s) for s in want.surfaces(pts)]) > 1e-9
    assert np.array_equal(made.lies_inside(pts)[safe], want.lies_inside(pts)[safe]) and want.lies_inside(pts).any()


def test_constructor_forms():
    rng = np.random.default_rng(1)
    M = P._rot(3, rng)
    want = CR.Cylinder((1.0, 2.0, 3.0), 1.5, 4.0, 2, rotation=M)
    forms = [cylinder(x=1.0, y=2.0, z=3.0, radius=1.5, depth=4.0, rotation=M), cylinder(vec(x=1.0, y=2.0, z=3.0), 1.5, 4.0, M),
             cylinder(vec(x=1.0, y=2.0, z=3.0), radius=1.5, depth=4.0, rotation=M, axis=2), cylinder(x=1.0, y=2.0, z=3.0, radius=1.5, depth=4.0, rotation=M, axis='z'),
             Cylinder(dict(x=1.0, y=2.0, z=3.0), 1.5, 4.0, 'z', M)]
    assert len({repr(f) for f in forms}) == 1 and forms[0].axis == 'z' and forms[0].dims == ('x', 'y', 'z')
    _same_samples(forms[0], want, rng)
    for axis in (0, 'x', -3):
        c = cylinder(x=1.0, y=2.0, z=3.0, radius=1.5, depth=4.0, axis=axis)
        assert c.axis == 'x' and c.rot is None and c.radial_axes == ('y', 'z')
        _same_samples(c, CR.Cylinder((1.0, 2.0, 3.0), 1.5, 4.0, 0), rng)
    # the axis as a direction: stored along the last dim, depth 2 |axis|, a rotation that takes e_z to the direction (Rodrigues; the antiparallel pole too)
    for direction in ((1.0, 2.0, -0.5), (0.0, 0.0, 3.0), (0.0, 0.0, -2.0), (1e-9, 0.0, -1.0), (2.0, 0.0, 0.0)):
        c = cylinder(vec(x=1.0, y=2.0, z=3.0), radius=0.7, axis=vec(x=direction[0], y=direction[1], z=direction[2]))
        norm = math.sqrt(sum(x * x for x in direction))
        assert c.axis == 'z' and c.depth == 2 * norm and c.rot.shape == (3, 3)
        assert np.allclose(c.rot @ c.rot.T, np.eye(3), rtol=0, atol=4 * P.EPS64) and abs(np.linalg.det(c.rot) - 1) < 8 * P.EPS64
        assert np.allclose(c.up, np.asarray(direction) / norm, rtol=0, atol=4 * P.EPS64)
        # any explicit matrix with the same third column describes the same body: its samples agree up to the bound
        u = np.asarray(direction) / norm
        a = np.cross(u, (0.3, -0.8, 0.52))
        a /= np.linalg.norm(a)
        explicit = CR.Cylinder((1.0, 2.0, 3.0), 0.7, 2 * norm, 2, rotation=np.stack([a, np.cross(u, a), u], axis=1))
        _same_samples(c, explicit, rng)
    c0 = cylinder(0, radius=1.0, axis=vec(x=0.0, y=2.0, z=0.0))
    assert c0.center == (0.0, 0.0, 0.0) and c0.depth == 4.0 and cylinder(0, radius=1.0, depth=1.0, axis=vec(x=0.0, y=2.0, z=0.0)).depth == 1.0
    with pytest.raises(AssertionError, match="rotation must be None"):
        cylinder(vec(x=0, y=0, z=0), radius=1.0, rotation=M, axis=vec(x=0.0, y=2.0, z=0.0))
    assert "PHIML-RECALL" in cylinder.__doc__


def test_class_methods_follow_the_reference_text():
    rng = np.random.default_rng(2)
    M, Q = P._rot(3, rng), P._rot(3, rng)
    c = cylinder(x=1.0, y=-2.0, z=0.5, radius=1.0, depth=4.0, axis='z')
    assert c.volume == math.pi * 4.0 and c.bounding_radius() == math.sqrt(1.0 + 4.0) and c.bounding_half_extent() == (1.0, 1.0, 2.0)
    # turned 90 degrees about x: up = (0, -1, 0) up to rounding; the reference formula with its 1e-5 under the root
    t = c.rotated(_rx(math.pi / 2))
    up = _rx(math.pi / 2) @ np.array([0.0, 0.0, 1.0])
    want = np.abs(up) * 2.0 + 1.0 * np.sqrt(np.maximum(1e-5, 1 - up ** 2))
    assert np.allclose(t.bounding_half_extent(), want, rtol=0, atol=1e-15) and abs(t.bounding_half_extent()[1] - (2.0 + math.sqrt(1e-5))) < 1e-15
    assert abs(t.bounding_half_extent()[0] - 1.0) < 1e-15 and abs(t.bounding_half_extent()[2] - 1.0) < 1e-15
    assert np.allclose(geom._bounding_box(t).half_size, want, rtol=0, atol=1e-15) and geom._bounding_box(t).center == (1.0, -2.0, 0.5)
    # rotated composes as M @ Q
    r = c.rotated(M).rotated(Q)
    assert np.array_equal(r.rot, M @ Q) and np.array_equal(c.rotated(M).rot, M) and r.rotation is r.rot
    _same_samples(r, CR.Cylinder((1.0, -2.0, 0.5), 1.0, 4.0, 2, rotation=M @ Q), rng)
    s = r.scaled(1.5)
    assert (s.radius, s.depth) == (1.5, 6.0) and np.array_equal(s.rot, r.rot) and s.center == r.center
    assert r.at((0.0, 1.0, 2.0)).center == (0.0, 1.0, 2.0) and r.at(vec(x=9.0)).center == (9.0, -2.0, 0.5)
    assert r.shifted((1.0, 1.0, 1.0)).center == (2.0, -1.0, 1.5) and r.shifted(vec(z=1.0)).center == (1.0, -2.0, 1.5)
    assert r.with_radius(0.25).radius == 0.25 and r.with_radius(0.25).depth == 4.0 and r.with_depth(0.5).depth == 0.5 and r.entry(3) is r
    assert np.allclose(r.up, (M @ Q)[:, 2], rtol=0, atol=1e-16)
    ob = Obstacle(c, angular_velocity=(0, 0, 0.5)).rotated(M)
    assert np.array_equal(ob.geometry.rot, M) and ob.angular_velocity == (0.0, 0.0, 0.5)
    # repr: every parameter with 17 significant digits
    M2 = M.copy()
    M2[1, 2] = np.nextafter(M2[1, 2], 2.0)
    variants = [c, c.rotated(M), c.rotated(M2), c.with_radius(np.nextafter(1.0, 2.0)), c.with_depth(np.nextafter(4.0, 5.0)), c.shifted((0, 0, 1e-16)),
                cylinder(x=1.0, y=-2.0, z=0.5, radius=1.0, depth=4.0, axis='y'), c.rotated(np.eye(3))]
    assert len({repr(v) for v in variants}) == len(variants) and repr(c) == repr(cylinder(x=1.0, y=-2.0, z=0.5, radius=1.0, depth=4.0, axis='z'))


def test_batched_cylinders():
    b = cylinder(x=[1.0, 2.0, 3.0], y=2.0, z=1.0, radius=[0.5, 0.75, 1.0], depth=2.0, axis='x')
    assert isinstance(b, geom.Batched) and b.batch_size == 3 and [g.radius for g in b.geometries] == [0.5, 0.75, 1.0] and [g.center[0] for g in b.geometries] == [1.0, 2.0, 3.0]
    assert all(isinstance(g, Cylinder) and g.axis == 'x' and g.depth == 2.0 for g in b.geometries)
    d = cylinder(x=1.0, y=2.0, z=1.0, radius=0.5, depth=[1.0, 2.0], axis='x')
    assert d.batch_size == 2 and d.entry(1).depth == 2.0
    pts = [np.array([1.0]), np.array([2.0]), np.array([1.0])]
    assert b.lies_inside(pts).shape == (3, 1) and b.shifted((1, 0, 0)).entry(0).center[0] == 2.0


def test_python_refusals(emu_backend):
    with pytest.raises(NotImplementedError, match="use a Box"):
        cylinder(x=1.0, y=2.0, radius=1.0, depth=1.0, axis='y')
    c = cylinder(x=1.0, y=2.0, z=3.0, radius=1.0, depth=1.0)
    with pytest.raises(NotImplementedError, match="infinite_cylinder"):
        geom.embed(c, 'w')
    assert geom.embed(c, 'z') is c                                    # (no dim to add)
    for bad in (0.3, np.eye(2), (0.1, 0.2, 0.3)):
        with pytest.raises(NotImplementedError, match=r"\(3, 3\) rotation matrix"):
            c.rotated(bad)
        with pytest.raises(NotImplementedError, match=r"\(3, 3\) rotation matrix"):
            cylinder(x=1.0, y=2.0, z=3.0, radius=1.0, depth=1.0, rotation=bad)
    v = _velocity(emu_backend, (6, 5, 4), np.random.default_rng(0))[0]
    with pytest.raises(NotImplementedError, match="union obstacle cannot have an angular velocity"):
        fluid.apply_boundary_conditions(v, Obstacle(union(c, Sphere(x=1, y=1, z=1, radius=1)), angular_velocity=(0, 0, 1)))


# ---- through fluid.py: the mapping against the composed C calls -------------------------------------------------------------------------------------------------
RES = (12, 10, 16)
EXT = dict(x=ZERO, y=BOUNDARY, z=ZERO)
BC = ((pc.CLO, pc.CLO), (pc.OPN, pc.OPN), (pc.CLO, pc.CLO))


def _velocity(backend, res, rng, dtype=np.float32, batch=None, dims='xyz', scale=0.3):
    """ a random staggered velocity on Box(0 .. res) with cells of size 1; walls in x and z, open in y (the projection has a solution for any obstacle motion) """
    kw = dict(zip(dims, res))
    bounds = Box(**{d: float(n) for d, n in kw.items()})
    ext = combine_sides(**{d: EXT[d] for d in dims})
    shapes = StaggeredGrid(0, ext, bounds, backend=backend, **kw).component_shapes
    vals = [(scale * rng.standard_normal(((batch,) if batch else ()) + tuple(s))).astype(dtype) for s in shapes]
    return StaggeredGrid(vals, ext, bounds, backend=backend, **kw), vals


M0 = P._rot(3, np.random.default_rng(33))
ROD = dict(center=(5.3, 4.6, 8.2), radius=2.1, depth=7.0, axis=0, rotation=M0, velocity=(0.3, -0.2, 0.1), angular_velocity=(0.2, 0.5, -0.4))


def _rod(**kw):
    a = dict(ROD, **kw)
    geo = cylinder(x=a['center'][0], y=a['center'][1], z=a['center'][2], radius=a['radius'], depth=a['depth'], rotation=a['rotation'], axis=a['axis'])
    return Obstacle(geo, a['velocity'], a['angular_velocity'])


def _rod_items(**kw):
    a = dict(ROD, **kw)
    return [dict(kind=_capi.OBSTACLE_CYLINDER, center=a['center'], half_size=[a['radius'], 0.5 * a['depth'], 0.0], axis=a['axis'], rotation=a['rotation'],
                 velocity=a['velocity'], angular_velocity=a['angular_velocity'])]


def _composed(backend, v, items, solve=None):
    """ apply, accessible, flags[, phihip_make_incompressible] through the context, on copies of v's tensors """
    ctx, grid = backend.ctx, v.grid_struct()
    arr = _capi.make_obstacles(items)
    vals = [t.clone().contiguous() for t in v.values]
    ctx.apply_obstacles(grid, arr, len(items), [t.data_ptr() for t in vals], backend.stream())
    res = tuple(v.resolution.values())
    acc, flags = backend.empty(res, torch.uint8), backend.empty(res, torch.uint8)
    g1 = v.grid_struct(batch=1)
    ctx.obstacle_accessible(g1, arr, len(items), acc.data_ptr(), backend.stream())
    ctx.build_cellflags(g1, acc.data_ptr(), 0, 1, flags.data_ptr(), backend.stream())
    p = None
    if solve is not None:
        fp64 = v.dtype == torch.float64
        p = backend.zeros((v.batch_size,) + res, v.dtype)
        ctx.make_incompressible(grid, [t.data_ptr() for t in vals], None, flags.data_ptr(), 1, 0, p.data_ptr(), 0, solve.with_defaults(fp64).to_c(fp64), True, backend.stream())
    return vals, flags, p


@DTYPES
def test_fluid_calls_equal_the_composed_c_calls(emu_backend, dtype):
    """ fluid.apply_boundary_conditions and fluid.make_incompressible with a rotated, moving, tumbling cylinder: the bits of the composed C calls on the same
    inputs; and the flags equal the reference's """
    v, _ = _velocity(emu_backend, RES, np.random.default_rng(3), dtype)
    ob, items = _rod(), _rod_items()
    solve = Solve('CG', 1e-5, 0)
    applied, flags, _ = _composed(emu_backend, v, items)
    got = fluid.apply_boundary_conditions(v, ob)
    assert all(torch.equal(a, b) for a, b in zip(got.values, applied)) and not all(torch.equal(a, b) for a, b in zip(got.values, v.values))
    want_v, flags, want_p = _composed(emu_backend, v, items, solve)
    v1, p1 = fluid.make_incompressible(v, [ob], solve)
    assert all(torch.equal(a, b) for a, b in zip(v1.values, want_v)) and torch.equal(p1.values, want_p) and float(p1.values.abs().max()) > 0
    assert torch.equal(fluid._MASKS.get(v, [ob], None), flags)
    ref = CR.Cylinder(ROD['center'], ROD['radius'], ROD['depth'], ROD['axis'], rotation=M0)
    acc = R.accessible([ref], RES, (0.0,) * 3, (1.0,) * 3)
    assert R.surface_clearance([ref], RES, BC, (0.0,) * 3, (1.0,) * 3) > CC.CLEARANCE and 20 < (acc == 0).sum() < acc.size
    assert np.array_equal(flags.cpu().numpy(), R.cell_flags(acc, None, RES, BC, False))
    print(f"projection around a tumbling cylinder {np.dtype(dtype).name}: {int((acc == 0).sum())} cells inside, {p1.solve_info.iterations} iterations")


def test_dimension_order_of_the_geometry_does_not_matter(emu_backend):
    """ a cylinder built with dims (z, x, y), its matrix permuted accordingly, gives the obstacle of the (x, y, z) one: identical bits, identical flags; the axis
    name, not its position in the geometry, selects the grid axis """
    v, _ = _velocity(emu_backend, RES, np.random.default_rng(4))
    for axis in 'xyz':
        for rot in (None, M0):
            c, Rad, depth = ROD['center'], ROD['radius'], ROD['depth']
            a = cylinder(x=c[0], y=c[1], z=c[2], radius=Rad, depth=depth, axis=axis, rotation=rot)
            perm = [2, 0, 1]
            b = cylinder(z=c[2], x=c[0], y=c[1], radius=Rad, depth=depth, axis=axis, rotation=None if rot is None else rot[np.ix_(perm, perm)])
            assert b.dims == ('z', 'x', 'y') and repr(a) != repr(b)
            oa, ob = Obstacle(a, ROD['velocity'], ROD['angular_velocity']), Obstacle(b, vec(x=0.3, y=-0.2, z=0.1), vec(x=0.2, y=0.5, z=-0.4))
            va, vb = fluid.apply_boundary_conditions(v, oa), fluid.apply_boundary_conditions(v, ob)
            assert all(torch.equal(s, t) for s, t in zip(va.values, vb.values))
            assert torch.equal(fluid._MASKS.get(v, [oa], None), fluid._MASKS.get(v, [ob], None))
            want, flags, _ = _composed(emu_backend, v, _rod_items(axis='xyz'.index(axis), rotation=rot))
            assert all(torch.equal(s, t) for s, t in zip(va.values, want)) and torch.equal(fluid._MASKS.get(v, [oa], None), flags)
    # and on a velocity whose dimensions are (z, y, x) the same body is the transposed obstacle
    vt, _ = _velocity(emu_backend, RES[::-1], np.random.default_rng(4), dims='zyx')
    a = cylinder(x=5.3, y=4.6, z=8.2, radius=2.1, depth=7.0, axis='x')
    flags_t = fluid._MASKS.get(vt, [Obstacle(a)], None).cpu().numpy()
    acc = R.accessible([CR.Cylinder((8.2, 4.6, 5.3), 2.1, 7.0, 2)], RES[::-1], (0.0,) * 3, (1.0,) * 3)
    assert np.array_equal((flags_t >> 6) & 1, acc)


def test_union_member_and_batched_radii(emu_backend):
    rng = np.random.default_rng(6)
    v, arrays = _velocity(emu_backend, RES, rng, batch=3)
    c = ROD['center']
    radii = [1.2, 2.1, 3.0]
    batched = cylinder(x=c[0], y=c[1], z=c[2], radius=radii, depth=7.0, axis='x', rotation=M0)
    out = fluid.apply_boundary_conditions(v, Obstacle(batched, ROD['velocity'], ROD['angular_velocity']))
    flags = fluid._MASKS.get(v, [Obstacle(batched)], None).cpu().numpy()
    for b, Rad in enumerate(radii):
        vb = v.with_values([t[b:b + 1].contiguous() for t in v.values])
        vb = StaggeredGrid([a[b] for a in arrays], combine_sides(**EXT), Box(x=12.0, y=10.0, z=16.0), backend=emu_backend, x=12, y=10, z=16)
        want, fl, _ = _composed(emu_backend, vb, _rod_items(radius=Rad))
        assert all(torch.equal(o[b:b + 1], w) for o, w in zip(out.values, want)) and np.array_equal(flags[b], fl.cpu().numpy())
    assert not np.array_equal(flags[0], flags[2])
    # a union of a cylinder and a box: one group, one linear velocity
    v1, _ = _velocity(emu_backend, RES, rng)
    box = Box(x=(6.0, 9.5), y=(2.5, 7.0), z=(3.0, 6.5))
    body = Obstacle(union(cylinder(x=c[0], y=c[1], z=c[2], radius=2.1, depth=7.0, axis='x', rotation=M0), box), velocity=(0.3, -0.2, 0.1))
    items = _rod_items(angular_velocity=(0, 0, 0)) + [dict(kind=_capi.OBSTACLE_BOX, center=[7.75, 4.75, 4.75], half_size=[1.75, 2.25, 1.75], velocity=(0.3, -0.2, 0.1))]
    items = [dict(it, group=1) for it in items]
    want, fl, _ = _composed(emu_backend, v1, items)
    got = fluid.apply_boundary_conditions(v1, body)
    assert all(torch.equal(a, b) for a, b in zip(got.values, want)) and torch.equal(fluid._MASKS.get(v1, [body], None), fl)


def test_mask_cache_tells_close_cylinders_apart(emu_backend):
    """ the packed flags are cached on repr(geometry): two cylinders that differ in the 15th digit of the rotation (or of the radius) get flags of their own """
    v, _ = _velocity(emu_backend, RES, np.random.default_rng(7))
    a = _rod()
    M1 = M0.copy()
    M1[0, 0] *= 1 + 4e-15
    assert M1[0, 0] != M0[0, 0] and f"{M1[0, 0]:.14g}" == f"{M0[0, 0]:.14g}"
    b, c = _rod(rotation=M1), _rod(radius=2.1 * (1 + 4e-15))
    fa = fluid._MASKS.get(v, [a], None)
    assert fluid._MASKS.get(v, [_rod()], None) is fa                                    # a hit
    fb, fc = fluid._MASKS.get(v, [b], None), fluid._MASKS.get(v, [c], None)
    assert fb is not fa and fc is not fa and fc is not fb
    # re-posed as Rotating_Bar does: a new key, and the flags of the new pose
    turned = a.rotated(_rz(0.4))
    ft = fluid._MASKS.get(v, [turned], None)
    ref = CR.Cylinder(ROD['center'], ROD['radius'], ROD['depth'], 0, rotation=M0 @ _rz(0.4))
    assert ft is not fa and np.array_equal(ft.cpu().numpy(), R.cell_flags(R.accessible([ref], RES, (0.0,) * 3, (1.0,) * 3), None, RES, BC, False))
    assert not torch.equal(ft, fa)


def test_static_cylinder_under_jit_compile_replays_the_eager_bits(emu_backend):
    from phiflow_amd.flow import NotConverged, advect
    v0, _ = _velocity(emu_backend, RES, np.random.default_rng(8), scale=0.05)
    rod = _rod(velocity=(0, 0, 0), angular_velocity=(0, 0, 0))

    def step(v, p, dt):
        v = advect.semi_lagrangian(v, v, dt)
        return fluid.make_incompressible(v, [rod], Solve('CG', 1e-5, x0=p, max_iterations=8, suppress=[NotConverged]))
    jstep = jit_compile(step)
    eager, traced = (v0, None), (v0, None)
    for _ in range(3):
        eager, traced = step(*eager, 0.1), jstep(*traced, 0.1)
        assert all(torch.equal(a, b) for a, b in zip(eager[0].values, traced[0].values)) and torch.equal(eager[1].values, traced[1].values)
    assert float(eager[1].values.abs().max()) > 0


def test_gradient_through_the_projection_equals_the_one_with_explicit_flags(emu_backend):
    """ d l2_loss / d v through make_incompressible(v, [cylinder]) against the same autograd nodes fed with the obstacle array and the flags built by hand """
    v, _ = _velocity(emu_backend, RES, np.random.default_rng(9), np.float64)
    rod, items = _rod(), _rod_items()
    solve = Solve('CG', 1e-5, 0)
    leaves = [t.detach().clone().requires_grad_(True) for t in v.values]
    v1, p1 = fluid.make_incompressible(v.with_values(leaves), [rod], solve)
    (l2_loss(v1) + 0.01 * l2_loss(p1)).backward()
    grads = [t.grad.clone() for t in leaves]
    # by hand: ApplyObstacles and MakeIncompressible with explicit obstacle arrays and flags
    _, flags, _ = _composed(emu_backend, v, items)
    still = [dict(it, velocity=(0, 0, 0), angular_velocity=(0, 0, 0)) for it in items]
    leaves2 = [t.detach().clone().requires_grad_(True) for t in v.values]
    shapes = [tuple(t.shape) for t in leaves2]
    meta_a = dict(be=emu_backend, grid=v.grid_struct(), obstacles=_capi.make_obstacles(items), obstacles_still=_capi.make_obstacles(still), count=1, shapes=shapes, dtype=v.dtype)
    vin = list(autodiff.ApplyObstacles.apply(meta_a, *leaves2))
    cs = solve.with_defaults(True).to_c(True)
    meta = dict(be=emu_backend, grid=v.grid_struct(), flags_ptr=flags.data_ptr(), flags=flags, balance=0, csolve=cs, csolve_bwd=cs, shapes=shapes, dtype=v.dtype)
    *new_v, p2 = autodiff.MakeIncompressible.apply(meta, emu_backend.zeros((1,) + RES, v.dtype), *vin)
    loss2 = sum((t ** 2).sum() for t in new_v) * 0.5 + 0.01 * 0.5 * (p2 ** 2).sum()
    loss2.backward()
    assert all(torch.equal(a, b.grad) for a, b in zip(grads, leaves2)) and max(float(g.abs().max()) for g in grads) > 0


# ---- sample_sdf -----------------------------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_sample_sdf_of_a_cylinder(emu_backend, dtype):
    """ phihip_sdf_from_analytic at the SDF grid's cell centres against the reference sdf: the float64 value rounded once to the array's type plus K_CYL eps64 of the
    coordinates' magnitude; center, volume and bounding_radius come from the geometry; a cylinder inside a union is accepted """
    ref = CR.Cylinder((1.0, 2.0, 3.0), 1.5, 4.0, 1, rotation=M0)
    c = cylinder(x=1.0, y=2.0, z=3.0, radius=1.5, depth=4.0, axis='y', rotation=M0)
    g = sample_sdf(c, dtype=dtype, backend=emu_backend, x=9, y=8, z=7)
    assert isinstance(g, SDFGrid) and g.values.dtype == dtype and g.values.shape == (9, 8, 7) and not g.approximate_outside
    assert g.center == (1.0, 2.0, 3.0) and g.volume == c.volume and g.bounding_radius() == c.bounding_radius()
    assert np.allclose(g.bounds.half_size, [1.2 * h for h in ref.bounding_half_extent()], rtol=0, atol=1e-14) and np.allclose(g.bounds.center, c.center, rtol=0, atol=1e-14)

    def check(grid, want_of):
        pts = [(l + (np.arange(n) + 0.5) * (u - l) / n).reshape([-1 if k == a else 1 for k in range(3)])
               for a, (l, u, n) in enumerate(zip(grid.bounds.lower, grid.bounds.upper, grid.values.shape))]
        want = want_of(pts)
        X = sum(np.abs(p) for p in pts) + 20.0
        bound = CC.K_CYL * P.EPS64 * X + (0.5 * P.eps_of(np.float32) * np.abs(want) if dtype == np.float32 else 0.0)
        err = np.abs(grid.values.astype(np.float64) - want)
        print(f"sample_sdf cylinder {grid.values.shape} {np.dtype(dtype).name}: worst error / bound {float((err / bound).max()):.3g}, {int((want < 0).sum())} values inside")
        assert (err <= bound).all() and (want < 0).any()
    check(g, ref.sdf)
    # other dim order of the geometry than of the bounds; a union of a cylinder, a box and a sphere
    bounds = Box(x=(-2.0, 5.0), y=(-1.0, 6.0), z=(0.0, 6.5))
    perm = [1, 2, 0]
    c2 = cylinder(y=2.0, z=3.0, x=1.0, radius=1.5, depth=4.0, axis='y', rotation=M0[np.ix_(perm, perm)])
    check(sample_sdf(c2, bounds, dtype=dtype, backend=emu_backend, x=6, y=5, z=4), ref.sdf)
    box, ball = R.Box((2.0, 1.0, 1.0), (4.0, 3.0, 5.0)), R.Sphere((0.0, 4.0, 2.0), 1.25)
    u = sample_sdf(union(c, Box(x=(2.0, 4.0), y=(1.0, 3.0), z=(1.0, 5.0)), Sphere(x=0.0, y=4.0, z=2.0, radius=1.25)), bounds, dtype=dtype, backend=emu_backend, x=7, y=6, z=5)
    check(u, lambda pts: np.minimum(np.minimum(ref.sdf(pts), box.sdf(pts)), ball.sdf(pts)))


# ---- the example and the timing tool --------------------------------------------------------------------------------------------------------------------------------
def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_runs(emu_backend):
    """ examples/stirred_tank.py --size 12 --steps 10 on the emulation backend: the rod is re-posed every step, the flow stays divergence-free on fluid cells """
    mod = _load(("examples", "stirred_tank.py"), "stirred_tank_example")
    lines = []
    v, p, obstacle, worst = mod.run(12, 10, backend=emu_backend, log=lines.append)
    assert len(lines) == 1 and "kinetic energy" in lines[0] and "max |div|" in lines[0] and worst <= 5e-5            # the max_div of the existing projection checks
    assert isinstance(obstacle.geometry, Cylinder) and obstacle.geometry.axis == 'x' and obstacle.is_rotating
    want = np.linalg.matrix_power(mod.rz(mod.OMEGA * mod.time_step(12)), 10)
    assert np.allclose(obstacle.geometry.rot, want, rtol=0, atol=1e-13)
    assert max(float(np.abs(a).max()) for a in v.numpy()) > 0.01             # the rod stirs
