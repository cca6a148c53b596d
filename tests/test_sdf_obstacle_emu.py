"""
Obstacles from a signed-distance grid (SDFGrid) under the CPU emulation (tests/hipemu): the kernels of phiflow_amd/csrc/obstacle_sdf.hpp element by
element through the C ABI (tests/sdf_obstacle_cases.py: the rule, the scenes, the grids), the refusals of the C ABI, the Python class against the restatement
tests/sdf_obstacle_ref.py, sample_sdf, the projection, batched grids, the backward pass and the example. tests/test_gpu_sdf_obstacle.py repeats the device side
on the MI355X. Every case prints its figures.
"""
import ast
import importlib.util
import itertools
import os

import numpy as np
import pytest

import parity_cases as pc
import project_elementwise_cases as P
import project_ref as R
import sdf_obstacle_cases as SC
import sdf_obstacle_ref as S
from phiflow_amd import _capi
from phiflow_amd.flow import (BOUNDARY, ZERO, Box, CenteredGrid, Obstacle, SDFGrid, Solve, Sphere, StaggeredGrid, advect, combine_sides, divergence, field, fluid, geom, resample,
                              sample_sdf, union, vec)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEM = pc.NumpyMem()
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


# ---- the reference stands alone; the tables cover what they claim (NumPy only) ----------------------------------------------------------------------------------
def test_reference_imports_nothing_under_test():
    tree = ast.parse(open(os.path.join(os.path.dirname(__file__), "sdf_obstacle_ref.py")).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names == {"numpy"}, names


def test_tables_cover_the_listed_grids_and_options():
    assert [g[0] for g in SC.GRIDS] == [(5, 7), (9, 70), (24, 20), (5, 6, 134), (12, 10, 16)] and {g[2] for g in SC.GRIDS} == {1, 3}
    assert {g[1] for g in SC.GRIDS[1:]} == {g[1] for g in P.OBSTACLE_GRIDS}          # f12's boundary mixes
    for D, table in SC.SDF_RES.items():
        assert all(len(r) == D for r in table)
        assert any(1 in r for r in table) and any(2 in r for r in table)               # every clamp
    assert (3, 4) in SC.SDF_RES[2] and (40, 33) in SC.SDF_RES[2]
    n = len(SC.SCENES) * len(SC.SDF_RES[2])
    seen = {tuple(o[k] for k in SC.OPTIONS) for o in SC.option_table(n)}
    assert seen == set(itertools.product((True, False), repeat=4))                     # approximate_outside x SDF dtype x moving x explicit center / radius
    assert SC.SCENES == ("star", "two blobs", "mixed", "partly outside", "outside", "covering")


@pytest.mark.parametrize("case", SC.GRIDS, ids=SC.case_id)
def test_every_listed_scene_finds_a_seed(case):
    """ decided by the reference alone: clearance of every sample from the zero level of the sampled distance and, with approximate_outside, from the bounds faces;
    the scenes stay within the bound's premise (Lipschitz constant <= 1, asserted by `reach`), the mixed list keeps its kinds in order """
    res, bc, batch = case
    dx = P.make_inputs(res, bc, np.float32, batch, "random", 5).dx
    for seed in (5,):
        table = SC.option_table(len(SC.SCENES) * len(SC.SDF_RES[len(res)]))
        for k, (name, sres) in enumerate(itertools.product(SC.SCENES, SC.SDF_RES[len(res)])):
            opts = table[(k + seed) % len(table)]
            obs = SC.pick_scene(name, res, bc, dx, seed + k, sres, opts, np.float64 if opts["sdf64"] else np.float32)
            assert R.surface_clearance(obs, res, bc, (0.0,) * len(res), dx) > SC.CLEARANCE
            for ob in obs:
                assert ob.reach > 0
            if name == "mixed":
                assert [type(o).__name__ for o in obs] == ["Box", "SdfObstacle", "Sphere", "SdfObstacle", "Box"]
                assert obs[2].velocity is not None and obs[3].velocity is not None and obs[1].velocity is None
            if name == "outside":
                assert all(l > n * h for l, n, h in zip(obs[0].lower, res, dx))


def test_restatement_of_the_sample_by_hand():
    """ multilinear, taps clamped: hand values on a 2 x 3 grid over [0, 2] x [0, 3] (cell centres at 0.5, 1.5 and 0.5, 1.5, 2.5) """
    vals = np.array([[1.0, 2.0, 4.0], [3.0, -1.0, 0.0]])
    ob = S.SdfObstacle(vals, (0, 0), (2, 3), approximate_outside=False)
    at = lambda x, y: float(ob.sample([np.array([x]), np.array([y])])[0])
    assert at(0.5, 0.5) == 1.0 and at(1.5, 2.5) == 0.0 and at(1.0, 0.5) == 2.0 and at(0.5, 2.0) == 3.0
    assert at(1.0, 1.0) == (1 + 2 + 3 - 1) / 4
    assert at(-7.0, 0.5) == 1.0 and at(0.5, 99.0) == 4.0 and at(5.0, -5.0) == 3.0          # clamped: the edge value extends
    assert bool(ob.lies_inside([np.array([1.9]), np.array([50.0])])[0])                       # ... to infinity without approximate_outside (edge value 0)
    box = S.SdfObstacle(vals, (0, 0), (2, 3), approximate_outside=True, center=(1.5, 2.0), bounding_radius=1.0)
    assert not bool(box.lies_inside([np.array([1.9]), np.array([50.0])])[0]) and bool(box.lies_inside([np.array([2.0]), np.array([3.0])])[0])     # inclusive bounds
    assert float(box.sdf([np.array([1.5]), np.array([7.0])])[0]) == 4.0                      # outside: |x - center| - bounding_radius
    # constructor defaults: center = the LOWER CORNER of the minimum cell (index (1, 1) -> (1 / 2 * 2, 1 / 3 * 3)), not its centre (1.5, 1.5)
    assert S.default_center(vals, (0, 0), (2, 3)) == (1.0, 1.0)
    assert S.default_bounding_radius(vals, (0, 0), (2, 3), (1.0, 1.0)) == float(np.hypot(0.5, 1.5)) and S.default_volume(vals, (0, 0), (2, 3)) == 1.0


# ---- the kernels, element by element -----------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("case", SC.GRIDS, ids=SC.case_id)
def test_sdf_obstacle_kernels(emu_ctx, case, dtype):
    worst = SC.run_sdf_obstacles(emu_ctx, MEM, case[0], case[1], dtype, case[2], seed=5)
    print(f"sdf-obstacle worst error / bound {worst:.3g} ({SC.case_id(case)}, {np.dtype(dtype).name})")
    assert worst <= 1.0


def test_c_abi_refusals(emu_ctx):
    check_c_abi_refusals(emu_ctx, MEM)


def check_c_abi_refusals(ctx, mem):
    """ every refusal is decided on the host before anything is launched; the one accepted call runs on buffers of `mem` """
    vals = mem.to_dev(np.ones((3, 4), np.float32))
    desc = lambda **kw: _capi.make_sdf_grid(kw.get("ptr", mem.ptr(vals)), kw.get("dtype", _capi.PHIHIP_F32), kw.get("res", (3, 4)), (0, 0), kw.get("upper", (1, 1)),
                                            (0.5, 0.5), 0.3, True)
    slot = ctx.sdf_bind(desc())
    g = _capi.make_grid(2, _capi.PHIHIP_F32, 1, (5, 7), (0, 0), (5, 7), ((1, 1), (1, 1)))
    g3 = _capi.make_grid(3, _capi.PHIHIP_F32, 1, (5, 7, 3), (0, 0, 0), (5, 7, 3), ((1, 1),) * 3)
    acc = mem.to_dev(np.zeros((5, 7, 3), np.uint8))
    v = [mem.to_dev(np.zeros((5, 7, 3), np.float32)) for _ in range(3)]      # (large enough for either grid)

    def both(item, grid=g, status=-3, word=""):
        arr = _capi.make_obstacles([item])
        for call in (lambda: ctx.obstacle_accessible(grid, arr, 1, mem.ptr(acc)), lambda: ctx.apply_obstacles(grid, arr, 1, [mem.ptr(a) for a in v])):
            with pytest.raises(_capi.PhiHipError) as e:
                call()
            assert e.value.status == status and word in str(e.value), str(e.value)
    try:
        ok = dict(kind=_capi.OBSTACLE_SDF, slot=slot, velocity=[0.5, 0.0])
        ctx.obstacle_accessible(g, _capi.make_obstacles([ok]), 1, mem.ptr(acc))
        mem.sync()
        both(dict(ok, slot=slot + 1), status=-1, word="not bound")
        both(dict(ok, slot=-1), status=-1, word="not bound")
        both(dict(ok, slot=_capi.SDF_SLOTS), status=-1, word="not bound")
        both(dict(ok, group=1), word="union")
        both(dict(ok, embed_mask=1), word="embedded")
        both(dict(ok, angular_velocity=[0.1]), word="angular velocity")
        both(ok, grid=g3, status=-1, word="rank")
        for bad, word in ((desc(ptr=0), "NULL"), (desc(dtype=7), "dtype"), (desc(res=(3, 0)), "res"), (desc(upper=(1, 0)), "positive size")):
            with pytest.raises(_capi.PhiHipError) as e:
                ctx.sdf_bind(bad)
            assert e.value.status == -1 and word in str(e.value), str(e.value)
    finally:
        ctx.sdf_release(slot)
    with pytest.raises(_capi.PhiHipError):
        ctx.sdf_release(slot)                     # released already
    slots = []                                    # a fixed number of slots per context (geometries of other tests may hold some of this context's)
    try:
        with pytest.raises(_capi.PhiHipError) as e:
            for _ in range(_capi.SDF_SLOTS + 1):
                slots.append(ctx.sdf_bind(desc()))
        assert e.value.status == -3 and "slots" in str(e.value)
        assert 1 <= len(slots) <= _capi.SDF_SLOTS and len(set(slots)) == len(slots) and all(0 <= s < _capi.SDF_SLOTS for s in slots)
    finally:
        for s in slots:
            ctx.sdf_release(s)
    import ctypes
    assert ctypes.sizeof(_capi.SdfGridStruct) == 8 + 4 * 6 + 8 * 10 and ctypes.sizeof(_capi.ObstacleStruct) == 184 and ctx.lib.version() == 102


# ---- the Python class --------------------------------------------------------------------------------------------------------------------------------------------
def _blob(sres, lower, upper, dtype=np.float64, seed=0, r_f=0.25, amp=0.3):
    rng = np.random.default_rng(seed)
    centre = [0.5 * (l + u) + 0.03 * (u - l) for l, u in zip(lower, upper)]
    return SC.blob_values(sres, lower, upper, centre, r_f, 5, amp, rng.uniform(0, 6)).astype(dtype)


def _points(rng, lower, upper, n=400, spread=0.6):
    """ points in and around the bounds, some exactly on cell centres and on the bounds faces """
    pts = [rng.uniform(l - spread * (u - l), u + spread * (u - l), n) for l, u in zip(lower, upper)]
    for p, l, u in zip(pts, lower, upper):
        p[:4] = (l, u, l, 0.5 * (l + u))
    return pts


def test_class_defaults_transforms_and_repr():
    lower, upper = (1.0, -2.0), (4.0, 3.0)
    vals = _blob((7, 9), lower, upper)
    bounds = Box(x=(1.0, 4.0), y=(-2.0, 3.0))
    g = SDFGrid(vals, bounds)
    ref = S.SdfObstacle(vals, lower, upper)
    assert g.approximate_outside and g.dims == ('x', 'y') and g.resolution == {'x': 7, 'y': 9}
    # defaults, with the quirk: center is the lower corner of the minimum cell
    arg = np.unravel_index(np.argmin(vals), vals.shape)
    assert g.center == ref.center == (1.0 + arg[0] / 7 * 3.0, -2.0 + arg[1] / 9 * 5.0)
    assert g.bounding_radius() == ref.bounding_radius > 0 and g.volume == S.default_volume(vals, lower, upper) > 0
    assert g.bounding_half_extent() == bounds.half_size
    e = SDFGrid(vals, bounds, approximate_outside=False, center=vec(x=2.0, y=0.5), volume=3.0, bounding_radius=1.25)
    assert e.center == (2.0, 0.5) and e.bounding_radius() == 1.25 and e.volume == 3.0 and not e.approximate_outside
    # transforms
    rng = np.random.default_rng(1)
    for made, want in ((g.shifted((0.5, -1.0)), ref.shifted((0.5, -1.0))), (g.shifted(vec(x=0.5, y=-1.0)), ref.shifted((0.5, -1.0))),
                       (g.at((3.0, 1.0)), ref.shifted([3.0 - ref.center[0], 1.0 - ref.center[1]])), (g.scaled(1.5), ref.scaled(1.5))):
        assert np.allclose(made.bounds.lower, want.lower, rtol=0, atol=1e-14) and np.allclose(made.bounds.upper, want.upper, rtol=0, atol=1e-14)
        assert np.allclose(made.center, want.center, rtol=0, atol=1e-14) and made.bounding_radius() == want.bounding_radius
        assert made.values is g.values                                                        # the array is shared
        pts = _points(rng, want.lower, want.upper)
        want2 = S.SdfObstacle(vals, made.bounds.lower, made.bounds.upper, True, made.center, made.bounding_radius())
        assert np.array_equal(made.lies_inside(pts), want2.lies_inside(pts)) and np.allclose(made.approximate_signed_distance(pts), want2.sdf(pts), rtol=0, atol=1e-14)
    assert g.scaled(2.0).volume == g.volume * 4 and g.at(g.center).bounds.lower == g.bounds.lower
    with pytest.raises(NotImplementedError, match="SDF does not yet support rotation"):
        g.rotated(0.3)
    with pytest.raises(NotImplementedError, match="SDF does not yet support rotation"):
        Obstacle(g).rotated(0.3)
    for name in ("gradient", "to_surface", "surf_normal", "surf_index"):
        with pytest.raises(NotImplementedError, match=name):
            SDFGrid(vals, bounds, **{name: vals})
    import torch
    with pytest.raises(NotImplementedError, match="requires grad"):
        SDFGrid(torch.tensor(vals, requires_grad=True), bounds)
    assert np.array_equal(SDFGrid(torch.tensor(vals), bounds).values, vals) and SDFGrid(vals.astype(np.float32), bounds).values.dtype == np.float32
    assert SDFGrid((vals * 100).astype(np.int64), bounds).values.dtype == np.float64
    # repr changes with bounds, values, the flag, center and radius: fluid._MaskCache keys on it
    other = vals.copy()
    other[3, 4] += 1e-9
    reprs = [repr(x) for x in (g, SDFGrid(vals, bounds), g.shifted((1e-9, 0)), SDFGrid(other, bounds), SDFGrid(vals, bounds, approximate_outside=False),
                               SDFGrid(vals, bounds, center=(2.0, 0.5)), SDFGrid(vals, bounds, bounding_radius=1.0), g.scaled(1.0 + 1e-9), SDFGrid(vals.astype(np.float32), bounds))]
    assert reprs[0] == reprs[1] and len(set(reprs)) == len(reprs) - 1
    assert repr(g.shifted((0.0, 0.0))) == repr(g)


@pytest.mark.parametrize("approx", [True, False])
@pytest.mark.parametrize("sres,lower,upper", [((7, 9), (1.0, -2.0), (4.0, 3.0)), ((1, 2), (0.0, 0.0), (1.0, 1.0)), ((3, 4, 5), (-1.0, 0.5, 2.0), (2.0, 1.5, 9.0))])
def test_host_queries_follow_the_restatement(sres, lower, upper, approx):
    """ resample(geometry, ...) and field.where(geometry, ...) evaluate these on the host """
    vals = _blob(sres, lower, upper, np.float32)
    dims = 'xyz'[:len(sres)]
    g = SDFGrid(vals, Box(**{d: (l, u) for d, l, u in zip(dims, lower, upper)}), approximate_outside=approx)
    ref = S.SdfObstacle(vals, lower, upper, approx)
    pts = _points(np.random.default_rng(2), lower, upper)
    assert np.array_equal(g.lies_inside(pts), ref.lies_inside(pts)) and g.lies_inside(pts).any() and not g.lies_inside(pts).all()
    d = np.abs(g.approximate_signed_distance(pts) - ref.sdf(pts))
    assert d.max() <= 8 * P.EPS64 * (np.abs(ref.sdf(pts)).max() + ref.reach), d.max()


def test_resample_and_where_take_an_sdf_grid(emu_backend):
    lower, upper = (2.0, 3.0), (12.0, 11.0)
    vals = _blob((20, 16), lower, upper, np.float32)
    g = SDFGrid(vals, Box(x=(2.0, 12.0), y=(3.0, 11.0)))
    ref = S.SdfObstacle(vals, lower, upper)
    s = CenteredGrid(1.0, ZERO, Box(x=16, y=14), x=16, y=14, backend=emu_backend)
    pts = R.cell_points((16, 14), (0.0, 0.0), (1.0, 1.0))
    hard = resample(g, to=s).numpy()
    assert np.array_equal(hard, ref.lies_inside(pts).astype(hard.dtype)) and 0 < hard.sum() < hard.size
    soft = resample(g, to=s, soft=True).numpy()
    want = np.clip(0.5 - ref.sdf(pts) / np.sqrt(0.5), 0, 1)
    assert np.abs(soft - want).max() <= 4 * P.eps_of(np.float32)
    w = field.where(g, 3.0, s).numpy()
    assert np.array_equal(w, np.where(ref.lies_inside(pts), 3.0, 1.0).astype(w.dtype))
    init = CenteredGrid(g, ZERO, Box(x=16, y=14), x=16, y=14, backend=emu_backend).numpy()
    assert np.array_equal(init, hard)


def _velocity(backend, res, bounds, ext, rng, dtype=np.float32, batch=None, scale=0.3):
    kw = dict(zip('xyz', res))
    shapes = StaggeredGrid(0, ext, bounds, backend=backend, **kw).component_shapes
    vals = [(scale * rng.standard_normal(((batch,) if batch else ()) + tuple(s))).astype(dtype) for s in shapes]
    return StaggeredGrid(vals, ext, bounds, backend=backend, **kw), vals


def test_python_refusals(emu_backend):
    bounds = Box(x=12, y=10)
    g = SDFGrid(_blob((9, 8), (2.0, 2.0), (9.0, 8.0), np.float32), Box(x=(2.0, 9.0), y=(2.0, 8.0)))
    v, _ = _velocity(emu_backend, (12, 10), bounds, ZERO, np.random.default_rng(0))
    for obstacle, word in ((Obstacle(union(g, Sphere(x=3, y=3, radius=1))), "union"), (Obstacle(g, angular_velocity=0.3), "angular velocity")):
        for call in (lambda: fluid.apply_boundary_conditions(v, obstacle), lambda: fluid.make_incompressible(v, obstacle)):
            with pytest.raises(NotImplementedError, match=word):
                call()
    v3, _ = _velocity(emu_backend, (6, 5, 4), Box(x=12, y=10, z=4), ZERO, np.random.default_rng(0))
    with pytest.raises(NotImplementedError, match="embed"):
        fluid.apply_boundary_conditions(v3, Obstacle(geom.embed(g, 'z')))
    for kw in (dict(rebuild='from-surface'), dict(cache_surface=True), dict(valid_dist=1.0)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            sample_sdf(Sphere(x=3, y=3, radius=1), x=4, y=4, backend=emu_backend, **kw)


def _ref_flags(ref_obs, res, bc_codes, dx):
    return R.cell_flags(R.accessible(ref_obs, res, (0.0,) * len(res), dx), None, res, bc_codes, False)


def test_mask_cache_misses_after_shifted(emu_backend):
    """ the packed flags are cached on repr(geometry): a shifted SDFGrid must not find its predecessor's """
    lower, upper = (2.0, 2.0), (9.0, 8.0)
    vals = _blob((9, 8), lower, upper, np.float32)
    ob = Obstacle(SDFGrid(vals, Box(x=(2.0, 9.0), y=(2.0, 8.0))), velocity=(1.0, 0.0))
    v, _ = _velocity(emu_backend, (12, 10), Box(x=12, y=10), ZERO, np.random.default_rng(0))
    bc = ((pc.CLO, pc.CLO), (pc.CLO, pc.CLO))
    flags0 = fluid._MASKS.get(v, [ob], None)
    assert fluid._MASKS.get(v, [ob], None) is flags0                                                    # a hit
    moved = ob.shifted((2.0, 1.0))
    flags1 = fluid._MASKS.get(v, [moved], None)
    assert flags1 is not flags0
    assert np.array_equal(flags0.cpu().numpy(), _ref_flags([S.SdfObstacle(vals, lower, upper)], (12, 10), bc, (1.0, 1.0)))
    assert np.array_equal(flags1.cpu().numpy(), _ref_flags([S.SdfObstacle(vals, lower, upper).shifted((2.0, 1.0))], (12, 10), bc, (1.0, 1.0)))
    assert not np.array_equal(flags0.cpu().numpy(), flags1.cpu().numpy())


# ---- sample_sdf --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_sample_sdf_against_the_host_distance(emu_backend, dtype):
    """ phihip_sdf_from_analytic at the SDF grid's cell centres against the host approximate_signed_distance of the same geometry. Bound: both sides evaluate
    (i + 0.5) h + lower, x - c, a rotation or squares, a root, | . | - half in float64: under a dozen roundings of X = sum |x_a| + |c_a| + |half_a| each, 12 eps64 X
    as f12's K_GEO; the float32 array adds its one rounding eps32 / 2 |d| """
    rot = Box(x=(1.0, 4.0), y=(2.0, 3.5)).rotated(0.4)
    cases = [(Box(x=(1.0, 4.0), y=(2.0, 3.5)), dict(x=9, y=7)), (rot, dict(x=8, y=8)), (Sphere(x=2.0, y=-1.0, radius=1.5), dict(x=1, y=6)),
             (Sphere(x=2.0, y=-1.0, z=0.5, radius=1.5), dict(x=5, y=6, z=7)),
             (union(Box(x=(1.0, 4.0), y=(2.0, 3.5)), Sphere(x=4.0, y=3.0, radius=1.0), rot), dict(x=11, y=10)),
             (union(*[Sphere(x=0.3 * k, y=0.2 * k, z=0.1 * k, radius=0.4) for k in range(19)]), dict(x=6, y=5, z=4))]       # more members than one launch takes
    for geometry, res in cases:
        g = sample_sdf(geometry, dtype=dtype, backend=emu_backend, **res)
        assert isinstance(g, SDFGrid) and not g.approximate_outside and g.values.dtype == dtype and g.values.shape == tuple(res.values())
        bb = geom._bounding_box(geometry)
        assert np.allclose(g.bounds.center, bb.center, rtol=0, atol=1e-14) and np.allclose(g.bounds.half_size, [1.2 * h for h in bb.half_size], rtol=0, atol=1e-14)
        pts = S.cell_centres(g.values.shape, g.bounds.lower, g.bounds.upper)
        want = geometry.approximate_signed_distance(pts)
        X = sum(np.abs(p) for p in pts) + sum(abs(c) for c in bb.center) + sum(bb.half_size) + 2 * sum(abs(h) for h in bb.half_size)
        bound = 12 * P.EPS64 * X + (0.5 * P.eps_of(np.float32) * np.abs(want) if dtype == np.float32 else 0.0)
        err = np.abs(g.values.astype(np.float64) - want)
        print(f"sample_sdf {type(geometry).__name__} {tuple(res.values())} {np.dtype(dtype).name}: worst error / bound {float((err / bound).max()):.3g}")
        assert (err <= bound).all()
    sphere = Sphere(x=2.0, y=-1.0, radius=1.5)
    g = sample_sdf(sphere, Box(x=(0, 4), y=(-3, 1)), x=8, y=8, backend=emu_backend)
    assert g.center == (2.0, -1.0) and g.bounding_radius() == 1.5 and abs(g.volume - np.pi * 1.5 ** 2) < 1e-12 and g.bounds.lower == (0.0, -3.0)
    b = sample_sdf(Box(x=(1.0, 4.0), y=(2.0, 3.5)), resolution=dict(x=4), y=4, approximate_outside=True, rel_margin=0.0, abs_margin=0.5, backend=emu_backend)
    assert b.approximate_outside and b.center == (2.5, 2.75) and b.volume == 4.5 and b.bounding_radius() == float(np.hypot(1.5, 0.75)) and b.bounds.lower == (0.0, 1.0)
    u = sample_sdf(union(sphere, Sphere(x=4.0, y=-1.0, radius=0.5)), x=16, y=16, backend=emu_backend)
    assert u.center == (2.5, -1.0) and u.bounding_radius() == S.default_bounding_radius(u.values, u.bounds.lower, u.bounds.upper, u.center)


# ---- projection, batches, backward, example ------------------------------------------------------------------------------------------------------------------------
def _projection_case(backend, res, dtype=np.float32, tries=8):
    """ make_incompressible(v, [Obstacle(SDFGrid)]): a moving blob in a box that is open along y (the soft mask leaves part of the old velocity on the faces between
    fluid and solid cells, so the net flux into the fluid is not zero: with walls all around the system would have no solution and the balanced residual stays).
    Decided by the reference alone: the first seed whose faces with mask 1 are all closed by the flags (both neighbours of such a face could be fluid at a thin tip:
    the pressure gradient would then change it) """
    D = len(res)
    dims = 'xyz'[:D]
    L = [float(n) for n in res]
    bc = tuple((pc.OPN, pc.OPN) if d == 1 else (pc.CLO, pc.CLO) for d in range(D))
    lin = (0.3, -0.2, 0.1)[:D]
    for k in range(tries):
        rng = np.random.default_rng(40 + k)
        lower, upper = [0.2 * l + rng.uniform(0, 0.5) for l in L], [0.8 * l + rng.uniform(0, 0.5) for l in L]
        sres = [2 * int(u - l) + 1 for l, u in zip(lower, upper)]
        vals = _blob(sres, lower, upper, np.float32, seed=k, r_f=0.3, amp=0.1)
        ref = S.SdfObstacle(vals, lower, upper, velocity=lin)
        acc = R.accessible([ref], res, (0.0,) * D, (1.0,) * D)
        ok = R.surface_clearance([ref], res, bc, (0.0,) * D, (1.0,) * D) > SC.CLEARANCE
        full = []
        for d in range(D):
            m = ref.sdf(R.face_points(d, res, bc, (0.0,) * D, (1.0,) * D)) <= 0
            closed = R.accessible_faces(acc[None], d, res, bc)[0] == 0
            ok = ok and bool((closed | ~m).all()) and m.any()
            full.append(np.broadcast_to(m, closed.shape))
        if ok:
            ob = Obstacle(SDFGrid(vals, Box(**{d: (l, u) for d, l, u in zip(dims, lower, upper)})), velocity=lin)
            return ob, ref, acc, full, lin, bc
    raise AssertionError("no seed closes every face under a mask of 1")


@pytest.mark.parametrize("res", [(24, 20), (12, 10, 16)], ids=["24x20", "12x10x16"])
def test_projection_around_an_sdf_obstacle(emu_backend, res):
    D = len(res)
    ob, ref, acc, full, lin, bc = _projection_case(emu_backend, res)
    bounds = Box(**dict(zip('xyz', [float(n) for n in res])))
    ext = combine_sides(**{d: (BOUNDARY if d == 'y' else ZERO) for d in 'xyz'[:D]})
    v, _ = _velocity(emu_backend, res, bounds, ext, np.random.default_rng(3), scale=0.1)
    v1, p = fluid.make_incompressible(v, [ob], Solve('CG', 1e-5, 0))
    div = divergence(v1).numpy()
    print(f"projection {res}: {int((acc == 0).sum())} cells inside, {int(p.solve_info.iterations[0])} iterations, max |div| on fluid cells {np.abs(div[acc == 1]).max():.3e}")
    assert (acc == 0).sum() > 0 and np.abs(div[acc == 1]).max() <= 5e-5            # the max_div of the existing projection checks
    for d, comp in enumerate(v1.numpy()):
        assert full[d].sum() > 0 and np.array_equal(comp[full[d]], np.full(int(full[d].sum()), lin[d], comp.dtype)), f"component {d}: faces under a mask of 1"
    flags = fluid._MASKS.get(v, [ob], None).cpu().numpy()
    assert np.array_equal(flags, R.cell_flags(acc, None, res, bc, False))


def test_batched_sdf_grid_gives_per_entry_masks(emu_backend):
    lower, upper = (2.0, 2.0), (10.0, 8.0)
    bounds = Box(x=(2.0, 10.0), y=(2.0, 8.0))
    vals = np.stack([_blob((10, 9), lower, upper, np.float32, seed=s, r_f=0.2 + 0.05 * s) for s in range(3)])
    batched = SDFGrid(vals, bounds)
    assert isinstance(batched, geom.Batched) and batched.batch_size == 3 and all(isinstance(batched.entry(b), SDFGrid) for b in range(3))
    rng = np.random.default_rng(4)
    v, arrays = _velocity(emu_backend, (12, 10), Box(x=12, y=10), ZERO, rng, batch=3)
    out = fluid.apply_boundary_conditions(v, Obstacle(batched, velocity=(0.5, -0.25))).numpy()
    flags = fluid._MASKS.get(v, [Obstacle(batched)], None).cpu().numpy()
    bc = ((pc.CLO, pc.CLO),) * 2
    for b in range(3):
        vb, _ = _velocity(emu_backend, (12, 10), Box(x=12, y=10), ZERO, rng)
        single = fluid.apply_boundary_conditions(vb.with_values([emu_backend.as_tensor(a[b:b + 1], vb.dtype) for a in arrays]),
                                                 Obstacle(SDFGrid(vals[b], bounds), velocity=(0.5, -0.25))).numpy()
        for d in range(2):
            assert np.array_equal(out[d][b], single[d].reshape(out[d][b].shape))
        assert np.array_equal(flags[b], _ref_flags([S.SdfObstacle(vals[b], lower, upper)], (12, 10), bc, (1.0, 1.0)))
    assert not np.array_equal(flags[0], flags[2])


def test_functional_gradient_through_a_step_with_an_sdf_obstacle(emu_backend):
    """ as tests/test_host_api.py test_functional_gradient_through_a_fluid_step, the obstacle a stationary SDFGrid: the backward of apply_obstacles runs the
    same kernel on the gradients """
    from phiflow_amd.flow import functional_gradient, l2_loss, precision
    from test_host_api import _fd_gradient_check
    rng = np.random.default_rng(21)
    with precision(64):
        bounds = Box(x=32, y=40)
        lower, upper = (8.0, 18.0), (22.0, 30.0)
        obstacle = Obstacle(SDFGrid(_blob((14, 12), lower, upper, np.float64, r_f=0.3), Box(x=(8.0, 22.0), y=(18.0, 30.0))))
        inflow = 0.6 * CenteredGrid(Sphere(x=16, y=6, radius=4), BOUNDARY, bounds, x=16, y=20, backend=emu_backend)
        solve = Solve('CG', 1e-12, 0)

        def simulate(velocity, smoke):
            for _ in range(2):
                smoke = advect.semi_lagrangian(smoke, velocity, 1.0) + inflow
                velocity = advect.semi_lagrangian(velocity, velocity, 1.0) + resample(smoke * (0, 0.5), to=velocity)
                velocity, pressure = fluid.make_incompressible(velocity, obstacle, solve)
            return l2_loss(smoke) + 0.1 * l2_loss(velocity) + 0.01 * l2_loss(pressure), smoke, velocity

        shapes = StaggeredGrid(0, 0, bounds, x=16, y=20, backend=emu_backend).component_shapes
        v_vals = [0.3 * rng.standard_normal(s) for s in shapes]
        s_vals = rng.random((16, 20))
        mk = lambda vs, ss: (StaggeredGrid(vs, 0, bounds, x=16, y=20, backend=emu_backend), CenteredGrid(ss, BOUNDARY, bounds, x=16, y=20, backend=emu_backend))
        g_v, g_s = functional_gradient(simulate, wrt=[0, 1], get_output=False)(*mk(v_vals, s_vals))
        loss_np = lambda arrs: float(simulate(*mk(arrs[:2], arrs[2]))[0])
        _fd_gradient_check(loss_np, v_vals + [s_vals], g_v.numpy() + [g_s.numpy()], rng, eps=1e-6, tol=1e-4)


def test_example_runs(emu_backend):
    """ examples/shaped_obstacle.py --size 32 --steps 3 on the emulation backend """
    spec = importlib.util.spec_from_file_location("shaped_obstacle_example", os.path.join(ROOT, "examples", "shaped_obstacle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    v, p, worst = mod.run(32, 3, backend=emu_backend, log=lines.append)
    assert len(lines) == 1 and "max |div| on fluid cells" in lines[0] and worst <= 5e-5
    ob = mod.make_obstacle(32)
    assert isinstance(ob.geometry, SDFGrid) and (ob.geometry.values < 0).sum() > 20 and ob.geometry.values[0].min() > 0 and ob.geometry.values[:, -1].min() > 0
    assert float(np.abs(v.numpy()[1]).max()) > 0.1            # the section deflects the flow
