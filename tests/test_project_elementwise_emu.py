"""
Element-wise parity of the projection stencils and obstacle kernels under the CPU emulation (tests/hipemu), in fp32 and fp64: every output sample of
phihip_divergence (flags, balance, finite guard), phihip_grad_subtract, phihip_laplace_apply (every tile configuration of MODE_APPLY), phihip_build_cellflags,
phihip_obstacle_accessible, phihip_apply_obstacles, phihip_centered_to_staggered and phihip_diffuse_explicit against the float64 restatement tests/project_ref.py
under a per-sample bound -- tests/project_elementwise_cases.py describes the rule. Each check asserts, inside the functions it calls, the pin of the restatement
to the oracle (<= 1e-12 S), the exact non-finite pattern, the per-sample bound and -- where query_plan exposes it -- the plan that ran.
tests/test_gpu_project_elementwise.py repeats the tables on the device. Every case prints its figures.
"""
import ast
import os

import numpy as np
import pytest

import adjoint_cases as A
import parity_cases as pc
import project_elementwise_cases as P
from parity_cases import CLO, OPN, PER

MEM = pc.NumpyMem()
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
SMALL = A.SMALL_CASES[::2]
_id = P.case_id
_DT = {"f32": np.float32, "f64": np.float64}


# ---- the reference stands alone ------------------------------------------------------------------------------------------------------------------------------------
def test_reference_imports_nothing_under_test():
    tree = ast.parse(open(os.path.join(os.path.dirname(__file__), "project_ref.py")).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names == {"numpy"}, names


# ---- coverage of the tables ----------------------------------------------------------------------------------------------------------------------------------------
def test_every_side_kind_on_every_internal_axis():
    """ every stencil entry point runs on all of ROW_CASES (run_stencils), so the table's coverage is each entry point's """
    for axis in (0, 1, 2):
        seen = {c[1][len(c[0]) - 3 + axis] for c in P.ROW_CASES if len(c[0]) - 3 + axis >= 0}
        assert seen == set(P.KINDS), (axis, seen)
    assert {c[0][-1] for c in P.ROW_CASES} == {4, 8, 64, 68, 70, 72, 130, 131, 134}
    assert {c[0][-2] for c in P.ROW_CASES} == {3, 4, 5, 9} and {c[0][0] for c in P.ROW_CASES if len(c[0]) == 3} == {1, 3, 7}
    # whole vectors between two CLOSED sides (full2 == false) and behind an OPEN upper side (the extra face), in both element types
    for V in (4, 2):
        assert any(c[1][-1] == (CLO, CLO) and c[0][-1] % V == 0 for c in P.ROW_CASES)
        assert any(c[1][-1][1] == OPN and c[0][-1] % V == 0 for c in P.ROW_CASES)
    assert {len(c[0]) for c in P.ROW_CASES} == {2, 3} and {len(c[0]) for c in P.OBSTACLE_GRIDS} == {2, 3}
    assert [c[0] for c in P.OBSTACLE_GRIDS] == [(24, 20), (12, 10, 16), (9, 70), (5, 6, 134)]


def test_wall_constants_are_non_zero_and_pairwise_different():
    for case in P.ROW_CASES:
        x = P.make_inputs(case[0], case[1], np.float32, case[2], "random", 0)
        flat = x.bcv.ravel()
        assert flat.size == 2 * len(case[0]) ** 2 and (flat != 0).all() and len(set(flat.tolist())) == flat.size
        assert np.array_equal(flat.astype(np.float32).astype(np.float64), flat)
        assert len(set(x.dx)) == len(x.dx) and all(np.frexp(h)[0] != 0.5 for h in x.dx)      # different per axis, no power of two
    x = P.make_inputs((3, 4, 4), P.ROW_CASES[0][1], np.float32, 1)
    assert x.bcv.size == 18


def test_batches_and_flag_modes_occur():
    assert {c[2] for c in P.ROW_CASES} == {1, 2, 3}
    assert P.MODES == ("none", "shared", "per")
    rng = np.random.default_rng(0)
    acc, act, mb = P.masks((6, 8), 3, "per", rng)
    assert mb == 3 and (acc[2] != 0).all() and not (acc[0] != 0).all() and not np.array_equal(acc[0] != 0, acc[1] != 0)      # different obstacles, the last entry none
    acc, act, mb = P.masks((6, 8), 3, "per", rng, all_inactive=True)
    assert not act[0].any() and act[1].any()


def test_every_tile_configuration_is_forced_under_mode_apply():
    """ run_laplace_plans forces every available id of a grid and asserts it through query_plan; here: the union over the table is every id a type has """
    ids = {"f32": set(), "f64": set()}
    for res, bc, name in P.LAPLACE_PLAN_CASES:
        ids[name] |= set(P.available_tiles(res[-1], _DT[name]))
    assert ids["f32"] == set(range(11)) and ids["f64"] == set(range(13))     # (the wide row tiles 11, 12 are fp64 only)
    widths = {(name, P.march_vector_width(res[-1], _DT[name])) for res, bc, name in P.LAPLACE_PLAN_CASES}
    assert widths == {("f32", 4), ("f32", 2), ("f32", -4), ("f32", 1), ("f64", 2), ("f64", -2), ("f64", 1)}
    assert P.march_vector_width(257, np.float32) == 1 and P.march_vector_width(7, np.float32) == 1 and P.march_vector_width(129, np.float64) == 1
    assert P.available_tiles(66, np.float32) == [4, 5, 6] and P.available_tiles(260, np.float32) == list(range(11)) and P.available_tiles(258, np.float64)[-2:] == [11, 12]


def test_the_plan_helpers_restate_the_expected_plans():
    """ literal plans: the vector / scalar choice of every row case, and the device-only groups """
    for res, bc, batch in P.ROW_CASES:
        for dtype, V in ((np.float32, 4), (np.float64, 2)):
            whole = res[-1] % V == 0
            assert P.divergence_plan(res, dtype)["vec"] == whole and P.grad_subtract_plan(res, bc, dtype)["vec"] == whole and P.c2s_plan(res, dtype)["vec"] == whole
            assert not P.divergence_plan(res, dtype, aligned=False)["vec"]
            assert P.divergence_plan(res, dtype)["planes"] == 1 and P.grad_subtract_plan(res, bc, dtype)["npatch"] < 16384
    assert P.divergence_plan((3, 4, 4), np.float32)["ltpr"] == 0 and P.divergence_plan((7, 5, 8), np.float32)["ltpr"] == 1 and P.divergence_plan((3, 5, 72), np.float32)["ltpr"] == 5
    assert [P.cellflags_plan(r) for r in ((3, 4, 4), (1, 9, 64), (7, 4, 70))] == [1, 4, 0] and P.cellflags_plan((1, 9, 64), aligned=False) == 0
    # several planes per workgroup: 2 planes per chunk, 2050 chunks, one plane in the last
    for (res, bc, batch), dtypes in zip(P.DEVICE_DIVERGENCE_CASES, ([np.float32, np.float64],) * 4):
        for dtype in dtypes:
            plan = P.divergence_plan(res, dtype)
            assert (plan["tiles"], plan["planes"], plan["chunks"], plan["last"]) == (1, 2, 2050, 1), plan
            assert plan["vec"] == (res[-1] == 8)
    # second trip of the patch loop
    for res, bc, batch in P.DEVICE_GRAD_CASES:
        for dtype in (np.float32, np.float64):
            plan = P.grad_subtract_plan(res, bc, dtype)
            assert plan["npatch"] == 16400 and plan["nblk"] == 16384 and plan["vec"] == (res[-1] == 8), plan
    # second trip of the balance loop
    plan = P.balance_plan(P.DEVICE_BALANCE_CASE[0])
    assert plan["cells"] == 2197000 > 8192 * 256 and plan["apply_blocks"] == 8192 and plan["trips"] == 2 and plan["sum_blocks"] == 4096


# ---- canary: the bound tells what the old rule cannot (NumPy only) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,res,bc", [("divergence", (9, 70), ((CLO, OPN), (PER, PER))), ("laplace", (5, 9, 260), ((CLO, OPN), (OPN, OPN), (PER, PER)))])
def test_a_tap_weight_off_by_4e_6_passes_the_old_rule_and_fails_the_bound(entry, res, bc):
    old_share, new_worst, clean = P.canary_scaled_tap(entry, res, bc)
    print(f"project-elementwise canary {entry} {res}: old rule flags {old_share:.3g} of the samples, worst error / bound {new_worst:.3g} (unperturbed fp32 reference {clean:.3g})")
    assert old_share == 0.0 and new_worst > 1.0 and clean <= 1.0


@pytest.mark.parametrize("res,bc", [((16, 20), ((CLO, CLO), (CLO, CLO))), ((9, 7, 10), ((CLO, CLO), (OPN, OPN), (CLO, OPN))), ((6, 20, 72), ((CLO, OPN), (PER, PER), (CLO, CLO)))])
def test_a_wall_constant_from_the_other_side_fails_the_bound(res, bc):
    """ at the sizes of test_stencils_match_oracle, `tiny interior` input: the old rule's figure is printed -- with constants of order 1 the swapped constant is as
    large as the array's maximum, so the old rule DOES see it on this input (it is the default constant 0 of make_case that hides it) """
    old_figure, new_worst = P.canary_swapped_wall(res, bc)
    print(f"project-elementwise canary swapped wall {res}: old rule's figure {old_figure:.3g} (its tolerance 5e-6), worst error / bound {new_worst:.3g}")
    assert new_worst > 1.0


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("case", P.ROW_CASES, ids=_id)
def test_rows_and_vectors(emu_ctx, case, dtype):
    """ random, graded, tiny-interior and non-finite inputs; flags absent, shared and per entry; one entry without active cells """
    P.run_stencils(emu_ctx, MEM, case[0], case[1], dtype, case[2], seed=1)


@DTYPES
@pytest.mark.parametrize("case", SMALL, ids=A.case_id)
def test_axes_of_one_to_three_cells(emu_ctx, case, dtype):
    P.run_stencils(emu_ctx, MEM, case[0], case[1], dtype, case[2], kinds=("random", "tiny", "nonfinite"), seed=2)


@DTYPES
@pytest.mark.parametrize("case", P.UNALIGNED_CASES, ids=_id)
def test_scalar_kernels_on_whole_vector_rows(emu_ctx, case, dtype):
    """ every floating-point buffer one element past a 16-byte boundary, the flags one byte past: bit-equal to the aligned run, and within the bound """
    P.run_stencils(emu_ctx, MEM, case[0], case[1], dtype, case[2], kinds=("random", "graded"), seed=3, offset=1)


@pytest.mark.parametrize("case", P.LAPLACE_PLAN_CASES, ids=lambda c: f"{_id(c)}-{c[2]}")
def test_every_plan_of_mode_apply(emu_ctx, case):
    res, bc, name = case
    ran = P.run_laplace_plans(emu_ctx, MEM, res, bc, _DT[name], batch=2, seed=4)
    assert ran == P.available_tiles(res[-1], _DT[name])


@DTYPES
@pytest.mark.parametrize("case", P.OBSTACLE_GRIDS, ids=_id)
def test_obstacle_kernels(emu_ctx, case, dtype):
    P.run_obstacles(emu_ctx, MEM, case[0], case[1], dtype, case[2], seed=5)


@pytest.mark.parametrize("case", P.ROW_CASES + SMALL, ids=_id)
def test_cell_flags_from_arbitrary_bytes(emu_ctx, case):
    rng = np.random.default_rng(6)
    for masks in (1, 3):
        for with_active in (True, False):
            pc.check_cellflags(emu_ctx, MEM, case[0], case[1], rng, batch_masks=masks, with_active=with_active)


@pytest.mark.parametrize("case", P.DEVICE_GRAD_CASES, ids=_id)
def test_grad_subtract_second_trip_of_the_patch_loop(emu_ctx, case):
    """ more than 16 384 patches: the one device-only group the emulation finishes in time (fp32, no flags; the device file runs both types with flags) """
    res, bc, batch = case
    assert P.grad_subtract_plan(res, bc, np.float32)["npatch"] > 16384
    del P.RECORDS[:]
    try:
        P.check_grad_subtract(emu_ctx, MEM, res, bc, np.float32, batch, "random", "none", seed=8)
    finally:
        P.report()
