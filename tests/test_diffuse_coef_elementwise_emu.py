"""
Diffusion with a varying / per-axis diffusivity (phiflow_amd/csrc/diffuse_coef.hpp) ELEMENT BY ELEMENT against the float64 restatement of
tests/diffuse_coef_ref.py, on the emulation library: the explicit step, x and the two sums after the first K iterations of the CG, batch entries that stop at
different iterations, and the Python level's translation of extrapolations. Checks, case tables and bounds: tests/diffuse_coef_elementwise_cases.py;
tests/test_gpu_diffuse_coef_elementwise.py runs the same tables on the MI355X and adds the grids that march several planes per workgroup (the smallest of
them, one iteration in fp64, takes the emulation 18 s). Every case prints its measured errors before it asserts.
"""
import numpy as np
import pytest

import diffuse_coef_elementwise_cases as E
from parity_cases import NumpyMem

MEM = NumpyMem()
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
METHODS = pytest.mark.parametrize("method", ['CG', 'CG-adaptive'])
_ids = lambda cases: [c.id for c in cases]
_tid = lambda t: f"K{t[0]}-refresh{t[1]}-{t[2]}"


def test_the_table_covers_every_wall_pair_on_every_axis_and_every_thin_axis():
    seen = E.wall_coverage(E.TABLE)
    for axis in (0, 1, 2):
        missing = [p for p in E.PAIRS if p not in seen[axis]]
        assert not missing, f"internal axis {axis} never meets (u kind, coefficient kind) {missing}"
    thin = E.thin_coverage(E.TABLE)
    assert set(thin) == {(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)}
    assert all(kinds == set(range(5)) for kinds in thin.values()), thin
    assert {c.batch for c in E.TABLE} == {1, 2, 3} and {c.form for c in E.TABLE} == set(E.FORMS)
    assert {c.trajectory for c in E.TABLE} == set(E.TRAJECTORIES)
    assert not any(c.affine for c in E.NON_AFFINE)
    assert len({c.id for c in E.TABLE}) == len(E.TABLE)


def test_the_plan_helper_restates_the_expected_plans():
    for (res, target), want in E.PLANS.items():
        assert E.plan(res, target) == want, (res, target)
    # the chunked cases are there for: several planes per workgroup, a ragged last chunk
    assert E.PLANS[((115, 33, 65), 1024)][2:] == (3, 39, 1) and E.PLANS[((231, 33, 65), 4096)][2:] == (2, 116, 1)


@DTYPES
@pytest.mark.parametrize("case", E.TABLE + E.NON_AFFINE + E.FULL, ids=_ids(E.TABLE + E.NON_AFFINE + E.FULL))
def test_explicit_step_equals_the_reference(emu_ctx, case, dtype):
    E.check_explicit(emu_ctx, MEM, case, dtype)


@DTYPES
@pytest.mark.parametrize("case", E.TABLE, ids=_ids(E.TABLE))
def test_first_iterations_of_the_cg_equal_the_reference(emu_ctx, case, dtype):
    E.check_cg_trajectory(emu_ctx, MEM, case, dtype)


@DTYPES
@pytest.mark.parametrize("trajectory", E.TRAJECTORIES, ids=_tid)
@pytest.mark.parametrize("case", E.FULL, ids=_ids(E.FULL))
def test_every_trajectory_setting_equals_the_reference(emu_ctx, case, trajectory, dtype):
    E.check_cg_trajectory(emu_ctx, MEM, case, dtype, *trajectory)


@DTYPES
@pytest.mark.parametrize("trajectory", [E.TRAJECTORIES[1], E.TRAJECTORIES[4]], ids=_tid)
@pytest.mark.parametrize("case", E.NON_AFFINE, ids=_ids(E.NON_AFFINE))
def test_first_iterations_without_constant_walls_equal_the_reference(emu_ctx, case, trajectory, dtype):
    E.check_cg_trajectory(emu_ctx, MEM, case, dtype, *trajectory)


@DTYPES
@METHODS
def test_batch_entries_that_stop_at_different_iterations(emu_ctx, method, dtype):
    E.check_batch_freeze(emu_ctx, MEM, dtype, method, check_every=1)


def test_batch_entries_that_stop_at_different_iterations_polled_every_tenth(emu_ctx):
    E.check_batch_freeze(emu_ctx, MEM, np.float32, 'CG', check_every=10)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ['mixed3d', 'heat_flow', 'constants2d'])
def test_python_extrapolations_against_literal_wall_tables(emu_backend, name, bits):
    E.check_python_walls(emu_backend, name, bits)


def test_the_reference_imports_nothing_under_test():
    import ast
    import diffuse_coef_ref
    tree = ast.parse(open(diffuse_coef_ref.__file__).read())
    names = [n.module or '' for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)] + [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    assert not [m for m in names if m.split('.')[0] == 'phiflow_amd'], names


def test_the_new_files_take_no_wall_table_from_the_library():
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    needle = "_scalar" + "_walls"
    for f in ("diffuse_coef_elementwise_cases.py", "test_diffuse_coef_elementwise_emu.py", "test_gpu_diffuse_coef_elementwise.py", "diffuse_coef_ref.py"):
        assert needle not in open(os.path.join(here, f)).read(), f
