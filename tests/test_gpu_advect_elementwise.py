"""
`-m gpu`: element-wise parity of the forward advection passes on the MI355X, in fp32 and fp64 -- the cases of tests/test_advect_elementwise_emu.py through device
memory, and four sizes the emulation is too slow for: (24, 40, 128) periodic, (40, 36, 256) closed (the benchmark's row length on the GEN LDS-DMA instantiation),
(24, 44, 200) mixed and rows of 264 cells. Reference and comparison rule: tests/advect_forward_cases.py. Every case prints its figures.
"""
import numpy as np
import pytest

import adjoint_cases as A
import advect_forward_cases as F
import parity_cases as pc

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
_id = F.case_id
THREE_PATHS = ("adaptive", "halo 1", "halo 0")
# the grading along the slowest axis, and walls at rest, on a few grids only: they differ from their siblings in the inputs, not in the code they reach
GRADED = [(c, "graded fast") for c in F.CASES] + [(F.CASES[k], "graded slow") for k in (4, 5, 10)]
NEAR_REST = [(c, "rest walls") for c in F.CASES] + [(F.CASES[k], "rest") for k in (0, 4, 8, 11)]
SMALL = A.SMALL_CASES[::2]
_id2 = lambda ck: f"{F.case_id(ck[0])}-{ck[1].replace(' ', '_')}"


@pytest.fixture(scope="module")
def ctx(gpu_backend):
    return gpu_backend.ctx


@pytest.fixture(scope="module")
def mem(gpu_backend):
    return pc.TorchMem(str(gpu_backend.device))


@DTYPES
@pytest.mark.parametrize("dt", [0.7, 2.9], ids=["cfl<1", "cfl3"])
@pytest.mark.parametrize("case", F.CASES, ids=_id)
def test_random_fields_on_every_path(ctx, mem, case, dt, dtype):
    res, bc, batch = case
    F.run_case(ctx, mem, res, bc, dtype, batch, dt, "random", seed=1)


@DTYPES
@pytest.mark.parametrize("case_kind", GRADED, ids=_id2)
def test_graded_fields_small_samples_matter(ctx, mem, case_kind, dtype):
    (res, bc, batch), kind = case_kind
    F.run_case(ctx, mem, res, bc, dtype, batch, 0.7, kind, seed=2, strengths=(1.0,), only_paths=THREE_PATHS)


@DTYPES
@pytest.mark.parametrize("case_kind", NEAR_REST, ids=_id2)
def test_fields_near_rest_window_follows_the_sign(ctx, mem, case_kind, dtype):
    (res, bc, batch), kind = case_kind
    F.run_case(ctx, mem, res, bc, dtype, batch, 2.9, kind, seed=3, strengths=(1.0,), only_paths=THREE_PATHS)


@DTYPES
@pytest.mark.parametrize("case", F.CASES[:6] + F.CASES[9:10], ids=_id)
def test_kinks_on_purpose_exempt_from_the_window_cap(ctx, mem, case, dtype):
    res, bc, batch = case
    F.run_case(ctx, mem, res, bc, dtype, batch, 0.7, "kinks (exempt from the window cap)", seed=4, strengths=(1.0,), only_paths=THREE_PATHS)


@DTYPES
@pytest.mark.parametrize("case", SMALL, ids=A.case_id)
def test_axes_of_one_to_three_cells(ctx, mem, case, dtype):
    res, bc, batch = case
    F.run_case(ctx, mem, res, bc, dtype, batch, 2.9, "random", seed=5, strengths=(0.6,), only_paths=THREE_PATHS)
    F.run_case(ctx, mem, res, bc, dtype, batch, 0.7, "rest walls", seed=6, strengths=(1.0,), only_paths=("adaptive", "halo 0"))


@DTYPES
@pytest.mark.parametrize("entry", F.ENTRIES[:6])
@pytest.mark.parametrize("case", F.DEVICE_CASES, ids=_id)
def test_device_only_sizes(ctx, mem, case, entry, dtype):
    """ one entry point per test: the float64 reference of a 40 x 36 x 256 array is what takes the time """
    res, bc, batch, dt = case
    F.run_case(ctx, mem, res, bc, dtype, batch, dt, "random", seed=7, entries=(entry,), strengths=(1.0,))


@DTYPES
@pytest.mark.parametrize("shared", [False, True], ids=["per-batch", "shared"])
@pytest.mark.parametrize("case", F.GRID_SAMPLE_CASES, ids=_id)
def test_grid_sample_value_min_max(ctx, mem, case, shared, dtype):
    F.run_grid_sample(ctx, mem, case[0], case[1], dtype, shared)


@DTYPES
def test_hand_derived_limiter_table(ctx, mem, dtype):
    F.check_limiter_table(ctx, mem, dtype)
