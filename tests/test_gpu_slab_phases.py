"""
`-m gpu`: element-wise parity of the slab-decomposed CG phases on the MI355X, in fp32 and fp64 -- every case of tests/slab_phase_cases.py through device memory:
the one-step chain on every cut and slab-axis boundary pair with and without flags, every row width with every input kind, forced tiles and chunks, unaligned
buffers, the negative controls. Reference and comparison rule: tests/slab_phase_cases.py. Every case prints its figures.
"""
import numpy as np
import pytest

import parity_cases as pc
import slab_phase_cases as S

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
KINDS = ("random", "graded slow", "tiny", "nonfinite")


@pytest.fixture(scope="module")
def ranks(gpu_backend):
    """ one context per emulated rank, all on the one device """
    from phiflow_amd import _capi
    ctxs = [_capi.Context(gpu_backend.library, gpu_backend.device.index or 0) for _ in range(3)]
    for c in ctxs:
        c.set_autotune(False)
    yield ctxs
    for c in ctxs:
        c.close()


@pytest.fixture(scope="module")
def mem(gpu_backend):
    return pc.TorchMem(str(gpu_backend.device))


@DTYPES
@pytest.mark.parametrize("flags", [True, False], ids=["flags", "plain"])
@pytest.mark.parametrize("case", S.CHAIN_CASES, ids=lambda c: "cuts=" + ",".join(map(str, c[1])))
def test_chain(ranks, mem, case, flags, dtype):
    """ cuts=0,3,5,7-plain-f32, the ragged fp32 row (7,4,13) with a near-cancelling entry, is the case that found the overlap stored with two different bit patterns
    (DESIGN.md f15 "Found"): `slab_residual sum r^2 | own` was 640 x its bound before the RAG instantiation """
    res, cuts, k = case
    S.run_chain(ranks, mem, res, S._bc(k), dtype, cuts, flags=flags, seed=1)


@DTYPES
def test_chain_that_runs_on_after_the_refresh(ranks, mem, dtype):
    """ max_iterations = 4: the MATVEC after residual(keep_going) computes, on the refreshed r and its halos """
    res, cuts, k = S.CHAIN_CASES[0]
    S.run_chain(ranks, mem, res, S._bc(k), dtype, cuts, flags=True, seed=4, max_iterations=4)


@pytest.mark.parametrize("a0", range(3), ids=["periodic", "closed-open", "open-closed"])
@pytest.mark.parametrize("k", range(len(S.WIDTH_CASES)), ids=lambda k: f"{S.WIDTH_CASES[k][0]}-n2={S.WIDTH_CASES[k][1][-1]}")
def test_row_widths(ranks, mem, k, a0):
    """ every input kind, flags absent and present, one-plane and two-plane slabs (a0 = 0, 1) and the uneven split (a0 = 2) """
    name, res, force = S.WIDTH_CASES[k]
    bc = (S.SLAB_BCS[a0],) + S._bc(k)[1:]
    cuts = [0, 1, 3, res[0]] if a0 < 2 or res[0] != 7 else S.UNEVEN7
    S.run_phases(ranks, mem, res, bc, S.DT[name], cuts, kinds=KINDS, flags=(False, True), seed=2 + k, force=force)


@pytest.mark.parametrize("k", range(len(S.TILE_CASES)), ids=lambda k: f"{S.TILE_CASES[k][0]}-{'x'.join(map(str, S.TILE_CASES[k][1]))}-chunk={S.TILE_CASES[k][3][1]}")
def test_tiles_and_chunks(ranks, mem, k):
    """ two tiles along each in-plane axis next to the plane halos; slabs cut into chunks of 1 and 2 planes (MATVEC: odd chunks march down) """
    name, res, cuts, force = S.TILE_CASES[k]
    S.run_phases(ranks, mem, res, S._bc(k), S.DT[name], cuts, kinds=("random", "nonfinite"), flags=(False, True), seed=20 + k, force=force)
    S.run_chain(ranks, mem, res, S._bc(k), S.DT[name], cuts, flags=True, seed=30 + k, force=force)


@DTYPES
def test_unaligned_buffers(ranks, mem, dtype):
    """ every field and halo plane one element past a 16-byte boundary, the flags one byte past: the UNAL instantiation on a whole-vector row """
    res = (7, 5, 12) if dtype == np.float32 else (7, 5, 10)
    S.run_phases(ranks, mem, res, S._bc(1), dtype, [0, 1, 3, 7], kinds=("random", "nonfinite"), flags=(False, True), seed=40, offset=1)


@DTYPES
def test_negative_controls(ranks, mem, dtype):
    counts = S.control_counts(ranks, mem, dtype, seed=3)
    print(f"slab-phases controls {np.dtype(dtype).name}: violations {counts}")
    assert counts[None] == 0
    for tamper in S.TAMPERS:
        assert counts[tamper] > 0, tamper
