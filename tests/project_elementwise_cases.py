"""
Element-wise parity of the projection stencils and obstacle kernels (phiflow_amd/csrc/project.hip, MODE_APPLY of stencil_march.hpp) in fp32 and fp64, through the
C ABI. Used by tests/test_project_elementwise_emu.py (emulation), tests/test_gpu_project_elementwise.py (MI355X) and tests/fuzz_parity.py. DESIGN.md "f12" holds
the derivation of the constants below.

Reference: tests/project_ref.py in float64 on the inputs AFTER rounding to the element type, pinned (<= 1e-12 S) to oracle/phi_oracle.py on every case.
Rule per sample, no sample dropped or masked:
        |kernel - ref| <= (K eps + K_REF eps64) S  (+ the shift term of the balance)
    S   the same stencil applied to |inputs| with |weights| and |wall constants| (project_ref returns it)
    K   counted from the kernel source, one u = eps / 2 per rounding, rounded up to whole eps; a contracted multiply-add (hipcc's default) has one rounding fewer
Output buffers start as NaN (bytes: 0xFF); the in-place entry points start from the input. Non-finite values of the reference must appear exactly where it has them.
"""
import math

import numpy as np

import project_ref as R
from parity_cases import CLO, OPN, PER, C, O, make_case, obstacle_items, tol

RECORDS = []          # one dict per comparison: printed by `report()`, the source of the tables in DESIGN.md
EPS64 = float(np.finfo(np.float64).eps)
K_REF = 8.0           # the reference's own float64 evaluation, in eps(float64) of S
PIN = 1e-12
# rounding counts (u = eps / 2 each), K = count / 2 rounded up to whole eps
K_DIV = {2: 2.0, 3: 3.0}         # divergence_kernel: per term hi - lo and (T)rdx = 2 u of the term; the first product and each fma round the partial sum once:
                                 # 2 roundings (2-D: fma(x, r1, 0), fma), 3 (3-D): 4 u / 5 u of S
K_GRAD = 2.0                     # grad_subtract_kernel :504: pr - pl, (T)rdx, the product, v - g (h is 0 or 1): 4 u
K_LAP_FLUX = {2: 3.0, 3: 3.0}    # stencil_march.hpp :778-782: hi - c | c - lo (1 u on either), their difference, (T)w, the product = 4 u; 1 / 2 additions: 5 u / 6 u;
                                 # fma(0, c, r) is exact
K_LAP_FLAGS = {2: 3.0, 3: 4.0}   # :765-772: per open face n - c, (T)w, the product = 3 u; 0 + t exact, then 3 / 5 additions: 6 u / 8 u
K_C2S = 2.0                      # centered_to_staggered_kernel :728-731: (T)scale, s * scale (1 u on either half), the sum, out + val: 4 u of |out| + S (x 0.5 exact)
K_DIFF = {2: 5.0, 3: 7.0}        # MODE_APPLY with ident 1: 4 u per term, D - 1 additions, fma(1, c, r) 1 u, affine_walls_kernel :1619 (T)add and the sum = 2 u per
                                 # CLOSED side a sample touches (up to D at a corner): 4 + 1 + 1 + 4 = 10 u (2-D), 4 + 2 + 1 + 6 = 13 u (3-D)
K_GEO = 12.0                     # obstacle geometry in float64, kernel and reference each: (i + off) dx + lower 2 u, x - c 1 u, the rotation 5 u (or the squares and
                                 # their sum, the root), |.| - half 1 u, / radius 1 u, 1 - . 1 u: 11 u each side, in eps64 of the coordinates' magnitude / radius
KINDS = [(PER, PER), (CLO, CLO), (OPN, OPN), (CLO, OPN), (OPN, CLO)]
DX_FACTORS = (1.0, 1.25, 0.8)    # x 0.37: different per axis, no power of two


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def report():
    for r in RECORDS:
        print("project-elementwise", " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in r.items()), flush=True)


def case_id(case):
    return "x".join(str(n) for n in case[0]) + "-" + "".join("pco"[lo] + "pco"[hi] for lo, hi in case[1])


# ---- launch plans, restated ----------------------------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def vec_cells(dtype):
    """ project.hip:47 vec_cells: 16 bytes per thread """
    return 4 if np.dtype(dtype) == np.float32 else 2


def divergence_plan(res, dtype, aligned=True):
    """ project.hip divergence_vec_ok / launch_divergence: the tile shape, then plan_columns (csrc/column_march.hpp) with target 4096, one chunk on 2-D grids """
    n0, n1, n2 = ([1] * (3 - len(res)) + list(res))
    V = vec_cells(dtype)
    vec = aligned and n2 % V == 0
    ltpr = 6
    if vec:
        while ltpr > 0 and (1 << (ltpr - 1)) * V >= n2:
            ltpr -= 1
    rows, cols = (256 >> ltpr, (1 << ltpr) * V) if vec else (4, 64)
    tiles = _cdiv(n1, rows) * _cdiv(n2, cols)
    chunks = _cdiv(4096, tiles) if len(res) == 3 else 1
    chunks = min(max(chunks, 1), n0)
    planes = _cdiv(n0, chunks)
    chunks = _cdiv(n0, planes)
    return dict(vec=vec, V=V if vec else 1, ltpr=ltpr if vec else 6, tiles=tiles, planes=planes, chunks=chunks, last=n0 - (chunks - 1) * planes, nblk=tiles * chunks)


def grad_subtract_plan(res, bc, dtype, aligned=True):
    """ project.hip:617-648 launch_grad_subtract: patches and workgroups of the kernel that runs """
    D = len(res)
    shapes = [([1] * (3 - D) + list(R.comp_shape(res, bc, d))) for d in range(D)]
    nmax = [max(s[a] for s in shapes) for a in range(3)]
    n2 = res[-1]
    V = vec_cells(dtype)
    vec = aligned and n2 % V == 0
    npatch = nmax[0] * _cdiv(nmax[1], 4) * (_cdiv(n2, 64 * V) if vec else _cdiv(nmax[2], 64))
    return dict(vec=vec, npatch=npatch, nblk=min(npatch, 16384))


def balance_plan(res):
    """ project.hip:448 balance_apply_kernel's grid, :348-356 run_balance """
    cells = int(np.prod(res))
    return dict(cells=cells, apply_blocks=min(_cdiv(cells, 256), 8192), trips=_cdiv(cells, min(_cdiv(cells, 256), 8192) * 256), sum_blocks=min(_cdiv(cells, 256), 4096))


def c2s_plan(res, dtype, aligned=True):
    """ project.hip:831-837 launch_c2s_vec """
    return dict(vec=aligned and res[-1] % vec_cells(dtype) == 0)


def cellflags_plan(res, aligned=True):
    """ project.hip:1454-1455 run_build_cellflags: dwords per thread of the byte-parallel kernel, 0 = one byte per thread """
    return 4 if (aligned and res[-1] % 16 == 0) else (1 if (aligned and res[-1] % 4 == 0) else 0)


TILE_SHAPES = [(1, 16), (2, 16), (2, 32), (4, 32), (4, 64), (1, 64), (2, 64), (1, 32), (1, 128), (2, 128), (4, 128), (2, 256), (4, 256)]     # march_dispatch.hpp:24


def march_vector_width(n2, dtype, unaligned=False):
    """ march_dispatch.hpp:32-41 """
    esize = np.dtype(dtype).itemsize
    vmax = 16 // esize
    if not unaligned and n2 % vmax == 0:
        return vmax
    if not unaligned and esize == 4 and n2 % 2 == 0:
        return 2
    rem = n2 % (64 * vmax)
    if rem != 0 and rem < vmax:
        return 1
    return -vmax if n2 >= 2 * vmax else 1


def march_tile_available(vec, dtype, tid, n2):
    """ march_dispatch.hpp:46-52 """
    esize = np.dtype(dtype).itemsize
    if tid >= 11:
        return esize == 8 and vec == 2 and n2 % vec == 0 and 128 < n2 // vec <= 256
    if tid >= 8:
        return vec == 16 // esize and n2 % vec == 0 and 64 < n2 // vec <= 128
    if vec == 1 or vec < 0:
        return tid == 5
    if vec == 2 and esize == 4:
        return tid in (4, 5, 6)
    return True


def available_tiles(n2, dtype):
    vec = march_vector_width(n2, dtype)
    return [t for t in range(len(TILE_SHAPES)) if march_tile_available(vec, dtype, t, n2)]


# ---- memory helpers ------------------------------------------------------------------------------------------------------------------------------------------------
def to_dev(mem, a, offset=0):
    """ the array on the device; offset: a view that starts `offset` elements past a 16-byte boundary of a larger allocation """
    if not offset:
        return mem.to_dev(a)
    flat = np.concatenate([np.zeros(offset, a.dtype), np.ascontiguousarray(a).ravel()])
    h = mem.to_dev(flat)[offset:].reshape(a.shape)
    assert mem.ptr(h) % 16 == (offset * a.dtype.itemsize) % 16, "the allocation itself is not 16-byte aligned"
    return h


def empty(mem, shape, dtype, offset=0):
    """ NaN (bytes: 0xFF) everywhere: an element the kernel does not write shows """
    fill = np.full(shape, 0xFF, np.uint8) if np.dtype(dtype) == np.uint8 else np.full(shape, np.nan, dtype)
    return to_dev(mem, fill, offset)


def _P(mem, hs):
    return [mem.ptr(h) for h in hs]


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------------------
def wall_constants(D, rng):
    """ [axis][side][component]: 2 D^2 non-zero constants of order 1, pairwise different, exact in float32 """
    mags = 0.25 + 0.0625 * rng.permutation(2 * D * D)
    return (mags * rng.choice([-1.0, 1.0], mags.shape)).astype(np.float32).astype(np.float64).reshape(D, 2, D)


class Inputs:
    pass


def make_inputs(res, bc, dtype, batch, kind="random", seed=0):
    """ kind: random | graded | graded slow | tiny | nonfinite """
    D = len(res)
    rng = np.random.default_rng(seed)
    x = Inputs()
    h = [0.37 * f for f in DX_FACTORS[3 - D:]]
    x.bcv = wall_constants(D, rng)
    x.dom, x.grid = make_case(tuple(res), bc, dtype, batch, upper=tuple(n * hh for n, hh in zip(res, h)), bc_val=x.bcv)
    x.res, x.bc, x.dx, x.batch, x.dtype, x.rng = tuple(res), bc, x.dom.dx, batch, dtype, rng
    amp = 1e-6 if kind == "tiny" else 1.0

    def field(shape):
        a = rng.standard_normal((batch,) + tuple(shape)) * amp
        if kind.startswith("graded"):
            for ax in ([D - 1, 0] if kind == "graded slow" else [D - 1]):
                n = shape[ax]
                a = a * np.exp(-18.0 * np.arange(n) / n).reshape([n if k == ax + 1 else 1 for k in range(a.ndim)])
        a = a.astype(dtype)
        if kind == "nonfinite" and a.size:
            flat = a.reshape(-1)
            idx = rng.integers(0, flat.size, size=max(3, flat.size // 40))
            flat[idx] = np.asarray([np.nan, np.inf, -np.inf], dtype)[np.arange(idx.size) % 3]
        return a
    x.v = [field(R.comp_shape(res, bc, d)) for d in range(D)]
    x.p = field(res)
    x.s = field(res)
    return x


def masks(res, batch, mode, rng, all_inactive=False):
    """ accessible and user-active bytes of ANY non-zero value; mode 'shared': one set, 'per': one per entry -- every entry a different block of inaccessible
    cells, the last entry none; all_inactive: entry 0 has no active cell. Returns (acc, act, mask_batch) with a leading axis of mask_batch """
    mb = batch if mode == "per" else 1
    acc = np.ones((mb,) + tuple(res), np.uint8)
    for b in range(mb):
        if mb > 1 and b == mb - 1:
            continue
        box = tuple(slice(int((0.2 + 0.15 * b) * n), max(int((0.2 + 0.15 * b) * n) + 1, int((0.6 + 0.1 * b) * n))) for n in res)
        acc[b][box] = 0
        # and the last cell but one of every axis, over the lower half of the others: behind an OPEN upper side the extra face takes the UPPER-face bit of
        # the last cell, which differs from its lower-face bit exactly when cell n - 2 is inaccessible and cell n - 1 is not
        for a, n in enumerate(res):
            if n >= 2:
                acc[b][tuple(slice(n - 2, n - 1) if k == a else slice(0, (m + 1) // 2 + b) for k, m in enumerate(res))] = 0
    acc = acc * rng.integers(1, 255, acc.shape).astype(np.uint8)
    act = (rng.random(acc.shape) < 0.9).astype(np.uint8) * rng.integers(1, 255, acc.shape).astype(np.uint8)
    if all_inactive:
        act[0] = 0
    return acc, act, mb


def build_flags(ctx, mem, x, acc, act, mb, offset=0):
    """ phihip_build_cellflags on the device, compared by equality with project_ref.cell_flags; returns (handle, flags [mb, *res]) """
    D = len(x.res)
    g = C.make_grid(D, C.PHIHIP_F32, mb, x.res, x.dom.lower, x.dom.upper, x.bc)
    shape = ((mb,) if mb > 1 else ()) + x.res
    dacc, dact, dfl = to_dev(mem, acc.reshape(shape), offset), to_dev(mem, act.reshape(shape), offset), empty(mem, shape, np.uint8, offset)
    ctx.build_cellflags(g, mem.ptr(dacc), mem.ptr(dact), mb, mem.ptr(dfl))
    mem.sync()
    got = mem.to_host(dfl)
    ref = R.cell_flags(acc.reshape(shape), act.reshape(shape), x.res, x.bc, mb > 1)
    assert np.array_equal(got, ref), f"cell flags differ at {np.argwhere(got != ref)[:4].tolist()} (res {x.res}, bc {x.bc}, mask_batch {mb}, offset {offset})"
    RECORDS.append(dict(entry="build_cellflags", path=f"W{cellflags_plan(x.res, not offset)} mb{mb}", dtype="uint8", res="x".join(map(str, x.res)), ratio=0.0))
    return dfl, ref.reshape((mb,) + x.res)


# ---- comparison ----------------------------------------------------------------------------------------------------------------------------------------------------
def pin(ref, oracle, S, what):
    """ the restatement agrees with the oracle's float64 result to 1e-12 of S; non-finite values at the same places """
    ref, oracle = np.asarray(ref, np.float64), np.asarray(oracle, np.float64)
    assert ref.shape == oracle.shape, (what, ref.shape, oracle.shape)
    fin = np.isfinite(ref) & np.isfinite(oracle) & np.isfinite(S)
    with np.errstate(invalid='ignore'):
        d = np.abs(ref - oracle)[fin]
    assert (d <= PIN * S[fin]).all(), f"{what}: the restatement differs from the oracle by {float((d / np.maximum(S[fin], 1e-300)).max()):.3e} S"


def compare(entry, path, x, kind, got, ref, bound, o32=None, r32=None, old_tol=None):
    """ one output array against the reference: the exact non-finite pattern, the per-sample bound. Records the worst error / bound, the share of samples the old
    rule (old_tol of max |fp32 oracle|) would flag, and the worst error / bound of the fp32 oracle and of the restatement evaluated in the element type """
    assert got.shape == ref.shape, (entry, path, got.shape, ref.shape)
    rec = dict(entry=entry, path=path, dtype=np.dtype(x.dtype).name, res="x".join(map(str, x.res)), kind=kind, ratio=0.0)
    RECORDS.append(rec)
    if not got.size:
        return 0.0
    g = got.astype(np.float64)
    same = np.array_equal(np.isnan(g), np.isnan(ref)) and np.array_equal(np.isinf(g), np.isinf(ref)) and np.array_equal(g[np.isinf(ref)], ref[np.isinf(ref)])
    assert same, (f"{entry} [{path}] {rec['dtype']} res {x.res} bc {x.bc} {kind}: non-finite values differ from the reference's at "
                  f"{np.argwhere((np.isnan(g) != np.isnan(ref)) | (np.isinf(g) != np.isinf(ref)))[:4].tolist()}")
    fin = np.isfinite(ref)
    b = np.where(np.isfinite(bound), bound, 0.0)

    def ratio_of(a):
        d = np.where(fin, np.abs(np.where(fin, a, 0.0) - np.where(fin, ref, 0.0)), 0.0)
        return np.where(b > 0, d / np.maximum(b, 1e-300), np.where(d > 0, np.inf, 0.0))
    ratio = ratio_of(g)
    rec["ratio"] = float(ratio.max())
    if o32 is not None and fin.all():
        o = np.asarray(o32, np.float64)
        rec["old_rule"] = float((np.abs(g - o) > old_tol * max(float(np.abs(o).max()), 1e-30)).mean())
        rec["oracle32"] = float(ratio_of(o).max())
    if r32 is not None and fin.all():
        rec["ref32"] = float(ratio_of(np.asarray(r32, np.float64)).max())
    if ratio.max() > 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{entry} [{path}] {rec['dtype']} res {x.res} bc {x.bc} {kind}: at {i}: kernel {got[i]!r} vs reference {ref[i]!r}, "
                             f"{ratio[i]:.3g} x the bound {b[i]:.3e}; {int((ratio > 1).sum())} of {ratio.size} samples beyond their bound")
    return rec["ratio"]


def _to64(arrays):
    return [np.asarray(a, np.float64) for a in arrays]


def _flag_state(ctx, mem, x, mode, all_inactive=False, offset=0):
    """ (flags handle or None, mask_batch, accessible 0/1 [mb, *res] or None, active 0/1 or None) """
    if mode == "none":
        return None, 1, None, None
    acc, act, mb = masks(x.res, x.batch, mode, x.rng, all_inactive)
    dfl, flags = build_flags(ctx, mem, x, acc, act, mb, offset)
    if offset:      # (built by the one-byte-per-thread kernel on unaligned buffers; the stencils get an aligned copy and make their own unaligned one)
        dfl = mem.to_dev(mem.to_host(dfl))
    return dfl, mb, (acc != 0).astype(np.uint8), ((flags >> 6) & 1).astype(np.uint8)


# ---- divergence ----------------------------------------------------------------------------------------------------------------------------------------------------
def divergence_bound(x, S, active, balanced, aligned=True):
    """ (K eps + K_REF eps64) S on active cells, 0 on inactive ones (they are selected, not computed); balanced: + eps / 2 S (the subtraction) + on active cells
    Sbar [(K + 1 + (m - 1) / 2) eps + ((ceil(nblk / 256) + 16) / 2 + K_REF) eps64],  Sbar = sum S / sum active: the error of sum(div) is at most the sum of the
    samples' bounds plus the m - 1 additions of a thread's partial sum in the element type (m = planes per chunk x cells per thread) plus the double-precision
    tree over the workgroup and the list of partial sums (balance_scalar_kernel: ceil(nblk / 256) additions per thread + two trees of 8); (T)shift and the
    subtraction round once each, |shift| <= Sbar """
    eps = eps_of(x.dtype)
    D = len(x.res)
    a = np.ones(S.shape) if active is None else np.broadcast_to(active, S.shape).astype(np.float64)
    Sm = np.where(a > 0, np.where(np.isfinite(S), S, 0.0), 0.0)
    bound = (K_DIV[D] * eps + K_REF * EPS64) * Sm
    if balanced:
        plan = divergence_plan(x.res, x.dtype, aligned)
        m = plan["planes"] * plan["V"]
        n = a.reshape(a.shape[0], -1).sum(axis=1)
        sbar = (Sm.reshape(a.shape[0], -1).sum(axis=1) / np.where(n > 0, n, 1.0)).reshape((-1,) + (1,) * D)
        bound = bound + 0.5 * eps * Sm + a * sbar * ((K_DIV[D] + 1.0 + 0.5 * (m - 1)) * eps + (0.5 * (_cdiv(plan["nblk"], 256) + 16) + K_REF) * EPS64)
    return bound


def check_divergence(ctx, mem, res, bc, dtype, batch=2, kind="random", mode="none", seed=0, offset=0, all_inactive=False, variants=None):
    """ phihip_divergence: plain, balanced, and with the finite guard; mode: flags absent ('none'), 'shared' or 'per' entry. offset: every floating-point buffer
    one element past a 16-byte boundary and the flags one byte past -- the scalar kernel; asserted bit-equal to the aligned run """
    x = make_inputs(res, bc, dtype, batch, kind, seed)
    D = len(res)
    dfl, mb, acc, active = _flag_state(ctx, mem, x, mode, all_inactive, offset)
    v64 = _to64(x.v)
    with np.errstate(invalid='ignore', over='ignore'):
        div64, S = R.divergence(v64, x.res, x.bc, x.bcv, x.dx)
        o64 = O.divergence(v64, x.dom)
        r32 = R.divergence(x.v, x.res, x.bc, x.bcv, x.dx, dtype)[0] if kind != "nonfinite" else None
        o32 = O.divergence(x.v, x.dom) if kind != "nonfinite" else None
    pin(div64, o64, S, "divergence")
    assert np.array_equal(np.isfinite(div64), np.isfinite(o64)), "divergence: the restatement's non-finite values differ from the oracle's"
    if variants is None:
        variants = [(0, 0), (0, 1)] if kind == "nonfinite" else [(0, 0), (1, 0)]
    a_b = None if active is None else np.broadcast_to(active, div64.shape)
    dv = [to_dev(mem, a) for a in x.v]
    dv_off = [to_dev(mem, a, 1) for a in x.v] if offset else None
    dfl_off = to_dev(mem, mem.to_host(dfl), 1) if (offset and dfl is not None) else None
    for bal, guard in variants:
        ref = R.mask_divergence(div64, a_b, bool(guard))
        want32, old32 = r32, o32
        if kind != "nonfinite":
            want32 = R.mask_divergence(r32, a_b, False)
            old32 = np.where(a_b > 0, o32, dtype(0)) if a_b is not None else o32
        if bal:
            if a_b is not None and not all_inactive:
                pin(R.balance(ref, a_b)[0], O.balance_divergence(ref, a_b.astype(np.float64)), S + np.abs(ref).mean(), "balance_divergence")
            ref, shift, n = R.balance(ref, a_b)
            if all_inactive:
                assert n[0] == 0 and shift[0] == 0.0
                old32 = None      # (the oracle divides 0 by 0 for such an entry: NaN everywhere in it)
            want32 = R.balance(want32, a_b, dtype)[0]
            if old32 is not None:
                old32 = O.balance_divergence(old32, None if a_b is None else a_b.astype(dtype))
        code = (C.DIV_BALANCE if bal else 0) | (C.DIV_FINITE_GUARD if guard else 0)
        out = empty(mem, (batch,) + x.res, dtype)
        ctx.divergence(x.grid, _P(mem, dv), mem.ptr(dfl) if dfl is not None else 0, mb, code, mem.ptr(out))
        mem.sync()
        got = mem.to_host(out)
        plan = divergence_plan(x.res, dtype)
        path = f"{'vec' if plan['vec'] else 'scalar'} flags={mode}{' balance' if bal else ''}{' guard' if guard else ''}{' all-inactive' if all_inactive else ''}"
        if all_inactive and mode != "none":
            assert not got[0].any(), "an entry without active cells: every sample 0, shift 0, nothing subtracted"
        compare("divergence", path, x, kind, got, ref, divergence_bound(x, S, a_b, bool(bal)), old32, want32, tol(dtype)['stencil'])
        if offset:
            out2 = empty(mem, (batch,) + x.res, dtype, 1)
            ctx.divergence(x.grid, _P(mem, dv_off), mem.ptr(dfl_off) if dfl_off is not None else 0, mb, code, mem.ptr(out2))
            mem.sync()
            got2 = mem.to_host(out2)
            assert not divergence_plan(x.res, dtype, False)["vec"]
            compare("divergence", path.replace("vec", "scalar (unaligned)"), x, kind, got2, ref, divergence_bound(x, S, a_b, bool(bal), aligned=False))
            if not bal:      # (the balanced result carries a sum taken in another order)
                assert np.array_equal(_bits(got2), _bits(got)), "divergence: the scalar kernel on unaligned buffers differs in bits from the vector kernel"


# ---- gradient subtraction --------------------------------------------------------------------------------------------------------------------------------------
def check_grad_subtract(ctx, mem, res, bc, dtype, batch=2, kind="random", mode="none", seed=0, offset=0):
    """ phihip_grad_subtract, in place """
    x = make_inputs(res, bc, dtype, batch, kind, seed)
    D = len(res)
    dfl, mb, acc, active = _flag_state(ctx, mem, x, mode, False, offset)
    v64, p64 = _to64(x.v), x.p.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        ref, S = R.grad_subtract(v64, p64, x.res, x.bc, x.dx, acc)
        hard = None if acc is None else [R.accessible_faces(acc, d, x.res, x.bc).astype(np.float64) for d in range(D)]
        o64 = O.gradient_subtract(v64, p64, x.dom, hard)
        if kind != "nonfinite":
            r32 = R.grad_subtract(x.v, x.p, x.res, x.bc, x.dx, acc, dtype)[0]
            o32 = O.gradient_subtract(x.v, x.p, x.dom, None if hard is None else [h.astype(dtype) for h in hard])
        else:
            r32 = o32 = [None] * D
    if kind != "nonfinite":
        for d in range(D):
            pin(ref[d], o64[d], S[d], f"gradient_subtract[{d}]")
    eps = eps_of(dtype)
    plan = grad_subtract_plan(x.res, x.bc, dtype)
    runs = [(0, f"{'vec' if plan['vec'] else 'scalar'} flags={mode}")] + ([(1, f"scalar (unaligned) flags={mode}")] if offset else [])
    first = None
    for off, path in runs:
        dv = [to_dev(mem, a, off) for a in x.v]
        dp = to_dev(mem, x.p, off)
        f = None if dfl is None else (to_dev(mem, mem.to_host(dfl), 1) if off else dfl)
        ctx.grad_subtract(x.grid, mem.ptr(f) if f is not None else 0, mb, mem.ptr(dp), _P(mem, dv))
        mem.sync()
        got = [mem.to_host(h) for h in dv]
        for d in range(D):
            if kind == "nonfinite":      # (h = 0 faces multiply: 0 * NaN = NaN in the kernel as in the reference's product)
                fin = np.isfinite(ref[d])
                assert np.array_equal(np.isfinite(got[d]), fin), f"grad_subtract[{d}]: non-finite pattern"
            compare(f"grad_subtract[{d}]", path, x, kind, got[d], ref[d], (K_GRAD * eps + K_REF * EPS64) * S[d], o32[d], r32[d], tol(dtype)['stencil'])
        if off:
            assert not grad_subtract_plan(x.res, x.bc, dtype, False)["vec"]
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, first)), "grad_subtract: the scalar kernel on unaligned buffers differs in bits"
        first = got


# ---- MODE_APPLY ----------------------------------------------------------------------------------------------------------------------------------------------------
def check_laplace(ctx, mem, res, bc, dtype, batch=2, kind="random", mode="none", seed=0, offset=0, force=None):
    """ phihip_laplace_apply. force = (tile id, chunk): that tile configuration through set_tuning_kernel(FAM_APPLY), asserted with query_plan; the caller restores
    the tuning. offset: p and out one element past a 16-byte boundary, the flags one byte past (the UNAL instantiation, byte-wise flag loads) """
    x = make_inputs(res, bc, dtype, batch, kind, seed)
    D = len(res)
    dfl, mb, acc, active = _flag_state(ctx, mem, x, mode)
    p64 = x.p.astype(np.float64)
    ref, S = R.masked_laplace(p64, x.res, x.bc, x.dx, acc, active)
    hard = None if acc is None else [R.accessible_faces(acc, d, x.res, x.bc).astype(np.float64) for d in range(D)]
    pin(ref, O.masked_laplace(p64, x.dom, hard, None if active is None else active.astype(np.float64)), S, "masked_laplace")
    r32 = R.masked_laplace(x.p, x.res, x.bc, x.dx, acc, active, dtype)[0]
    o32 = O.masked_laplace(x.p, x.dom, None if hard is None else [h.astype(dtype) for h in hard], None if active is None else active.astype(dtype))
    vec = march_vector_width(res[-1], dtype, bool(offset))
    path = f"vec={vec} flags={mode}"
    if force is not None:
        tid, chunk = force
        rows, tpr = TILE_SHAPES[tid]
        ctx.set_tuning_kernel(0, rows, tpr, chunk)
        plan = ctx.query_plan(x.grid, mode != "none", 0)
        one = vec == 1 or vec < 0
        want = dict(rows=1 if one else rows, tpr=64 if one else tpr, vec=march_vector_width(res[-1], dtype), chunk=min(chunk, res[0]) if D == 3 else 1)
        assert {k: plan[k] for k in want} == want, f"laplace_apply {res} {np.dtype(dtype).name}: plan {plan}, expected {want}"
        path += f" tile={tid} chunk={want['chunk']}"
    elif not offset:
        assert ctx.query_plan(x.grid, mode != "none", 0)["vec"] == vec
    K = K_LAP_FLUX[D] if mode == "none" else K_LAP_FLAGS[D]
    dp, out = to_dev(mem, x.p, offset), empty(mem, x.p.shape, dtype, offset)
    f = None if dfl is None else (to_dev(mem, mem.to_host(dfl), 1) if offset else dfl)
    ctx.laplace_apply(x.grid, mem.ptr(f) if f is not None else 0, mb, mem.ptr(dp), mem.ptr(out))
    mem.sync()
    got = mem.to_host(out)
    compare("laplace_apply", path, x, kind, got, ref, (K * eps_of(dtype) + K_REF * EPS64) * S, o32, r32, tol(dtype)['stencil'])
    if offset:
        dp0, out0 = to_dev(mem, x.p), empty(mem, x.p.shape, dtype)
        ctx.laplace_apply(x.grid, mem.ptr(dfl) if dfl is not None else 0, mb, mem.ptr(dp0), mem.ptr(out0))
        mem.sync()
        assert np.array_equal(_bits(got), _bits(mem.to_host(out0))), "laplace_apply: the UNAL instantiation on unaligned buffers differs in bits from the aligned run"


def run_laplace_plans(ctx, mem, res, bc, dtype, batch=2, seed=0):
    """ every tile configuration the grid's vector width has, chunk 2 and 1, flags shared / per entry / absent """
    del RECORDS[:]
    ran = []
    try:
        for tid in available_tiles(res[-1], dtype):
            for k, (chunk, mode) in enumerate(((2, "per"), (1, "none"), (2, "shared"))):
                check_laplace(ctx, mem, res, bc, dtype, batch, "random" if k else "graded", mode, seed + tid, force=(tid, chunk))
            ran.append(tid)
    finally:
        ctx.set_tuning_kernel(0, 0, 0, 0)
        report()
    return ran


# ---- resample, diffusion, scaling ------------------------------------------------------------------------------------------------------------------------------------
def check_centered_to_staggered(ctx, mem, res, bc, dtype, batch=2, kind="random", seed=0, offset=0, rotations=range(4)):
    """ phihip_centered_to_staggered, plain and accumulating with a zero vector component (that component's bits stay); the scalar's sides run through every pair
    of kinds with non-zero constants below and above """
    x = make_inputs(res, bc, dtype, batch, kind, seed)
    D = len(res)
    eps = eps_of(dtype)
    vector = [0.3, -1.5, 0.1][:D]
    s64 = x.s.astype(np.float64)
    plan = c2s_plan(x.res, dtype, not offset)
    for k in rotations:
        s_codes = tuple((PER, PER) if x.bc[a][0] == PER else KINDS[1 + (a + k) % 4] for a in range(D))      # (the scalar is periodic exactly where the grid is)
        s_consts = [(float(np.float32(0.75 + 0.25 * a + k)), float(np.float32(-1.25 - 0.5 * a - k))) for a in range(D)]
        path = f"{'vec' if plan['vec'] else 'scalar'}{' (unaligned)' if offset else ''} s={''.join('pco'[lo] + 'pco'[hi] for lo, hi in s_codes)}"
        ref, S = R.centered_to_staggered(s64, x.res, x.bc, s_codes, s_consts, vector)
        o64 = O.centered_to_staggered(s64, x.dom, s_codes, s_consts, vector)
        r32 = R.centered_to_staggered(x.s, x.res, x.bc, s_codes, s_consts, vector, None, dtype)[0]
        o32 = O.centered_to_staggered(x.s, x.dom, s_codes, s_consts, vector)
        ds = to_dev(mem, x.s, offset)
        out = [empty(mem, a.shape, dtype, offset) for a in x.v]
        ctx.centered_to_staggered(x.grid, mem.ptr(ds), s_codes, s_consts, vector, False, _P(mem, out))
        mem.sync()
        for d in range(D):
            pin(ref[d], o64[d], S[d], f"centered_to_staggered[{d}]")
            compare(f"centered_to_staggered[{d}]", path, x, kind, mem.to_host(out[d]), ref[d], (K_C2S * eps + K_REF * EPS64) * S[d], o32[d], r32[d], tol(dtype)['stencil'])
        if offset:
            ds0, out0 = to_dev(mem, x.s), [empty(mem, a.shape, dtype) for a in x.v]
            ctx.centered_to_staggered(x.grid, mem.ptr(ds0), s_codes, s_consts, vector, False, _P(mem, out0))
            mem.sync()
            assert all(np.array_equal(_bits(mem.to_host(a)), _bits(mem.to_host(b))) for a, b in zip(out, out0)), \
                "centered_to_staggered: the scalar kernel on unaligned buffers differs in bits from the aligned run"
        zero = k % D
        vector0 = [0.0 if d == zero else c for d, c in enumerate(vector)]
        ref, S = R.centered_to_staggered(s64, x.res, x.bc, s_codes, s_consts, vector0, _to64(x.v))
        acc = [to_dev(mem, a, offset) for a in x.v]
        ctx.centered_to_staggered(x.grid, mem.ptr(ds), s_codes, s_consts, vector0, True, _P(mem, acc))
        mem.sync()
        for d in range(D):
            got = mem.to_host(acc[d])
            if d == zero:
                assert np.array_equal(_bits(got), _bits(x.v[d])), f"centered_to_staggered accumulate: the component with a zero vector entry ({d}) changed"
            compare(f"centered_to_staggered+=[{d}]", path, x, kind, got, ref[d], (K_C2S * eps + K_REF * EPS64) * S[d])


def check_diffuse_explicit(ctx, mem, res, bc, dtype, batch=2, kind="random", seed=0, kdts=(0.011, -0.007)):
    """ phihip_diffuse_explicit of the staggered field with its wall constants (the marching kernels with ident 1 + affine_walls_kernel), kdt of both signs """
    x = make_inputs(res, bc, dtype, batch, kind, seed)
    D = len(res)
    eps = eps_of(dtype)
    v64 = _to64(x.v)
    dv = [to_dev(mem, a) for a in x.v]
    for kdt in kdts:
        ref, S = R.diffuse_explicit(v64, x.res, x.bc, x.bcv, x.dx, kdt)
        o64 = O.diffuse_explicit(v64, 1.0, kdt, x.dom)
        r32 = R.diffuse_explicit(x.v, x.res, x.bc, x.bcv, x.dx, kdt, dtype)[0]
        o32 = O.diffuse_explicit(x.v, 1.0, kdt, x.dom)
        out = [empty(mem, a.shape, dtype) for a in x.v]
        ctx.diffuse_explicit(x.grid, _P(mem, dv), _P(mem, out), kdt)
        mem.sync()
        for d in range(D):
            pin(ref[d], o64[d], S[d], f"diffuse_explicit[{d}]")
            vec = march_vector_width(R.comp_shape(x.res, x.bc, d)[-1], dtype)
            compare(f"diffuse_explicit[{d}]", f"vec={vec} kdt={kdt}", x, kind, mem.to_host(out[d]), ref[d], (K_DIFF[D] * eps + K_REF * EPS64) * S[d], o32[d], r32[d],
                    tol(dtype)['stencil'])


# ---- obstacles -------------------------------------------------------------------------------------------------------------------------------------------------
CLEARANCE = 1e-9


def to_oracle(ob):
    if isinstance(ob, R.Box):
        return O.BoxObstacle(ob.lower, ob.upper, ob.velocity, ob.angular_velocity, ob.rotation)
    if isinstance(ob, R.Sphere):
        return O.SphereObstacle(ob.center, ob.radius, ob.velocity, ob.angular_velocity)
    if isinstance(ob, R.Embedded):
        return O.EmbeddedObstacle(to_oracle(ob.inner), ob.axes, ob.velocity)
    return O.UnionObstacle(tuple(to_oracle(m) for m in ob.members), ob.velocity)


def _rot(D, rng):
    if D == 2:
        t = rng.uniform(0.2, 1.2)
        return np.asarray([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def scene(name, res, dx, rng):
    """ obstacles of one named scene on a domain [0, res * dx], positions jittered by the seed """
    D = len(res)
    L = [n * h for n, h in zip(res, dx)]
    j = lambda: rng.uniform(-0.03, 0.03)
    pt = lambda *f: tuple((f[a] + j()) * L[a] for a in range(D))
    fr = (0.3, 0.45, 0.55), (0.62, 0.7, 0.8)
    lin = (0.4, -0.7, 0.25)[:D]
    ang = 0.8 if D == 2 else (0.5, -0.3, 0.9)
    rmin = min(L)
    if name == "box":
        return [R.Box(pt(*fr[0][:D]), pt(*fr[1][:D]))]
    if name == "rotated box":
        return [R.Box(pt(*fr[0][:D]), pt(*fr[1][:D]), rotation=_rot(D, rng), velocity=lin, angular_velocity=ang)]
    if name == "sphere":
        return [R.Sphere(pt(0.5, 0.45, 0.55), (0.23 + j()) * rmin, velocity=lin, angular_velocity=ang)]
    if name == "embedded":      # a cylinder along the first axis and a slab across the last one
        return [R.Embedded(R.Sphere(pt(0.4, 0.5, 0.5)[1:], (0.2 + j()) * min(L[1:])), tuple(range(1, D)), velocity=lin),
                R.Embedded(R.Box((pt(0.7, 0.7, 0.72)[-1],), (pt(0.8, 0.8, 0.83)[-1],)), (D - 1,))]
    if name == "union of three":
        return [R.Union([R.Box(pt(0.2, 0.2, 0.2), pt(0.45, 0.5, 0.4)), R.Sphere(pt(0.5, 0.5, 0.45), (0.18 + j()) * rmin),
                         R.Box(pt(0.4, 0.55, 0.5), pt(0.8, 0.7, 0.9), rotation=_rot(D, rng))], velocity=lin)]
    if name == "union across 16":   # 12 singles + a union of 9: the union must not be cut at entry 16 of a launch
        singles = [R.Sphere(pt(*(0.1 + 0.8 * rng.random(3))), (0.04 + 0.04 * rng.random()) * rmin, velocity=lin if k % 3 == 0 else None) for k in range(12)]
        return singles + [R.Union([R.Sphere(pt(*(0.15 + 0.7 * rng.random(3))), (0.05 + 0.05 * rng.random()) * rmin) for _ in range(9)], velocity=lin)]
    if name == "20 moving spheres":
        return [R.Sphere(pt(*(0.05 + 0.9 * rng.random(3))), (0.03 + 0.05 * rng.random()) * rmin, velocity=tuple(rng.uniform(-1, 1, D)),
                         angular_velocity=(None if k % 2 else ang)) for k in range(20)]
    if name == "outside and covering":
        return [R.Sphere(tuple(-3.0 * l for l in L), 0.4 * rmin, velocity=lin), R.Box(tuple(-0.37 * l - 0.11 for l in L), tuple(1.41 * l + 0.13 for l in L), velocity=lin)]
    if name == "outside":
        return [R.Box(tuple(1.5 * l for l in L), tuple(1.9 * l for l in L), velocity=lin)]
    if name == "margin":        # the box's upper face along the fast axis lies 0.95 cell radii below the cell centres of column 64, the first column of the
        radius = math.sqrt(sum((0.5 * h) ** 2 for h in dx))      # next 4 x 64 patch: the soft mask there is 0.05, decided by the culling margin alone
        face = 64.5 * dx[-1] - (0.95 + 0.01 * j()) * radius
        return [R.Box(tuple((0.23 + j()) * l for l in L[:-1]) + (face - 3.0 * dx[-1],), tuple((0.81 + j()) * l for l in L[:-1]) + (face,), velocity=lin)]
    raise ValueError(name)


SCENES = ("box", "rotated box", "sphere", "embedded", "union of three", "union across 16", "20 moving spheres", "outside and covering", "outside")
OBSTACLE_GRIDS = [((24, 20), ((CLO, CLO), (OPN, OPN)), 2), ((12, 10, 16), ((CLO, OPN), (PER, PER), (CLO, CLO)), 2), ((9, 70), ((PER, PER), (OPN, CLO)), 1),
                  ((5, 6, 134), ((OPN, OPN), (CLO, CLO), (PER, PER)), 3)]


def pick_scene(name, res, bc, dx, seed, tries=8):
    """ the first seed (seed + 1000 k) whose geometry leaves every sample position farther than CLEARANCE cells from every surface: decided by the reference alone """
    lower = (0.0,) * len(res)
    for k in range(tries):
        obs = scene(name, res, dx, np.random.default_rng(seed + 1000 * k))
        if R.surface_clearance(obs, res, bc, lower, dx) > CLEARANCE:
            return obs
    raise AssertionError(f"scene {name!r} on {res}: no seed of {tries} keeps the samples {CLEARANCE} cells off the surfaces")


def check_obstacles(ctx, mem, res, bc, dtype, batch, obstacles, kind="random", seed=0, exact=False, what="scene"):
    """ phihip_obstacle_accessible (equality), phihip_build_cellflags of it (equality), phihip_apply_obstacles (in place, bound from project_ref.apply_obstacles).
    exact: the dyadic case -- sample positions ON surfaces, both sides exact, so no clearance is asked """
    x = make_inputs(res, bc, dtype, batch, kind, seed)
    if exact:      # dx = 1, lower = 0
        x.dom, x.grid = make_case(tuple(res), bc, dtype, batch, bc_val=x.bcv)
        x.dx = x.dom.dx
    D = len(res)
    lower = (0.0,) * D
    if kind == "nonfinite":      # NaN and Inf where the first obstacle's mask is exactly 1: safe_mul makes them 0, a moving obstacle then adds its velocity
        planted = 0
        for d in range(D):
            inside = np.argwhere(np.broadcast_to(obstacles[0].sdf(R.face_points(d, x.res, x.bc, lower, x.dx)) <= 0, x.v[d].shape[1:]))
            for i, bad in zip(inside[:3], (np.nan, np.inf, -np.inf)):
                x.v[d][(slice(None),) + tuple(i)] = bad
                planted += 1
        assert planted, f"{what}: no sample inside the first obstacle"
    if not exact:
        c = R.surface_clearance(obstacles, x.res, x.bc, lower, x.dx)
        assert c > CLEARANCE, f"{what}: a sample lies {c:.2e} cells from a surface"
    oracle_obs = [to_oracle(ob) for ob in obstacles]
    items = obstacle_items(oracle_obs, D)
    arr = C.make_obstacles(items)
    g1 = C.make_grid(D, x.grid.dtype, 1, x.res, x.dom.lower, x.dom.upper, x.bc, x.bcv)
    dacc = empty(mem, x.res, np.uint8)
    ctx.obstacle_accessible(g1, arr, len(items), mem.ptr(dacc))
    mem.sync()
    acc = R.accessible(obstacles, x.res, lower, x.dx)
    active_o, _, _ = O.obstacle_masks(oracle_obs, x.dom, np.float64)
    differ = int((acc != (active_o[0] > 0).astype(np.uint8)).sum())
    # (exact: the oracle, like the reference project, takes its positions from linspace and is an ulp off the half-integers: it is no yardstick ON a surface)
    assert exact or differ == 0, f"{what}: the restatement's accessible mask differs from the oracle's in {differ} cells"
    got = mem.to_host(dacc)
    assert np.array_equal(got, acc), f"obstacle_accessible [{what}] res {res}: differs at {np.argwhere(got != acc)[:4].tolist()}"
    dfl = empty(mem, x.res, np.uint8)
    ctx.build_cellflags(g1, mem.ptr(dacc), 0, 1, mem.ptr(dfl))
    mem.sync()
    assert np.array_equal(mem.to_host(dfl), R.cell_flags(acc, None, x.res, x.bc, False)), f"build_cellflags of the accessible mask [{what}]"
    RECORDS.append(dict(entry="obstacle_accessible", path=what, dtype="uint8", res="x".join(map(str, x.res)), ratio=0.0, inside=int((acc == 0).sum()), oracle_differs=differ))
    v64 = _to64(x.v)
    with np.errstate(invalid='ignore', over='ignore'):
        ref, E, G = R.apply_obstacles(v64, obstacles, x.res, x.bc, lower, x.dx)
        o64 = O.apply_boundary_conditions(v64, oracle_obs, x.dom)
        r32 = R.apply_obstacles(x.v, obstacles, x.res, x.bc, lower, x.dx, dtype)[0]
        o32 = O.apply_boundary_conditions(x.v, oracle_obs, x.dom)
    dv = [to_dev(mem, a) for a in x.v]
    ctx.apply_obstacles(x.grid, arr, len(items), _P(mem, dv))
    mem.sync()
    eps = eps_of(dtype)
    for d in range(D):
        scale = np.abs(ref[d]) + E[d]
        if kind != "nonfinite" and not exact:
            pin(ref[d], o64[d], scale, f"apply_boundary_conditions[{d}]")
        nonfin = kind == "nonfinite"
        compare(f"apply_obstacles[{d}]", what, x, kind, mem.to_host(dv[d]), ref[d], eps * E[d] + EPS64 * (K_REF * scale + K_GEO * G[d]), None if nonfin else o32[d], None if nonfin else r32[d],
                tol(dtype)['stencil'])


def dyadic_obstacles(res):
    """ dx = 1, lower = 0: cell centres at half-integers. Box bounds at half-integers and a sphere of radius 2 about a cell centre put centres exactly ON the
    surfaces: lies_inside is inclusive, and every quantity is exact in float64 on both sides """
    D = len(res)
    box = R.Box(tuple(1.5 for _ in res), tuple(min(n - 1.5, 4.5) for n in res))
    centre = tuple(float(min(n - 3, 6)) + 0.5 for n in res)
    return [box, R.Sphere(centre, 2.0)]


# ---- one case, every entry point -----------------------------------------------------------------------------------------------------------------------------------
MODES = ("none", "shared", "per")


def run_stencils(ctx, mem, res, bc, dtype, batch, kinds=("random", "graded", "tiny", "nonfinite"), seed=0, offset=0, entries=("divergence", "grad_subtract", "laplace_apply",
                 "centered_to_staggered", "diffuse_explicit")):
    """ the projection stencils on one grid: every input kind, flags absent / shared / per entry; prints the figures of the case (also when a check fails) """
    del RECORDS[:]
    try:
        for kind in tuple(kinds) + (("graded slow",) if len(res) == 3 and "graded" in kinds else ()):
            for mode in MODES:
                if "divergence" in entries:
                    check_divergence(ctx, mem, res, bc, dtype, batch, kind, mode, seed, offset)
                if "grad_subtract" in entries:
                    check_grad_subtract(ctx, mem, res, bc, dtype, batch, kind, mode, seed + 1, offset)
                if "laplace_apply" in entries and kind != "nonfinite":
                    check_laplace(ctx, mem, res, bc, dtype, batch, kind, mode, seed + 2, offset)
            if kind == "nonfinite":
                continue
            if "centered_to_staggered" in entries:
                check_centered_to_staggered(ctx, mem, res, bc, dtype, batch, kind, seed + 3, offset, rotations=range(4) if kind == "random" else (1,))
            if "diffuse_explicit" in entries and not offset:
                check_diffuse_explicit(ctx, mem, res, bc, dtype, batch, kind, seed + 4)
        if "divergence" in entries and batch > 1:
            check_divergence(ctx, mem, res, bc, dtype, batch, "random", "per", seed + 5, all_inactive=True)
    finally:
        report()


def run_obstacles(ctx, mem, res, bc, dtype, batch, seed=0, scenes=SCENES):
    del RECORDS[:]
    try:
        dx = make_inputs(res, bc, dtype, batch, "random", seed).dx
        for k, name in enumerate(scenes):
            check_obstacles(ctx, mem, res, bc, dtype, batch, pick_scene(name, res, bc, dx, seed + k), "random", seed + k, what=name)
            if name in ("box", "rotated box", "sphere"):      # stationary: NaN under a mask of 1 becomes 0; moving and rotating: the obstacle's velocity
                check_obstacles(ctx, mem, res, bc, dtype, batch, pick_scene(name, res, bc, dx, seed + k), "nonfinite", seed + k, what=name)
            if name == "box":
                check_obstacles(ctx, mem, res, bc, dtype, batch, pick_scene(name, res, bc, dx, seed + k), "graded", seed + k, what=name)
        if res[-1] > 64:
            check_obstacles(ctx, mem, res, bc, dtype, batch, pick_scene("margin", res, bc, dx, seed), "random", seed, what="margin")
        check_obstacles(ctx, mem, res, bc, dtype, batch, dyadic_obstacles(res), "random", seed, exact=True, what="dyadic")
    finally:
        report()


# ---- canary: NumPy only, no kernel ---------------------------------------------------------------------------------------------------------------------------------
def canary_scaled_tap(entry, res, bc, factor=4e-6, seed=0):
    """ the float32 reference with ONE tap's weight scaled by 1 + factor: (share of samples the old rule flags, worst error / new bound) """
    x = make_inputs(res, bc, np.float32, 2, "random", seed)
    D = len(res)
    T = np.float32
    if entry == "divergence":
        ref, S = R.divergence(_to64(x.v), x.res, x.bc, x.bcv, x.dx)
        val = R.divergence(x.v, x.res, x.bc, x.bcv, x.dx, T)[0]
        f = R.all_faces(x.v[D - 1], D - 1, x.res, x.bc, x.bcv.astype(T))
        tap = R._two(f, D, x.res[D - 1], 0)[1] * T(1.0 / x.dx[D - 1])          # the upper face of the fast axis
        bad = val + T(factor) * tap
        o32, K = O.divergence(x.v, x.dom), K_DIV[D]
    else:
        ref, S = R.masked_laplace(x.p.astype(np.float64), x.res, x.bc, x.dx)
        val = R.masked_laplace(x.p, x.res, x.bc, x.dx, dtype=T)[0]
        hi = np.roll(x.p, -1, axis=D) if x.bc[D - 1][0] == PER else np.concatenate([x.p[..., 1:], np.zeros_like(x.p[..., :1])], axis=-1)
        bad = val + T(factor) * (hi * T(1.0 / (x.dx[D - 1] ** 2)))
        o32, K = O.masked_laplace(x.p, x.dom), K_LAP_FLUX[D]
    old = np.abs(bad.astype(np.float64) - o32) > tol(T)['stencil'] * np.abs(o32).max()
    new = np.abs(bad.astype(np.float64) - ref) / ((K * eps_of(T) + K_REF * EPS64) * S)
    clean = np.abs(val.astype(np.float64) - ref) / ((K * eps_of(T) + K_REF * EPS64) * S)
    return float(old.mean()), float(new.max()), float(clean.max())


def canary_swapped_wall(res, bc, seed=0):
    """ the float32 divergence with the wall constants of the two sides of the fast axis exchanged, `tiny` input: (the old rule's figure max |err| / max |oracle|,
    worst error / new bound) """
    x = make_inputs(res, bc, np.float32, 2, "tiny", seed)
    D = len(res)
    ref, S = R.divergence(_to64(x.v), x.res, x.bc, x.bcv, x.dx)
    swapped = x.bcv.copy()
    swapped[D - 1, 0], swapped[D - 1, 1] = x.bcv[D - 1, 1], x.bcv[D - 1, 0]
    bad = R.divergence(x.v, x.res, x.bc, swapped, x.dx, np.float32)[0].astype(np.float64)
    o32 = O.divergence(x.v, x.dom)
    return float(np.abs(bad - o32).max() / np.abs(o32).max()), float((np.abs(bad - ref) / ((K_DIV[D] * eps_of(np.float32) + K_REF * EPS64) * S)).max())


# ---- case tables ---------------------------------------------------------------------------------------------------------------------------------------------------
# rows and vectors: n2 in {4, 8, 64, 68, 70, 72, 130, 131, 134} x n1 in {3, 4, 5, 9} x n0 in {1, 3, 7}; every side kind on every internal axis (a0, a1, a2);
# whole vectors between two CLOSED sides (full2 == false), behind an OPEN upper side (the extra face), ragged rows, fp64 V = 2 whole where fp32 is ragged (70, 130, 134)
ROW_CASES = [
    ((3, 4, 4), ((PER, PER), (CLO, OPN), (CLO, CLO)), 2), ((7, 5, 8), ((CLO, CLO), (PER, PER), (OPN, OPN)), 3), ((1, 9, 64), ((PER, PER), (OPN, CLO), (CLO, OPN)), 2),
    ((3, 3, 68), ((OPN, OPN), (CLO, CLO), (PER, PER)), 1), ((7, 4, 70), ((CLO, OPN), (OPN, OPN), (OPN, CLO)), 2), ((3, 5, 72), ((OPN, CLO), (PER, PER), (CLO, CLO)), 3),
    ((1, 9, 130), ((OPN, OPN), (CLO, OPN), (PER, PER)), 2), ((3, 4, 131), ((CLO, CLO), (OPN, CLO), (OPN, OPN)), 1), ((7, 3, 134), ((PER, PER), (CLO, CLO), (CLO, OPN)), 2),
    ((9, 8), ((CLO, OPN), (PER, PER)), 3), ((5, 64), ((PER, PER), (CLO, CLO)), 2), ((4, 70), ((OPN, CLO), (OPN, OPN)), 1), ((3, 131), ((CLO, CLO), (OPN, CLO)), 2),
    ((9, 72), ((OPN, OPN), (CLO, OPN)), 2), ((5, 8), ((CLO, CLO), (OPN, CLO)), 2), ((3, 9, 64), ((PER, PER), (OPN, OPN), (OPN, CLO)), 1),
]
# the scalar kernels on whole-vector rows: the n2 in {8, 64, 72} grids with unaligned buffers
UNALIGNED_CASES = [c for c in ROW_CASES if c[0][-1] in (8, 64, 72)]
# MODE_APPLY plans: (res, bc, dtype name)
LAPLACE_PLAN_CASES = [((5, 9, n2), bc, "f32") for n2, bc in ((64, ((CLO, OPN), (PER, PER), (CLO, CLO))), (66, ((PER, PER), (OPN, CLO), (OPN, OPN))),
                                                              (70, ((OPN, OPN), (CLO, CLO), (PER, PER))), (131, ((CLO, CLO), (OPN, OPN), (CLO, OPN))),
                                                              (7, ((PER, PER), (CLO, OPN), (OPN, CLO))), (257, ((OPN, CLO), (PER, PER), (CLO, CLO))),
                                                              (260, ((CLO, OPN), (OPN, OPN), (PER, PER))))]
LAPLACE_PLAN_CASES += [((5, 9, n2), bc, "f64") for n2, bc in ((64, ((CLO, CLO), (PER, PER), (OPN, CLO))), (67, ((PER, PER), (CLO, OPN), (CLO, CLO))),
                                                               (129, ((OPN, OPN), (OPN, CLO), (PER, PER))), (130, ((CLO, OPN), (CLO, CLO), (OPN, OPN))),
                                                               (258, ((OPN, CLO), (PER, PER), (CLO, OPN))))]
LAPLACE_PLAN_CASES += [((5, 260), ((CLO, OPN), (PER, PER)), "f32"), ((9, 64), ((PER, PER), (CLO, CLO)), "f32"), ((9, 258), ((OPN, OPN), (CLO, OPN)), "f64"),
                       ((1, 5, 66), ((PER, PER), (CLO, CLO), (OPN, CLO)), "f32")]
# MI355X only (the emulation needs more than 10 s): several planes per workgroup, the second trip of the patch loop and of the balance loops
DEVICE_DIVERGENCE_CASES = [((4099, 3, 5), ((PER, PER), (CLO, OPN), (OPN, CLO)), 1), ((4099, 3, 5), ((CLO, OPN), (PER, PER), (CLO, CLO)), 1),
                           ((4099, 2, 8), ((PER, PER), (OPN, OPN), (CLO, CLO)), 1), ((4099, 2, 8), ((CLO, OPN), (CLO, CLO), (PER, PER)), 1)]
DEVICE_GRAD_CASES = [((16400, 3, 8), ((CLO, OPN), (PER, PER), (OPN, OPN)), 1), ((16400, 3, 5), ((PER, PER), (CLO, CLO), (CLO, OPN)), 1)]
DEVICE_BALANCE_CASE = ((130, 130, 130), ((CLO, CLO), (PER, PER), (CLO, CLO)), 1)
