"""
Element-wise parity of the adjoint kernels (phiflow_amd/csrc/adjoint.hip and the adjoint forms of the diffusion kernels), in fp32 and fp64,
driven through the C ABI like tests/parity_cases.py. Used by tests/test_adjoint_elementwise_emu.py (emulation) and
tests/test_gpu_adjoint_elementwise.py (MI355X).

Yardstick: tests/adjoint_ref.py -- the oracle's forward functions restated in torch float64 and differentiated by torch.autograd. Every check
  * PINS the restatement: its forward equals the oracle's float64 forward on the case's inputs to 1e-12 of the largest element;
  * compares every gradient array ELEMENT BY ELEMENT: |kernel - reference| <= tol * scale with
        scale = max(max|ref|, max|g| max|field| max(1, dt / dx))          per output array
    (so a reference that is identically zero -- the velocity gradient along a periodic axis of one cell -- is compared with rounding noise sensibly),
        tol   = 1e-12 (TOL64['advect']) for the fp64 kernels, advect_tol(float32, dom) for the fp32 kernels: the project's own bound; its
                derivation (pass A forms absolute index coordinates in the element type: n eps / 2) applies unchanged;
  * fp32: the inputs are rounded to fp32 first and the float64 reference evaluates those numbers (truth_check's convention); the error of the
    same reference evaluated in float32 is recorded next to the kernel's (RECORDS), not asserted.
Undecided samples are handled in the INPUTS:
  * lookup kinks: no sample is excluded. fp32 cases build their velocities (`banded_velocity`) so that every lookup coordinate of the reference
    stays >= 4 n_max eps(T) cells from an integer -- asserted --, i.e. four times the coordinate rounding: kernel and reference take the same taps.
    fp64 cases use plain random inputs with a margin of 1e-9 asserted.
  * limiter switches and ties of the extremal tap (MacCormack): a sample whose reference margin is below 64 eps(T) max|field| gets its upstream
    cotangent set to zero for the kernel and the reference alike (its limiter branch enters the result only multiplied by its own cotangent);
    the share of such samples is asserted to be <= 1 %.
"""
import numpy as np
import torch

import adjoint_ref as R
import diffuse_coef_ref
from parity_cases import CLO, OPN, PER, TOL32, TOL64, C, O, advect_tol, make_case

RECORDS = []          # one dict per compared entry point: printed by `report()`, the source of the table in DESIGN.md


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def coord_margin_needed(dtype, dom):
    return 1e-9 if np.dtype(dtype) == np.float64 else 4.0 * max(dom.res) * eps_of(np.float32)


def elem_tol(dtype, dom):
    return TOL64['advect'] if np.dtype(dtype) == np.float64 else advect_tol(np.float32, dom)


def report():
    for r in RECORDS:
        print("adjoint-elementwise", " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in r.items()), flush=True)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------------
def _band(comp):
    return (0.05, 0.45) if comp % 2 == 0 else (0.55, 0.95)


def make_inputs(res, bc, dtype, batch, dt, seed, k0=0, slab_axis=None, extent=None):
    """ domain, grid struct and a velocity for an adjoint case.
    fp64: random normal velocity and random wall values on the closed sides.
    fp32: every value of component a -- stored samples and wall values -- is dx_a / dt (k + r), r uniform in the component's band ([0.05, 0.45] or
    [0.55, 0.95]), k = k0, or k0 + 4 in the upper half of the domain along `slab_axis`. Two- and four-point means of such values are an integer
    plus a number in the band (k differs by multiples of 4), and so is the limiter's half-cell shift: every lookup coordinate stays 0.05 cells from
    an integer. k = 0 / -1: displacements below one cell (gather form); k0 + 4: samples that left their neighbourhood (atomic fallback); a slab
    boundary puts both into one launch. """
    D = len(res)
    rng = np.random.default_rng(seed)
    upper = tuple(float(e) for e in extent) if extent else None
    dom0 = O.Domain(res, (0.0,) * D, upper or tuple(float(n) for n in res), bc)
    f32 = np.dtype(dtype) == np.float32
    bcv = np.zeros((D, 2, D))
    for a in range(D):
        for s in range(2):
            for c in range(D):
                if bc[a][s] == CLO:
                    bcv[a][s][c] = dom0.dx[c] / dt * (k0 + rng.uniform(*_band(c))) if f32 else 0.3 * rng.standard_normal()
    if f32:
        bcv = bcv.astype(np.float32).astype(np.float64)
    dom, grid = make_case(tuple(res), bc, dtype, batch, upper=upper, bc_val=bcv)
    v = []
    for c in range(D):
        shape = (batch,) + dom.comp_shape(c)
        if f32:
            k = np.full(shape, float(k0))
            if slab_axis is not None:
                sl = [slice(None)] * (D + 1)
                sl[slab_axis + 1] = slice(shape[slab_axis + 1] // 2, None)
                k[tuple(sl)] += 4.0
            v.append((dom.dx[c] / dt * (k + rng.uniform(*_band(c), size=shape))).astype(np.float32))
        else:
            v.append(rng.standard_normal(shape))
    return dom, grid, v, rng


def scalar_rule(bc, rng, dtype, flip=False):
    """ a scalar's boundary rule on the grid's axes: periodic where the grid is; elsewhere (CLO, OPN) / (OPN, CLO) / ... by the velocity's own
    sides (or swapped: a constant side below an open wall), with non-zero constants on both sides """
    codes = tuple((PER, PER) if lo == PER else ((hi, lo) if flip else (lo, hi)) for lo, hi in bc)
    consts = [(float(np.float32(rng.normal())), float(np.float32(0.25 + rng.normal()))) for _ in bc]
    return codes, consts


def random_like(arrays, rng, dtype):
    return [rng.standard_normal(a.shape).astype(dtype) for a in arrays]


def _amax(arrays):
    return max([float(np.abs(a).max()) for a in arrays if a.size] + [0.0])


def _t64(arrays, grad=False):
    return [R.tensor(a, torch.float64, grad) for a in arrays]


def _t32(arrays, grad=False):
    return [R.tensor(a, torch.float32, grad) for a in arrays]


# ---- comparison --------------------------------------------------------------------------------------------------------------------------------------------
def compare(entry, dtype, dom, got, ref, ref32, floor, margins=None, zeroed=0.0, tol=None):
    """ element-wise comparison of the gradient arrays `got` with the float64 reference `ref`; `floor` = max|g| max|field| max(1, dt / dx) """
    tol = elem_tol(dtype, dom) if tol is None else tol
    worst = worst32 = 0.0
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape, (entry, k, a.shape, b.shape)
        if not b.size:
            continue
        scale = max(float(np.abs(b).max()), floor)
        assert np.isfinite(a).all(), f"{entry} [{k}]: non-finite gradient"
        diff = np.abs(a.astype(np.float64) - b)
        err = float(diff.max()) / scale
        worst = max(worst, err)
        if ref32 is not None:
            worst32 = max(worst32, float(np.abs(ref32[k].astype(np.float64) - b).max()) / scale)
        if err > tol:
            where = np.unravel_index(int(diff.argmax()), diff.shape)
            raise AssertionError(f"{entry} {np.dtype(dtype).name} res {dom.res} bc {dom.bc}: gradient array {k} differs at {where}: kernel {a[where]!r} vs "
                                 f"reference {b[where]!r} ({err:.3e} of the scale {scale:.3e}; bound {tol:.3e}; {int((diff > tol * scale).sum())} elements beyond it)")
    rec = dict(entry=entry, dtype=np.dtype(dtype).name, res="x".join(str(n) for n in dom.res), err=worst)
    if ref32 is not None:
        rec.update(err_ref32=worst32, ratio=worst / max(worst32, 1e-300))
    if margins is not None:
        rec.update(margin=margins.coord)
    rec.update(zeroed=float(zeroed))
    RECORDS.append(rec)
    return worst


def _assert_margin(margins, dtype, dom, what):
    need = coord_margin_needed(dtype, dom)
    assert margins.coord >= need, f"{what}: a lookup coordinate of the reference is {margins.coord:.3e} cells from an integer (needed: {need:.3e})"


def _zero_undecided(g_list, margins, fields, dtype, what):
    """ cotangents with the undecided samples of the limiter set to zero; returns (cotangents, share of zeroed samples) """
    thr = 64.0 * eps_of(dtype) * _amax(fields)
    out, n_zero, n_all = [], 0, 0
    for g, m in zip(g_list, margins.limiter):
        bad = m.numpy() < thr
        n_zero += int(bad.sum()); n_all += bad.size
        g = g.copy()
        g[bad] = 0
        out.append(g)
    return out, n_zero / max(n_all, 1)


SEED_TRIES = 6      # MacCormack cases: the first of seed, seed + 1000, ... for which the REFERENCE ALONE leaves <= 1 % of the samples undecided (on grids of
                    # a few cells one sample whose limiter window is a single constant -- new == lo == hi exactly -- is already 10 %)


def _P(mem, hs):
    return None if hs is None else [mem.ptr(h) for h in hs]


def _dev(mem, arrays):
    return [mem.to_dev(a) for a in arrays]


def _zeros(mem, arrays):
    return [mem.to_dev(np.zeros_like(a)) for a in arrays]


def _host(mem, hs):
    return [mem.to_host(h) for h in hs]


def _floor(g, f, dt, dom):
    return _amax(g) * _amax(f) * max(1.0, abs(dt) / min(dom.dx))


# ---- staggered advection (semi-Lagrangian and MacCormack) ---------------------------------------------------------------------------------------------
def _staggered(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis, extent, forms, mac, strength=1.0):
    name = "mac_cormack_staggered_backward" if mac else "advect_staggered_backward"
    f32 = np.dtype(dtype) == np.float32
    for form in forms:
        for attempt in range(SEED_TRIES if mac else 1):
            share = _staggered_form(ctx, mem, res, bc, dtype, batch, dt, seed + 1000 * attempt, k0, slab_axis, extent, form, mac, strength, name, f32,
                                    last=attempt == SEED_TRIES - 1)
            if share is not None:
                break


def _staggered_form(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis, extent, form, mac, strength, name, f32, last):
    """ one form on one seed; returns None (nothing ran) if the reference leaves more than 1 % of the samples undecided and another seed may be tried """
    dom, grid, v, rng = make_inputs(res, bc, dtype, batch, dt, seed, k0, slab_axis, extent)
    f_other = random_like(v, rng, dtype)
    g0 = random_like(v, rng, dtype)
    dv = _dev(mem, v)
    fwd_ref = (lambda f, u, m=None: R.mac_cormack_staggered(f, u, dt, dom, strength, m)) if mac else (lambda f, u, m=None: R.semi_lagrangian_staggered(f, u, dt, dom, m))
    fwd_orc = (lambda f, u: O.mac_cormack_staggered(f, u, dt, dom, strength)) if mac else (lambda f, u: O.semi_lagrangian_staggered(f, u, dt, dom))
    self_adv = form == 'self'
    f = v if self_adv else f_other
    what = f"{name}[{form}]"
    # the reference's forward: pin, margins, undecided samples
    m = R.Margins()
    with torch.no_grad():
        out = fwd_ref(_t64(f), _t64(v), m)
    R.pin(out, fwd_orc([a.astype(np.float64) for a in f], [a.astype(np.float64) for a in v]), what)
    _assert_margin(m, dtype, dom, what)
    g, share = _zero_undecided(g0, m, f, dtype, what) if mac else (g0, 0.0)
    if share > 0.01 and not last:
        return None
    assert share <= 0.01, f"{what}: {share:.2%} of the samples sit within 64 eps max|field| of a limiter switch (seeds {seed % 1000} + 1000 k tried)"
    # the reference's gradients
    def grads(T):
        if self_adv:
            x = T(v, True)
            return R.vjp(fwd_ref(x, x), T(g), x)
        xf, xv = T(f, True), T(v, True)
        gr = R.vjp(fwd_ref(xf, xv), T(g), xf + xv)
        return gr[:len(f)], gr[len(f):]
    ref, ref32 = grads(_t64), (grads(_t32) if f32 else None)
    # the kernels
    df, dg = (dv if self_adv else _dev(mem, f)), _dev(mem, g)
    want_f, want_v = form != 'gf_none', form != 'gv_none'
    assert want_f or not mac, "the MacCormack adjoint always returns the field gradient"
    gf, gv = (_zeros(mem, v) if want_f else None), (_zeros(mem, v) if want_v else None)
    if mac:
        ctx.mac_cormack_staggered_backward(grid, _P(mem, df), _P(mem, dv), _P(mem, dg), dt, strength, _P(mem, gf), _P(mem, gv))
    else:
        ctx.advect_staggered_backward(grid, _P(mem, df), _P(mem, dv), _P(mem, dg), dt, _P(mem, gf), _P(mem, gv))
    mem.sync()
    floor = _floor(g, f, dt, dom)
    if self_adv:
        got = [a.astype(np.float64) + b.astype(np.float64) for a, b in zip(_host(mem, gf), _host(mem, gv))]
        compare(what, dtype, dom, got, ref, ref32, floor, m, share)
    else:
        if want_f:
            compare(what + ".field", dtype, dom, _host(mem, gf), ref[0], ref32[0] if f32 else None, floor, m, share)
        if want_v:
            compare(what + ".velocity", dtype, dom, _host(mem, gv), ref[1], ref32[1] if f32 else None, floor, m, share)
    return share


def check_advect_staggered(ctx, mem, res, bc, dtype, batch=2, dt=0.7, seed=0, k0=0, slab_axis=None, extent=None,
                           forms=('self', 'both', 'gv_none', 'gf_none')):
    _staggered(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis, extent, forms, mac=False)


def check_mac_cormack_staggered(ctx, mem, res, bc, dtype, batch=2, dt=0.7, seed=0, k0=0, slab_axis=None, extent=None, forms=('self', 'both', 'gv_none'),
                                strength=1.0):
    _staggered(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis, extent, forms, mac=True, strength=strength)


# ---- centred scalar advected by the staggered velocity ---------------------------------------------------------------------------------------------------------
def _centered(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis, extent, flip, mac, strength):
    for attempt in range(SEED_TRIES if mac else 1):
        if _centered_seed(ctx, mem, res, bc, dtype, batch, dt, seed + 1000 * attempt, k0, slab_axis, extent, flip, mac, strength, attempt == SEED_TRIES - 1) is not None:
            break


def _centered_seed(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis, extent, flip, mac, strength, last):
    dom, grid, v, rng = make_inputs(res, bc, dtype, batch, dt, seed, k0, slab_axis, extent)
    s_codes, s_consts = scalar_rule(bc, rng, dtype, flip)
    what = "mac_cormack_centered_backward" if mac else "advect_centered_backward"
    f32 = np.dtype(dtype) == np.float32
    s = rng.standard_normal((batch,) + dom.res).astype(dtype)
    g = rng.standard_normal((batch,) + dom.res).astype(dtype)
    fwd_ref = (lambda x, u, m=None: R.mac_cormack_centered(x, u, dt, dom, s_codes, s_consts, strength, m)) if mac else \
              (lambda x, u, m=None: R.semi_lagrangian_centered(x, u, dt, dom, s_codes, s_consts, m))
    m = R.Margins()
    with torch.no_grad():
        out = fwd_ref(R.tensor(s), _t64(v), m)
    s64, v64 = s.astype(np.float64), [a.astype(np.float64) for a in v]
    R.pin(out, O.mac_cormack_centered(s64, v64, dt, dom, s_codes, s_consts, strength) if mac else O.semi_lagrangian_centered(s64, v64, dt, dom, s_codes, s_consts), what)
    _assert_margin(m, dtype, dom, what)
    share = 0.0
    if mac:
        (g,), share = _zero_undecided([g], m, [s, np.asarray(s_consts)], dtype, what)
        if share > 0.01 and not last:
            return None
        assert share <= 0.01, f"{what}: {share:.2%} of the samples sit within 64 eps max|field| of a limiter switch (seeds {seed % 1000} + 1000 k tried)"

    def grads(T):
        xs, xv = T([s], True)[0], T(v, True)
        return R.vjp(fwd_ref(xs, xv), T([g]), [xs] + xv)
    ref, ref32 = grads(_t64), (grads(_t32) if f32 else None)
    ds, dv, dg = mem.to_dev(s), _dev(mem, v), mem.to_dev(g)
    gs, gv = mem.to_dev(np.zeros_like(s)), _zeros(mem, v)
    if mac:
        ctx.mac_cormack_centered_backward(grid, mem.ptr(ds), s_codes, s_consts, _P(mem, dv), mem.ptr(dg), dt, strength, mem.ptr(gs), _P(mem, gv))
    else:
        ctx.advect_centered_backward(grid, mem.ptr(ds), s_codes, s_consts, _P(mem, dv), mem.ptr(dg), dt, mem.ptr(gs), _P(mem, gv))
    mem.sync()
    floor = _floor([g], [s, np.asarray(s_consts)], dt, dom)
    compare(what, dtype, dom, [mem.to_host(gs)] + _host(mem, gv), ref, ref32, floor, m, share)
    return share


def check_advect_centered(ctx, mem, res, bc, dtype, batch=2, dt=0.7, seed=0, k0=0, slab_axis=None, extent=None, flip=False):
    _centered(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis, extent, flip, False, 1.0)


def check_mac_cormack_centered(ctx, mem, res, bc, dtype, batch=2, dt=0.7, seed=0, k0=0, slab_axis=None, extent=None, flip=False, strength=0.8):
    _centered(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis, extent, flip, True, strength)


# ---- linear maps: centred -> staggered, explicit diffusion ---------------------------------------------------------------------------------------------------------
def check_centered_to_staggered(ctx, mem, res, bc, dtype, batch=2, seed=0, flip=False):
    dom, grid, v, rng = make_inputs(res, bc, dtype, batch, 1.0, seed)
    s_codes, s_consts = scalar_rule(bc, rng, dtype, flip)
    D = dom.rank
    vector = [0.3, -1.5, 0.1][:D]
    f32 = np.dtype(dtype) == np.float32
    s = rng.standard_normal((batch,) + dom.res).astype(dtype)
    g = random_like(v, rng, dtype)
    with torch.no_grad():
        out = R.centered_to_staggered(R.tensor(s), dom, s_codes, s_consts, vector)
    R.pin(out, O.centered_to_staggered(s.astype(np.float64), dom, s_codes, s_consts, vector), "centered_to_staggered")

    def grads(T):
        x = T([s], True)[0]
        return R.vjp(R.centered_to_staggered(x, dom, s_codes, s_consts, vector), T(g), [x])
    ref, ref32 = grads(_t64), (grads(_t32) if f32 else None)
    gs, dg = mem.to_dev(np.zeros_like(s)), _dev(mem, g)
    ctx.centered_to_staggered_backward(grid, s_codes, vector, _P(mem, dg), mem.ptr(gs))
    mem.sync()
    compare("centered_to_staggered_backward", dtype, dom, [mem.to_host(gs)], ref, ref32, _amax(g) * max(abs(x) for x in vector))


def check_diffuse(ctx, mem, res, bc, dtype, batch=2, seed=0, kdt=0.1, flip=False):
    """ diffuse_explicit_backward (staggered), diffuse_explicit_centered(adjoint=True), diffuse_explicit_centered_coef(adjoint=True) with a coefficient
    field and with per-axis factors """
    dom, grid, v, rng = make_inputs(res, bc, dtype, batch, 1.0, seed)
    s_codes, s_consts = scalar_rule(bc, rng, dtype, flip)
    D = dom.rank
    f32 = np.dtype(dtype) == np.float32
    to64 = lambda arrays: [a.astype(np.float64) for a in arrays]
    # staggered
    g = random_like(v, rng, dtype)
    with torch.no_grad():
        R.pin(R.diffuse_explicit(_t64(v), kdt, dom), O.diffuse_explicit(to64(v), kdt, 1.0, dom), "diffuse_explicit")

    def grads(T):
        x = T(v, True)
        return R.vjp(R.diffuse_explicit(x, kdt, dom), T(g), x)
    ref, ref32 = grads(_t64), (grads(_t32) if f32 else None)
    gin, dg = _zeros(mem, v), _dev(mem, g)
    ctx.diffuse_explicit_backward(grid, _P(mem, dg), _P(mem, gin), kdt)
    mem.sync()
    amp = max(1.0, 4 * D * kdt / min(dom.dx) ** 2)
    compare("diffuse_explicit_backward", dtype, dom, _host(mem, gin), ref, ref32, _amax(g) * amp)
    # centred, constant diffusivity
    s = rng.standard_normal((batch,) + dom.res).astype(dtype)
    gs = rng.standard_normal((batch,) + dom.res).astype(dtype)
    with torch.no_grad():
        R.pin(R.diffuse_explicit_centered(R.tensor(s), kdt, dom, s_codes, s_consts), O.diffuse_explicit_centered(s.astype(np.float64), kdt, 1.0, dom, s_codes, s_consts),
              "diffuse_explicit_centered")

    def grads_c(T):
        x = T([s], True)[0]
        return R.vjp(R.diffuse_explicit_centered(x, kdt, dom, s_codes, s_consts), T([gs]), [x])
    ref, ref32 = grads_c(_t64), (grads_c(_t32) if f32 else None)
    dgs, gin_s = mem.to_dev(gs), mem.to_dev(np.zeros_like(s))
    ctx.diffuse_explicit_centered(grid, mem.ptr(dgs), s_codes, s_consts, mem.ptr(gin_s), kdt, adjoint=True)
    mem.sync()
    compare("diffuse_explicit_centered(adjoint)", dtype, dom, [mem.to_host(gin_s)], ref, ref32, _amax([gs]) * amp)
    # centred, coefficient field (batch entry shared or per entry) and per-axis factors
    kd = [kdt * (1.0 + 0.5 * d) for d in range(D)]
    a_codes = tuple((PER, PER) if lo == PER else (OPN, CLO) for lo, _ in s_codes)
    a_vals = [(0.0, 0.75)] * D
    for label, cb in (("coef field", 1), ("coef field per entry", batch), ("per-axis factors", 0)):
        coef = (0.25 + rng.random((cb,) + dom.res)).astype(dtype) if cb else None
        c64 = None if coef is None else coef.astype(np.float64)
        with torch.no_grad():
            out = R.diffuse_explicit_centered_coef(R.tensor(s), None if coef is None else R.tensor(coef), kd, dom.dx, s_codes, s_consts, a_codes, a_vals)
        R.pin(out, diffuse_coef_ref.explicit(s.astype(np.float64), c64, kd, dom.dx, s_codes, s_consts, a_codes, a_vals), "diffuse_explicit_centered_coef")

        def grads_k(T):
            x = T([s], True)[0]
            a = None if coef is None else T([coef])[0]
            return R.vjp(R.diffuse_explicit_centered_coef(x, a, kd, dom.dx, s_codes, s_consts, a_codes, a_vals), T([gs]), [x])
        ref, ref32 = grads_k(_t64), (grads_k(_t32) if f32 else None)
        dcoef = mem.to_dev(coef) if coef is not None else None
        gin_s = mem.to_dev(np.zeros_like(s))
        ctx.diffuse_explicit_centered_coef(grid, mem.ptr(dgs), s_codes, s_consts, mem.ptr(dcoef) if coef is not None else 0, max(cb, 1), a_codes, a_vals, kd,
                                           mem.ptr(gin_s), adjoint=True)
        mem.sync()
        compare(f"diffuse_explicit_centered_coef(adjoint, {label})", dtype, dom, [mem.to_host(gin_s)], ref, ref32, _amax([gs]) * 1.5 * 1.5 * amp)


# ---- grid_sample ---------------------------------------------------------------------------------------------------------------------------------------------
def check_grid_sample(ctx, mem, shape, codes, dtype, batch=2, points=301, shared_values=False, seed=0, spread=2.5):
    """ phihip_grid_sample_backward: gradients of the values and of the coordinates. The coordinates are INPUTS (their split into integer and
    fraction is exact in any element type); fp32: integer + a number in [0.05, 0.95]; fp64: uniform over `spread` array lengths around the array """
    D = len(shape)
    rng = np.random.default_rng(seed)
    f32 = np.dtype(dtype) == np.float32
    consts = [(float(np.float32(rng.normal())), float(np.float32(rng.normal()))) for _ in shape]
    vb = 1 if shared_values else batch
    values = rng.standard_normal((vb,) + tuple(shape)).astype(dtype)
    if f32:
        coords = [(rng.integers(-int(spread * n) - 1, int((spread + 1) * n) + 1, (batch, points)) + rng.uniform(0.05, 0.95, (batch, points))).astype(dtype) for n in shape]
    else:
        coords = [((rng.random((batch, points)) * (2 * spread + 1) - spread) * n).astype(dtype) for n in shape]
    g = rng.standard_normal((batch, points)).astype(dtype)
    dom = O.Domain(shape, (0.0,) * D, (1.0,) * D, codes)
    bc_val = [[[consts[a][s], 0.0, 0.0] for s in range(2)] for a in range(D)]
    grid = C.make_grid(D, C.PHIHIP_F64 if not f32 else C.PHIHIP_F32, batch, shape, (0.0,) * D, (1.0,) * D, codes, bc_val)
    m = R.Margins()
    expand = lambda t: t.expand((batch,) + tuple(shape))
    with torch.no_grad():
        out = R.grid_sample(expand(R.tensor(values)), _t64(coords), codes, consts, m)
    R.pin(out, O.grid_sample(np.broadcast_to(values.astype(np.float64), (batch,) + tuple(shape)), [c.astype(np.float64) for c in coords], codes, consts), "grid_sample")
    need = 1e-9 if not f32 else 4.0 * (spread + 1) * max(shape) * eps_of(np.float32)
    assert m.coord >= need, f"grid_sample: a coordinate is {m.coord:.3e} from an integer (needed: {need:.3e})"

    def grads(T):
        xv, xc = T([values], True)[0], T(coords, True)
        return R.vjp(R.grid_sample(expand(xv), xc, codes, consts), T([g]), [xv] + xc)
    ref, ref32 = grads(_t64), (grads(_t32) if f32 else None)
    dvals, dc, dg = mem.to_dev(values), _dev(mem, coords), mem.to_dev(g)
    gv, gc = mem.to_dev(np.zeros_like(values)), _zeros(mem, coords)
    ctx.grid_sample_backward(grid, mem.ptr(dvals), vb, _P(mem, dc), points, mem.ptr(dg), mem.ptr(gv), _P(mem, gc))
    mem.sync()
    floor = _amax([g]) * max(_amax([values]), _amax([np.asarray(consts)]))
    compare("grid_sample_backward" + (" shared values" if shared_values else ""), dtype, dom, [mem.to_host(gv)] + _host(mem, gc), ref, ref32, floor, m)


# ---- the largest case: an extruded flow (GPU) -------------------------------------------------------------------------------------------------------------
def check_extruded_staggered(ctx, mem, n0, plane_res, dtype=np.float32, dt=0.7, seed=0):
    """ periodic staggered advection on (n0, *plane_res) with a 2-D field, velocity and cotangent repeated along axis 0 and zero velocity along it:
    every plane of the field gradient and of the in-plane velocity gradients equals the 2-D reference of that plane. (n0 = 256 with a 256 x 256
    plane is the one size where the launches reach their 65 536-block cap.) The arrays are built where the memory lives: no host copy. """
    bc2 = ((PER, PER), (PER, PER))
    dom2, _, v2, rng = make_inputs(plane_res, bc2, dtype, 1, dt, seed, k0=0, slab_axis=0)
    f2, g2 = random_like(v2, rng, dtype), random_like(v2, rng, dtype)
    res = (n0,) + tuple(plane_res)
    dom, grid = make_case(res, ((PER, PER),) * 3, dtype, 1)
    m = R.Margins()
    with torch.no_grad():
        out = R.semi_lagrangian_staggered(_t64(f2), _t64(v2), dt, dom2, m)
    R.pin(out, O.semi_lagrangian_staggered([a.astype(np.float64) for a in f2], [a.astype(np.float64) for a in v2], dt, dom2), "extruded plane")
    _assert_margin(m, dtype, dom, "extruded plane")
    xf, xv = _t64(f2, True), _t64(v2, True)
    gr = R.vjp(R.semi_lagrangian_staggered(xf, xv, dt, dom2), _t64(g2), xf + xv)
    ref_f, ref_v = gr[:2], gr[2:]
    zero_plane = np.zeros(plane_res, dtype)
    ext = lambda a: mem.extrude(a[0], n0)
    # component 0 (along the extrusion): field and cotangent zero, velocity zero; components 1, 2: the plane's components 0, 1
    df = [ext(zero_plane[None]), ext(f2[0]), ext(f2[1])]
    dv = [ext(zero_plane[None]), ext(v2[0]), ext(v2[1])]
    dg = [ext(zero_plane[None]), ext(g2[0]), ext(g2[1])]
    gf = [mem.extrude(zero_plane, n0) for _ in range(3)]
    gv = [mem.extrude(zero_plane, n0) for _ in range(3)]
    ctx.advect_staggered_backward(grid, _P(mem, df), _P(mem, dv), _P(mem, dg), dt, _P(mem, gf), _P(mem, gv))
    mem.sync()
    floor = _floor(g2, f2, dt, dom2)
    tol = elem_tol(dtype, dom)
    for c in (0, 1):
        for what, arr, ref in (("field", gf[c + 1], ref_f[c]), ("velocity", gv[c + 1], ref_v[c])):
            # every plane against the reference, in slabs of planes (no host copy of the whole array)
            worst = 0.0
            scale = max(float(np.abs(ref).max()), floor)
            for k0 in range(0, n0, 32):
                slab = mem.to_host(arr[:, k0:k0 + 32]).astype(np.float64)
                assert np.isfinite(slab).all()
                worst = max(worst, float(np.abs(slab - ref[:, None]).max()) / scale)
            RECORDS.append(dict(entry=f"advect_staggered_backward[extruded {n0}].{what}", dtype=np.dtype(dtype).name, res="x".join(map(str, res)), err=worst,
                                margin=m.coord, zeroed=0.0))
            assert worst <= tol, f"extruded {what} gradient [{c}]: {worst:.3e} of the scale (bound {tol:.3e})"


# ---- dense check of the projection's adjoint --------------------------------------------------------------------------------------------------------------------
def check_project_backward_dense(ctx, mem, res=(12, 10), bc=((CLO, CLO), (CLO, OPN)), obstacle=((5.0, 4.5), 2.2), seed=3):
    """ make_incompressible_backward (fp64) with an obstacle against the FULL Jacobian of the oracle's projection: the map is affine, so column j of
    the Jacobian is the difference of the oracle's projections of the unit vector e_j and of zero; its transpose applied to the cotangent is
    compared element by element (at most 700 unknowns). """
    from parity_cases import solve_params
    dtype = np.float64
    dom, grid = make_case(res, bc, dtype, batch=1)
    rng = np.random.default_rng(seed)
    D = dom.rank
    shapes = [(1,) + dom.comp_shape(d) for d in range(D)]
    sizes = [int(np.prod(s)) for s in shapes]
    assert sum(sizes) <= 700
    obstacles = [O.SphereObstacle(tuple(obstacle[0]), float(obstacle[1]))]
    active, hard, _ = O.obstacle_masks(obstacles, dom, dtype)
    assert 0 < int((active[0] > 0).sum()) < active[0].size, "the case needs solid and fluid cells"
    dacc, dflags = mem.to_dev((active[0] > 0).astype(np.uint8)), mem.empty(dom.res, np.uint8)
    ctx.build_cellflags(grid, mem.ptr(dacc), 0, 1, mem.ptr(dflags))
    balance = not dom.flexible()
    g_v = [rng.standard_normal(s) for s in shapes]
    g_p = rng.standard_normal((1,) + dom.res) * active
    if balance:
        g_p = g_p - active * (g_p.sum() / active.sum())
    dgv, dgp = _dev(mem, g_v), mem.to_dev(g_p)
    ctx.make_incompressible_backward(grid, mem.ptr(dflags), 1, balance, _P(mem, dgv), mem.ptr(dgp), solve_params(dtype, rtol=1e-13))
    mem.sync()
    got = np.concatenate([a.ravel() for a in _host(mem, dgv)])

    def forward(vel):
        div = O.divergence(vel, dom) * active
        rhs = O.balance_divergence(div, active) if balance else div
        p, _ = O.cg(lambda q: O.masked_laplace(q, dom, hard, active), rhs, np.zeros_like(rhs), 1e-14, 0.0, 4000, 50)
        return O.gradient_subtract(vel, p, dom, hard), p
    zero = [np.zeros(s) for s in shapes]
    v0, p0 = forward(zero)
    ref = np.zeros(sum(sizes))
    j = 0
    for d in range(D):
        for i in range(sizes[d]):
            e = [np.zeros(s) for s in shapes]
            e[d].reshape(-1)[i] = 1.0
            v1, p1 = forward(e)
            ref[j] = sum(float(np.vdot(g, a - b)) for g, a, b in zip(g_v, v1, v0)) + float(np.vdot(g_p, p1 - p0))
            j += 1
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max()) / scale
    RECORDS.append(dict(entry="make_incompressible_backward[dense, obstacle]", dtype="float64", res="x".join(map(str, res)), err=err, zeroed=0.0))
    # both sides solve to a relative residual of 1e-13 .. 1e-14; the solution's error is that times the condition number (~ n^2): the bound of the
    # projected check_project_backward (1e-7), element by element
    assert err <= 1e-7, f"make_incompressible_backward: element {int(np.abs(got - ref).argmax())} differs by {err:.3e} of the largest element"


# ---- case tables -----------------------------------------------------------------------------------------------------------------------------------------------
P2, P3 = ((PER, PER),) * 2, ((PER, PER),) * 3
MIX2 = [((CLO, CLO), (OPN, OPN)), ((CLO, OPN), (OPN, CLO)), ((PER, PER), (CLO, OPN)), ((OPN, CLO), (PER, PER))]
MIX3 = [((CLO, CLO), (OPN, OPN), (PER, PER)), ((CLO, OPN), (OPN, CLO), (CLO, CLO)), ((PER, PER), (OPN, OPN), (OPN, CLO)), ((OPN, CLO), (PER, PER), (CLO, OPN))]

# (res, bc, batch, dt, k0, slab_axis): pass B tiles are 8 x 32 in-plane and 2 (fp64) / 4 (fp32) planes deep: extents one below, at and one above a multiple
# of the tile; (9, 17, 66), (12, 24, 64), (13, 25, 97) have tiles that take the `inside` path next to ragged last tiles; the components' shapes differ by one
# from each other wherever a side is closed or open (unequal tile counts in the all-components launches)
TILE_CASES = [
    ((16, 20), P2, 2, 0.2, 0, None), ((7, 31), MIX2[0], 1, 0.7, -1, None), ((8, 32), MIX2[1], 2, 2.9, 0, 1), ((9, 33), MIX2[2], 1, 0.7, 0, 0),
    ((17, 65), MIX2[3], 2, 0.7, -1, 0), ((24, 64), MIX2[0], 1, 0.2, 0, 1),
    ((12, 20, 72), P3, 2, 0.7, 0, None), ((9, 17, 66), MIX3[0], 1, 0.7, 0, 2), ((12, 24, 64), MIX3[1], 2, 2.9, -1, 1), ((13, 25, 97), MIX3[2], 1, 0.2, 0, 0),
    ((3, 7, 31), MIX3[3], 2, 0.7, 0, None), ((4, 8, 32), MIX3[0], 1, 0.7, -1, 2), ((5, 9, 33), MIX3[1], 2, 0.7, 0, 1),
]


# the diffuse adjoints march more than one plane per workgroup once tiles x planes exceeds the plan's 4096 workgroups (plan_columns, csrc/column_march.hpp):
# one (4 x 64) tile and 4100 planes give 2 planes per workgroup, the a0 neighbours carried in registers from the first to the second. (res, bc, batch)
CHUNKED_DIFFUSE_CASES = [((4100, 3, 5), MIX3[1], 1)]


def _kinds(n):
    """ boundary kinds of an axis of n cells that the library stores faces for (tests/fuzz_parity.py: ONE cell between two closed sides has none) """
    return [k for k in ((PER, PER), (CLO, CLO), (OPN, OPN), (CLO, OPN), (OPN, CLO)) if not (n == 1 and k == (CLO, CLO))]


# ends of the array in pass C and the c2s adjoint: axes of 1, 2 and 3 cells under every kind, as first, middle and last axis
SMALL_CASES = []
for _n in (1, 2, 3):
    for _i, _k in enumerate(_kinds(_n)):
        SMALL_CASES.append(((_n, 5), (_k, MIX2[_i % 4][1]), 1 + _i % 2))
        SMALL_CASES.append(((6, _n), (MIX2[_i % 4][0], _k), 2 - _i % 2))
        SMALL_CASES.append(((4, _n, 5), (MIX3[_i % 4][0], _k, MIX3[(_i + 1) % 4][2]), 1 + _i % 2))
        SMALL_CASES.append(((_n, 3, _n), (_k, MIX3[_i % 4][1], _k), 1))


def run_entry(ctx, mem, entry, res, bc, dtype, batch=2, dt=0.7, seed=0, k0=0, slab_axis=None, flip=False):
    """ one entry point on one case """
    if entry == 'advect_staggered':
        check_advect_staggered(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis)
    elif entry == 'advect_centered':
        check_advect_centered(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis, flip=flip)
    elif entry == 'mac_cormack_staggered':
        check_mac_cormack_staggered(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis)
    elif entry == 'mac_cormack_centered':
        check_mac_cormack_centered(ctx, mem, res, bc, dtype, batch, dt, seed, k0, slab_axis, flip=flip)
    elif entry == 'centered_to_staggered':
        check_centered_to_staggered(ctx, mem, res, bc, dtype, batch, seed, flip=flip)
    elif entry == 'diffuse':
        check_diffuse(ctx, mem, res, bc, dtype, batch, seed, flip=flip)
    else:
        raise ValueError(entry)


ENTRIES = ('advect_staggered', 'advect_centered', 'mac_cormack_staggered', 'mac_cormack_centered', 'centered_to_staggered', 'diffuse')


def case_id(case):
    """ pytest id of a (res, bc, ...) case: 9x17x66-ccoopp (p periodic, c closed / constant, o open) """
    return "x".join(str(n) for n in case[0]) + "-" + "".join("pco"[lo] + "pco"[hi] for lo, hi in case[1])


def run_case(ctx, mem, res, bc, dtype, batch=2, dt=0.7, seed=0, k0=0, slab_axis=None, flip=False, entries=ENTRIES):
    """ every entry point of `entries` on one case; prints the figures of the case (also when a check fails) """
    del RECORDS[:]
    try:
        for entry in entries:
            run_entry(ctx, mem, entry, res, bc, dtype, batch, dt, seed, k0, slab_axis, flip)
    finally:
        report()


# (shape, codes) of the grid_sample cases: each with shared and per-batch values
GRID_SAMPLE_CASES = [((6, 7), ((PER, PER), (CLO, OPN))), ((33, 9), ((OPN, CLO), (OPN, OPN))), ((5, 4, 9), ((OPN, CLO), (PER, PER), (CLO, CLO))),
                     ((1, 2, 3), ((PER, PER), (CLO, OPN), (OPN, OPN)))]


def run_grid_sample(ctx, mem, shape, codes, dtype, shared_values):
    del RECORDS[:]
    try:
        check_grid_sample(ctx, mem, shape, codes, dtype, batch=2, points=301, shared_values=shared_values, seed=len(shape))
        check_grid_sample(ctx, mem, shape, codes, dtype, batch=1, points=4099, shared_values=shared_values, seed=7)     # more than one workgroup, ragged
    finally:
        report()


# (res, bc, batch, obstacle or None) of the projection adjoint in fp32 (parity_cases.check_project_backward with dtype=float32)
PROJECT_CASES = [((16, 20), ((CLO, CLO), (CLO, CLO)), 2, None), ((16, 20), ((OPN, OPN), (CLO, OPN)), 2, None), ((7, 13), ((CLO, OPN), (PER, PER)), 1, None),
                 ((16, 20), ((PER, PER), (CLO, OPN)), 2, ((8.0, 9.0), 3.5)), ((9, 7, 10), ((CLO, CLO), (OPN, OPN), (CLO, OPN)), 2, None),
                 ((12, 10, 16), ((CLO, CLO),) * 3, 1, ((6.0, 5.0, 8.0), 3.0))]


def run_project_backward(ctx, mem, res, bc, batch, obstacle, dtype):
    import parity_cases as pc
    dom, grid = make_case(res, bc, dtype, batch=batch)
    obstacles = [O.SphereObstacle(tuple(obstacle[0]), float(obstacle[1]))] if obstacle else ()
    pc.check_project_backward(ctx, mem, dom, grid, np.random.default_rng(15), obstacles=obstacles, dtype=dtype)


# GPU only: (res, bc, batch, dt, k0, slab_axis). Large grids (many tiles on the `inside` path, rows of 136 and 384 cells: advect_tol grows with the row) and
# a row of 264 cells (two patches of the vector kernels)
LARGE_CASES = [((48, 40, 136), MIX3[2], 1, 0.7, 0, 1), ((40, 36, 384), MIX3[0], 1, 0.7, -1, 0), ((6, 264), MIX2[2], 2, 0.7, 0, 1), ((3, 5, 264), MIX3[2], 2, 0.7, 0, 2)]
