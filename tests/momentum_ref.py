"""
Float64 restatements of the method-of-lines step -- TEST INFRASTRUCTURE, imports nothing under test:
  * advect.differential (phi/physics/advect.py:108-124), staggered and centred, written out with index gathers (NOT built on the oracle: the pin in
    tests/test_momentum_emu.py compares it with a composition of oracle.pad_component / component_at_faces). The formulas are torch float64 ops, so
    autograd of the same code gives the reference gradients (as tests/adjoint_ref.py does); the NumPy entry points return (value, S) with S the
    restatement evaluated with the absolute value of every term, the four-face mean included -- the scale of the bound K eps S of tests/momentum_cases.py.
  * fluid.incompressible_rk4 (phi/physics/fluid.py:312-334) on oracle.make_incompressible / pressure_gradient / laplace_component, pure NumPy.

Arrays carry a leading batch dim. Staggered fields are lists of stored-face arrays described by an oracle Domain; centred rules are
(codes[D][2], consts[D][2]) with oracle codes (PERIODIC wrap / OPEN edge copy / CLOSED constant).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import phi_oracle as O   # noqa: E402


# ---- padded gathers ---------------------------------------------------------------------------------------------------------------------------
def take(a, axis, pos, codes, consts):
    """ samples of the (B, *shape) tensor `a` at the integer positions `pos` along spatial `axis`; a position outside the array wraps (PERIODIC), copies
    the edge sample (OPEN) or is the constant of that side (CLOSED). codes / consts: (lower, upper) of this axis. """
    ax = axis + 1
    n = a.shape[ax]
    pos = np.asarray(pos, np.int64)
    idx = pos.copy()
    const = np.zeros(len(pos))
    is_const = np.zeros(len(pos), bool)
    for side, out in ((0, pos < 0), (1, pos >= n)):
        if codes[side] == O.PERIODIC:
            idx[out] = np.mod(pos[out], n)
        elif codes[side] == O.OPEN:
            idx[out] = 0 if side == 0 else n - 1
        else:
            idx[out] = 0
            is_const |= out
            const[out] = consts[side]
    got = a.index_select(ax, torch.as_tensor(idx))
    if is_const.any():
        shp = [1] * a.dim()
        shp[ax] = len(pos)
        got = torch.where(torch.as_tensor(is_const).reshape(shp), torch.as_tensor(const, dtype=a.dtype).reshape(shp), got)
    return got


def _c(x, absolute):
    return abs(float(x)) if absolute else float(x)


def t_advect_staggered(u, v, dom, absolute=False):
    """ out_c[f] = -sum_d W_d(f) (U_c[f + e_d] - U_c[f - e_d]) / (2 dx_d) on the stored faces of every component c (lists of (B, *faces) tensors).
    absolute: every term with its absolute value (inputs, constants, differences as sums, no final sign). """
    D = dom.rank
    off = [dom.face_offset(c) for c in range(D)]
    if absolute:
        u, v = [x.abs() for x in u], [x.abs() for x in v]
    outs = []
    for c in range(D):
        U = u[c]
        acc = 0.0
        for d in range(D):
            n = U.shape[d + 1]
            cu = [_c(dom.bc_val[d][s][c], absolute) for s in range(2)]
            hi, lo = take(U, d, np.arange(n) + 1, dom.bc[d], cu), take(U, d, np.arange(n) - 1, dom.bc[d], cu)
            g = hi + lo if absolute else hi - lo
            if d == c:
                W = v[c]
            else:
                # the four d-faces around the c-face: faces f_d, f_d + 1 along d (stored index = physical - offset), cells m - 1, m along c (m physical)
                W = 0.0
                for pd in range(2):
                    for pc in range(2):
                        a = v[d]
                        gathers = {d: (np.arange(dom.res[d]) + pd - off[d], [_c(dom.bc_val[d][s][d], absolute) for s in range(2)]),
                                   c: (np.arange(U.shape[c + 1]) + off[c] - 1 + pc, [_c(dom.bc_val[c][s][d], absolute) for s in range(2)])}
                        for axis in sorted(gathers):       # one pad per axis in spatial order: the later axis sees the padded array
                            a = take(a, axis, gathers[axis][0], dom.bc[axis], gathers[axis][1])
                        W = W + 0.25 * a
            acc = acc + W * g * (0.5 / dom.dx[d])
        outs.append(acc if absolute else -acc)
    return outs


def t_advect_centered(u, v, dx, codes, consts, absolute=False):
    """ u, v (B, D, *res): out_c[i] = -sum_d v_d[i] (U_c[i + e_d] - U_c[i - e_d]) / (2 dx_d), U padded with u's rule """
    D = u.dim() - 2
    if absolute:
        u, v = u.abs(), v.abs()
    comps = []
    for c in range(D):
        U = u[:, c]
        acc = 0.0
        for d in range(D):
            n = U.shape[d + 1]
            cu = [_c(consts[d][s], absolute) for s in range(2)]
            hi, lo = take(U, d, np.arange(n) + 1, codes[d], cu), take(U, d, np.arange(n) - 1, codes[d], cu)
            acc = acc + v[:, d] * (hi + lo if absolute else hi - lo) * (0.5 / dx[d])
        comps.append(acc if absolute else -acc)
    return torch.stack(comps, dim=1)


def _t64(x):
    return torch.as_tensor(np.asarray(x, np.float64))


def advect_staggered(u, v, dom):
    """ NumPy entry: lists of stored-face arrays -> (outs, Ss) """
    tu, tv = [_t64(x) for x in u], [_t64(x) for x in v]
    return [o.numpy() for o in t_advect_staggered(tu, tv, dom)], [o.numpy() for o in t_advect_staggered(tu, tv, dom, absolute=True)]


def advect_centered(u, v, dx, codes, consts):
    tu, tv = _t64(u), _t64(v)
    return t_advect_centered(tu, tv, dx, codes, consts).numpy(), t_advect_centered(tu, tv, dx, codes, consts, absolute=True).numpy()


def advect_staggered_oracle(u, v, dom):
    """ the same term composed from the oracle's pieces: pad_component pads u_c, component_at_faces is `vel.at(grad)` """
    D = dom.rank
    outs = []
    for c in range(D):
        a = np.asarray(u[c], np.float64)
        acc = np.zeros_like(a)
        for d in range(D):
            w = [(0, 0)] * D
            w[d] = (1, 1)
            p = O.pad_component(a, c, w, dom)
            n = a.shape[d + 1]
            g = np.take(p, np.arange(2, n + 2), axis=d + 1) - np.take(p, np.arange(0, n), axis=d + 1)
            W = np.asarray(v[c], np.float64) if d == c else O.component_at_faces([np.asarray(x, np.float64) for x in v], d, c, dom)
            acc = acc + W * g / (2 * dom.dx[d])
        outs.append(-acc)
    return outs


# ---- the Runge-Kutta step ---------------------------------------------------------------------------------------------------------------------
def momentum_rhs(v, nu, dom):
    """ pde(v) = advect.differential(v, v) + diffuse.differential(v, nu) """
    adv = advect_staggered(v, v, dom)[0]
    return [a + nu * O.laplace_component(np.asarray(x, np.float64), c, dom) for c, (a, x) in enumerate(zip(adv, v))]


def rk4_step(v, p, dt, nu, dom, rtol=1e-13, atol=1e-13, refresh=50, max_iter=4000, pde=None):
    """ fluid.incompressible_rk4 (fluid.py:312-334) line for line; every projection starts from x0 = 0 (`Solve('CG', rtol, atol)`) """
    pde = pde or (lambda w: momentum_rhs(w, nu, dom))

    def project(w):
        w_new, dp, info, _ = O.make_incompressible(w, dom, rtol=rtol, atol=atol, max_iter=max_iter, refresh=refresh)
        assert bool(np.all(info.converged)), "the reference's CG did not converge"
        return w_new, dp

    def rhs(w, q):
        return [a - g for a, g in zip(pde(w), O.pressure_gradient(q, dom))]

    def axpy(w, s, r):
        return [a + s * b for a, b in zip(w, r)]
    v1, p1 = v, p
    rhs1 = rhs(v1, p1)
    v2, delta_p = project(axpy(v, dt / 2, rhs1))
    p2 = p1 + delta_p / dt
    rhs2 = rhs(v2, p2)
    v3, delta_p = project(axpy(v, dt / 2, rhs2))
    p3 = p2 + delta_p / dt
    rhs3 = rhs(v3, p3)
    v4, delta_p = project(axpy(v, dt, rhs2))
    p4 = p3 + delta_p / dt
    rhs4 = rhs(v4, p4)
    total = [a + 2 * b + 2 * c + d for a, b, c, d in zip(rhs1, rhs2, rhs3, rhs4)]
    p_old = (1 / 6) * (p1 + 2 * p2 + 2 * p3 + p4)
    v_new, delta_p = project(axpy(v, dt / 6, total))
    return v_new, p_old + delta_p / dt


def rk4_run(v, p, dt, steps, nu, dom, **kw):
    for _ in range(steps):
        v, p = rk4_step(v, p, dt, nu, dom, **kw)
    return v, p


def periodic_domain(n, size=2 * np.pi):
    D = len(n)
    return O.Domain(n, (0.0,) * D, (size,) * D, ((O.PERIODIC, O.PERIODIC),) * D)


def face_coordinates(dom, c):
    """ coordinates of the stored faces of component c, one broadcastable array per axis """
    axes = []
    for a in range(dom.rank):
        h = dom.dx[a]
        if a == c:
            x = dom.lower[a] + (dom.face_offset(c) + np.arange(dom.comp_shape(c)[a])) * h
        else:
            x = dom.lower[a] + (np.arange(dom.res[a]) + 0.5) * h
        axes.append(x)
    return np.meshgrid(*axes, indexing='ij')


def taylor_green(dom, perturbed=False):
    """ 2-D Taylor-Green vortex (sin x cos y, -cos x sin y) at the faces, batch dim 1; perturbed: plus two shear modes (divergence-free, not an
    eigenfunction of the advection term) """
    x, y = face_coordinates(dom, 0)
    vx = np.sin(x) * np.cos(y)
    xx, yy = face_coordinates(dom, 1)
    vy = -np.cos(xx) * np.sin(yy)
    if perturbed:
        vx = vx + 0.3 * np.sin(2 * y + 0.5)
        vy = vy + 0.3 * np.sin(2 * xx + 1.0)
    return [vx[None], vy[None]]


def energy(v):
    return float(sum((np.asarray(c, np.float64) ** 2).sum() for c in v))
