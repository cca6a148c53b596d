"""
Float64 restatements of the grid differential operators of phi/field/_field_math.py (laplace :119-145, spatial_gradient at='center' :229-233,
divergence of a centred vector field :627-632, curl :642-673), order 2 -- TEST INFRASTRUCTURE, imports nothing under test.

NumPy forms, built on oracle.pad_scalar / pad_component, return (value, S): S is the sum of the absolute values of the stencil's terms
|w_k U_k| at every element, the scale of the element-wise bound (2 D + 6) eps S of tests/diffops_cases.py.
Torch forms (same formulas with torch ops, float64) are differentiated by autograd for the backward checks; with `absolute=True` every term
enters with its absolute weight, so that autograd of it against |grad_out| gives S = sum |w_k| |grad_out_k| of the transposed stencil.

Arrays carry a leading batch dim. Centred rules are (codes[D][2], consts[D][2]) with oracle codes (PERIODIC wrap / OPEN edge copy / CLOSED
constant); staggered fields are described by an oracle Domain.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import phi_oracle as O   # noqa: E402


def _axis_widths(D, axis):
    w = [(0, 0)] * D
    w[axis] = (1, 1)
    return w


def _lo_mid_hi(p, axis):
    ax = axis + 1
    n = p.shape[ax]
    return np.take(p, np.arange(0, n - 2), axis=ax), np.take(p, np.arange(1, n - 1), axis=ax), np.take(p, np.arange(2, n), axis=ax)


def _abs_consts(consts):
    return [(abs(c[0]), abs(c[1])) for c in consts]


# ---- NumPy: values and S ------------------------------------------------------------------------------------------------------------------
def laplace_centered(a, dx, codes, consts, weights):
    """ a (B, *res) -> sum_d w_d (U[+e_d] + U[-e_d] - 2 U) / dx_d^2 """
    a = np.asarray(a, np.float64)
    D = a.ndim - 1
    out, S = np.zeros_like(a), np.zeros_like(a)
    for axis in range(D):
        w = weights[axis] / dx[axis] ** 2
        lo, mid, hi = _lo_mid_hi(O.pad_scalar(a, _axis_widths(D, axis), codes, consts), axis)
        out = out + w * (lo + hi - 2 * mid)
        alo, amid, ahi = _lo_mid_hi(O.pad_scalar(np.abs(a), _axis_widths(D, axis), codes, _abs_consts(consts)), axis)
        S = S + abs(w) * (alo + ahi + 2 * amid)
    return out, S


def laplace_staggered(v, dom, weight=1.0):
    """ every component on its own face lattice with that component's wall constants """
    outs, Ss = [], []
    absdom = O.Domain(dom.res, dom.lower, dom.upper, dom.bc, np.abs(dom.bc_val))
    for c, a in enumerate(v):
        a = np.asarray(a, np.float64)
        out, S = np.zeros_like(a), np.zeros_like(a)
        for axis in range(dom.rank):
            w = weight / dom.dx[axis] ** 2
            lo, mid, hi = _lo_mid_hi(O.pad_component(a, c, _axis_widths(dom.rank, axis), dom), axis)
            out = out + w * (lo + hi - 2 * mid)
            alo, amid, ahi = _lo_mid_hi(O.pad_component(np.abs(a), c, _axis_widths(dom.rank, axis), absdom), axis)
            S = S + abs(w) * (alo + ahi + 2 * amid)
        outs.append(out)
        Ss.append(S)
    return outs, Ss


def gradient_centered(a, dx, codes, consts):
    """ a (B, *res) -> (B, D, *res): (U[+e_d] - U[-e_d]) / (2 dx_d) """
    a = np.asarray(a, np.float64)
    D = a.ndim - 1
    out, S = [], []
    for axis in range(D):
        w = 0.5 / dx[axis]
        lo, _, hi = _lo_mid_hi(O.pad_scalar(a, _axis_widths(D, axis), codes, consts), axis)
        alo, _, ahi = _lo_mid_hi(O.pad_scalar(np.abs(a), _axis_widths(D, axis), codes, _abs_consts(consts)), axis)
        out.append(w * (hi - lo))
        S.append(w * (ahi + alo))
    return np.stack(out, axis=1), np.stack(S, axis=1)


def divergence_centered(v, dx, codes, consts):
    """ v (B, D, *res) -> (B, *res): sum_d (V_d[+e_d] - V_d[-e_d]) / (2 dx_d) """
    v = np.asarray(v, np.float64)
    D = v.ndim - 2
    out, S = np.zeros_like(v[:, 0]), np.zeros_like(v[:, 0])
    for axis in range(D):
        w = 0.5 / dx[axis]
        lo, _, hi = _lo_mid_hi(O.pad_scalar(v[:, axis], _axis_widths(D, axis), codes, consts), axis)
        alo, _, ahi = _lo_mid_hi(O.pad_scalar(np.abs(v[:, axis]), _axis_widths(D, axis), codes, _abs_consts(consts)), axis)
        out = out + w * (hi - lo)
        S = S + w * (ahi + alo)
    return out, S


def curl_staggered(v, dom):
    """ stored components [vx, vy] of a 2-D staggered field -> (B, nx + 1, ny + 1). All faces are baked; vx is padded along y with the
    boundary's y component and vy along x with its x component (the reference's literal choice, _field_math.py:655-656). """
    assert dom.rank == 2
    absdom = O.Domain(dom.res, dom.lower, dom.upper, dom.bc, np.abs(dom.bc_val))

    def terms(vx, vy, d):
        vx, vy = O.bake_component(vx, 0, d), O.bake_component(vy, 1, d)
        vxp = O.pad_component(vx, 1, [(0, 0), (1, 1)], d)
        vyp = O.pad_component(vy, 0, [(1, 1), (0, 0)], d)
        return vyp[:, 1:], vyp[:, :-1], vxp[:, :, 1:], vxp[:, :, :-1]
    yh, yl, xh, xl = terms(np.asarray(v[0], np.float64), np.asarray(v[1], np.float64), dom)
    ayh, ayl, axh, axl = terms(np.abs(np.asarray(v[0], np.float64)), np.abs(np.asarray(v[1], np.float64)), absdom)
    dx, dy = dom.dx
    return (yh - yl) / dx - (xh - xl) / dy, (ayh + ayl) / dx + (axh + axl) / dy


def curl_centered(v, codes, consts):
    """ v (B, 2, nx, ny) -> (B, nx + 1, ny + 1): (vx - vy)[ll] - (vx + vy)[ul] + (vx + vy)[lr] - (vx - vy)[ur], no 1 / dx (as the reference) """
    v = np.asarray(v, np.float64)
    B = v.shape[0]
    p = O.pad_scalar(v.reshape((B * 2,) + v.shape[2:]), [(1, 1), (1, 1)], codes, consts).reshape((B, 2, v.shape[2] + 2, v.shape[3] + 2))
    ap = O.pad_scalar(np.abs(v).reshape((B * 2,) + v.shape[2:]), [(1, 1), (1, 1)], codes, _abs_consts(consts)).reshape(p.shape)
    pos, neg, tot = p[:, 0] + p[:, 1], p[:, 0] - p[:, 1], ap[:, 0] + ap[:, 1]
    out = neg[:, :-1, :-1] - pos[:, :-1, 1:] + pos[:, 1:, :-1] - neg[:, 1:, 1:]
    S = tot[:, :-1, :-1] + tot[:, :-1, 1:] + tot[:, 1:, :-1] + tot[:, 1:, 1:]
    return out, S


# ---- torch: the same formulas, differentiable -----------------------------------------------------------------------------------------------
def t_pad_axis(a, axis, codes, consts):
    """ pad spatial `axis` of a (B, *res) tensor by one sample per side """
    ax = axis + 1
    n = a.shape[ax]
    parts = []
    for side, idx in ((0, n - 1), (1, 0)):
        code = codes[axis][side]
        if code == O.PERIODIC:
            part = a.narrow(ax, idx, 1)
        elif code == O.OPEN:
            part = a.narrow(ax, 0 if side == 0 else n - 1, 1)
        else:
            shp = list(a.shape)
            shp[ax] = 1
            part = torch.full(shp, float(consts[axis][side]), dtype=a.dtype)
        parts.append(part)
    return torch.cat([parts[0], a, parts[1]], dim=ax)


def _t_lo_mid_hi(p, axis):
    ax = axis + 1
    n = p.shape[ax]
    return p.narrow(ax, 0, n - 2), p.narrow(ax, 1, n - 2), p.narrow(ax, 2, n - 2)


def t_laplace(a, dx, codes, consts, weights, absolute=False):
    out = torch.zeros_like(a)
    for axis in range(a.dim() - 1):
        w = weights[axis] / dx[axis] ** 2
        lo, mid, hi = _t_lo_mid_hi(t_pad_axis(a, axis, codes, consts), axis)
        out = out + (abs(w) * (lo + hi + 2 * mid) if absolute else w * (lo + hi - 2 * mid))
    return out


def t_gradient(a, dx, codes, consts, absolute=False):
    out = []
    for axis in range(a.dim() - 1):
        lo, _, hi = _t_lo_mid_hi(t_pad_axis(a, axis, codes, consts), axis)
        out.append((0.5 / dx[axis]) * (hi + lo if absolute else hi - lo))
    return torch.stack(out, dim=1)


def t_divergence(v, dx, codes, consts, absolute=False):
    out = torch.zeros_like(v[:, 0])
    for axis in range(v.dim() - 2):
        lo, _, hi = _t_lo_mid_hi(t_pad_axis(v[:, axis], axis, codes, consts), axis)
        out = out + (0.5 / dx[axis]) * (hi + lo if absolute else hi - lo)
    return out


def _comp_rule(dom, comp):
    return [list(p) for p in dom.bc], [(dom.bc_val[a][0][comp], dom.bc_val[a][1][comp]) for a in range(dom.rank)]


def t_laplace_staggered(v, dom, weight=1.0, absolute=False):
    return [t_laplace(a, dom.dx, *_comp_rule(dom, c), [weight] * dom.rank, absolute) for c, a in enumerate(v)]


def t_bake(a, d, dom):
    """ all n + 1 faces of stored component d along its own axis """
    lo, hi = dom.valid_faces(d)
    codes, consts = _comp_rule(dom, d)
    p = t_pad_axis(a, d, codes, consts)
    n = p.shape[d + 1]
    return p.narrow(d + 1, 0 if not lo else 1, n - (0 if not lo else 1) - (0 if not hi else 1))


def t_curl_staggered(v, dom, absolute=False):
    vx, vy = t_bake(v[0], 0, dom), t_bake(v[1], 1, dom)
    vxp = t_pad_axis(vx, 1, *_comp_rule(dom, 1))        # (the y component's constant pads vx along y)
    vyp = t_pad_axis(vy, 0, *_comp_rule(dom, 0))
    dx, dy = dom.dx
    if absolute:
        return (vyp[:, 1:] + vyp[:, :-1]) / dx + (vxp[:, :, 1:] + vxp[:, :, :-1]) / dy
    return (vyp[:, 1:] - vyp[:, :-1]) / dx - (vxp[:, :, 1:] - vxp[:, :, :-1]) / dy


def t_curl_centered(v, codes, consts, absolute=False):
    B = v.shape[0]
    p = v.reshape((B * 2,) + tuple(v.shape[2:]))
    p = t_pad_axis(t_pad_axis(p, 0, codes, consts), 1, codes, consts)       # x first, then y (the later axis wins in the pad's corners)
    p = p.reshape((B, 2) + tuple(p.shape[1:]))
    pos, neg = p[:, 0] + p[:, 1], p[:, 0] - p[:, 1]
    if absolute:
        return pos[:, :-1, :-1] + pos[:, :-1, 1:] + pos[:, 1:, :-1] + pos[:, 1:, 1:]
    return neg[:, :-1, :-1] - pos[:, :-1, 1:] + pos[:, 1:, :-1] - neg[:, 1:, 1:]


def vjp(fn, inputs, grad_out):
    """ input gradients of the torch restatement `fn(*inputs)` (a tensor or a list of tensors) against grad_out, as float64 NumPy arrays """
    xs = [torch.tensor(np.asarray(x, np.float64), requires_grad=True) for x in inputs]
    out = fn(*xs)
    outs = out if isinstance(out, (list, tuple)) else [out]
    gs = grad_out if isinstance(grad_out, (list, tuple)) else [grad_out]
    total = sum((o * torch.as_tensor(np.asarray(g, np.float64))).sum() for o, g in zip(outs, gs))
    grads = torch.autograd.grad(total, xs, allow_unused=True)
    return [np.zeros(x.shape) if g is None else g.numpy() for g, x in zip(grads, xs)]
