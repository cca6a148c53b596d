"""
fp64 NumPy restatement of advection by a centred velocity (phi/physics/advect.py:20-36, 156-179; phi/field/_resample.py:257-259), built from
the oracle's `grid_sample` and `cell_positions`. The oracle's own `integrate_points` samples a staggered velocity only.
Arrays are (batch, C, *res); a batch of 1 is shared.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import phi_oracle as O   # noqa: E402


def _dom(res, lower, upper):
    return O.Domain(res, lower, upper, [(O.PERIODIC, O.PERIODIC)] * len(res))


def index_coords(points, res, lower, upper):
    """ world points -> fractional cell indices (global_to_local(x) * res - 0.5) """
    return [(p - lower[a]) / (upper[a] - lower[a]) * res[a] - 0.5 for a, p in enumerate(points)]


def sample_vector(vel, points, res, lower, upper, codes, consts):
    """ the centred vector field `vel` (B, D, *res) at world points (B, *res) per axis -> list of D arrays """
    coords = index_coords(points, res, lower, upper)
    return [O.grid_sample(np.ascontiguousarray(vel[:, d]), coords, codes, consts) for d in range(vel.shape[1])]


def integrate(points, vel, dt, res, lower, upper, codes, consts, integrator='euler'):
    """ where `points` end up after dt (advect.euler / advect.rk4) with the velocity sampled from the centred field `vel` """
    v0 = sample_vector(vel, points, res, lower, upper, codes, consts)
    if integrator == 'euler':
        return [p + dt * u for p, u in zip(points, v0)]
    v_half = sample_vector(vel, [p + 0.5 * dt * u for p, u in zip(points, v0)], res, lower, upper, codes, consts)
    v_half2 = sample_vector(vel, [p + 0.5 * dt * u for p, u in zip(points, v_half)], res, lower, upper, codes, consts)
    v_full = sample_vector(vel, [p + dt * u for p, u in zip(points, v_half2)], res, lower, upper, codes, consts)
    v_rk4 = [(a + 2 * (b + c) + d) / 6. for a, b, c, d in zip(v0, v_half, v_half2, v_full)]
    return [p + dt * u for p, u in zip(points, v_rk4)]


def semi_lagrangian(field, vel, dt, res, lower, upper, codes, consts, v_codes=None, v_consts=None, integrator='euler'):
    """ field (Bf, C, *res) advected by the centred velocity vel (Bv, D, *res) on the same grid -> (B, C, *res), fp64.
    codes / consts: the field's extrapolation; v_codes / v_consts: the velocity's (only rk4 samples it between cells). """
    field = np.asarray(field, np.float64)
    vel = np.asarray(vel, np.float64)
    B = max(field.shape[0], vel.shape[0])
    field = np.broadcast_to(field, (B,) + field.shape[1:])
    vel = np.broadcast_to(vel, (B,) + vel.shape[1:])
    pts = [np.broadcast_to(p[None], (B,) + p.shape) for p in O.cell_positions(_dom(res, lower, upper), np.float64)]
    v_codes = codes if v_codes is None else v_codes
    v_consts = consts if v_consts is None else v_consts
    back = integrate(pts, vel, -dt, res, lower, upper, v_codes, v_consts, integrator)
    coords = index_coords(back, res, lower, upper)
    return np.stack([O.grid_sample(np.ascontiguousarray(field[:, c]), coords, codes, consts) for c in range(field.shape[1])], axis=1)
