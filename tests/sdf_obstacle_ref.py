"""
NumPy restatement (float64) of phi.geom.SDFGrid, written from the reference's text and independent of the library. Imports nothing under test.

Reference lines restated (phi = the reference project):
    sampled value        phi/geom/_sdf_grid.py:150-151, 184-185   float_idx = (location - lower) / size * resolution;  grid_sample(sdf, float_idx - .5, ZERO_GRADIENT)
    grid_sample          [PHIML-RECALL] phiml.math.grid_sample with ZERO_GRADIENT: multilinear interpolation, every tap index clamped to [0, n - 1]
    lies_inside          :149-156   approximate_outside: bounds.lies_inside(x) & (sdf_val <= 0), both inclusive (Box.lies_inside, phi/geom/_box.py:174-185); else sdf_val <= 0
    signed distance      :183-191   approximate_outside: where(within bounds, sdf_val, |x - center| - bounding_radius); else sdf_val
    constructor          :48-64     center = bounds.local_to_global(argmin_index / res) -- the LOWER CORNER of the minimum cell (a literal quirk, restated as written);
                                    bounding_radius = max |cell centre - center| over cells with sdf <= 0; volume = count(sdf < 0) * prod(dx)
    shifted / at / scaled  :202-215

`SdfObstacle` carries the duck-typed interface tests/project_ref.py takes (accessible, apply_obstacles, surface_clearance): lies_inside, sdf, surfaces, reach,
center, velocity, angular_velocity. The obstacle loop and cell_flags are project_ref's, not rewritten here.
"""
import numpy as np


def multilinear_clamped(values, idx):
    """ values [n_0, .., n_{D-1}] at fractional indices idx[a] (broadcastable arrays): taps floor(idx) and floor(idx) + 1, each clamped to [0, n - 1],
    weights 1 - f and f with f = idx - floor(idx); interpolated along the last axis first """
    values = np.asarray(values, np.float64)
    D = values.ndim
    shape = np.broadcast(*idx).shape
    lo, hi, f = [], [], []
    for a in range(D):
        n = values.shape[a]
        x = np.broadcast_to(np.asarray(idx[a], np.float64), shape)
        fl = np.floor(x)
        f.append(np.where(x < 0, 0.0, np.where(x > n - 1, 0.0, x - fl)))      # beyond the first / last tap both taps are the same value
        i = np.clip(fl, -1, n).astype(np.int64)
        lo.append(np.clip(i, 0, n - 1))
        hi.append(np.clip(i + 1, 0, n - 1))

    def level(a, index):
        if a == D:
            return values[tuple(index)]
        return level(a + 1, index + [lo[a]]) * (1.0 - f[a]) + level(a + 1, index + [hi[a]]) * f[a]
    return level(0, [])


def default_center(values, lower, upper):
    values = np.asarray(values)
    arg = np.unravel_index(int(np.argmin(values)), values.shape)
    return tuple(lower[a] + (arg[a] / values.shape[a]) * (upper[a] - lower[a]) for a in range(values.ndim))


def cell_centres(res, lower, upper):
    D = len(res)
    return [(lower[a] + (np.arange(res[a]) + 0.5) * ((upper[a] - lower[a]) / res[a])).reshape([-1 if k == a else 1 for k in range(D)]) for a in range(D)]


def default_bounding_radius(values, lower, upper, center):
    values = np.asarray(values)
    pts = cell_centres(values.shape, lower, upper)
    dist = np.sqrt(sum((p - c) ** 2 for p, c in zip(pts, center)))
    return float(np.where(values <= 0, dist, 0.0).max())


def default_volume(values, lower, upper):
    values = np.asarray(values)
    return float((values < 0).sum() * np.prod([(u - l) / n for l, u, n in zip(lower, upper, values.shape)]))


class SdfObstacle:
    def __init__(self, values, lower, upper, approximate_outside=True, center=None, bounding_radius=None, velocity=None):
        self.values = np.asarray(values)
        self.lower, self.upper = tuple(float(x) for x in lower), tuple(float(x) for x in upper)
        self.approximate_outside = bool(approximate_outside)
        self.center = tuple(center) if center is not None else default_center(self.values, self.lower, self.upper)
        self.bounding_radius = float(bounding_radius) if bounding_radius is not None else default_bounding_radius(self.values, self.lower, self.upper, self.center)
        self.velocity, self.angular_velocity = velocity, None

    def sample(self, pts):
        res = self.values.shape
        idx = [(np.asarray(p, np.float64) - l) / (u - l) * float(n) - 0.5 for p, l, u, n in zip(pts, self.lower, self.upper, res)]
        return multilinear_clamped(self.values, idx)

    def within(self, pts):
        ok = np.ones(np.broadcast(*pts).shape, bool)
        for p, l, u in zip(pts, self.lower, self.upper):
            ok = ok & (p >= l) & (p <= u)
        return ok

    def lies_inside(self, pts):
        inside = self.sample(pts) <= 0
        return (self.within(pts) & inside) if self.approximate_outside else inside

    def sdf(self, pts):
        val = self.sample(pts)
        if not self.approximate_outside:
            return val
        return np.where(self.within(pts), val, np.sqrt(sum((p - c) ** 2 for p, c in zip(pts, self.center))) - self.bounding_radius)

    def surfaces(self, pts):
        """ what a discrete decision hangs on: the sampled value (<= 0) and, with approximate_outside, every coordinate's distance to the two bounds faces of its axis """
        out = [self.sample(pts)]
        if self.approximate_outside:
            for p, l, u in zip(pts, self.lower, self.upper):
                out += [np.asarray(p, np.float64) - l, np.asarray(p, np.float64) - u]
        return out

    @property
    def lipschitz(self):
        """ largest |difference of neighbouring values| / cell size over the axes: the slope of the multilinear interpolant along an axis never exceeds it """
        worst = 0.0
        for a, n in enumerate(self.values.shape):
            if n > 1:
                worst = max(worst, float(np.abs(np.diff(self.values.astype(np.float64), axis=a)).max()) / ((self.upper[a] - self.lower[a]) / n))
        return worst

    @property
    def reach(self):
        """ X = sum_a |x_a| + reach bounds, in units of eps64, the rounding of the sampled distance: the index (x - lower) / size * res - 0.5 carries a few eps64 of
        (|x_a| + |lower_a| + |upper_a|) / h_a, which the interpolant turns into at most that times max |difference of neighbouring values| -- <= h_a here, asserted:
        the scenes are scaled to a Lipschitz constant <= 1 --, and the interpolation itself a few eps64 of max |value|; outside the bounds |x - center| - radius """
        assert self.lipschitz <= 1.0 + 1e-12, f"the bound's derivation needs a grid with Lipschitz constant <= 1, got {self.lipschitz}"
        return (sum(abs(l) + abs(u) for l, u in zip(self.lower, self.upper)) + float(np.abs(self.values.astype(np.float64)).max())
                + sum(abs(c) for c in self.center) + abs(self.bounding_radius))

    def shifted(self, delta):
        return SdfObstacle(self.values, [l + d for l, d in zip(self.lower, delta)], [u + d for u, d in zip(self.upper, delta)], self.approximate_outside,
                           [c + d for c, d in zip(self.center, delta)], self.bounding_radius, self.velocity)

    def scaled(self, factor):
        """ :211-215: bounds.scaled(factor) (about the bounds' centre) shifted by (center - bounds.center) * (factor - 1); center stays, the radius scales """
        bc = [0.5 * (l + u) for l, u in zip(self.lower, self.upper)]
        half = [0.5 * (u - l) * factor for l, u in zip(self.lower, self.upper)]
        move = [(c - b) * (factor - 1) for c, b in zip(self.center, bc)]
        return SdfObstacle(self.values, [b - h + m for b, h, m in zip(bc, half, move)], [b + h + m for b, h, m in zip(bc, half, move)], self.approximate_outside,
                           self.center, self.bounding_radius * factor, self.velocity)
