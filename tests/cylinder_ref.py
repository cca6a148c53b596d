"""
NumPy restatement of the finite cylinder, written from the reference's text (phi/geom/_cylinder.py:67-92, 137-144) and independent of the library:
a float64 class with the duck-typed interface of tests/project_ref.py's Box / Sphere (lies_inside, sdf, surfaces, reach, center, velocity, angular_velocity), so
that project_ref.accessible, cell_flags, apply_obstacles and surface_clearance take it unchanged. Imports nothing under test.

    local = M^T (x - c)       (rotate(.., invert=True), the box-frame convention), M: cylinder frame -> world, rows and columns in grid axis order
    h     = local[axis],  r = the other two components
    lies_inside = r.r <= R^2 and h >= -depth / 2 and h <= depth / 2          (all inclusive)
    sdf         = max(sqrt(r.r) - R, |h| - depth / 2)
"""
import numpy as np


class Cylinder:
    def __init__(self, center, radius, depth, axis, rotation=None, velocity=None, angular_velocity=None):
        self.center, self.radius, self.depth, self.axis = tuple(float(c) for c in center), float(radius), float(depth), int(axis)
        self.rotation = None if rotation is None else np.asarray(rotation, np.float64)
        self.velocity, self.angular_velocity = velocity, angular_velocity
        assert len(self.center) == 3 and 0 <= self.axis < 3

    def _rad2_h(self, pts):
        r = [p - c for p, c in zip(pts, self.center)]
        if self.rotation is not None:
            M = self.rotation
            r = [sum(M[c][a] * r[c] for c in range(3)) for a in range(3)]
        radial = [r[a] for a in range(3) if a != self.axis]
        return radial[0] * radial[0] + radial[1] * radial[1], r[self.axis]

    def lies_inside(self, pts):
        rad2, h = self._rad2_h(pts)
        inside = (rad2 <= self.radius * self.radius) & (h >= -0.5 * self.depth) & (h <= 0.5 * self.depth)
        return inside & np.ones(np.broadcast(*pts).shape, bool)

    def surfaces(self, pts):
        """ both surfaces: the mantle and the caps (surface_clearance keeps the samples off either) """
        rad2, h = self._rad2_h(pts)
        return [np.sqrt(rad2) - self.radius, np.abs(h) - 0.5 * self.depth]

    def sdf(self, pts):
        mantle, caps = self.surfaces(pts)
        return np.maximum(mantle, caps) + np.zeros(np.broadcast(*pts).shape)

    @property
    def reach(self):
        return sum(abs(c) for c in self.center) + self.radius + 0.5 * self.depth

    @property
    def up(self):
        e = np.zeros(3)
        e[self.axis] = 1.0
        return e if self.rotation is None else self.rotation @ e

    def bounding_radius(self):
        return float(np.sqrt(self.radius ** 2 + (0.5 * self.depth) ** 2))

    def bounding_half_extent(self, epsilon=1e-5):
        if self.rotation is None:
            return tuple(0.5 * self.depth if a == self.axis else self.radius for a in range(3))
        up = self.up
        return tuple(np.abs(up) * 0.5 * self.depth + self.radius * np.sqrt(np.maximum(epsilon, 1 - up ** 2)))

    def culling_extent(self, margin):
        """ the samples with sdf <= margin lie within this of the centre along each world axis (issue f16, checked in test_culling_box_is_conservative) """
        up = self.up
        return np.abs(up) * (0.5 * self.depth + margin) + (self.radius + margin) * np.sqrt(np.maximum(0.0, 1 - up ** 2))
