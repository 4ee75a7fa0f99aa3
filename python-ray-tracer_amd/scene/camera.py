"""Camera and the pixel grid, reference scene/camera.py:7-26.

The reference materialises pixel_loc as a float64 (3,w,h) array with np.mgrid (24 B/pixel that its
kernel then reads back, kernels.py:19).  np.mgrid with a complex step evaluates `index*step + start`
with step = (stop-start)/float(n-1): a closed form.  Camera.generate_pixel_locations() returns that
same array (bit-identical, pinned by tests/golden/host_helpers.npz) as a PixelGrid that also
carries the closed form, so the render facade can hand the five scalars to the kernel and skip the
array entirely."""
import numpy as np

from .rotation import euler_rotation


class PixelGrid(np.ndarray):
    """float64 (3,w,h) pixel-location array + `.raygen = (px, y0, dy, z0, dz)` with
    grid[:, x, y] == (px, x*dy + y0, y*dz + z0)."""
    raygen = None

    def __array_finalize__(self, obj):
        # slices / arithmetic results no longer match the closed form
        self.raygen = None


class Camera:
    """aperture, focus_distance: a thin lens (depth of field, Renderer.set_lens): its radius in world units (0: the pinhole
    camera of the reference) and the distance of the plane of sharp focus along the forward axis rotation[:, 0]."""

    def __init__(self, resolution, position, euler, fov=45.0, true_aspect=False, aperture=0.0, focus_distance=1.0):
        self.resolution = resolution
        self._position = position
        self.rotation = euler_rotation(euler[0], euler[1], euler[2])
        self.field_of_view = fov
        self.true_aspect = true_aspect      # False: the reference's AR = int(w/h); True: AR = w/h
        a, f = float(aperture), float(focus_distance)
        if not (np.isfinite(a) and a >= 0.0):
            raise ValueError(f"aperture must be finite and >= 0, not {aperture!r}")
        if not (np.isfinite(f) and f > 0.0):
            raise ValueError(f"focus_distance must be finite and > 0, not {focus_distance!r}")
        self.aperture, self.focus_distance = a, f

    @property
    def position(self):
        return np.array(self._position)

    @property
    def lens(self):
        """(aperture, focus_distance), the arguments of Renderer.set_lens."""
        return self.aperture, self.focus_distance

    def focus_on(self, point):
        """The focus_distance that puts `point` in focus: its distance from the camera along the forward axis,
        dot(point - position, rotation[:, 0])."""
        d = np.asarray(point, dtype=np.float64).reshape(3) - np.asarray(self.position, dtype=np.float64).reshape(3)
        return float(np.dot(d, np.asarray(self.rotation, dtype=np.float64)[:, 0]))

    def raygen(self):
        """(px, y0, dy, z0, dz).  AR = int(width/height) truncates as the reference does
        (camera.py:22): 1 for 16:9, 0 for portrait frames.  true_aspect=True uses w/h instead
        (an undistorted 16:9 image; not what the reference renders)."""
        width, height = self.resolution
        ar = width / height if self.true_aspect else int(width / height)
        px = float(1 / np.tan(np.radians(self.field_of_view) / 2))
        dy = (-ar - ar) / float(width - 1) if width > 1 else 1.0
        dz = (-1 - 1) / float(height - 1) if height > 1 else 1.0
        return px, float(ar), dy, 1.0, dz

    def generate_pixel_locations(self):
        width, height = self.resolution
        px, y0, dy, z0, dz = self.raygen()
        grid = np.empty((3, width, height), dtype=np.float64)
        grid[0] = px
        grid[1] = (np.arange(width, dtype=np.float64) * dy + y0)[:, None]
        grid[2] = (np.arange(height, dtype=np.float64) * dz + z0)[None, :]
        out = grid.view(PixelGrid)
        out.raygen = (px, y0, dy, z0, dz)
        return out
