"""The GPU feature tests' shared harness (tests/feature_gpu.py) on the CPU: check() refuses one uint8 level, one float32 ulp
and the sign of zero at a sampled pixel, and walk_entry_points() makes each module's entry calls and names the step whose frame
is wrong.  A stub renderer answers every entry with the true frame of a synthetic fixture."""
import numpy as np
import pytest

import feature_gpu as H

W, HT = 8, 6


def _fixture(aa=1, **over):
    rng = np.random.default_rng(7)
    u8 = rng.integers(0, 256, (3, W, HT)).astype(np.uint8)
    f32 = rng.uniform(1.0, 255.0, (3, W, HT)).astype(np.float32)
    co = np.array([[2, 0], [2, 5], [3, 1], [4, 4], [5, 2], [5, 3], [6, 0], [7, 5], [7, 1], [3, 3]])      # every x >= 2 (the slab)
    f32[1, 3, 1] = 0.0                                            # a +0.0 at a sampled pixel
    plain = u8 ^ 0x40
    g = dict(w=W, h=HT, depth=2, aa=aa, seed=5, coords=co, cam_origin=np.zeros(3), cam_rot=np.eye(3),
             u8=u8[:, co[:, 0], co[:, 1]].T.copy(), u8_plain=plain[:, co[:, 0], co[:, 1]].T.copy(),
             rgb64=f32[:, co[:, 0], co[:, 1]].T.astype(np.float64))
    g.update(over)
    return g, u8, f32, plain


def test_check_is_exact_at_the_sampled_pixels_only():
    g, u8, f32, plain = _fixture()
    H.check(g, u8, f32, "exact")
    H.check(g, u8, None, "exact, uint8 alone")

    off = u8.copy()
    off[2, 4, 4] += 1 if off[2, 4, 4] < 255 else -1
    with pytest.raises(AssertionError, match=r"level: uint8 differs at 1 of 10 pixels, e\.g\. \[\[4, 4\]\]"):
        H.check(g, off, f32, "level")

    ulp = f32.copy()
    ulp[0, 5, 3] = np.nextafter(ulp[0, 5, 3], np.float32(np.inf))
    assert np.array_equal(np.rint(ulp), np.rint(f32))             # (not a difference uint8 would show)
    with pytest.raises(AssertionError, match=r"ulp: float32 differs at 1 of 10 pixels, e\.g\. \[\[5, 3\]\]"):
        H.check(g, u8, ulp, "ulp")

    neg = f32.copy()
    neg[1, 3, 1] = -0.0
    assert (neg == f32).all()                                     # equal by value, not by bits
    with pytest.raises(AssertionError, match=r"zero: float32 differs at 1 of 10 pixels, e\.g\. \[\[3, 1\]\]"):
        H.check(g, u8, neg, "zero")

    other8, other32 = u8.copy(), f32.copy()                       # (0, 0) and (4, 3) are not sampled
    other8[:, 0, 0] ^= 0xFF
    other32[:, 4, 3] = -1.0
    H.check(g, other8, other32, "unsampled")


def test_check_honours_x0_and_key():
    g, u8, f32, plain = _fixture()
    slab8, slab32 = np.roll(u8, -2, axis=1), np.roll(f32, -2, axis=1)        # column 0 of these is column 2 of the frame
    H.check(g, slab8, slab32, "slab", x0=2)
    with pytest.raises(AssertionError, match="uint8"):
        H.check(g, slab8, slab32, "slab read as the frame")
    with pytest.raises(AssertionError, match="float32"):
        H.check(g, u8, slab32, "float32 slab read as the frame")
    H.check(g, plain, None, "the second key", key="u8_plain")
    H.check(g, plain, f32, "the second key, float32 from rgb64", key="u8_plain")
    with pytest.raises(AssertionError, match="uint8"):
        H.check(g, plain, None, "the second frame under the first key")
    with pytest.raises(AssertionError, match="uint8"):
        H.check(g, u8, None, "the first frame under the second key", key="u8_plain")


class Stub:
    """Records the entry calls of a walk and answers each with the true frame, or with `wrong` = (step, "u8" or "f32") off by one
    level or one ulp at a sampled pixel.  Device memory is a dict of what was last rendered into each allocation."""

    def __init__(self, u8, f32, wrong=None):
        self.u8, self.f32, self.wrong, self.entries, self.mem, self.explicit, self.slot = u8, f32, wrong, [], {}, False, None

    def _frames(self, step):
        self.entries.append(step)
        u8, f32 = self.u8.copy(), self.f32.copy()
        if self.wrong == (step, "u8"):
            u8[0, 6, 0] ^= 1
        if self.wrong == (step, "f32"):
            f32[2, 6, 0] = np.nextafter(f32[2, 6, 0], np.float32(0.0))
        return u8, f32

    def params(self, amb, lamb, refl, depth, aa, **kw):
        assert (amb, lamb, refl) == tuple(H.IGNORED.values()) and kw == dict(spp=0, seed=5)
        return "params"

    def render(self, amb, lamb, refl, depth, aa, *, u8, f32, flags, spp, seed):
        assert (amb, lamb, refl, spp, seed) == (*H.IGNORED.values(), 0, 5)
        return self._frames("explicit" if self.explicit else ("per_pixel" if flags == H.AA_PER_PIXEL else "render"))

    def malloc(self, n):
        self.mem[len(self.mem) + 1] = None
        return len(self.mem)

    def free(self, d):
        del self.mem[d]

    def _store(self, step, d8, d32, n=None):
        u8, f32 = self._frames(step)
        self.mem[d8] = u8 if n is None else np.stack([u8] * n)
        if d32 is not None:
            self.mem[d32] = f32 if n is None else np.stack([f32] * n)

    def render_device(self, p, x0, x1, d8, d32, plane_stride):
        assert (p, x0, x1, plane_stride) == ("params", 0, W, W * HT)
        self._store("device", d8, d32)

    def render_sequence(self, p, x0, x1, n, d8, d32, plane_stride, frame_stride, cameras, streams, frames_per_launch):
        assert (n, frame_stride, streams, frames_per_launch) == (3, 3 * W * HT, None, 2)
        assert cameras is None or cameras.shape == (3, 12)
        self._store("sequence" if cameras is None else "sequence_cameras", d8, d32, n)

    def render_begin(self, slot, amb, lamb, refl, depth, aa, o8, o32, **kw):
        self.slot = (slot, o8, o32)

    def render_end(self, slot):
        assert slot == self.slot[0]
        self.slot[1][...], self.slot[2][...] = self._frames("begin_end")

    def sync(self):
        pass

    def h2d(self, d, host):
        assert not host.any()
        self.mem[d] = None

    def d2h(self, host, d):
        host[...] = self.mem[d]


def _setup(r, g, explicit=False):
    r.explicit = explicit
    return W, HT


ROWS = {   # module -> (cameras, begin_end)
    "materials": (False, False), "refraction": (False, False), "scatter": (False, True), "soft_shadows": (False, True),
    "lens": (True, True), "textures": (True, True), "lighting": (True, True), "sky": (True, True)}
STEPS = {"render": "^rt_render:", "device": "^rt_render_device:", "sequence": "^rt_render_sequence cameras=False frame 0:",
         "sequence_cameras": "^rt_render_sequence cameras=True frame 0:", "begin_end": "^rt_render_begin/end:",
         "explicit": "^explicit pixel_loc:", "per_pixel": "^RT_FLAG_AA_PER_PIXEL:"}


def _walk(stub, g, big=False, cameras=True, begin_end=True, explicit=True):
    H.walk_entry_points(stub, g, _setup, big, cameras=cameras, begin_end=begin_end, explicit=explicit)
    assert not stub.mem, "device memory left allocated"
    return stub.entries


@pytest.mark.parametrize("module", list(ROWS))
def test_walk_makes_each_modules_entry_calls(module):
    cameras, begin_end = ROWS[module]
    g, u8, f32, _ = _fixture(aa=1)
    want = ["render", "device", "sequence"] + ["sequence_cameras"] * cameras + ["begin_end"] * begin_end + ["explicit", "per_pixel"]
    assert _walk(Stub(u8, f32), g, cameras=cameras, begin_end=begin_end) == want


def test_walk_steps_that_depend_on_the_fixture():
    full = list(STEPS)
    for aa, skipped in ((0, {"per_pixel"}), (2, {"explicit", "per_pixel"})):
        g, u8, f32, _ = _fixture(aa=aa)
        assert _walk(Stub(u8, f32), g) == [s for s in full if s not in skipped], aa
    g, u8, f32, _ = _fixture(aa=1)
    assert _walk(Stub(u8, f32), g, explicit=False) == [s for s in full if s != "explicit"]        # the 256-sphere case
    big = Stub(u8, f32, wrong=("device", "f32"))                 # a large fixture: no begin/end, and no float32 device buffer to read
    assert _walk(big, g, big=True) == [s for s in full if s != "begin_end"]


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("step", list(STEPS))
def test_walk_names_the_step_with_a_wrong_frame(step, kind):
    g, u8, f32, _ = _fixture(aa=1)
    stub = Stub(u8, f32, wrong=(step, kind))
    with pytest.raises(AssertionError, match=STEPS[step] + (" uint8" if kind == "u8" else " float32") + r" differs at 1 of 10 pixels, e\.g\. \[\[6, 0\]\]"):
        _walk(stub, g)
    assert stub.entries[-1] == step                               # (the walk stopped there)
