"""What Film touches of a Renderer, with no device behind it: every device call is recorded in `calls` as a tuple (kind, *positional
arguments), followed by the dict of keyword arguments for the kinds listed with True below.  malloc hands out distinct addresses
(4096, 8192, ...), d2h fills the host array with zeros and is not recorded.  The Film call-sequence tests of test_film, test_denoise,
test_temporal, test_variance, test_temporal_moments, test_bloom, test_meter and test_film_provenance run on it."""
import numpy as np

# Renderer method -> (the kind recorded, whether the keyword arguments are recorded too)
RECORDED = {"film_accumulate": ("accumulate", False), "film_accumulate_moments": ("accumulate_moments", False),
            "film_resolve": ("resolve", False), "film_resolve_metered": ("resolve_metered", False), "render_guides": ("guides", False),
            "film_denoise": ("denoise", True), "film_denoise_variance": ("denoise_variance", True),
            "film_denoise_variance_temporal": ("denoise_variance_temporal", True), "film_temporal": ("temporal", True),
            "film_temporal_moments": ("temporal_moments", True), "film_bloom": ("bloom", True), "film_meter": ("meter", True),
            "film_meter_solve": ("solve", True)}


class NoDevice:
    closed = False

    def __init__(self, w=8, h=4):
        self.w, self.h, self.calls, self.next = w, h, [], 0
        self.camera = (np.zeros(3), np.eye(3).reshape(9))

    def malloc(self, n):
        self.calls.append(("malloc", n))
        self.next += 4096
        return self.next

    def free(self, d):
        self.calls.append(("free", d))

    def sync(self, stream=None):
        self.calls.append(("sync", stream))

    def d2h(self, host, d):
        host[...] = 0

    def h2d(self, d, host):
        self.calls.append(("h2d", d, host.tobytes()))


def _recorder(kind, with_keywords):
    def call(self, *a, **kw):
        self.calls.append((kind,) + a + ((kw,) if with_keywords else ()))
    return call


for _name, (_kind, _with_keywords) in RECORDED.items():
    setattr(NoDevice, _name, _recorder(_kind, _with_keywords))
