"""CPU-only tests: what Film records of its derived pictures (the temporal mean, the filtered mean, the mean plus glow, the metering),
on the recording stub of film_stub.py.  A picture belongs to what it was made from: a request whose chain is broken is refused
before any device call, and the film's buffers are those of film.BUFFERS, each freed once."""
import numpy as np
import pytest

from film_stub import NoDevice

from python_ray_tracer_amd import Film, film as F
from python_ray_tracer_amd import _lib as L


def _film(r, **kw):
    film = Film(r, **kw)
    film.accumulate(L.rt_params(), 2)
    return film


def _shown(r):
    """(kind, source address, ws, h, n[, state]) of the last resolve call the stub recorded."""
    call = [c for c in r.calls if c[0] in ("resolve", "resolve_metered")][-1]
    return call[:6] if call[0] == "resolve_metered" else call[:5]


# The four sequences that showed a picture made from something older or something else: what leads to the request, the request,
# the fragments its refusal holds, the step to run again, and what the accepted request then reads
STALE = {
    "A": (lambda f: (f.temporal(), f.denoise(temporal=True)), dict(denoised=True),
          ("call denoise() first", "temporal mean"), lambda f: f.denoise(), lambda f: ("resolve", f.d_denoised, 8, 4, 1)),
    "B": (lambda f: (f.denoise(), f.bloom(denoised=True), f.denoise(sigma=0.5)), dict(bloom=True, denoised=True),
          ("call bloom() with the same",), lambda f: f.bloom(denoised=True), lambda f: ("resolve", f.d_bloom, 8, 4, 1)),
    "C": (lambda f: (f.bloom(), f.meter(bloom=True), f.bloom(strength=0.5)), dict(bloom=True, auto_exposure=True),
          ("call meter() with the same",), lambda f: f.meter(bloom=True), lambda f: ("resolve_metered", f.d_bloom, 8, 4, 1, f.d_meter_state)),
    "D": (lambda f: (f.temporal(), f.denoise(temporal=True), f.temporal(max_history=2)), dict(denoised=True, temporal=True),
          ("call denoise(temporal=True) first",), lambda f: f.denoise(temporal=True), lambda f: ("resolve", f.d_denoised, 8, 4, 1)),
}


@pytest.mark.parametrize("name", sorted(STALE))
def test_a_picture_of_something_older_or_something_else_is_refused(name):
    before, request, fragments, again, shown = STALE[name]
    r = NoDevice()
    with _film(r) as film:
        before(film)
        for call in (lambda: film.resolve(**request), lambda: film.resolve_device(d_u8=1, **request)):
            n = len(r.calls)
            with pytest.raises(ValueError) as e:
                call()
            assert all(fragment in str(e.value) for fragment in fragments), str(e.value)
            assert len(r.calls) == n                              # refused before any device call: no malloc, no launch
        again(film)
        film.resolve(**request)
        assert _shown(r) == shown(film)
        film.resolve_device(d_u8=1, **request)
        assert _shown(r) == shown(film)


def test_a_step_whose_source_is_missing_reaches_no_device_call():
    r = NoDevice()
    with _film(r) as film:
        n = len(r.calls)
        for step in (film.denoise, film.bloom, film.meter):       # (the filter used to render guides and allocate before it refused)
            with pytest.raises(ValueError, match="call temporal\\(\\) first"):
                step(temporal=True)
        assert len(r.calls) == n and not (film.d_guides or film.d_denoised or film.d_bloom or film.d_meter_hist)


def _make(film, product, denoised=False, temporal=False, bloom=False):
    """Write `product` with the step that makes it on the way to, or from, what resolve(denoised, temporal, bloom) shows: each step
    takes the flags it has and ignores the others."""
    {"sum": lambda: film.accumulate(L.rt_params(), 1), "temporal": lambda: film.temporal(),
     "denoised": lambda: film.denoise(temporal=temporal), "bloom": lambda: film.bloom(denoised=denoised, temporal=temporal),
     "meter": lambda: film.meter(denoised=denoised, temporal=temporal, bloom=bloom)}[product]()


# every edge of the graph: (the product, the flags of the source it is made from)
EDGES = [("temporal", {}), ("denoised", {}), ("denoised", dict(temporal=True)), ("bloom", {}), ("bloom", dict(temporal=True)),
         ("bloom", dict(denoised=True)), ("meter", {}), ("meter", dict(temporal=True)), ("meter", dict(denoised=True)), ("meter", dict(bloom=True))]


@pytest.mark.parametrize("product,flags", EDGES, ids=[f"{F.products(**fl)[-1]}->{p}" for p, fl in EDGES])
def test_writing_the_upstream_again_and_nothing_else_makes_a_product_stale(product, flags):
    chain = F.products(**flags)
    r = NoDevice()
    with _film(r, moments=True) as film:
        assert not film.current(product)
        for step in chain[1:] + (product,):                       # what the product is made from, upstream first, then the product
            _make(film, step, **flags)
        assert film.current(product) and all(film.current(p) for p in chain[1:])
        film.variance()                                           # writes a work buffer: no product
        for other in ("temporal", "denoised", "bloom", "meter"):  # a plain write of every product that is not on the way
            if other not in chain and other != product:
                _make(film, other)
                assert film.current(other)
        assert film.current(product), "a write of something the product does not read made it stale"
        _make(film, chain[-1], **flags)                           # the product it reads, written again
        assert not film.current(product) and all(film.current(p) for p in chain[1:])
        _make(film, product, **flags)
        assert film.current(product)
        film.accumulate(L.rt_params(), 1)                         # more passes: everything downstream of the sum
        assert not any(film.current(p) for p in ("temporal", "denoised", "bloom", "meter"))
    with pytest.raises(ValueError, match="product"):
        film.current("sum")


def test_every_buffer_is_in_the_table_and_freed_once():
    r = NoDevice()
    p = L.rt_params()
    film = Film(r, moments=True)
    for frame in range(3):                                        # two next_frame() cycles: one swaps, one blends the plain mean
        r.camera = (np.array([0.1 * frame, 0.0, 0.0]), np.eye(3).reshape(9))
        film.next_frame()
        film.accumulate(p, 2)
        film.guides()
        if frame != 1:
            film.temporal()
            film.denoise(temporal=True)
            film.denoise(variance=True, temporal=True)
            film.variance(temporal=True)
            film.bloom(denoised=True, temporal=True)
            film.meter(denoised=True, temporal=True, bloom=True)
            film.resolve(denoised=True, temporal=True, bloom=True, auto_exposure=True, f32=True, flags=L.RT_FLAG_U8_HWC)
            film.resolve_device(d_u8=1, temporal=True)
        film.denoise()
        film.denoise(variance=True)
        film.variance()
        film.bloom()
        film.meter(rate=0.5)
        film.resolve(auto_exposure=True)
        assert film.current("meter") and film.exposure().shape == (4,) and film.histogram().shape == (L.RT_METER_BINS,)
        film.reset_meter()
        assert not film.current("meter")
    film.clear()
    film.accumulate(p, 1)
    film.temporal()
    assert all(getattr(film, name) for name in F.BUFFERS), [name for name in F.BUFFERS if not getattr(film, name)]
    assert {name for name in vars(film) if name.startswith("d_")} == set(F.BUFFERS)
    film.close()
    handed_out = [4096 * (i + 1) for i in range(sum(c[0] == "malloc" for c in r.calls))]
    assert sorted(c[1] for c in r.calls if c[0] == "free") == handed_out      # every address freed, each once
    assert not any(getattr(film, name) for name in F.BUFFERS)
    n = len(r.calls)
    film.close()
    assert len(r.calls) == n                                      # closing twice frees nothing more
