"""Bloom on the CPU (rt_film_bloom): the header, the binding and the exported symbol; properties of the numpy restatement
bloom.bloom_reference on constructed inputs; the text the kernels compile (python-ray-tracer_amd/csrc/rt_bloom.h: the per-element
functions, the tile kernel's phases, the plan; rt_film_launch.h: check_film_bloom) run by tests/algo/bloom_check.cpp under
AddressSanitizer and UBSan and compared bit for bit with bloom_reference; Film's call sequences and ValueErrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from film_stub import NoDevice
from test_film import same_bits
import bloom_cases as bc

from python_ray_tracer_amd import Film, bloom as B
from python_ray_tracer_amd import _lib as L

ALGO = os.path.join(REPO, "tests", "algo")

CONTRACT = ("m_c = s[c][p] / (double)n;      out[c][p] = m_c",
            "levels == 0:  nothing else is evaluated",
            "mx = m_0 > m_1 ? m_0 : m_1;   mx = mx > m_2 ? mx : m_2",
            "mx > threshold:  g = (mx - threshold) / mx;   b_0[c][p] = m_c > 0 ? m_c * g : +0.0        else:  b_0[c][p] = +0.0",
            "wl = strength / (double)levels   (once)",
            "for i = 0 .. levels-1:    step = 1 << i;     k = (1/16, 1/4, 3/8, 1/4, 1/16)",
            "t[c][x,y]       = T after:  T = +0.0;  for d = -2..2:  qx = x + step*d;  0 <= qx < ws:  T = T + k[d] * b_i[c][qx, y]",
            "b_{i+1}[c][x,y] = B after:  B = +0.0;  for d = -2..2:  qy = y + step*d;  0 <= qy < h:   B = B + k[d] * t[c][x, qy]",
            "out[c][p] = out[c][p] + wl * b_{i+1}[c][p]")


def test_header_binding_exported_symbol_and_contract(tmp_path):
    hdr = open(os.path.join(REPO, "include", "mi355rt.h")).read()
    assert "int rt_film_bloom(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const rt_bloom *bl," in hdr
    assert "#define RT_ABI_VERSION 7" in hdr and L.RT_ABI_VERSION == 7
    assert (L.RT_BLOOM_MAX_LEVELS, L.RT_BLOOM_WORK_PLANES, L.RT_BLOOM_NO_TILES) == (8, 6, 1)
    bl = L.PROTOTYPES["rt_film_bloom"]
    assert bl[0] is C.c_int and len(bl[1]) == 12 and all(bl[1][i] is C.c_int64 for i in (2, 5, 8, 10)) and bl[1][6] == C.POINTER(L.rt_bloom)
    assert bl[1][3] is C.c_int and bl[1][4] is C.c_int and "rt_film_bloom" in L.LATER_ENTRIES
    assert C.sizeof(L.rt_bloom) == 24 and [f[0] for f in L.rt_bloom._fields_] == ["threshold", "strength", "levels", "flags"]
    src = tmp_path / "size.c"
    src.write_text('#include "mi355rt.h"\n_Static_assert(sizeof(rt_bloom) == 24, "rt_bloom is 24 bytes");\n'
                   '_Static_assert(RT_BLOOM_MAX_LEVELS == 8 && RT_BLOOM_WORK_PLANES == 6 && RT_BLOOM_NO_TILES == 1, "constants");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)])
    lib = L.load()                                               # the cross-compiled library
    assert lib.rt_abi_version() == 7 and hasattr(lib, "rt_film_bloom")
    at = hdr.index("rt_film_bloom: d_sum is a film sum")
    for line in CONTRACT:                                         # header and numpy restatement state the same arithmetic, line for line
        assert line in hdr[at:], line
        assert line in B.bloom_reference.__doc__, line
    for name in ("README.md", "DESIGN.md"):
        assert "rt_film_bloom" in open(os.path.join(REPO, name)).read(), name


# ---------------------------------------------------------------------------------------------------------------------
# The generator, and properties of the restatement

def test_the_generator_exercises_both_branches_of_the_bright_pass():
    for ws, h in ((37, 29), (64, 64), (97, 71), (5, 300)):
        for n in (1, 7):
            s = bc.bloom_sums(ws, h, n)
            assert 0.1 < bc.glowing_share(s, n) < 0.9, (ws, h, n, bc.glowing_share(s, n))
            m = s / n
            assert (m == 0.0).mean() > 0.05 and (m < 0.0).any() and (m.max(axis=0) >= 1e4).any() and m.max() <= 1e4
            assert not s.flags.writeable and bc.bloom_sums(ws, h, n) is s


@pytest.mark.parametrize("n", [1, 7])
def test_levels_zero_high_threshold_and_zero_strength_return_the_mean_bit_for_bit(n):
    s = bc.bloom_sums(37, 29, n)
    mean = s / np.float64(n)
    assert same_bits(B.bloom_reference(s, n, 255.0, 0.5, 0), mean)
    for levels in (1, 3, 8):
        assert same_bits(B.bloom_reference(s, n, 1e9, 0.5, levels), mean)       # nothing is brighter than the threshold
        assert same_bits(B.bloom_reference(s, n, 255.0, 0.0, levels), mean)     # adding +0.0 leaves the mean, negatives included
        assert not same_bits(B.bloom_reference(s, n, 255.0, 0.5, levels), mean)
    four = np.concatenate([s, np.full((1,) + s.shape[1:], np.nan)])             # a four-plane buffer: only planes 0..2 are read
    assert same_bits(B.bloom_reference(four, n, 255.0, 0.5, 3), B.bloom_reference(s, n, 255.0, 0.5, 3))


def test_delta_response():
    ws, h = 97, 71
    s = np.zeros((3, ws, h))
    cx, cy = ws // 2, h // 2
    s[:, cx, cy] = (256.0, 128.0, 64.0)
    k = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    glow = B.bloom_reference(s, 1, 0.0, 1.0, 1) - s
    want = np.zeros_like(s)
    for c, v in enumerate((256.0, 128.0, 64.0)):
        want[c, cx - 2:cx + 3, cy - 2:cy + 3] = v * np.outer(k, k)
    assert same_bits(glow, want)                                  # exactly 256 k (x) k on the 5 x 5 around it: every product a dyadic number
    glow = B.bloom_reference(s, 1, 0.0, 1.0, 4) - s               # reach 2 * (1 + 2 + 4 + 8) = 30 < 35: the support stays inside
    assert glow[:, 0].max() == 0.0 and glow[:, -1].max() == 0.0 and glow[:, :, 0].max() == 0.0 and glow[:, :, -1].max() == 0.0
    assert tuple(glow.sum(axis=(1, 2))) == (256.0, 128.0, 64.0)
    assert (glow >= 0.0).all() and glow[0, cx, cy] == glow[0].max()
    assert same_bits(glow[1], glow[0] / 2) and same_bits(glow[2], glow[0] / 4)          # the glow keeps the hue
    wide = B.bloom_reference(s, 1, 0.0, 1.0, 8) - s
    sums = wide.sum(axis=(1, 2))
    assert (sums < (256.0, 128.0, 64.0)).all() and (sums > 0).all()                     # light leaves the frame and is lost
    # the threshold takes its share off the brightest channel and scales the others with it
    g = (256.0 - 64.0) / 256.0
    part = B.bloom_reference(s, 1, 64.0, 1.0, 1) - s
    assert same_bits(part, want * g)


def test_a_negative_channel_of_a_bright_pixel_contributes_plus_zero():
    s = np.zeros((3, 9, 9))
    s[:, 4, 4] = (1000.0, -50.0, 0.0)
    out = B.bloom_reference(s, 1, 255.0, 1.0, 2)
    assert same_bits(out[1], s[1]) and same_bits(out[2], s[2])    # +0.0 everywhere: the negative mean stays, nothing spreads
    assert not np.signbit(out[2]).any() and out[0, 3, 4] > 0.0
    neg = np.where(s == 0.0, 0.0, -s)                             # (-1000, 50, +0.0): the brightest channel is the second
    assert same_bits(B.bloom_reference(neg, 1, 0.0, 1.0, 2)[0], neg[0])


def test_reference_value_errors():
    s = np.zeros((3, 4, 4))
    for bad in (dict(threshold=-1.0), dict(threshold=np.nan), dict(strength=np.inf), dict(strength=-0.5), dict(levels=9), dict(levels=-1)):
        kw = dict(threshold=255.0, strength=0.25, levels=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            B.bloom_reference(s, 1, **kw)
    with pytest.raises(ValueError):
        B.bloom_reference(s, 0)
    with pytest.raises(ValueError):
        B.bloom_reference(s[:2], 1)
    with pytest.raises(ValueError):
        B.bloom_reference(s.astype(np.float32), 1)
    with pytest.raises(ValueError, match="flags"):
        B.check_bloom(255.0, 0.25, 2, 2)
    assert B.check_bloom(0, 0, 0, 1) == (0.0, 0.0, 0, 1)


# ---------------------------------------------------------------------------------------------------------------------
# The kernels' text under the sanitizers against the restatement

def check_cases():
    """[dict(s, n, levels, threshold, strength, pads, compare)]: every frame at levels 0, 1, 3 and 8 with odd strides, thresholds 0 and
    255, both n; then one non-finite input."""
    cases = []
    k = 0
    for ws, h in bc.FRAMES:
        for levels in (0, 1, 3, 8):
            n = (1, 7)[k % 2]
            cases.append(dict(s=bc.bloom_sums(ws, h, n), n=n, levels=levels, threshold=(255.0, 0.0, 255.0)[k % 3], strength=(0.5, 4.0)[(k // 2) % 2],
                              pads=((1, 3, 5), (0, 0, 0), (3, 5, 1))[k % 3], compare=1))
            k += 1
    cases.append(dict(s=bc.nonfinite_sums(37, 29, 2), n=2, levels=3, threshold=255.0, strength=0.5, pads=(1, 1, 1), compare=0))
    return cases


def test_kernel_text_under_sanitizers_matches_numpy(tmp_path):
    exe, table, got = str(tmp_path / "bloom_check"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ALGO, "bloom_check.cpp")])
    cases = check_cases()
    with open(table, "wb") as fh:
        fh.write(np.array([len(cases)], "<i8").tobytes())
        for c in cases:
            _, ws, h = c["s"].shape
            fh.write(np.array([ws, h, c["n"], c["levels"], *c["pads"], c["compare"]], "<i8").tobytes())
            fh.write(np.array([c["threshold"], c["strength"]], "<f8").tobytes())
            padded = np.full((3, ws * h + c["pads"][0]), 1e300)
            padded[:, :ws * h] = c["s"].reshape(3, -1)
            fh.write(padded.astype("<f8").tobytes())
    res = subprocess.run([exe, table, got], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stdout + res.stderr
    assert res.stdout.strip() == f"cases={len(cases)} ok", res.stdout
    raw = open(got, "rb").read()
    at = 0
    glowing = 0
    for i, c in enumerate(cases):
        want = B.bloom_reference(c["s"], c["n"], c["threshold"], c["strength"], c["levels"])
        out = np.frombuffer(raw, "<f8", want.size, at).reshape(want.shape)
        at += 8 * want.size
        if not c["compare"]:
            assert not np.isfinite(want).all()
            continue
        bad = np.argwhere(out.view(np.uint64) != want.view(np.uint64))
        assert bad.size == 0, (i, want.shape, c["levels"], len(bad), bad[:4], out[tuple(bad[0])], want[tuple(bad[0])])
        assert np.isfinite(want).all()
        if c["levels"]:
            glowing += int((want != c["s"] / np.float64(c["n"])).sum())
    assert at == len(raw) and glowing > 20000 and len(cases) == 4 * len(bc.FRAMES) + 1


# ---------------------------------------------------------------------------------------------------------------------
# Film's call sequences, before the library sees anything

def test_film_bloom_call_sequences_and_value_errors():
    r = NoDevice()
    p = L.rt_params()
    with Film(r) as film:
        with pytest.raises(ValueError, match="no pass"):
            film.bloom()
        film.accumulate(p, 2)
        n = len(r.calls)
        film.resolve()                                            # bloom=False: exactly the calls made before
        assert [c[0] for c in r.calls[n:]] == ["malloc", "resolve", "free"] and film.d_bloom is None and film.d_bloom_work is None
        with pytest.raises(ValueError, match="bloom\\(\\)"):
            film.resolve(bloom=True)
        for bad in (dict(levels=9), dict(threshold=-1.0), dict(strength=float("nan"))):
            with pytest.raises(ValueError):
                film.bloom(**bad)
        with pytest.raises(ValueError, match="denoise\\(\\)"):      # the source is what resolve would show: it must exist
            film.bloom(denoised=True)
        n = len(r.calls)
        film.bloom()
        assert r.calls[n:n + 2] == [("malloc", 24 * 32), ("malloc", 48 * 32)]
        assert r.calls[n + 2] == ("bloom", film.d_sum, 8, 4, 2, film.d_bloom, film.d_bloom_work,
                                  dict(threshold=255.0, strength=0.25, levels=6, stream=None))
        assert len({film.d_sum, film.d_bloom, film.d_bloom_work}) == 3
        film.resolve(bloom=True, white=400.0)
        assert [c for c in r.calls if c[0] == "resolve"][-1][1:5] == (film.d_bloom, 8, 4, 1)
        with pytest.raises(ValueError, match="denoise\\(\\)"):      # a source that does not exist yet
            film.resolve(bloom=True, denoised=True)
        film.denoise()
        with pytest.raises(ValueError, match="bloom\\(\\)"):
            film.resolve(bloom=True, denoised=True)
        n = len(r.calls)
        film.bloom(threshold=300, strength=1, levels=2, denoised=True)
        assert [c[0] for c in r.calls[n:]] == ["bloom"] and r.calls[-1][1:5] == (film.d_denoised, 8, 4, 1)
        film.resolve(bloom=True, denoised=True)
        assert [c for c in r.calls if c[0] == "resolve"][-1][1:5] == (film.d_bloom, 8, 4, 1)
        with pytest.raises(ValueError, match="bloom\\(\\)"):
            film.resolve(bloom=True)
        film.accumulate(p, 1)                                     # more passes: the glow was that of the earlier mean
        with pytest.raises(ValueError):
            film.resolve(bloom=True, denoised=True)
        film.bloom(levels=0)
        film.resolve(bloom=True)
        film.clear()
        film.accumulate(p, 3)
        with pytest.raises(ValueError, match="bloom\\(\\)"):
            film.resolve(bloom=True)
        held = {film.d_bloom, film.d_bloom_work}
    assert held <= {c[1] for c in r.calls if c[0] == "free"}
