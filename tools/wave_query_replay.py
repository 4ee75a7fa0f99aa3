#!/usr/bin/env python3
"""Replay a workload's frame in float64 on the CPU with the render kernel's 8x8 tiles and count, per bounce, the wave-level scene
queries and how many of them end their cull with an empty mask (CPU only, numpy, no GPU).

    python tools/wave_query_replay.py [--workload c2_1920x1080_s8_d3] [--slab 240]

A wave is a tile of 8x8 pixels (lane >> 3 -> x, lane & 7 -> y, rt_layout.h TILE).  A closest-hit wave-query is a tile with a live
lane at a bounce; a shadow wave-query is a (tile, light) pair with a lane whose Lambert term is positive.  A query's cull mask is
empty when EVERY querying lane holds a miss certificate for EVERY sphere.  The replay's certificate is the exact one with a relative
margin of 1e-5: the line misses the sphere (D < -m) or, for rays without an anchor and for the sphere a shadow ray starts on, the
sphere lies behind the origin (s > m and |L|^2 - r^2 > m), m = 1e-5 (|L|^2 + r^2).  The kernel's float32 certificates (rt_cull.h)
have margins of 2^-19 to 2^-18 of the same sums, so the counts are the kernel's up to the few queries within those margins of a
boundary.  Primary rays use the camera as their anchor, shadow rays their light, reflected rays none.
The frame is replayed at one sample per pixel through the pixel centres (the stochastic configurations: their first-order picture).
Also printed: the wave-level light iterations and how many the facing skip (rt_facing.h) takes out, and the share of queries that
miss a bounding sphere of the whole scene (a pre-test in front of the cull would save at most that).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from python_ray_tracer_amd import workloads  # noqa: E402

TILE = 8
MARGIN = 1e-5


def tiles(a, fn):
    """(w, h) bool -> (w/8, h/8): fn over each tile's 64 lanes"""
    w, h = a.shape
    return fn(a.reshape(w // TILE, TILE, h // TILE, TILE), axis=(1, 3))


def line_D(A, R, c, r2):
    """s = (A-c).R, |A-c|^2 and D = s^2 - |A-c|^2 + r2 of the line through A with unit direction R"""
    L = A - c
    s = (L * R).sum(-1)
    ll = (L * L).sum(-1)
    return s, ll, s * s - ll + r2


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def replay_slab(wl, x0, x1, tot):
    w, h, depth = wl["w"], wl["h"], wl["depth"]
    sp, li, pl = (np.asarray(a, np.float64) for a in (wl["spheres"], wl["lights"], wl["planes"]))
    S, Ln, Pn = sp.shape[1], li.shape[1], pl.shape[1]
    C, r2 = sp[0:3].T, sp[3] * sp[3]
    lights = li[0:3].T
    p0, pn = pl[0:3].T, pl[3:6].T
    pnu = unit(pn) if Pn else pn
    cam = wl["camera"]
    px, y0, dy, z0, dz = cam.raygen()
    rot, co = np.asarray(cam.rotation, np.float64), np.asarray(cam.position, np.float64)
    ws = x1 - x0
    X, Y = np.meshgrid(np.arange(x0, x1), np.arange(h), indexing="ij")
    d = unit(np.stack([np.full((ws, h), px), X * dy + y0, Y * dz + z0], -1) @ rot.T)
    o = np.broadcast_to(co, d.shape).copy()
    alive = np.ones((ws, h), bool)
    if S:                                                      # a bounding sphere of the whole scene
        bc = C.mean(0)
        br2 = float((np.linalg.norm(C - bc, axis=1) + sp[3]).max()) ** 2

    def add(key, b, n):
        tot.setdefault(key, np.zeros(depth + 1, np.int64))[b] += int(n)

    for b in range(depth + 1):
        wav = tiles(alive, np.any)
        add("closest", b, wav.sum())
        best = np.full((ws, h), 999.0)
        idx = np.full((ws, h), -1)
        typ = np.zeros((ws, h), int)
        open_any = np.zeros((ws, h), bool)
        for k in range(S):
            s, ll, D = line_D(o, d, C[k], r2[k])
            cc = ll - r2[k]
            m = MARGIN * (ll + r2[k])
            cert = (D < -m) if b == 0 else ((D < -m) | ((s > m) & (cc > m)))
            open_any |= alive & ~cert
            q = np.sqrt(np.maximum(D, 0))
            t1 = -s - q
            t = np.where(t1 > 0, t1, -s + q)
            hit = alive & (D >= 0) & ~((s >= 0) & (cc >= 0)) & (t > 0) & (t < best)
            best = np.where(hit, t, best); idx = np.where(hit, k, idx); typ = np.where(hit, 1, typ)
        add("closest_empty", b, (wav & ~tiles(open_any, np.any)).sum())
        if S:
            s, ll, D = line_D(o, d, bc, br2)
            bcert = (D < 0) if b == 0 else ((D < 0) | ((s > 0) & (ll - br2 > 0)))
            add("closest_boundmiss", b, (wav & ~tiles(alive & ~bcert, np.any)).sum())
        for k in range(Pn):
            den = d @ pn[k]
            num = ((p0[k] - o) * pn[k]).sum(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = num / den
            hit = alive & (np.abs(den) >= 0.001) & (t > 0) & (t < best)
            best = np.where(hit, t, best); idx = np.where(hit, k, idx); typ = np.where(hit, 2, typ)
        alive = alive & (typ != 0)
        Pt = o + best[..., None] * d
        N = np.zeros_like(Pt)
        if S:
            with np.errstate(divide="ignore", invalid="ignore"):
                N = np.where((typ == 1)[..., None], unit(Pt - C[np.clip(idx, 0, S - 1)]), N)
        if Pn:
            N = np.where((typ == 2)[..., None], pnu[np.clip(idx, 0, Pn - 1)], N)
        Pb = Pt + 0.0002 * N
        selfk = np.where(typ == 1, idx, -1)
        for m_ in range(Ln):
            vv = lights[m_] - Pb
            it = tiles(alive, np.any)
            add("light_iterations", b, it.sum())
            add("facing_skipped", b, (it & ~tiles(alive & ~((vv * N).sum(-1) < 0), np.any)).sum())
            with np.errstate(divide="ignore", invalid="ignore"):
                Ld = unit(vv)
            want = alive & (wl["lamb"] * (Ld * N).sum(-1) > 0)
            wq = tiles(want, np.any)
            add("shadow", b, wq.sum())
            add("shadow_lanes", b, want.sum())
            open_any = np.zeros((ws, h), bool)
            for k in range(S):
                _, ll, D = line_D(lights[m_], Ld, C[k], r2[k])
                cert = D < -MARGIN * (ll + r2[k])
                so, llo, Do = line_D(Pb, Ld, C[k], r2[k])
                mo = MARGIN * (llo + r2[k])
                cert = np.where(selfk == k, cert | (Do < -mo) | ((so > mo) & (llo - r2[k] > mo)), cert)
                open_any |= want & ~cert
            add("shadow_empty", b, (wq & ~tiles(open_any, np.any)).sum())
            if S:
                _, _, D = line_D(lights[m_], Ld, bc, br2)
                add("shadow_boundmiss", b, (wq & ~tiles(want & ~(D < 0), np.any)).sum())
        Rd = d - 2 * (d * N).sum(-1)[..., None] * N
        with np.errstate(divide="ignore", invalid="ignore"):
            o = np.where(alive[..., None], Pt + 0.0002 * N + 0.0002 * Rd, o)
            d = np.where(alive[..., None], unit(Rd), d)


def fmt(n):
    return f"{int(n):,}".replace(",", " ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default=workloads.HEADLINE, choices=sorted(workloads.CONFIGS))
    ap.add_argument("--slab", type=int, default=240, help="columns replayed at a time (a multiple of 8; bounds the memory)")
    a = ap.parse_args()
    wl = workloads.build(a.workload)
    if wl["w"] % TILE or wl["h"] % TILE or a.slab % TILE:
        sys.exit("frame and slab sizes must be multiples of 8")
    tot = {}
    for x0 in range(0, wl["w"], a.slab):
        replay_slab(wl, x0, min(x0 + a.slab, wl["w"]), tot)
    z = np.zeros(wl["depth"] + 1, np.int64)
    g = lambda k: tot.get(k, z)   # noqa: E731
    print(f"workload {a.workload}: {wl['w']}x{wl['h']}, depth {wl['depth']}, {wl['spheres'].shape[1]} spheres, "
          f"{wl['planes'].shape[1]} planes, {wl['lights'].shape[1]} lights; waves are 8x8 tiles, 1 sample per pixel")
    print("| bounce | closest wave-queries | with empty cull mask | shadow wave-queries | with empty cull mask |")
    print("|---|---|---|---|---|")
    for b in range(wl["depth"] + 1):
        print(f"| {b} | {fmt(g('closest')[b])} | {fmt(g('closest_empty')[b])} | {fmt(g('shadow')[b])} | {fmt(g('shadow_empty')[b])} |")
    c, ce, s, se = (int(g(k).sum()) for k in ("closest", "closest_empty", "shadow", "shadow_empty"))
    pct = lambda n, d: f"{100.0 * n / d:.1f} %" if d else "-"   # noqa: E731
    print(f"| all | {fmt(c)} | {fmt(ce)} ({pct(ce, c)}) | {fmt(s)} | {fmt(se)} ({pct(se, s)}) |")
    print(f"wave-queries: {fmt(c + s)}, with an empty cull mask: {fmt(ce + se)}")
    print(f"wave-level light iterations: {fmt(g('light_iterations').sum())}, facing-skipped: {fmt(g('facing_skipped').sum())}; "
          f"lane-level shadow queries: {fmt(g('shadow_lanes').sum())}")
    worst = max([0.0] + [float(n) / float(d) for k in ("closest", "shadow") for n, d in zip(g(k + "_boundmiss"), g(k)) if d])
    print(f"queries that miss a bounding sphere of the whole scene: at most {100.0 * worst:.1f} % of the queries of a bounce")


if __name__ == "__main__":
    main()
