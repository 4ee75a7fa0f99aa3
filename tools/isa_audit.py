#!/usr/bin/env python3
"""Static audit of one render kernel's gfx950 ISA: which source construct produced every select, compare, move, lane
read/write and exec-mask instruction, per region of the bounce (CPU only, no GPU).

    python tools/isa_audit.py [--tree DIR] [--kernel "false, true, 2, false, false, 0, rt::Family::PLAIN"] [--ground] [--groups N] [--top 40]

Compiles a translation unit that instantiates just that kernel from DIR's rt_device.h (default: this tree; the headline
kernel) with the Makefile's flags plus -gline-tables-only, checks with tools/isa_compare.py's parser that the line info
(--ground: its ground-plane twin, the eighth template argument GROUND = true; --groups N with it: that twin's small-scene twin for N
cull groups, the ninth argument NG; --kernel may also spell all of them)
changes no instruction, disassembles the code object and asks llvm-symbolizer for every instruction's inline stack.
The stack (render_kernel > sample > trace_bounce > closest_hit > sphere_closest ...) and a few source markers place an
instruction in a region; its mnemonic places it in a class.  Prints
  * per region: static counts per class, their price in cycles (profiles/r03_valu_prices.json, 7 waves per SIMD), the
    region's weight from the loop nest (x bounces, x lights, x spheres: trip counts, an upper bound — the cull skips most
    float64 sphere tests) and price x weight, ordered by the weighted price of the AUDITED classes (v_cndmask, v_cmp/v_cmpx,
    v_mov, v_readlane/v_readfirstlane, v_writelane, DPP, exec-mask scalar instructions);
  * per source line: the audited instructions it produced, ordered the same way.
Static counts are not dynamic counts: tools/instr_breakdown.py under rocprofv3 --pmc gives those.
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_compare  # noqa: E402

CSRC = os.path.join("python-ray-tracer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # as the Makefile
LLVM = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "llvm", "bin")
AUDITED = ("cndmask", "cmp", "mov", "readlane", "writelane", "dpp", "exec")
OTHER = ("f64", "trans64", "f32int", "cvt", "salu", "lds", "mem", "ctl")
HELPERS = ("lanes_where", "lane_of", "m_nlt_abs", "m_nlt_neg", "m_ngt", "m_ne", "push_any", "opaque", "pin_lds")
HEADLINE = "false, true, 2, false, false, 0, rt::Family::PLAIN"


def makefile_flags(tree):
    mk = open(os.path.join(tree, CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*\?=\s*(.*)$", mk, flags=re.M).group(1)
    return flags.replace("$(ARCH)", "gfx950").split()


def classify(ins):
    """mnemonic + operands -> class"""
    op = ins.split()[0]
    if "dpp" in op or " row_" in ins or " quad_perm" in ins or "wave_shr" in ins or "row_bcast" in ins:
        return "dpp"
    if op.startswith("v_cndmask"):
        return "cndmask"
    if op.startswith("v_cmp"):
        return "cmp"
    if op.startswith(("v_mov", "v_accvgpr")):
        return "mov"
    if op.startswith(("v_readlane", "v_readfirstlane")):
        return "readlane"
    if op.startswith("v_writelane"):
        return "writelane"
    if op.startswith("s_") and ("saveexec" in op or re.search(r"\bexec\b", ins)):
        return "exec"
    if op.startswith(("v_rsq_f64", "v_rcp_f64", "v_sqrt_f64")):
        return "trans64"
    if op.startswith("v_cvt"):
        return "cvt"
    if op.startswith("v_"):
        return "f64" if re.search(r"_(f64|[iu]64|b64)", op) else "f32int"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_", "s_load", "s_buffer_load")):
        return "mem"
    if op.startswith(("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_endpgm", "s_barrier", "s_sleep", "s_setprio")):
        return "ctl"
    return "salu"


def price_table(path):
    d = {c["class"]: c["w7"]["cycles_simd_span"] for c in json.load(open(path))["classes"]}
    return {"cndmask": d["v_cndmask_b32_e64 (mask in an SGPR pair written outside the loop)"],
            "cmp": d["v_cmp_lt_f64_e64->sgpr"], "mov": d["v_mov_b32"], "mov64": d["v_mov_b64"],
            "readlane": d["v_readlane_b32"], "writelane": d["v_readlane_b32"], "dpp": d["v_mov_b32_dpp"],
            "exec": d["s_and_b64"], "salu": d["s_and_b64"], "f64": d["v_fma_f64"], "trans64": d["v_rsq_f64"],
            "f32int": d["v_fma_f32"], "cvt": d["v_cvt_f64_f32"], "lds": d["ds_read_b64 (wave-uniform address)"],
            "lds_b128": d["ds_read_b128 (wave-uniform address)"], "lds_w64": d["ds_write_b64 (8 B per lane, consecutive)"],
            "mem": 0.0, "ctl": 0.0}


def price(cls, ins, P):
    op = ins.split()[0]
    if cls == "mov" and "b64" in op:
        return P["mov64"]
    if cls == "lds":
        return P["lds_b128"] if "b128" in op else (P["lds_w64"] if op.startswith("ds_write_b64") else P["lds"])
    return P[cls]


class Source:
    """rt_device.h of the audited tree: markers -> line numbers (a marker that is missing is an error, not a guess)."""
    def __init__(self, path):
        self.lines = open(path).read().split("\n")

    def line(self, text, after=1):
        for i in range(after - 1, len(self.lines)):
            if text in self.lines[i]:
                return i + 1
        sys.exit(f"isa_audit: marker not found in rt_device.h: {text!r}")

    def text(self, n):
        return self.lines[n - 1].strip() if 0 < n <= len(self.lines) else ""


def region_of(stack, M):
    """stack: [(function, line)] outermost first, frames of rt_device.h only."""
    reg = "other"
    names = [f for f, _ in stack]
    for f, ln in stack:
        if f.startswith("render_kernel"):
            reg = "prologue (staging, tile)" if ln < M["rk_cam"] else ("ray generation" if ln <= M["rk_sample"] else "store")
        elif f.startswith("sample"):
            reg = "colour accumulation"
        elif f.startswith("trace_bounce"):
            if ln < M["tb_park"]:
                reg = "hit point / normal"
            elif ln == M["tb_set"] or ln >= M["tb_get"]:
                reg = "reflection"
            else:
                reg = "light direction and Lambert"
        elif f.startswith("closest_hit"):
            if ln >= M["ch_planes"]:
                reg = "plane test"
            elif ln >= M["ch_best"]:
                reg = "closest-hit select"
            elif any(n.startswith("cull_mask") for n in names):
                reg = "closest-hit cull"
            else:
                reg = "closest-hit setup (renormalise, loop)"
        elif f.startswith("sphere_closest"):
            reg = "closest-hit running winner" if ln >= M["sc_take"] else "float64 sphere test"
        elif f.startswith("any_hit_masks"):                  # (trees that have it: the lane-mask form of any_hit's loops)
            if ln >= M["am_planes"]:
                reg = "shadow plane test"
            elif any(n.startswith("cull_mask") for n in names):
                reg = "shadow cull"
            else:
                reg = "shadow setup (renormalise, loop, exit ballots)"
        elif f.startswith("any_hit"):
            if ln >= M["ah_planes"]:
                reg = "shadow plane test"
            elif any(n.startswith("cull_mask") for n in names):
                reg = "shadow cull"
            else:
                reg = "shadow setup (renormalise, loop, exit ballots)"
        elif f.startswith("sphere_any"):
            reg = "any-hit sphere test"
    return reg


def weights(B, L, S, Pn):
    g = (S + 3) // 4
    return {"prologue (staging, tile)": 1, "ray generation": 1, "store": 1, "other": 1, "colour accumulation": B,
            "hit point / normal": B, "reflection": B, "light direction and Lambert": B * L,
            "closest-hit setup (renormalise, loop)": B, "closest-hit cull": B * g, "float64 sphere test": B * S,
            "closest-hit running winner": B * S, "closest-hit select": B, "plane test": B * Pn,
            "shadow setup (renormalise, loop, exit ballots)": B * L, "shadow cull": B * L * g,
            "any-hit sphere test": B * L * S, "shadow plane test": B * L * Pn}


def run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    if r.returncode:
        sys.exit(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--kernel", default=HEADLINE, help="template arguments of rt::render_kernel")
    ap.add_argument("--prices", default=os.path.join(REPO, "profiles", "r03_valu_prices.json"))
    ap.add_argument("--bounces", type=int, default=4, help="traces per sample (depth + 1); headline: 4")
    ap.add_argument("--lights", type=int, default=3)
    ap.add_argument("--spheres", type=int, default=8)
    ap.add_argument("--planes", type=int, default=1)
    ap.add_argument("--top", type=int, default=40, help="source lines listed (0: all)")
    ap.add_argument("--ground", action="store_true", help="the kernel's ground-plane twin (GROUND = true)")
    ap.add_argument("--groups", type=int, default=0, help="with --ground: the small-scene twin for that many cull groups (NG = 1 or 2)")
    a = ap.parse_args()
    if a.groups and not a.ground:
        sys.exit("isa_audit: --groups wants --ground (the small-scene kernels are twins of the ground-plane kernels)")
    if a.ground:
        if len(a.kernel.split(",")) != 7:
            sys.exit("isa_audit: --ground wants --kernel with its seven arguments up to the family")
        a.kernel += ", true" + (f", {a.groups}" if a.groups else "")
    tree = os.path.abspath(a.tree)
    hdr = os.path.join(tree, CSRC, "rt_device.h")
    src = Source(hdr)
    P = price_table(a.prices)
    fn = lambda t: src.line(t)   # noqa: E731
    M = {"rk_cam": fn("const V3 o{p.cam_o[0]"), "rk_sample": fn("const V3 c = sample<"),
         "tb_park": fn("dpark(lds.acc, 1, lds.wave)"), "tb_set": fn("dpark.set(d);"), "tb_get": fn("d = dpark.get();"),
         "ch_best": fn("double best = 999.0;"), "ch_planes": fn("const double *pl = lds.recs() + (F32"),
         "sc_take": src.line("if (n > 0.0) {", fn("void sphere_closest(")),
         "ah_planes": fn("const double *pl = lds.recs() + (MODE >= 1")}
    if any("bool any_hit_masks(" in ln for ln in src.lines):
        M["am_planes"] = src.line("const double *pl = lds.recs()", fn("bool any_hit_masks("))
    flags = makefile_flags(tree)
    with tempfile.TemporaryDirectory() as tmp:
        tu = os.path.join(tmp, "one.hip")
        open(tu, "w").write(f'#include "rt_device.h"\ntemplate __global__ void rt::render_kernel<{a.kernel}>(const rt::KParams);\n')
        base = [HIPCC] + flags + ["-I", os.path.join(tree, CSRC), "--cuda-device-only"]
        plain = run(base + ["-Rpass-analysis=kernel-resource-usage", "-S", "-o", os.path.join(tmp, "p.s"), tu])
        run(base + ["-gline-tables-only", "-S", "-o", os.path.join(tmp, "g.s"), tu])
        fp = isa_compare.functions(open(os.path.join(tmp, "p.s")).read())
        fg = isa_compare.functions(open(os.path.join(tmp, "g.s")).read())
        sym = [n for n in fp if "render_kernel" in n]
        if len(sym) != 1:
            sys.exit(f"isa_audit: expected one render kernel, found {sym}")
        sym = sym[0]
        nolabels = lambda t: [ln for ln in t.split("\n") if not re.match(r"\.L(tmp|func_begin)\d+:", ln)]   # noqa: E731
        same = nolabels(fp[sym]) == nolabels(fg.get(sym, ""))     # (line info adds labels of its own, nothing else)
        res = isa_compare.resources(plain.stderr).get(sym, {})
        obj = os.path.join(tmp, "g.o")
        run(base + ["-gline-tables-only", "--no-gpu-bundle-output", "-c", "-o", obj, tu])
        dis = run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", f"--disassemble-symbols={sym}", obj]).stdout
        ins = []
        for ln in dis.split("\n"):
            m = re.match(r"\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", ln)
            if m:
                ins.append((int(m.group(2), 16), m.group(1)))
        out = run([LLVM + "/llvm-symbolizer", f"--obj={obj}", "--inlines", "--functions=short"],
                  input="".join(f"0x{adr:x}\n" for adr, _ in ins)).stdout
        stacks = []
        for blk in out.strip("\n").split("\n\n"):
            ls = blk.split("\n")
            st = []
            for i in range(0, len(ls) - 1, 2):
                m = re.match(r"(.*):(\d+):(\d+)$", ls[i + 1])
                if m and os.path.basename(m.group(1)) == "rt_device.h":
                    st.append((ls[i], int(m.group(2))))
            stacks.append(st[::-1])
    if len(stacks) != len(ins):
        sys.exit(f"isa_audit: {len(ins)} instructions but {len(stacks)} symbolizer answers")

    W = weights(a.bounces, a.lights, a.spheres, a.planes)
    per_region = collections.defaultdict(lambda: collections.Counter())
    cost_region = collections.defaultdict(lambda: [0.0, 0.0])          # audited, all
    per_line = collections.defaultdict(lambda: collections.Counter())
    cost_line = collections.Counter()
    for (adr, text), st in zip(ins, stacks):
        cls = classify(text)
        reg = region_of(st, M)
        c = price(cls, text, P)
        per_region[reg][cls] += 1
        cost_region[reg][1] += c
        if cls in AUDITED:
            cost_region[reg][0] += c
            own = [fr for fr in st if fr[0].split("<")[0] not in HELPERS]       # the line that calls a one-instruction helper
            inner = own[-1] if own else ("?", 0)
            k = (reg, inner[0].split("<")[0], inner[1])
            per_line[k][text.split()[0]] += 1
            cost_line[k] += c

    print(f"kernel rt::render_kernel<{a.kernel}>  ({len(ins)} instructions)")
    print("resources: " + ", ".join(f"{k} {v}" for k, v in res.items() if k in ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")))
    print(f"line info leaves the instruction stream unchanged: {'yes' if same else 'NO'}")
    print(f"weights: bounces {a.bounces}, lights {a.lights}, spheres {a.spheres} (cull groups of 4), planes {a.planes}")
    print("prices (cycles per wave-instruction, 7 waves/SIMD): " + ", ".join(f"{k} {P[k]:.2f}" for k in AUDITED + ("f64", "trans64", "f32int", "salu")))
    print()
    cols = AUDITED + OTHER
    print(f"{'region':48s}" + "".join(f"{c:>9s}" for c in cols) + f"{'weight':>8s}{'aud.cyc':>9s}{'all.cyc':>9s}{'aud x w':>10s}{'all x w':>10s}")
    tot = collections.Counter()
    ta = tw = taw = tww = 0.0
    for reg in sorted(per_region, key=lambda r: -cost_region[r][0] * W[r]):
        cnt, (ca, cw), w = per_region[reg], cost_region[reg], W[reg]
        tot.update(cnt)
        ta += ca; tw += cw; taw += ca * w; tww += cw * w
        print(f"{reg:48s}" + "".join(f"{cnt[c]:9d}" for c in cols) + f"{w:8d}{ca:9.0f}{cw:9.0f}{ca * w:10.0f}{cw * w:10.0f}")
    print(f"{'total':48s}" + "".join(f"{tot[c]:9d}" for c in cols) + f"{'':8s}{ta:9.0f}{tw:9.0f}{taw:10.0f}{tww:10.0f}")
    print()
    print("audited instructions by source line (static count, price x region weight):")
    keys = sorted(per_line, key=lambda k: -cost_line[k] * W[k[0]])
    for k in keys[:a.top or None]:
        reg, f, ln = k
        ops = " ".join(f"{n}x{o}" for o, n in sorted(per_line[k].items()))
        print(f"{cost_line[k] * W[reg]:8.0f}  {reg:34.34s} {f}:{ln}  {ops}\n{'':10s}{src.text(ln)[:150]}")
    if a.top and len(keys) > a.top:
        rest = sum(cost_line[k] * W[k[0]] for k in keys[a.top:])
        print(f"{rest:8.0f}  ({len(keys) - a.top} more lines; --top 0 lists them)")


if __name__ == "__main__":
    main()
