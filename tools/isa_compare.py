#!/usr/bin/env python3
"""Compare the gfx950 ISA and resource usage of the kernels of two source trees (CPU only, no GPU).

    python tools/isa_compare.py [--base REV] [--base-asm FILE] [--twins]

Builds `make -C python-ray-tracer_amd/csrc asm` once for the working tree and once for REV (default HEAD, extracted with
`git archive` into a temporary directory), then, for every kernel of REV:
  * the instruction stream, with comments and assembler directives dropped and `.LBB` / `.Lfunc_end` labels and the
    kernel's own symbol renumbered, must be identical in the working tree (where it is not, the line also says whether the two
    streams at least hold every mnemonic equally often: the same instructions in another order or in other registers);
  * so must its -Rpass-analysis=kernel-resource-usage lines (VGPRs, SGPRs, scratch, LDS, occupancy, spills).
A render_kernel instantiation is matched by its first six template arguments (AA, PARK, WPW, COUNT, LAT, MODE) and its feature
family (rt::Family, rt_device.h), whichever way the tree spells the family: as the seventh argument `Family F` (mangled
`LNS_6FamilyE<n>E`; an eighth argument GROUND = true behind it makes the kernel the "ground" twin of its family, a kernel of its
own that a tree without the argument does not have, and GROUND = false or absent is the family's generic kernel; a ninth argument
NG = 1 or 2 behind that makes it the "ground_small1" or "ground_small2" twin of the ground twin, the small-scene kernel for that many cull groups), or, in trees from before that parameter, as up to five trailing bool arguments MAT, REFR, SCAT, SOFT and
LENS, of which a missing one counts as false.  So a tree of either form compares with one of the other, and a tree with more
families with one with fewer.  Kernels of the working tree that the base does not have are listed as NEW.
--twins also prints each ground-plane kernel next to its generic PLAIN twin, each small-scene kernel next to its ground-plane twin, each MAT kernel next to its PLAIN twin, each REFR kernel next to its MAT twin, each SCAT kernel next to its
REFR twin, each SOFT kernel next to its SCAT twin, each LENS and LENS_SOFT kernel next to its SCAT and SOFT twin, and each
texture kernel (TEX_SCAT, TEX_SOFT, TEX_LENS, TEX_LENS_SOFT) next to its SCAT, SOFT, LENS and LENS_SOFT twin, and each lighting
kernel (LIT_SCAT, LIT_SOFT, LIT_LENS, LIT_LENS_SOFT) next to its texture twin, and each sky kernel (SKY_SCAT, SKY_SOFT, SKY_LENS,
SKY_LENS_SOFT) next to its lighting twin.  Exit status 1 if any kernel differs.
--tree-asm FILE does the same for the working tree's build.  Under every kernel that differs stands what the change did to its
line count and resources, and at the end the kernels that now have more scratch, more spills or fewer waves per SIMD.
--base-asm FILE takes REV's build from an earlier run instead of building it again (a build is minutes of one core): FILE is REV's
rt_kernel.gfx950.s and FILE.log what its `make asm` wrote to stderr (the resource-usage remarks).  What is compared is the same.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("python-ray-tracer_amd", "csrc")


def build(tree):
    r = subprocess.run(["make", "-s", "-C", os.path.join(tree, CSRC), "-B", "asm"], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stdout + r.stderr)
    return open(os.path.join(tree, CSRC, "rt_kernel.gfx950.s")).read(), r.stderr


FAMILIES = ("", "mat", "refr", "scat", "soft", "lens", "lens_soft",    # rt::Family in enum order; "" is PLAIN
            "tex_scat", "tex_soft", "tex_lens", "tex_lens_soft", "lit_scat", "lit_soft", "lit_lens", "lit_lens_soft",
            "sky_scat", "sky_soft", "sky_lens", "sky_lens_soft")
# --twins: (family, its twin, the family's title), and how a twin is called in the heading ("" is PLAIN: "default")
TWINS = (("ground", "", "ground-plane kernel"), ("ground_small1", "ground", "small-scene kernel, 1 cull group"),
         ("ground_small2", "ground", "small-scene kernel, 2 cull groups"), ("mat", "", "material kernel"), ("refr", "mat", "refraction kernel"), ("scat", "refr", "scatter kernel"),
         ("soft", "scat", "area-light kernel"), ("lens", "scat", "lens kernel"), ("lens_soft", "soft", "lens area-light kernel"),
         ("tex_scat", "scat", "texture kernel"), ("tex_soft", "soft", "texture area-light kernel"),
         ("tex_lens", "lens", "texture lens kernel"), ("tex_lens_soft", "lens_soft", "texture lens area-light kernel"),
         ("lit_scat", "tex_scat", "lighting kernel"), ("lit_soft", "tex_soft", "lighting area-light kernel"),
         ("lit_lens", "tex_lens", "lighting lens kernel"), ("lit_lens_soft", "tex_lens_soft", "lighting lens area-light kernel"),
         ("sky_scat", "lit_scat", "sky kernel"), ("sky_soft", "lit_soft", "sky area-light kernel"),
         ("sky_lens", "lit_lens", "sky lens kernel"), ("sky_lens_soft", "lit_lens_soft", "sky lens area-light kernel"))
TWIN_NAMES = {"": "default", "ground": "ground-plane", "mat": "material", "refr": "refraction", "scat": "scatter", "soft": "area-light", "lens": "lens",
              "lens_soft": "lens area-light", "tex_scat": "texture", "tex_soft": "texture area-light", "tex_lens": "texture lens",
              "tex_lens_soft": "texture lens area-light", "lit_scat": "lighting", "lit_soft": "lighting area-light",
              "lit_lens": "lighting lens", "lit_lens_soft": "lighting lens area-light"}


def key(name):
    """Kernel symbol -> ((kernel, its first six template arguments), its family: one of FAMILIES)."""
    m = re.match(r"_ZN2rt\d+(\w+?)I((?:L[bi]\d+E)+)(?:LNS_6FamilyE(\d+)E)?(?:Lb([01])E)?(?:Li(\d+)E)?EEvNS_7KParamsE$", name)
    if not m:
        return name, ""
    args = re.findall(r"L[bi](\d+)E", m.group(2))
    if m.group(3) is not None:
        fam = FAMILIES[int(m.group(3))]
        if m.group(4) == "1":                                  # GROUND, behind the family: PLAIN's ground-plane twin
            fam = (fam + "_ground").lstrip("_")
        if m.group(5) not in (None, "0"):                      # NG, behind GROUND: the ground twin's small-scene twin
            fam += "_small" + m.group(5)
    else:
        mat, refr, scat, soft, lens = ((args[6:] + ["0"] * 5)[i] == "1" for i in range(5))
        fam = (("lens_soft" if soft else "lens") if lens else "soft" if soft else "scat" if scat else "refr" if refr else
               "mat" if mat else "")
    return (m.group(1),) + tuple(args[:6]), fam


def functions(asm):
    out = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:", asm, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        lines = []
        for ln in body.split("\n"):
            ln = ln.split(";")[0].rstrip()
            if not ln.strip() or ln.lstrip().startswith(".") and not ln.startswith(".L"):
                continue
            lines.append(ln.replace(name, "<fn>"))
        text = "\n".join(lines)
        labels = {}
        text = re.sub(r"\.(LBB|Lfunc_end)\d+_?\d*", lambda x: labels.setdefault(x.group(0), f".L{len(labels)}"), text)
        out[name] = text
    return out


def mnemonics(text):
    """A normalized stream -> {mnemonic: count} (labels dropped)."""
    return collections.Counter(ln.split()[0] for ln in text.splitlines() if ln.strip() and not ln.rstrip().endswith(":"))


def resources(log):
    out, cur = {}, None
    for ln in log.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = m.group(1); out[cur] = {}
            continue
        m = re.search(r"remark:\s+([^:]+): (\S+) \[-Rpass-analysis", ln)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("--base-asm", help="REV's rt_kernel.gfx950.s from an earlier build; its stderr in FILE.log")
    ap.add_argument("--tree-asm", help="the working tree's rt_kernel.gfx950.s from an earlier build; its stderr in FILE.log")
    ap.add_argument("--twins", action="store_true")
    a = ap.parse_args()
    if a.base_asm:
        base_asm, base_log = open(a.base_asm).read(), open(a.base_asm + ".log").read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            arch = subprocess.run(["git", "-C", REPO, "archive", a.base, CSRC, "include"], capture_output=True, check=True).stdout
            subprocess.run(["tar", "-x", "-C", tmp], input=arch, check=True)
            base_asm, base_log = build(tmp)
    new_asm, new_log = (open(a.tree_asm).read(), open(a.tree_asm + ".log").read()) if a.tree_asm else build(REPO)
    bf, nf = functions(base_asm), functions(new_asm)
    br, nr = resources(base_log), resources(new_log)
    new_by_key = {}
    for n in nf:
        new_by_key[key(n)] = n
    bad = 0
    worse = []                                  # kernels with more scratch, more spills or fewer waves per SIMD than in the base
    WATCH = (("ScratchSize [bytes/lane]", 1), ("VGPRs Spill", 1), ("SGPRs Spill", 1), ("Occupancy [waves/SIMD]", -1))
    for b in sorted(bf):
        n = new_by_key.get(key(b))
        if n is None:
            print(f"MISSING  {b}"); bad += 1; continue
        same_isa = bf[b] == nf[n]
        same_res = br.get(b) == nr.get(n)
        counts = "" if same_isa else f"  (mnemonic counts {'equal' if mnemonics(bf[b]) == mnemonics(nf[n]) else 'DIFFER'})"
        print(f"{'same' if same_isa and same_res else 'DIFF'}  isa={'=' if same_isa else '!'} res={'=' if same_res else '!'} "
              f"{len(bf[b].splitlines()):6d} lines  {key(b)[0]}{' ' + key(b)[1] if key(b)[1] else ''}{counts}")
        bad += not (same_isa and same_res)
        if not (same_isa and same_res):         # what the change did to the kernel's resources
            rb, rn = br.get(b, {}), nr.get(n, {})
            cols = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]")
            print(f"      {len(nf[n].splitlines()) - len(bf[b].splitlines()):+5d} lines  " +
                  "  ".join(f"{c.split(' [')[0]} {rb.get(c, '?')}->{rn.get(c, '?')}" for c in cols))
            if any(sign * (int(rn.get(c, 0)) - int(rb.get(c, 0))) > 0 for c, sign in WATCH):
                worse.append(f"{key(b)[0]}{' ' + key(b)[1] if key(b)[1] else ''}")
    base_keys = {key(b) for b in bf}
    new = sorted(n for n in nf if key(n) not in base_keys)
    for n in new:
        print(f"NEW   {key(n)[0]} {key(n)[1]}")
    print(f"{len(bf)} kernels of {a.base} compared, {bad} differ; {len(new)} new")
    print(f"kernels with more scratch, more spills or fewer waves per SIMD than in {a.base}: {len(worse)}" + "".join(f"\n  {w}" for w in worse))
    if a.twins:
        cols = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill", "LDS Size [bytes/block]")
        for fam, twin, title in TWINS:
            print(f"\n{title} (AA, PARK, WPW, COUNT, LAT, MODE)  VGPRs SGPRs scratch occupancy spill LDS   {TWIN_NAMES[twin]} twin")
            for (k, f_), n in sorted(new_by_key.items(), key=str):
                if f_ != fam:
                    continue
                t = new_by_key.get((k, twin))
                m_, d_ = nr.get(n, {}), nr.get(t, {})
                print(f"  {','.join(k[1:]):20s}  " + " ".join(f"{m_.get(c, '?'):>5s}" for c in cols) + "   " +
                      " ".join(f"{d_.get(c, '?'):>5s}" for c in cols))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
