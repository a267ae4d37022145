#!/usr/bin/env python3
"""Makes and checks kFrameShortTable (araytracingjourney_amd/csrc/art_frame.hip): which of the short exact forms each of the 32 k_frame instances takes.
    python3 tools/short_math_sweep.py --base PARENT_art_frame.hip [--jobs 6] [--work DIR] [--subsets 0-7,0x...] [--out-dir profiles]
    python3 tools/short_math_sweep.py --base PARENT_art_frame.hip --check      (the committed table only: the Makefile's code and tools/kres.sh's remarks, against the baseline)
Compiles art_frame.hip for the device with the Makefile's flags and -DART_SHORT_FORCE=n for every candidate n (every instance takes subset n, masked by what means
something in it: bits 0-10 only with the guards of kFrameFastMath, bit 13 only with the alpha test; kFrameMoves stays the committed table) and once the baseline (--base:
art_frame.hip inside a checkout of the parent commit, e.g. a `git worktree`, so that it includes that commit's headers; default: subset 0 of this source).  Reads the assembly: vector instructions (lines beginning v_), v_readlane / v_writelane,
and the kernel info behind each kernel -- the figures tests/test_alpha.py and tests/test_ray_masks.py pin are those of this code.  An instance may take subset n only if its
VGPRs, scratch, occupancy and LDS equal the baseline's, with no more SGPRs, no more lane accesses and no more vector instructions; of those it takes the one with the
fewest vector instructions (then the fewest lane accesses, then the smallest n).  Results are kept per n in --work, so a sweep can be taken up again.
--check compiles the source as committed (no override) as the Makefile does and as tools/kres.sh does (the resource remarks: asking for them moves the code of some
instances a little) and fails unless every instance has the baseline's line both ways.  The table holds for one compiler and one source."""
import argparse, concurrent.futures, json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "araytracingjourney_amd", "csrc", "art_frame.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-std=c++17"]
KEYS = (("sgpr", r"^; TotalNumSgprs: (\d+)"), ("vgpr", r"^; NumVgprs: (\d+)"), ("scratch", r"^; ScratchSize: (\d+)"), ("occ", r"^; Occupancy: (\d+)"), ("lds", r"^; LDSByteSize: (\d+)"))
BITS = [f"surface 1/sqrt {k}" for k in range(9)] + ["camera 1/sqrt", "light 1/sqrt", "camera fx/W", "surface wrap", "alpha wrap"]
GUARDED, EVERYWHERE, ALPHA_ONLY = 0x7FF, 0x1800, 0x2000   # what a bit hangs on: the guards of kFrameFastMath | nothing | the alpha test


def default_subsets():
    """Not all 2^14: the surface block's sites were searched on their own first (each site alone, each site left out: the first and the third together are what costs the
    default instances their 64th register, profiles/README.md "short math"), so the block is tried with none, all, and all but one of those two; with each of those the
    camera's and the light's normalisation in every combination over the two forms every instance kept its line with (fx / W and the surface wrap); and the unguarded
    forms in every combination."""
    out = set()
    for sites in (0, 0x1FF, 0x1FE, 0x1FB):
        for cam_light in range(4):
            out.add(sites | cam_light << 9 | EVERYWHERE)
    for free in range(8):
        out.add(free << 11)
    return ",".join(map(str, sorted(out)))


def compile_one(tag, define, work, src=SRC):
    """-> {instance: v_, lane accesses, kernel info}; cached in work/short_<tag>.json"""
    cache = os.path.join(work, f"short_{tag}.json")
    if os.path.exists(cache):
        return json.load(open(cache))
    asm = os.path.join(work, f"short_{tag}.s")
    cmd = ["/opt/rocm/bin/hipcc", *FLAGS, *define, "-I", os.path.dirname(SRC), "--cuda-device-only", "-x", "hip", src, "-S", "-o", asm]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode:
        sys.exit(f"{tag}: the compiler failed\n{p.stderr[-2000:]}")
    out, cur, last = {}, None, None
    for l in open(asm):
        m = re.match(r"^(_ZN3art7k_frame\w+):", l)
        if m: cur = last = m.group(1); out[cur] = dict(v=0, lanes=0, div_scale=0); continue
        if l.startswith(".Lfunc_end"): cur = None
        if cur:
            t = l.lstrip()
            if t.startswith("v_"):
                out[cur]["v"] += 1
                if t.startswith(("v_readlane", "v_writelane")): out[cur]["lanes"] += 1
                if t.startswith("v_div_scale"): out[cur]["div_scale"] += 1
        elif last:
            for key, pat in KEYS:
                m = re.match(pat, l)
                if m: out[last][key] = int(m.group(1))
            if l.startswith("; Occupancy"): last = None
    os.remove(asm)
    json.dump(out, open(cache, "w"))
    return out


def kres(define, src=SRC):
    """tools/kres.sh's figures: {instance: (vgpr, scratch, spill, occ, lds, sgpr)}"""
    cmd = ["/opt/rocm/bin/hipcc", *FLAGS, *define, "-I", os.path.dirname(SRC), "--cuda-device-only", "-x", "hip", src, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull]
    q = subprocess.run(cmd, capture_output=True, text=True)
    if q.returncode:
        sys.exit(f"kres: the compiler failed\n{q.stderr[-2000:]}")
    res, name = {}, None
    for l in q.stderr.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", l)
        if m: name = m.group(1); res[name] = {}
        for key, pat in (("sgpr", r" TotalSGPRs: (\d+)"), ("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("spill", r"VGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, l)
            if m and name and key not in res[name]: res[name][key] = int(m.group(1))
    return {k: v for k, v in res.items() if "k_frame" in k}


def parse_subsets(text):
    out = []
    for part in text.split(","):
        lo, _, hi = part.partition("-")
        out += list(range(int(lo, 0), int(hi or lo, 0) + 1))
    return sorted(set(out))


def instance_index(dem):
    flags = [x.strip() == "true" for x in re.search(r"k_frame<(.*?)>", dem).group(1).split(",")]
    return flags[0] << 4 | flags[1] << 3 | flags[2] << 2 | flags[3] << 1 | flags[4], flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=6)
    ap.add_argument("--work", default=None)
    ap.add_argument("--base", default=None)
    ap.add_argument("--subsets", default=default_subsets(), help="comma-separated values and ranges a-b of ART_SHORT_FORCE; default: default_subsets()")
    ap.add_argument("--out-dir", default=None, help="writes short_math_kres_parent.txt, short_math_kres_new.txt (the chosen subsets' lines) and short_math_static_all.txt there")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp()
    os.makedirs(work, exist_ok=True)
    base = compile_one("base", [], work, a.base) if a.base else None
    if a.check:
        now = compile_one("committed", [], work)
        base = base or now
        kb, kn = kres([], a.base or SRC), kres([])
        bad = 0
        for k in base:
            same = all(now[k][x] == base[k][x] for x in ("vgpr", "scratch", "occ", "lds")) and all(kn[k][x] == kb[k][x] for x in ("vgpr", "scratch", "spill", "occ", "lds"))
            worse = now[k]["v"] > base[k]["v"] or now[k]["lanes"] > base[k]["lanes"] or now[k]["sgpr"] > base[k]["sgpr"] or kn[k]["sgpr"] > kb[k]["sgpr"]
            if not same or worse:
                bad += 1
                print("MOVED", k, base[k], now[k], kb[k], kn[k])
        print(f"{len(base)} instances, {bad} moved")
        sys.exit(1 if bad else 0)
    subsets = parse_subsets(a.subsets)
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        got = dict(zip(subsets, ex.map(lambda n: compile_one(str(n), [f"-DART_SHORT_FORCE={n}u"], work), subsets)))
    base = base or got[0]
    names = subprocess.run(["c++filt"], input="\n".join(base), capture_output=True, text=True).stdout.split("\n")
    table, lines, kp, kn = [0] * 32, [], [], []
    for mangled, dem in zip(base, names):
        idx, flags = instance_index(dem)
        fastm = flags[1] and not flags[3] and not flags[4]
        means = (GUARDED if fastm else 0) | EVERYWHERE | (ALPHA_ONLY if flags[4] else 0)
        b = base[mangled]
        eff = {n & means: n for n in subsets}   # what subset n is in this instance -> a compilation that holds it
        pick = lambda e: got[eff[e]][mangled]
        def fits(n):
            r = pick(n)
            return all(r[k] == b[k] for k in ("vgpr", "scratch", "occ", "lds")) and r["sgpr"] <= b["sgpr"] and r["lanes"] <= b["lanes"] and r["v"] <= b["v"]
        cands = sorted(eff)
        ok = [n for n in cands if fits(n)] or [0]
        best = min(ok, key=lambda n: (pick(n)["v"], pick(n)["lanes"], n))
        table[idx] = best
        r = pick(best)
        short = dem.split("(")[0].replace("void art::", "")
        lines.append((idx, f"{short:44s} subset {best:#06x} of {len(ok):3d} that fit ({len(cands)} tried)   v_ {b['v']:5d} -> {r['v']:5d}   v_div_scale {b['div_scale']:3d} -> {r['div_scale']:3d}   "
                           f"lane accesses {b['lanes']:3d} -> {r['lanes']:3d}   vgpr {b['vgpr']} -> {r['vgpr']}  sgpr {b['sgpr']} -> {r['sgpr']}  scratch {b['scratch']} -> {r['scratch']}  occupancy {b['occ']} -> {r['occ']}"))
        kp.append((idx, f"vgpr {b['vgpr']:3d} sgpr {b['sgpr']:3d} scratch {b['scratch']:5d} occ {b['occ']} lds {b['lds']:6d}  {short}"))
        kn.append((idx, f"vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']:5d} occ {r['occ']} lds {r['lds']:6d}  {short}"))
        if fastm:   # the instances with the guards: every candidate's line, so that what does not fit is on record too
            for n in cands:
                r = pick(n)
                lines.append((idx, f"    {short}  subset {n:#06x}  v_ {r['v']:5d}  lanes {r['lanes']:3d}  vgpr {r['vgpr']}  sgpr {r['sgpr']}  scratch {r['scratch']}  {'fits' if fits(n) else '-'}"))
    order = lambda ls: "\n".join(l for _, l in sorted(ls, key=lambda t: -t[0]))
    text = order(lines)
    print("\n".join(l for l in text.split("\n") if not l.startswith("    ")))
    print("bits: " + ", ".join(f"{1 << i} {b}" for i, b in enumerate(BITS)))
    print("constexpr uint16_t kFrameShortTable[32] = {" + ", ".join(f"{t:#06x}" for t in table) + "};")
    if a.out_dir:
        head = "# tools/short_math_sweep.py: the Makefile's code of art_frame.hip (hipcc -S --cuda-device-only), kernel info behind each k_frame instance\n"
        open(os.path.join(a.out_dir, "short_math_kres_parent.txt"), "w").write(head + "# the baseline (the parent commit's unit)\n" + order(kp) + "\n")
        open(os.path.join(a.out_dir, "short_math_kres_new.txt"), "w").write(head + "# each instance at the subset the table gives it\n" + order(kn) + "\n")
        open(os.path.join(a.out_dir, "short_math_static_all.txt"), "w").write(
            "# every k_frame instance: the baseline -> the subset it takes (lines beginning v_, v_div_scale_f32, v_readlane + v_writelane); indented: every candidate subset of the four\n"
            "# instances with the guards.  subsets tried: " + a.subsets + "\n# bits: " + ", ".join(f"{1 << i} {b}" for i, b in enumerate(BITS)) + "\n" + text +
            "\nconstexpr uint16_t kFrameShortTable[32] = {" + ", ".join(f"{t:#06x}" for t in table) + "};\n")


if __name__ == "__main__":
    main()
