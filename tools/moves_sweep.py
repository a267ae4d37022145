#!/usr/bin/env python3
"""Checks and proposes kFrameMovesTable (araytracingjourney_amd/csrc/art_frame.hip): which of the instruction-saving forms each of the 32 k_frame instances takes.
The committed table was not printed by this rule: it is the largest subset that keeps an instance's resource line (the mask form first), with the instances that then had
more lane accesses or vector instructions than the parent set to 0 by hand (the comment at the table).  What this prints satisfies the same conditions and has the fewest
vector instructions per instance; take it when the table has to be made again.
    python3 tools/moves_sweep.py [--jobs 8] [--work DIR] [--static-out profiles/moves_static_all.txt]
Compiles art_frame.hip for the device 64 times with the Makefile's flags and -DART_MOVES_FORCE=n (every instance takes subset n; 0 is the code without any of the forms) and, with --base, once for the source to compare against,
each time twice: as the Makefile does (the assembly: vector instructions, lines beginning v_; v_readlane / v_writelane; the kernel info behind each kernel) and as
tools/kres.sh does (the compiler's kernel-resource-usage remarks: asking for them moves the code of some instances a little, and both have to hold).  An instance may take subset n only if, against the baseline (--base, else subset 0), its VGPRs, scratch, spills, occupancy and LDS are equal in both compilations, it has no more
SGPRs, no more lane accesses and no more vector instructions; of those it takes the one with the fewest vector instructions (then the fewest lane accesses, then the
largest n).  Prints the table in the order art_frame.hip indexes it and, with --static-out, the per-instance counts of the baseline and of the chosen subset.
The table holds for one compiler and one source: run this again after touching k_frame, the packet walks or the toolchain; tools/kres.sh must then report subset 0's lines."""
import argparse, concurrent.futures, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "araytracingjourney_amd", "csrc", "art_frame.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-std=c++17"]


def compile_subset(n, work, src=SRC):
    """-> n, {instance: the Makefile's code (counts, resources from the assembly's kernel info) and tools/kres.sh's (the resource remarks: asking for them moves some instances)}"""
    asm = os.path.join(work, f"moves_{n}.s")
    cmd = ["/opt/rocm/bin/hipcc", *FLAGS, f"-DART_MOVES_FORCE={n}u", "-I", os.path.dirname(SRC), "--cuda-device-only", "-x", "hip", src]
    p = subprocess.run([*cmd, "-S", "-o", asm], capture_output=True, text=True)
    q = subprocess.run([*cmd, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull], capture_output=True, text=True)
    if p.returncode or q.returncode:
        sys.exit(f"subset {n}: the compiler failed\n{(p.stderr + q.stderr)[-2000:]}")
    res, name = {}, None
    for l in q.stderr.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", l)
        if m: name = m.group(1); res[name] = {}
        for key, pat in (("k_sgpr", r" TotalSGPRs: (\d+)"), ("k_vgpr", r" VGPRs: (\d+)"), ("k_scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("k_occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("k_spill", r"VGPRs Spill: (\d+)"), ("k_lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, l)
            if m and name and key not in res[name]: res[name][key] = int(m.group(1))
    out, cur, last = {}, None, None
    for l in open(asm):
        m = re.match(r"^(_ZN3art7k_frame\w+):", l)
        if m: cur = last = m.group(1); out[cur] = dict(res[cur], v=0, lanes=0); continue
        if l.startswith(".Lfunc_end"): cur = None
        if cur:
            t = l.lstrip()
            if t.startswith("v_"):
                out[cur]["v"] += 1
                if t.startswith(("v_readlane", "v_writelane")): out[cur]["lanes"] += 1
        elif last:
            for key, pat in (("sgpr", r"^; TotalNumSgprs: (\d+)"), ("vgpr", r"^; NumVgprs: (\d+)"), ("scratch", r"^; ScratchSize: (\d+)"), ("occ", r"^; Occupancy: (\d+)"), ("lds", r"^; LDSByteSize: (\d+)")):
                m = re.match(pat, l)
                if m: out[last][key] = int(m.group(1))
            if l.startswith("; Occupancy"): last = None
    os.remove(asm)
    return n, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--work", default=None)
    ap.add_argument("--static-out", default=None)
    ap.add_argument("--base", default=None, help="the unit with k_frame to compare against, e.g. the parent commit's (git show <commit>:araytracingjourney_amd/csrc/art_frame.hip > file; any path: art_trace.hip of a commit from before the split, which held k_frame then, does too); default: subset 0 of this source")
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp()
    os.makedirs(work, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        got = dict(ex.map(lambda n: compile_subset(n, work), range(64)))
    if a.base:
        got[0] = compile_subset(64, work, a.base)[1]   # (the baseline only: subset 0 of this source stays a candidate through n = 0 below)
        zero = compile_subset(0, work)[1]
    else:
        zero = got[0]
    names = subprocess.run(["c++filt"], input="\n".join(got[0]), capture_output=True, text=True).stdout.split("\n")
    table, lines = [0] * 32, []
    for mangled, dem in zip(got[0], names):
        flags = [x.strip() == "true" for x in re.search(r"k_frame<(.*?)>", dem).group(1).split(",")]
        idx = flags[0] << 4 | flags[1] << 3 | flags[2] << 2 | flags[3] << 1 | flags[4]
        base = got[0][mangled]
        def fits(n):
            r = (zero if n == 0 else got[n])[mangled]
            return (all(r[k] == base[k] for k in ("vgpr", "scratch", "occ", "lds", "k_vgpr", "k_scratch", "k_spill", "k_occ", "k_lds")) and r["sgpr"] <= base["sgpr"] and r["k_sgpr"] <= base["k_sgpr"]
                    and r["lanes"] <= base["lanes"] and r["v"] <= base["v"])
        ok = [n for n in range(64) if fits(n) and not (n & 4 and not n & 2)]   # (bit 2 means nothing without bit 1)
        pick = lambda n: (zero if n == 0 else got[n])[mangled]
        if not ok:   # (not even subset 0 is as good as the baseline: it takes 0, and the line below shows by how much it is worse)
            ok = [0]
        best = min(ok, key=lambda n: (pick(n)["v"], pick(n)["lanes"], -n))
        table[idx] = best
        r = pick(best)
        lines.append((idx, f"{dem.split('(')[0].replace('void art::', ''):44s} subset {best:2d}   v_ {base['v']:5d} -> {r['v']:5d}   lane accesses {base['lanes']:3d} -> {r['lanes']:3d}   "
                           f"vgpr {base['vgpr']} -> {r['vgpr']}  sgpr {base['sgpr']} -> {r['sgpr']}  scratch {base['scratch']} -> {r['scratch']}  occupancy {base['occ']} -> {r['occ']}"))
    text = "\n".join(l for _, l in sorted(lines, reverse=True))
    print(text)
    print("constexpr uint8_t kFrameMovesTable[32] = {" + ", ".join(map(str, table)) + "};")
    if a.static_out:
        open(a.static_out, "w").write("# every k_frame instance: the baseline (the parent commit's source) -> the subset it takes; lines beginning v_, v_readlane + v_writelane (tools/moves_sweep.py)\n" + text + "\n")


if __name__ == "__main__":
    main()
