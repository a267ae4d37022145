"""Are the kernels of two builds of libart the same machine code?  For a change that must not move an instruction (a code move, a rename, a split of a unit):

    python tools/kernel_diff.py OLD/libart.so NEW/libart.so

Every kernel in the gfx950 code objects of either library (kernel_resources.code_objects) is disassembled with llvm-objdump and compared by mangled name: the instruction
stream, and the resource figures kernel_resources() reads.  A stream is what is left of a kernel's disassembly without addresses and encodings; branch operands are
offsets already, and an address made from the program counter (s_getpc_b64, then s_add_u32 / s_addc_u32 with the distance) is replaced by the symbol it lands on, so a
kernel may sit anywhere in its code object, beside any neighbours; a kernel with a copy in several code objects (a rocPRIM template, once per unit that calls it) is
compared as the set of its distinct streams, so a unit more or less that calls it changes nothing.  Prints the kernels that differ or exist on one side only and exits 1 if there are any.  No GPU is needed."""
import bisect
import os
import re
import subprocess
import sys
import tempfile

from kernel_resources import LLVM, code_objects, kernel_resources


def symbols(obj):
    """[(address, name, size)] of the code object's defined symbols, sorted"""
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", obj], capture_output=True, text=True, check=True).stdout
    syms = [(int(m.group(1), 16), m.group(4), int(m.group(3), 16)) for m in re.finditer(r"^([0-9a-f]{16}) .{7} (\S+)\s+([0-9a-f]{16}) (?:\.\w+ )?(\S+)$", out, re.M) if m.group(2) != "*UND*"]
    return sorted(syms)


def streams(path):
    """{symbol: [instruction text]} for every function of every gfx950 code object of the library"""
    funcs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(path)):
            obj = os.path.join(tmp, f"co{i}.o")
            with open(obj, "wb") as fh:
                fh.write(co)
            syms = symbols(obj)
            addrs = [a for a, _, _ in syms]
            end_of = {n: a + size for a, n, size in syms}

            def where(addr):   # symbol + offset of an address of this code object
                k = bisect.bisect_right(addrs, addr) - 1
                return f"{syms[k][1]}+{addr - syms[k][0]}" if k >= 0 else hex(addr)

            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", obj], capture_output=True, text=True, check=True).stdout
            cur, end, pc_of = None, 0, {}
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                if m:
                    cur, end, pc_of = [], end_of.get(m.group(1), 0), {}
                    funcs.setdefault(m.group(1), []).append(cur)   # (a library template's kernel has a copy in every unit that uses it)
                    continue
                m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", line)
                if cur is None or not m:
                    continue
                ins, addr = m.group(1), int(m.group(2), 16)
                if addr >= end:   # the padding behind a function
                    continue
                g = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", ins)
                if g:
                    pc_of = {g.group(1): addr + 4, g.group(2): None}   # the counter after this instruction, in the low register
                a = re.match(r"s_add_u32 s(\d+), s(\d+), (0x[0-9a-f]+|-?\d+)$", ins)
                if a and a.group(2) in pc_of and pc_of[a.group(2)] is not None:
                    d = int(a.group(3), 0)
                    d -= (1 << 32) if d >= (1 << 31) else 0
                    ins = f"s_add_u32 s{a.group(1)}, s{a.group(2)}, <{where(pc_of[a.group(2)] + d)}>"
                    pc_of = {k: None for k in pc_of}   # the high half follows
                elif re.match(r"s_addc_u32 s(\d+), s(\d+), (0x[0-9a-f]+|-?\d+)$", ins) and re.match(r"s_addc_u32 s\d+, s(\d+),", ins).group(1) in pc_of:
                    ins = re.sub(r", (0x[0-9a-f]+|-?\d+)$", ", <high>", ins)
                    pc_of = {}
                cur.append(ins)
    return {name: sorted(set(map(tuple, copies))) for name, copies in funcs.items()}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = sys.argv[1], sys.argv[2]
    res_old, res_new = kernel_resources(old), kernel_resources(new)
    str_old, str_new = streams(old), streams(new)
    bad = 0
    for name in sorted(set(res_old) | set(res_new)):
        if name not in res_old or name not in res_new:
            print(f"only in {'the new' if name in res_new else 'the old'} library: {name}")
            bad += 1
            continue
        why = []
        if res_old[name] != res_new[name]:
            why.append("figures " + ", ".join(f"{k} {res_old[name][k]} -> {res_new[name][k]}" for k in res_old[name] if res_old[name][k] != res_new[name][k]))
        a, b = str_old.get(name, []), str_new.get(name, [])
        if not a or not b:
            why.append("no disassembly found")
        elif a != b and (len(a) > 1 or len(b) > 1):
            why.append(f"its copies in several code objects: {len(a)} -> {len(b)} distinct streams")
        elif a != b:
            a, b = a[0], b[0]
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            why.append(f"stream {len(a)} -> {len(b)} instructions, first difference at {at}: {a[at] if at < len(a) else '(end)'} | {b[at] if at < len(b) else '(end)'}")
        if why:
            print(f"differs: {name}: " + "; ".join(why))
            bad += 1
    n_ins = sum(len(s) for k in res_new for s in str_new.get(k, []))
    print(f"{len(res_old)} kernels in the old library, {len(res_new)} in the new, {n_ins} instructions compared: {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
