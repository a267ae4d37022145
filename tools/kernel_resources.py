"""Register, scratch and occupancy figures of libart's kernels, read from the gfx950 code objects inside libart.so.

    python tools/kernel_resources.py [PATTERN ...]     # kernels whose mangled name holds every PATTERN

The code objects are the clang offload bundles in the .hip_fatbin section; each is unbundled in memory and its AMDGPU metadata
note is read with llvm-readelf --notes.  No GPU is needed.  tests/test_alpha.py uses kernel_resources() to pin the frame kernels."""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "araytracingjourney_amd", "libart.so")
LLVM = "/opt/rocm/llvm/bin" if os.path.isdir("/opt/rocm/llvm/bin") else os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _section(path, name):
    with open(path, "rb") as f:
        elf = f.read()
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    def sh(i):
        return struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize)
    stroff = sh(shstrndx)[4]
    for i in range(shnum):
        s = sh(i)
        nm = elf[stroff + s[0]:elf.index(b"\0", stroff + s[0])].decode()
        if nm == name:
            return elf[s[4]:s[4] + s[5]]
    raise RuntimeError(f"{path}: no section {name}")


def code_objects(path=LIB):
    """the gfx950 code objects of every bundle in the library's fat binary"""
    fat = _section(path, ".hip_fatbin")
    out, at = [], 0
    while True:
        at = fat.find(MAGIC, at)
        if at < 0:
            return out
        n, = struct.unpack_from("<Q", fat, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fat, p)
            triple = fat[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "amdgcn" in triple and "gfx950" in triple:
                out.append(fat[at + off:at + off + size])
        at = p


def kernel_resources(path=LIB):
    """{mangled kernel name: {'vgpr', 'agpr', 'sgpr', 'scratch', 'spill_v', 'spill_s', 'lds', 'waves_per_simd'}}
    (k_frame<true, true, false, false> is _ZN3art7k_frameILb1ELb1ELb0ELb0EEEvNS_9FrameArgsE: template arguments in order, Lb1 = true)"""
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(path)):
            f = os.path.join(tmp, f"co{i}.o")
            with open(f, "wb") as fh:
                fh.write(co)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True, check=True).stdout
            for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                block = ".agpr_count:" + block
                def field(key, default=0):
                    m = re.search(r"\." + re.escape(key) + r":\s+(\S+)", block)
                    return m.group(1) if m else default
                name = field("name", "")
                if not name:
                    continue
                kernels[name] = dict(vgpr=int(field("vgpr_count")), agpr=int(field("agpr_count")), sgpr=int(field("sgpr_count")),
                                     scratch=int(field("private_segment_fixed_size")), spill_v=int(field("vgpr_spill_count")),
                                     spill_s=int(field("sgpr_spill_count")), lds=int(field("group_segment_fixed_size")))
    for k in kernels.values():
        v = k["vgpr"] + k["agpr"]   # unified register file of CDNA: 512 per SIMD lane, granule 8
        k["waves_per_simd"] = min(8, 512 // max(8, (v + 7) // 8 * 8)) if v else 8
    return kernels


if __name__ == "__main__":
    pats = sys.argv[1:]   # (mangled: k_frame<true, ...> is "k_frameILb1...")
    for name, k in sorted(kernel_resources().items()):
        if all(p in name for p in pats):
            print(f"{k['vgpr']:4d} vgpr {k['agpr']:3d} agpr {k['sgpr']:3d} sgpr {k['scratch']:6d} B scratch {k['lds']:6d} B lds  spills v{k['spill_v']} s{k['spill_s']}  "
                  f"{k['waves_per_simd']} waves/SIMD  {name}")
