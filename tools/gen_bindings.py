#!/usr/bin/env python3
"""Generates the two bindings of libart's C ABI from the headers themselves, so that the headers are the only place an entry point is written down by hand:

    bindings/art_sys.rs              from include/art.h: the raw Rust binding a maintainer of the reference would add -- every #define, struct,
                                     opaque handle, callback type and function, plus a compile-time layout block whose sizes come from gcc (sizeof / offsetof of
                                     the C structs).  There is no Rust toolchain in this image, so the file is generated and checked for completeness
                                     (tests/test_host.py), not compiled.
    araytracingjourney_amd/_abi.py   from include/art.h and include/art_parity.h: the ctypes binding every test, bench.py, the tools and renderer.py go through
                                     (_lib.py re-exports it) -- every #define as an int, every struct as a ctypes.Structure, the callback type, and the
                                     (restype, argtypes) tables SYMBOLS (art.h) and PARITY_SYMBOLS (art_parity.h).  `const char *` is c_char_p, every other
                                     pointer or array is c_void_p, scalars map by name.  No compiler is involved: tests compare the classes with gcc's layout.

    python tools/gen_bindings.py            # writes both files
    python tools/gen_bindings.py --check    # exit 1, naming the file, if a committed file is not what the headers generate"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HDR = os.path.join(INCLUDE, "art.h")
PARITY_HDR = os.path.join(INCLUDE, "art_parity.h")
OUT_RS = os.path.join(ROOT, "bindings", "art_sys.rs")
OUT_PY = os.path.join(ROOT, "araytracingjourney_amd", "_abi.py")

SCALAR = {"int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64", "int64_t": "i64", "uint8_t": "u8", "uint16_t": "u16", "float": "f32", "double": "f64", "size_t": "usize",
          "char": "c_char", "void": "c_void", "int": "i32"}
CTYPES = {"int32_t": "c_int32", "uint32_t": "c_uint32", "uint64_t": "c_uint64", "int64_t": "c_int64", "uint8_t": "c_uint8", "uint16_t": "c_uint16", "float": "c_float",
          "double": "c_double", "size_t": "c_size_t", "int": "c_int"}
RUST_KEYWORDS = {"type": "light_type", "in": "in_", "ref": "ref_", "box": "box_", "move": "move_", "fn": "fn_"}


def strip_comments(s):
    return re.sub(r"/\*.*?\*/", " ", s, flags=re.S)


def parse(path):
    """What the header at `path` itself declares (not what it includes): consts [(name, value)], opaque handles [name], structs [(name, packed, [(field, C type, array
    length or None)])], callback typedefs [(return type, name, parameters)] and functions [(return type, name, parameters)], each in the header's order"""
    src = strip_comments(open(path).read())
    consts = re.findall(r"^#define\s+(ART_\w+)\s+\(?(-?\d+)u?\)?\s*$", src, flags=re.M)
    opaque = re.findall(r"typedef\s+struct\s+(\w+)\s+\1\s*;", src)
    structs = []
    for m in re.finditer(r"(#pragma pack\(push, 1\)\s*)?typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\2\s*;", src, flags=re.S):
        packed, name, body = bool(m.group(1)), m.group(2), m.group(3)
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            # one declaration may name several fields of one type: "uint32_t a, b;" / "float pos[3];"
            tm = re.match(r"^((?:const\s+)?\w+(?:\s*\*)*)\s*(.*)$", decl)
            ctype, names = tm.group(1), tm.group(2)
            for n in names.split(","):
                am = re.match(r"^(\**)\s*(\w+)(?:\[(\d+)\])?$", n.strip())
                ptr, fname, arr = am.group(1), am.group(2), am.group(3)
                fields.append((fname, ctype + ptr, arr))
        structs.append((name, packed, fields))
    fnptr = [(ret, name, " ".join(params.split())) for ret, name, params in re.findall(r"typedef\s+(\w+)\s*\(\s*\*\s*(\w+)\s*\)\s*\((.*?)\)\s*;", src, flags=re.S)]
    funcs = []
    for m in re.finditer(r"^(const char \*|int32_t )\s*(art_\w+)\s*\((.*?)\)\s*;", src, flags=re.M | re.S):
        funcs.append((m.group(1).strip(), m.group(2), " ".join(m.group(3).split())))
    return consts, opaque, structs, fnptr, funcs


def c_params(params):
    """[(C type, name)] of a parameter list; an array parameter is a pointer"""
    out = []
    for p in ([] if params in ("void", "") else params.split(",")):
        m = re.match(r"^(.*?)(\w+)\s*(\[\w*\])?$", p.strip())
        out.append((m.group(1).strip() + (" *" if m.group(3) else ""), m.group(2)))
    return out


def c_layout(path, structs):
    """sizeof of every struct and offsetof of every field of `structs` (parse(path)[2], or some of them), from gcc: {"Name": size, "Name.field": offset}"""
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.abspath(path)}"', "int main(void) {"]
    for name, _, fields in structs:
        prog.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for fname, _, _ in fields:
            prog.append(f'  printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    prog.append("  return 0; }")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(c, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-I", INCLUDE, "-o", exe, c])   # -I: a copy of art_parity.h elsewhere still finds art.h
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))


# ---- Rust -------------------------------------------------------------------------------------------------------------------------------------------------------
def rust_type(ctype):
    """C declarator type (without the name) -> Rust"""
    m = re.match(r"^(const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)$", ctype.strip())
    if not m:
        raise ValueError(f"cannot map C type {ctype!r}")
    const, base, stars = bool(m.group(1)), m.group(2), m.group(3)
    r = SCALAR.get(base, base)
    levels = re.findall(r"\*\s*(const)?", stars)
    for i in range(len(levels)):
        # pointer level i (innermost first): constness of what it points to
        pointee_const = const if i == 0 else bool(levels[i - 1])
        r = ("*const " if pointee_const else "*mut ") + r
    return r


def field_name(n):
    return RUST_KEYWORDS.get(n, n)


def rust_params(params):
    return ", ".join(f"{field_name(name)}: {rust_type(ctype)}" for ctype, name in c_params(params))


def generate_rs(hdr=HDR):
    consts, opaque, structs, fnptr, funcs = parse(hdr)
    lay = c_layout(hdr, structs)
    # (the second line names this tool as it was called while it wrote the Rust file only: the file stays byte for byte what it was)
    L = ["// art_sys.rs -- raw binding of include/art.h (libart: the MI355X ray-tracing core that stands in for vk_renderer's Vulkan RT path).",
         "// GENERATED by tools/gen_rust_bindings.py from the header; do not edit.  Where it would live in the reference: src/vk_renderer/art_sys.rs,",
         "// linked with `cargo:rustc-link-lib=art` (libart.so is built by araytracingjourney_amd/csrc/Makefile).  Every function returns 0 or a negative",
         "// ART_E_* code (art_last_error() has the message); the reference panics instead (unwrap / expect): a wrapper would panic on non-zero.",
         "#![allow(non_camel_case_types, dead_code)]", "use core::ffi::{c_char, c_void};", ""]
    for name, val in consts:
        ty = "i32" if name.startswith("ART_E_") or name == "ART_OK" else ("usize" if name.endswith("_BYTES") else "u32")
        L.append(f"pub const {name}: {ty} = {val};")
    L.append("")
    for name in opaque:
        L.append(f"#[repr(C)] pub struct {name} {{ _private: [u8; 0] }}")
    L.append("")
    for ret, name, params in fnptr:
        L.append(f"pub type {name} = Option<unsafe extern \"C\" fn({rust_params(params)}) -> {SCALAR[ret]}>;")
    L.append("")
    for name, packed, fields in structs:
        L.append(f"#[repr(C{', packed' if packed else ''})] #[derive(Clone, Copy)]")
        L.append(f"pub struct {name} {{")
        for fname, ctype, arr in fields:
            L.append(f"    pub {field_name(fname)}: {f'[{rust_type(ctype)}; {arr}]' if arr else rust_type(ctype)},")
        L.append("}")
    L.append("")
    L.append("// layout: sizeof / offsetof of the C structs (gcc, x86-64), checked at compile time")
    for name, packed, fields in structs:
        L.append(f"const _: () = assert!(core::mem::size_of::<{name}>() == {lay[name]});")
        if not packed:   # (offset_of! on a packed struct needs no reference either, but keep to the stable subset)
            for fname, _, _ in fields:
                L.append(f"const _: () = assert!(core::mem::offset_of!({name}, {field_name(fname)}) == {lay[name + '.' + fname]});")
    L.append("")
    L.append('#[link(name = "art")]')
    L.append('extern "C" {')
    for ret, name, params in funcs:
        r = "*const c_char" if ret.startswith("const char") else "i32"
        L.append(f"    pub fn {name}({rust_params(params)}) -> {r};")
    L.append("}")
    return "\n".join(L) + "\n"


# ---- ctypes -----------------------------------------------------------------------------------------------------------------------------------------------------
def ctypes_type(ctype, callbacks=(), char_p=False):
    """C declarator type (without the name) -> ctypes: any pointer is c_void_p (a parameter or return value `const char *`: c_char_p), a callback typedef is itself"""
    t = " ".join(ctype.split())
    if "*" in t:
        return "C.c_char_p" if char_p and t.replace(" ", "") == "constchar*" else "C.c_void_p"
    base = t.replace("const ", "")
    return base if base in callbacks else "C." + CTYPES[base]


def generate_py(hdr=HDR, parity_hdr=PARITY_HDR):
    L = ["# GENERATED by tools/gen_bindings.py from include/art.h and include/art_parity.h; do not edit.",
         "# To change the binding, edit the header, run `python tools/gen_bindings.py` and commit its outputs (tests/test_host.py compares this file with the headers).",
         '"""ctypes form of libart\'s C ABI: the constants, structs and callback type of both headers, and the (restype, argtypes) of every function --',
         'SYMBOLS for include/art.h (the boundary), PARITY_SYMBOLS for include/art_parity.h (the parity / rehearsal / measurement surface of the same library)."""',
         "import ctypes as C", ""]
    callbacks = []
    for path, table in ((hdr, "SYMBOLS"), (parity_hdr, "PARITY_SYMBOLS")):
        consts, _, structs, fnptr, funcs = parse(path)
        L.append(f"# ---- include/{os.path.basename(path)} ----")
        L += [f"{name} = {val}" for name, val in consts]
        for ret, name, params in fnptr:
            ps = c_params(params)
            L.append(f"{name} = C.CFUNCTYPE({', '.join([ctypes_type(ret)] + [ctypes_type(t, char_p=True) for t, _ in ps])})   # {', '.join(n for _, n in ps)}")
            callbacks.append(name)
        for name, packed, fields in structs:
            L += ["", "", f"class {name}(C.Structure):"] + (["    _pack_ = 1"] if packed else [])
            rows = [f'("{fname}", {ctypes_type(ctype, callbacks)}{f" * {arr}" if arr else ""})' for fname, ctype, arr in fields]
            L.append("    _fields_ = [" + ",\n                ".join(rows) + "]")
        L += ["", "", f"{table} = {{"]
        for ret, name, params in funcs:
            L.append(f'    "{name}": ({ctypes_type(ret, char_p=True)}, [{", ".join(ctypes_type(t, char_p=True) for t, _ in c_params(params))}]),')
        L += ["}", ""]
    return "\n".join(L)


def main():
    stale = []
    for out, text in ((OUT_RS, generate_rs()), (OUT_PY, generate_py())):
        rel = os.path.relpath(out, ROOT)
        if "--check" in sys.argv:
            if not os.path.exists(out) or open(out).read() != text:
                print(f"{rel} is stale: run python tools/gen_bindings.py")
                stale.append(rel)
            continue
        os.makedirs(os.path.dirname(out), exist_ok=True)
        open(out, "w").write(text)
        print(f"wrote {rel}: {text.count(chr(10))} lines")
    sys.exit(1 if stale else 0)


if __name__ == "__main__":
    main()
