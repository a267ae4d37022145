"""ctypes loader of libart.so.  The C ABI itself -- constants, structs, prototypes -- is _abi.py, generated from include/art.h and include/art_parity.h by
tools/gen_bindings.py and re-exported here; this module adds what is not ABI.  Fails loudly: there is no Python or CPU fallback."""
import ctypes as C
import os

from . import _abi
from ._abi import *  # noqa: F401,F403  (_lib.ArtRayCast, _lib.SYMBOLS, _lib.ART_FLAG_* ...: the names everything binds through)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ART_LIB_PATH") or os.path.join(_HERE, "libart.so")   # ART_LIB_PATH: another build of the same sources, for A/B measurements (tools/); libart itself reads no environment


class ArtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libart error {code}: {msg}")
        self.code = code


class ArtStats(_abi.ArtStats):
    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if not n.startswith("reserved")}


_lib = None


def load():
    """Load libart.so; raises if the HIP extension has not been built (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C araytracingjourney_amd/csrc` (libart has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(_abi.SYMBOLS.items()) + list(_abi.PARITY_SYMBOLS.items()):
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code):
    if code != _abi.ART_OK:
        raise ArtError(code, load().art_last_error().decode("utf-8", "replace"))
