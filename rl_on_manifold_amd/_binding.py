"""What the ctypes binding modules share: one per row of build.TARGETS, named naming(key).binding.  A binding module
holds its structs, its SIGNATURES and the constants of its header; library() gives it the rest.  No numerics here.

The libraries are the product: if one is missing or cannot be loaded, load() raises -- there is no CPU / PyTorch
fallback anywhere in the package.
"""
import ctypes as C
import os
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
Names = namedtuple('Names', 'file env symbols binding')


def naming(key):
    """What is spelled after a library's key in build.TARGETS: its file name; its environment variable, which redirects what
    the binding loads (with _OUT appended: where build.py writes); the prefix of its C symbols; the module that binds it.
    The main library, `hip`, predates the others and has no infix."""
    infix = '' if key == 'hip' else key + '_'
    return Names('libatacom_%s.so' % key, 'ATACOM_%sLIB' % infix.upper(), 'atacom_' + infix, ('_lib_' + infix).rstrip('_'))


# the status codes and dtype tags of every public header (ATACOM_*_OK ..., ATACOM_*_F32 / F64)
OK, E_INVALID, E_HIP, E_UNSUPPORTED = 0, -1, -2, -3
F32, F64 = 0, 1


class AtacomError(RuntimeError):
    pass


def new_args(cls):
    """A zeroed argument struct with its struct_size filled in."""
    a = cls()
    a.struct_size = C.sizeof(cls)
    return a


_loaded = {}


def load(path, name, signatures):
    """Load (once) and return the shared library `name` at `path` with `signatures` applied: {symbol: (restype, argtypes)},
    argtypes None for a function without arguments.  Raises if it is not built."""
    if path in _loaded:
        return _loaded[path]
    # The process must use ONE HIP runtime.  PyTorch-ROCm bundles its own libamdhip64; if a library of ours were
    # dlopen'ed first it would pull in /opt/rocm's copy and the two runtimes would fight over the device (observed:
    # hipGetDeviceCount -> "no ROCm-capable device").  Importing torch first makes the .so bind to torch's runtime.
    try:
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001  (a pure-C consumer of the ABI does not need torch)
        pass
    if not os.path.exists(path):
        raise AtacomError("%s is not built (%s). Run `python -m rl_on_manifold_amd.build` -- "
                          "there is no CPU fallback." % (name, path))
    lib = C.CDLL(path)
    for symbol, (restype, argtypes) in signatures.items():
        fn = getattr(lib, symbol)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _loaded[path] = lib
    return lib


def library(key, signatures):
    """(LIB_PATH, load, check) of the library `key` of build.TARGETS.  The path is the library's file next to this module unless
    its environment variable points at an alternative build of it (kernel-tuning experiments do); load() loads it once with
    `signatures` applied and raises if it is not built; check(rc) raises AtacomError with the text of the library's
    last_error function for a non-zero code."""
    n = naming(key)
    path = os.environ.get(n.env) or os.path.join(HERE, n.file)

    def load_lib():
        return load(path, n.file, signatures)

    def check(rc):
        if rc != 0:
            raise AtacomError(getattr(load_lib(), n.symbols + 'last_error')().decode())
    return path, load_lib, check
