"""The loader behind the ctypes binding modules (_lib, _lib_point, _lib_point_policy, _lib_point_compact, _lib_point_vec,
_lib_returns).  No numerics here.

The libraries are the product: if one is missing or cannot be loaded, load() raises -- there is no CPU / PyTorch
fallback anywhere in the package.
"""
import ctypes as C
import os


class AtacomError(RuntimeError):
    pass


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


def checker(load_lib, last_error):
    """check(rc) of one library: raises AtacomError with the text of its `last_error` function for a non-zero code."""
    def check(rc):
        if rc != 0:
            raise AtacomError(getattr(load_lib(), last_error)().decode())
    return check
