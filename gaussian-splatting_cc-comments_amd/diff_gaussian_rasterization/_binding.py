"""The one place where the Python layer meets the C ABI of libgsr_hip.so, and the argument checks its modules share.

Declarations are data.  A module that calls into the library declares the entry points it uses as one table, tagged with the header
the table mirrors, and the ctypes mirrors of that header's structs beside it:

    _lib, _run = _binding.declare("gsr_vq.h", {"gsr_vq_assign_scratch_bytes": (c_size_t, [c_int] * 3), ...}, {"gsr_x_args": XArgs})

_lib() is the loaded library with every table declared so far applied to it, _run(name, *args) calls an entry point that returns a
status and raises on a failure.  A module that calls entry points of another module's table imports that module (which declares
it) and says so with needs=: fused_vq and fused_rigidity need "gsr_knn.h".  tests/test_binding_cpu.py holds TABLES to include/*.h.

Nothing here loads the library at import; _C (the loader) is imported when it is first needed.
"""
import ctypes

import torch

TABLES = []   # (header, {entry point: (restype, argtypes)}, {C struct name: ctypes.Structure}), in the order of declaration
_loader = None   # the module _C, which imports this one: fetched by the first lib()


def declare(header, functions, structs=None, needs=()):
    """Adds one table -> (lib, run), what the declaring module keeps as its _lib and _run."""
    missing = [h for h in needs if h not in {t[0] for t in TABLES}]
    if missing:
        raise ImportError(f"the table of {header} needs {missing}: import the module that declares it first")
    TABLES.append((header, functions, structs or {}))
    return lib, run


def bind(L):
    """Applies the tables to a loaded library.  An older build of the ABI (_C.use_library) may lack the newer entry points: a name
    it does not export is skipped, so a call to it fails with AttributeError, and nothing stands in for it."""
    for _, functions, _ in TABLES[getattr(L, "_gsr_tables", 0):]:
        for name, (restype, argtypes) in functions.items():
            fn = getattr(L, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
    L._gsr_tables = len(TABLES)
    return L


def lib():
    """The loaded library, with every table declared so far applied"""
    global _loader
    if _loader is None:
        from . import _C as _loader
    L = _loader.lib()
    return L if L._gsr_tables == len(TABLES) else bind(L)


def check(rc):
    """The status of an entry point: anything but 0 raises with the library's message."""
    if rc != 0:
        raise RuntimeError(f"gsr error {rc}: {lib().gsr_last_error().decode()}")


def run(name, *args):
    """The one place a kernel entry point is called from by name."""
    check(getattr(lib(), name)(*args))


# ---- pointers and strides ---------------------------------------------------------------------------------------------------------
def ptr(t):
    """A tensor's address, NULL for None"""
    return None if t is None else t.data_ptr()


def pointers(tensors):
    """A list of tensors (or None) -> a C array of their addresses"""
    return (ctypes.c_void_p * len(tensors))(*[ptr(t) for t in tensors])


def strided(t):
    """A 2-D tensor whose second dimension is dense and whose rows do not overlap (else a contiguous copy)"""
    dense = t.shape[1] <= 1 or t.stride(1) == 1
    apart = t.shape[0] <= 1 or t.stride(0) >= max(1, t.shape[1])
    return t if dense and apart else t.contiguous()


def stride0(t):
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


# ---- argument checks: none of them touches the library ------------------------------------------------------------------------------
def check_device(what, *tensors):
    """HIP tensors on one device -> the device; `what` names the kernels in the refusal."""
    dev = tensors[0].device
    if dev.type != "cuda" or any(t.device != dev for t in tensors):
        raise RuntimeError(f"the tensors must be HIP (cuda) tensors on one device; the {what} have no CPU path")
    return dev


def check_int(name, v, lo, hi=None):
    """An int that is no bool, in lo..hi, or at least lo where hi is None"""
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{name} must be an int, got {v!r}")
    if hi is None and v < lo:
        raise ValueError(f"{name} must be at least {lo}; got {v}")
    if hi is not None and not lo <= v <= hi:
        raise ValueError(f"{name} must lie in {lo}..{hi}; got {v}")


def check_number(name, v, kind="a Python float", got=lambda v: type(v).__name__):
    """A Python number that is not a bool -> float"""
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{name} must be {kind}, got {got(v)}")
    return float(v)


def check_matrix(name, t, dims="two dimensions", cols=None):
    """A 2-D float32 tensor, any strides, of `cols` columns where given; `dims` words the shape in the refusal."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    if t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise RuntimeError(f"{name} must have {dims}; got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32; got {t.dtype}")


def check_rows(named, cols, other=None):
    """named: [(name, tensor)], float32 (P, cols[name]) each with P >= 1 the rows of the first; a name that cols does not hold has
    its shape checked by other(name, tensor, P).  -> P"""
    for n, t in named:
        if not torch.is_tensor(t):
            raise TypeError(f"{n} must be a tensor")
    first_name, first = named[0]
    P = int(first.shape[0]) if first.dim() else 0
    for n, t in named:
        if n not in cols:
            other(n, t, P)
        elif tuple(t.shape) != (P, cols[n]) or P < 1:
            raise RuntimeError(f"{n} must be (P, {cols[n]}) with P >= 1 rows as {first_name}; got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{n} must be float32; got {t.dtype}")
    return P
