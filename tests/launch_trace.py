"""TEST INFRASTRUCTURE: record the kernel launches of a forward pass without launching anything.

Usage in a CPU test:   ``with launch_trace() as lines: net.forward_into(x, out)``.
Installed the way emu_backend.py installs the emulator, but over the PRODUCT library (it loads without a GPU, tests/test_abi.py): inside the context
`monai_amd._lib.lib()` is that library with `call` replaced by a recorder that launches nothing, the "must be a ROCm tensor" half of `require_device`
is lifted (the dtype half stays) and `query` stays real -- configuration selection, tile counts and buffer sizes are host arithmetic, so the recorded
plan is the plan the MI355X runs.  Every call becomes one text line: the entry name, then its arguments read off `_lib.SIGNATURES` -- integers and
floats verbatim, raw pointers as null / non-null, int32 (and floating-point) arrays as lists, an `mh_tensor5` as `N C D H W n_stride has_nrm
nrm_n_stride`.  No addresses."""
import contextlib
import ctypes as C
import os


def _tensor5(a) -> str:
    t = a._obj                      # the MhTensor5 behind C.byref(...)
    return f"[{t.N} {t.C} {t.D} {t.H} {t.W} {t.n_stride} {int(bool(t.nrm))} {t.nrm_n_stride}]"


def _pointer(a) -> str:
    v = a.value if isinstance(a, C.c_void_p) else a
    return "non-null" if v else "null"


def _array(a) -> str:
    return "null" if a is None else "(" + ",".join(repr(v) for v in a) + ")"


def _line(signatures, name: str, args) -> str:
    from monai_amd import _lib

    argtypes = signatures[name][1]
    assert len(argtypes) == len(args), (name, len(argtypes), len(args))
    out = [name[3:] if name.startswith("mh_") else name]
    for ty, a in zip(argtypes, args):
        if ty is C.POINTER(_lib.MhTensor5):
            out.append(_tensor5(a))
        elif ty in (C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)):
            out.append(_array(a))
        elif ty in (C.c_int, C.c_int64):
            out.append(str(int(a)))
        elif ty is C.c_float:
            out.append(repr(float(a)))
        else:                       # c_void_p, and int64 tables of places (addresses by another name)
            out.append(_pointer(a))
    return " ".join(out)


@contextlib.contextmanager
def launch_trace():
    import torch

    from monai_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):      # a fresh checkout: the .so is git-ignored; hipcc cross-compiles without a GPU
        from monai_amd import build

        build.build()
    lines: list = []
    saved = (_lib._LIB, _lib.require_device)
    lib = _lib.Library(_lib.LIB_PATH)
    lib.call = lambda name, *args: lines.append(_line(_lib.SIGNATURES, name, args))

    def host_ok(*tensors, dtypes=(torch.float32,)):
        for t in tensors:
            if t is not None and t.dtype not in dtypes:
                raise _lib.UnsupportedOnDevice(f"monai_amd: dtype {t.dtype} is not accepted on this path (expected one of {dtypes})")

    _lib._LIB, _lib.require_device = lib, host_ok
    try:
        yield lines
    finally:
        _lib._LIB, _lib.require_device = saved
