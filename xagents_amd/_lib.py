"""ctypes binding of libxagents_hip.so, derived from its C header at import.

include/xagents_hip.h is the only declaration of the ABI. The reader in _header.py turns its
`#define XA_*` integers, `typedef struct Xa*` blocks and prototypes into this module's XA_*
constants, Xa* ctypes.Structure classes and _SIGNATURES table, so a new entry point or
argument field is declared once, in the header, and the binding cannot disagree with what
the kernels were compiled against. A declaration the reader does not know fails the import.

There is no CPU fallback: if the HIP library is missing or fails to load, every
device op raises. Torch tensors are passed as raw device pointers plus sizes; the
stream is torch's current HIP stream so the calls compose with torch ops and can
be captured into a hipGraph (torch.cuda.CUDAGraph).
"""
import ctypes
from ctypes import c_void_p
from pathlib import Path

import torch

from xagents_amd._header import read_header

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / 'libxagents_hip.so'

_abi = read_header((PKG_DIR.parent / 'include' / 'xagents_hip.h').read_text())
globals().update(_abi.constants)  # XA_*
globals().update(_abi.structs)    # Xa*
_SIGNATURES = _abi.signatures     # name -> (restype, [argtypes])
MLP_HIDDEN = _abi.constants['XA_MLP_HIDDEN']
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


class HipLibraryError(RuntimeError):
    pass


def load(path=None):
    """Load (once) and return the ctypes handle. Raises if the .so is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise HipLibraryError(
            f'{p} not found: build it with `python -m xagents_amd._build` '
            f'(or __graft_entry__.build()). There is no CPU fallback.'
        )
    lib = ctypes.CDLL(str(p))
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        # the product library must be built from the sources in this tree (diagnostic
        # builds loaded by path are exempt)
        from xagents_amd._build import source_hash
        built, want = lib.xa_build_hash().decode(), source_hash()
        if built != want:
            raise HipLibraryError(
                f'{p} is stale: built from sources {built}, this tree is {want}; rebuild with '
                f'`python -m xagents_amd._build` (or __graft_entry__.build())')
        _lib = lib
    return lib


def check(ret, name):
    if ret != 0:
        msg = load().xa_last_error().decode()
        raise HipLibraryError(f'{name} failed ({ret}): {msg}')


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HipLibraryError('xagents_amd device ops need tensors on a HIP device')
    if not t.is_contiguous():
        raise HipLibraryError('xagents_amd device ops need contiguous tensors')
    return t.data_ptr()


if hasattr(torch._C, '_cuda_getCurrentRawStream') and hasattr(torch._C, '_cuda_getDevice'):
    _raw_stream, _cur_dev = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice

    def stream():
        """The current HIP stream of the current device (a capture stream inside hipGraph
        capture), as a raw handle: two C calls instead of torch.cuda.current_stream()'s
        Python wrappers (~3 us per launch on the C3 host path, tools/c3_host_profile.py)."""
        return _raw_stream(_cur_dev())
else:
    def stream():
        return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    check(getattr(load(), name)(*args), name)


def mapped_address(host):
    """Device address of a pinned host tensor (pinned memory is mapped): a launch loads or
    stores there over the host link."""
    dev = c_void_p()
    call('xa_host_device_pointer', c_void_p(host.data_ptr()), ctypes.byref(dev))
    return dev.value


def mapped_pinned(shape, dtype):
    """(zero-filled pinned host tensor, its device address)."""
    host = torch.zeros(shape, dtype=dtype).pin_memory()
    return host, mapped_address(host)
