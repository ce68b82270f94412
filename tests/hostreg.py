"""Does this host's HIP runtime page-lock memory the process already has?

Asked of the runtime alone (hipHostRegister / hipHostUnregister on a fresh anonymous
mapping), never through the project's library: some hosts refuse every such
registration (hipErrorInvalidValue) and page-lock only what is allocated page-locked
(hipHostMalloc). Tests and bench.py's end-to-end leg use the answer to choose their
output arrays; a refusal by project code on a host where the runtime accepts is then an
error, not a property of the host."""
from __future__ import annotations

import ctypes as C
import functools
import mmap

PROBE_BYTES = 8 << 20  # page-aligned, the size of the arrays the tests register


@functools.lru_cache(maxsize=None)
def host_register_error() -> int:
    """0 where hipHostRegister accepts an 8 MiB anonymous mapping (released again), else
    the hipError_t it returned (cleared, so that no later call reports it)."""
    import torch  # noqa: F401  (the process's HIP runtime: the one torch loaded)
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipHostRegister.argtypes = [C.c_void_p, C.c_size_t, C.c_uint]
    hip.hipHostUnregister.argtypes = [C.c_void_p]
    m = mmap.mmap(-1, PROBE_BYTES)
    buf = (C.c_char * PROBE_BYTES).from_buffer(m)
    try:
        rc = int(hip.hipHostRegister(C.addressof(buf), PROBE_BYTES, 0))
        if rc == 0:
            rc = int(hip.hipHostUnregister(C.addressof(buf)))
        hip.hipGetLastError()
        return rc
    finally:
        del buf
        m.close()
