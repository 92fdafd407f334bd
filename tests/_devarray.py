"""Device arrays for the tests of the *_device entry points (not a test module)."""
import ctypes as C

import numpy as np

from fitgpu import _lib


class DevArray:
    """A numpy array's copy in device memory, through the HIP runtime libfitgpu.so resolved at load
    time: hipMalloc & co looked up through the library's own handle, which searches its dependencies.
    Not through torch: its wheel carries a HIP runtime of its own, and when the engine's runtime
    started first in the process, torch's finds no GPU."""
    _hip = None

    @classmethod
    def hip(cls):
        if cls._hip is None:
            cls._hip = C.CDLL(_lib.LIB_PATH)
            cls._hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            cls._hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            cls._hip.hipFree.argtypes = [C.c_void_p]
        return cls._hip

    def __init__(self, a):
        self.shape, self.dtype, self.nbytes, self.n = a.shape, a.dtype, max(a.nbytes, 4), a.size
        self.p = C.c_void_p()
        assert self.hip().hipMalloc(C.byref(self.p), self.nbytes) == 0
        a = np.ascontiguousarray(a)
        assert self.hip().hipMemcpy(self.p, C.c_void_p(a.ctypes.data), a.nbytes, 1) == 0  # host to device

    def data_ptr(self):
        return self.p.value

    def numel(self):
        return self.n

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        assert self.hip().hipMemcpy(C.c_void_p(out.ctypes.data), self.p, out.nbytes, 2) == 0  # device to host
        return out

    def __del__(self):
        if self.p:
            self.hip().hipFree(self.p)
            self.p = None
