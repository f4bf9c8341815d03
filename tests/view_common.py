"""helpers shared by the -m gpu tests of the view entries (test_gpu_views.py, test_gpu_forcing.py, test_gpu_*_view.py,
test_gpu_reference_fieldops.py).  Nothing here is cached: a context carries state (the timer switch, the grown staging buffers, the
vector_setup tables), so every test file keeps the contexts it shares between its tests in its own functools.lru_cache.  torch, pyoracle
and transport_se_amd are imported inside the functions, so that collection needs none of them."""
import contextlib
import ctypes as C

import numpy as np


class FakeArray:
    """a device array described by hand: an address (of a real allocation, or one a refusal test wants turned down) with strides in
    doubles of our choosing"""
    def __init__(self, shape, strides_doubles, ptr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr="<f8", data=(int(ptr), False), strides=tuple(8 * s for s in strides_doubles),
                                             version=3)


def oracle(ne, qsize):
    import pyoracle as po
    return po.Oracle(ne, qsize, nu_q=1e19)


def make_hip(o, qsize, nlev=72, weights=None, setup=None):
    """a fresh context of `qsize` tracers on the mesh of the oracle `o`, at 72 levels with the oracle's own vertical coordinate, at 64 or
    80 with remap_ld's.  weights: (spheremp, rspheremp) in place of the mesh's own; setup: the (D, metinv, mp) of vector_setup"""
    from gpu_common import elem_from_oracle
    from transport_se_amd.hip_mod import HipMod
    if nlev == 72:
        hv = (o.hyai, o.hybi, 1.0e5)
    else:
        import remap_ld
        if nlev == 80:
            import nlev80_common  # noqa: F401  (teaches remap_ld the 80-level grid)
        v = remap_ld.hvcoord(nlev)
        hv = (v.hyai, v.hybi, v.ps0)
    elem = elem_from_oracle(o)
    if weights is not None:
        elem["spheremp"], elem["rspheremp"] = np.ascontiguousarray(weights[0]), np.ascontiguousarray(weights[1])
    h = HipMod(elem, o.Dvv, hv, qsize, 1e19, device=0, nlev=nlev)
    assert h.nlev == nlev and h.nelemd == o.nelem
    if setup is not None:
        h.vector_setup(*setup)
    return h


def raw_field(h, name):
    """the whole allocation of a library field as a flat host array"""
    p, nbytes = h.device_ptr(name)
    assert p and nbytes, name
    out = np.empty(nbytes // 8)
    h.synchronize()
    assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(p), C.c_size_t(nbytes), C.c_int(2)) == 0
    return out


@contextlib.contextmanager
def capturing(stream):
    """the body runs while `stream` (a torch stream) is being captured; the capture is ended and its graph destroyed whatever the body did"""
    hiprt = C.CDLL("libamdhip64.so")
    assert hiprt.hipStreamBeginCapture(C.c_void_p(stream.cuda_stream), C.c_int(2)) == 0     # hipStreamCaptureModeRelaxed
    try:
        yield
    finally:
        graph = C.c_void_p()
        assert hiprt.hipStreamEndCapture(C.c_void_p(stream.cuda_stream), C.byref(graph)) == 0
        if graph.value:
            hiprt.hipGraphDestroy(graph)


class RawAllocation:
    """nbytes allocated with the runtime itself (not from torch's pool), holding the host array `fill` if one is given, and the range
    the runtime reports for it (it may round the size up): a view of nbytes that ends one double beyond that range is to be refused,
    the one at the allocation's start served.  ptr: the address; end: the end of the reported range; beyond: the address at which
    nbytes end one double past it.  The test frees it at its end (free)."""
    def __init__(self, nbytes, fill=None):
        self._rt = hiprt = C.CDLL("libamdhip64.so")
        self._raw, self.nbytes = C.c_void_p(), nbytes
        assert hiprt.hipMalloc(C.byref(self._raw), C.c_size_t(nbytes)) == 0
        if fill is not None:
            assert fill.nbytes == nbytes and fill.flags.c_contiguous
            assert hiprt.hipMemcpy(self._raw, C.c_void_p(fill.ctypes.data), C.c_size_t(nbytes), C.c_int(1)) == 0
        abase, asize = C.c_void_p(), C.c_size_t()
        assert hiprt.hipMemGetAddressRange(C.byref(abase), C.byref(asize), self._raw) == 0
        assert abase.value == self._raw.value and asize.value >= nbytes and asize.value % 8 == 0
        self.ptr, self.end = self._raw.value, abase.value + asize.value
        self.beyond = self.end - nbytes + 8

    def read(self, shape):
        """the allocation's contents as a host array of `shape`"""
        out = np.empty(shape)
        assert out.nbytes == self.nbytes
        assert self._rt.hipMemcpy(C.c_void_p(out.ctypes.data), self._raw, C.c_size_t(self.nbytes), C.c_int(2)) == 0
        return out

    def free(self):
        assert self._rt.hipFree(self._raw) == 0
