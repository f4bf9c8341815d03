"""The host tables tse_init builds from the reference-style edge descriptors (csrc/tse_tables.cpp), read on the CPU through the
test entry of the -DTSE_AB_HOOKS library (tse_test_tables / tse_test_table / tse_test_tables_free; not in the product library)."""
import ctypes as C

import numpy as np

from transport_se_amd import _lib

COUNTS = ("ncol_send", "ncol_recv", "nmm_send", "nmm_recv", "nslots", "cse", "n_bnd", "n_int", "npatch", "np_bnd", "np_int",
          "zero0", "halo0")
# element type of every table; (dtype, 2): the {x, y} pairs uploaded as int2
TABLES = {"send_peer": np.int32, "recv_peer": np.int32, "send_len": np.int32, "recv_len": np.int32, "mm_send_len": np.int32,
          "mm_recv_len": np.int32, "send_src": (np.int32, 2), "mm_send_src": (np.int32, 2), "dss_tab": (np.int32, 2), "nbr": np.int32,
          "order": np.int32, "ord_bnd": np.int32, "ord_int": np.int32, "slot_of": np.int32, "pperm": np.uint64, "pexp": np.uint8,
          "send_src_s": (np.int32, 2), "etab": np.uint32, "rl_all": np.int32, "rl_bnd": np.int32, "rl_int": np.int32,
          "pslots": np.int32, "pring": np.uint32, "plds": np.uint16, "pering": np.int32, "pnb": np.uint8, "plist_bnd": np.int32,
          "plist_int": np.int32}


def _hooks():
    L = _lib.lib(_lib.HOOKS_SO)
    if not getattr(L, "_tables_typed", False):
        L.tse_test_tables.argtypes = [C.POINTER(_lib.InitArgs), C.c_int, C.POINTER(C.c_void_p)]
        L.tse_test_table.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.tse_test_tables_free.argtypes = [C.c_void_p]; L.tse_test_tables_free.restype = None
        L._tables_typed = True
    return L


def host_tables(desc, strips=False):
    """dict of the tables (numpy copies) and the counts of tse_init for the descriptors of cube_mesh.edge_descriptors"""
    L = _hooks()
    n = desc["putmapP"].shape[0]
    keep = []

    def arr(x):
        x = np.ascontiguousarray(x, dtype=np.int32); keep.append(x); return x.ctypes.data_as(C.c_void_p)
    a = _lib.InitArgs()
    a.nelemd = n
    a.putmapP, a.getmapP, a.reverse = arr(desc["putmapP"]), arr(desc["getmapP"]), arr(desc["reverse"])
    for side in ("send", "recv"):
        cyc = np.array(desc[side], dtype=np.int32).reshape(-1, 3)
        setattr(a, "n" + side, cyc.shape[0])
        for col, nm in enumerate(("peer", "ptrP", "lengthP")):
            setattr(a, "%s_%s" % (side, nm), arr(cyc[:, col]))
    h = C.c_void_p()
    if L.tse_test_tables(C.byref(a), int(strips), C.byref(h)):
        raise RuntimeError(L.tse_last_error().decode())
    try:
        def get(name):
            p, nb = C.c_void_p(), C.c_size_t()
            assert L.tse_test_table(h, name.encode(), C.byref(p), C.byref(nb)) == 0, L.tse_last_error().decode()
            return C.string_at(p, nb.value) if nb.value else b""
        out = {"raw": {}}   # raw: the bytes tse_init uploads
        out.update({k: int(v) for k, v in zip(COUNTS, np.frombuffer(get("counts"), dtype=np.int32))})
        for name, t in TABLES.items():
            raw = get(name)
            out["raw"][name] = raw
            out[name] = np.frombuffer(raw, dtype=t[0]).reshape(-1, 2) if isinstance(t, tuple) else np.frombuffer(raw, dtype=t)
        return out
    finally:
        L.tse_test_tables_free(h)


def check_remap_grids(dp1, dp2):
    """check_remap_grids (csrc/tse_tables.cpp; what tse_remap_q_ppm runs before any upload or launch) on dp1, dp2[E][nlev][4][4]:
    None for a good pair, else ((element, column, level), message) of the first offender"""
    L = _hooks()
    L.tse_test_remap_grids.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    d1, d2 = np.ascontiguousarray(dp1, dtype=np.float64), np.ascontiguousarray(dp2, dtype=np.float64)
    assert d1.shape == d2.shape and d1.shape[2:] == (4, 4)
    where = (C.c_int * 3)(-1, -1, -1)
    if L.tse_test_remap_grids(d1.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p), d1.shape[0], d1.shape[1], where):
        return tuple(where), L.tse_last_error().decode()
    return None
