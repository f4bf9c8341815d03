"""The state%Q / state%lnps entries of the C ABI (tse_state_q, tse_copy_q_d2h, tse_copy_lnps_d2h) and of the Fortran seam's
device-resident route: declared with the documented signatures, listed in _lib.SYMBOLS, exported by the built library, and refused
without a context that holds them (no GPU needed)."""
import os
import re

from transport_se_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "tse_state_q": "int tse_state_q(tse_ctx *ctx, int nt)",
    "tse_copy_q_d2h": "int tse_copy_q_d2h(tse_ctx *ctx, double *q_elem1, size_t elem_stride, int qsize_d)",
    "tse_copy_lnps_d2h": "int tse_copy_lnps_d2h(tse_ctx *ctx, double *lnps_elem1, size_t elem_stride)",
}


def _header_declarations():
    text = open(os.path.join(ROOT, "include", "transport_se_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(2): " ".join(m.group(0).split()).rstrip(";").strip()
            for m in re.finditer(r"\b(int)\s+(tse_[a-z0-9_]+)\s*\([^)]*\)\s*;", text)}


def test_header_declares_the_q_entries_with_their_signatures():
    decl = _header_declarations()
    for name, sig in SIGNATURES.items():
        assert name in decl, name
        assert decl[name].replace("( ", "(").replace(" )", ")") == sig, decl[name]


def test_q_entries_are_listed_and_exported():
    for name in SIGNATURES:
        assert name in _lib.SYMBOLS, name
    L = _lib.lib()
    missing = [n for n in SIGNATURES if not hasattr(L, n)]
    assert not missing, missing


def test_fortran_seam_has_the_resident_route():
    """cuda_mod_hip.F90 binds the three entries and offers the resident-loop routines to a Fortran host"""
    src = open(os.path.join(ROOT, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    for c_name in ("tse_state_q", "tse_copy_q_d2h", "tse_copy_lnps_d2h", "tse_prim_run_subcycle", "tse_dcmip_init", "tse_dcmip_set_initial"):
        assert "name='%s'" % c_name in src, c_name
    for name, args in (("dcmip_init_hip", "elem, hvcoord, test_case"), ("prim_run_subcycle_hip", "elem, hvcoord, tl, dt, nsub"),
                       ("copy_state_d2h_hip", "elem, tl, want_qdp, want_q")):
        assert re.search(r"subroutine\s+%s\s*\(\s*%s\s*\)" % (name, re.escape(args)), src), name
        assert re.search(r"public\s*::[^\n]*\b%s\b" % name, src), name
