"""The level count as a build setting, without a GPU: the 64-level library (libtransport_se_hip_L64.so) exports the whole C ABI
and reports its level count; the vertical-coordinate reader and the namelist front end take the reference's 12k_top-64 grid;
tests/remap_model.py, the any-nlev restatement of remap_Q_ppm the 64-level GPU tests check against, equals the oracle at 72."""
import os
import subprocess

import numpy as np
import pytest

from transport_se_amd import _lib
from transport_se_amd import prim_main as pm
from transport_se_amd.hybvcoord import DATA, HvCoord

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VC = os.path.join(ROOT, "tests", "golden", "vcoord")
M64, I64 = os.path.join(VC, "12k_top-64m.ascii"), os.path.join(VC, "12k_top-64i.ascii")


def test_the_64_level_library_exports_every_symbol_and_reports_its_level_count():
    assert _lib.so_path(64).endswith("libtransport_se_hip_L64.so") and _lib.so_path(None) == _lib.so_path(72) == _lib.SO
    L64 = _lib.lib(nlev=64)
    missing = [s for s in _lib.SYMBOLS if not hasattr(L64, s)]
    assert not missing, missing
    assert L64.tse_nlev() == 64
    assert _lib.lib().tse_nlev() == 72 == _lib.DEFAULT_NLEV
    assert _lib.lib(nlev=72) is _lib.lib()
    with pytest.raises(RuntimeError, match="built for nlev = 72, not 64"):
        _lib._check_nlev(_lib.lib(), _lib.SO, 64)


def test_a_library_for_another_level_count_refuses_a_mismatched_host():
    """HipMod loads the library of its hvcoord's level count and checks it; a 64-level coordinate with nlev=72 is refused"""
    from transport_se_amd.hip_mod import HipMod, TseError
    hv = HvCoord(M64, I64)
    with pytest.raises(TseError, match="nlev = 72 needs 73"):
        HipMod({}, np.zeros((4, 4)), (hv.hyai, hv.hybi, hv.ps0), 1, 0.0, nlev=72)


@pytest.mark.parametrize("nlev,msg", [(96, "NLEV <= 72"), (60, "multiple of 8"), (70, "multiple of 4")])
def test_level_counts_the_kernels_cannot_serve_fail_at_compile_time(tmp_path, nlev, msg):
    src = os.path.join(ROOT, "transport_se_amd", "csrc", "tse_api.hip")
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-DNLEV=%d" % nlev, src],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path), timeout=600)
    out = res.stdout.decode()
    assert res.returncode != 0 and "static assertion failed" in out and msg in out, out[-2000:]


def test_hvcoord_reads_the_12k_top_64_grid_and_refuses_mismatched_files():
    hv = HvCoord(M64, I64)
    assert (hv.nlev, hv.nlevp) == (64, 65)
    assert hv.hyai.size == hv.hybi.size == 65 and hv.hyam.size == hv.hybm.size == 64
    assert np.all(np.diff(hv.etai) > 0) and np.all((hv.etam > hv.etai[:-1]) & (hv.etam < hv.etai[1:]))
    hv72 = HvCoord()
    assert (hv72.nlev, hv72.hyai.size) == (72, 73)
    # the reference's checks (hybvcoord_mod.F90:76-102): the interface file must hold plev + 1 levels
    with pytest.raises(ValueError, match="Error: hyai input file and HOMME plevp do not match 65 73"):
        HvCoord(M64, os.path.join(DATA, "acme-72i.ascii"))
    with pytest.raises(ValueError, match="Error: hyai input file and HOMME plevp do not match 73 65"):
        HvCoord(os.path.join(DATA, "acme-72m.ascii"), I64)
    with pytest.raises(ValueError, match="Error: hyai input file and HOMME plevp do not match 73 65"):
        HvCoord(M64, I64, nlev=72)


NL = """
&ctl_nl
  test_case = "dcmip1-1"
  ne = 4
  qsize = 4
  nmax = 6
  tstep = 900
  qsplit = 1, rsplit = 3
  limiter_option = 8
/
&vert_nl
  vfile_mid = "%s"
  vfile_int = "%s"
/
"""


def test_namelist_picks_the_grid_its_vfile_lines_name(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    # the reference's own namelists name the shipped acme-72 files: served from the package wherever the run starts
    s = pm.settings(pm.parse_namelists(NL % ("vcoord/acme-72m.ascii", "vcoord/acme-72i.ascii")))
    hv = pm.vertical_coordinate(s)
    ref = HvCoord()
    assert hv.nlev == 72 and np.array_equal(hv.hyai, ref.hyai) and np.array_equal(hv.hybm, ref.hybm)
    assert pm.vertical_coordinate(pm.settings(pm.parse_namelists(NL % ("", "")))).nlev == 72
    # 12k_top-64 (the commented-out lines of test/dcmip1-1/dcmip1-1.nl): opened relative to the working directory
    nl64 = NL % ("vcoord/12k_top-64m.ascii", "vcoord/12k_top-64i.ascii")
    with pytest.raises(SystemExit, match="error in hvcoord_init"):
        pm.vertical_coordinate(pm.settings(pm.parse_namelists(nl64)))
    os.makedirs("vcoord")
    for src in (M64, I64):
        with open(src) as f, open(os.path.join("vcoord", os.path.basename(src)), "w") as g:
            g.write(f.read())
    hv = pm.vertical_coordinate(pm.settings(pm.parse_namelists(nl64)))
    assert hv.nlev == 64 and np.array_equal(hv.hyai, HvCoord(M64, I64).hyai)
    # mismatched pair: the reference's message, then hvcoord_init's
    with pytest.raises(SystemExit, match="hyai input file and HOMME plevp do not match"):
        pm.vertical_coordinate(pm.settings(pm.parse_namelists(NL % ("vcoord/12k_top-64m.ascii", "vcoord/acme-72i.ascii"))))


def _column(nlev, seed, hv):
    rng = np.random.default_rng(seed)
    ps = 1e5 * (1 + 0.02 * rng.standard_normal((1, 4, 4)))
    dp2 = np.diff(hv.hyai)[:, None, None] * hv.ps0 + np.diff(hv.hybi)[:, None, None] * ps
    dp1 = dp2 * (1 + 0.06 * rng.standard_normal(dp2.shape).clip(-2, 2))
    dp1 *= dp2.sum(0) / dp1.sum(0)
    q = rng.random((5, nlev, 4, 4)) * dp1
    return q, dp1, dp2


@pytest.mark.parametrize("alg", [0, 2])
def test_remap_model_equals_the_oracle_at_72_levels(alg):
    """the numpy restatement reproduces pyoracle.remap_q_ppm BIT FOR BIT (tolerance 0) at 72 levels, alg 0 and 2, on columns
    whose layers move by up to 12 % (several new levels take their mass from two old cells and more)"""
    import pyoracle as po
    from remap_model import remap_q_ppm
    hv = HvCoord()
    po.set_vert_remap_q_alg(alg)
    try:
        for seed in range(3):
            q, dp1, dp2 = _column(72, seed, hv)
            assert np.array_equal(remap_q_ppm(q, dp1, dp2, alg), po.remap_q_ppm(q, dp1, dp2))
    finally:
        po.set_vert_remap_q_alg(0)


@pytest.mark.parametrize("alg", [0, 2])
def test_remap_model_at_64_levels_keeps_mass_and_constants(alg):
    from remap_model import remap_q_ppm
    hv = HvCoord(M64, I64)
    q, dp1, dp2 = _column(64, 7, hv)
    out = remap_q_ppm(q, dp1, dp2, alg)
    assert np.abs(out.sum(1) - q.sum(1)).max() <= 1e-13 * np.abs(q.sum(1)).max()
    c = remap_q_ppm(np.stack([dp1 * 0.25]), dp1, dp2, alg)[0]          # a constant mixing ratio stays constant
    assert np.abs(c / dp2 - 0.25).max() < 1e-14
