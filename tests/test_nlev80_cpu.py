"""80 levels without a GPU: libtransport_se_hip_L80.so cross-compiles, exports the whole C ABI and reports its level count; every
other count above 72 still fails to compile with the rule in the message; the 80-level coordinate fixtures are what the reference's
write_level_files rule gives (tests/vcoord_levels.py) and that rule reproduces the reference-made 64-level files; the remap model
(tests/remap_model.py) stays within the pointwise longdouble bound (tests/remap_ld.py) at 80 levels."""
import os
import subprocess

import numpy as np
import pytest

import nlev80_common as c80
import remap_ld as rl
import remap_model as rm
import vcoord_levels as vl
from step_ld import has_extended_precision, ratio
from transport_se_amd import _lib
from transport_se_amd.hybvcoord import DATA, HvCoord

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 0.01   # test_remap_bound_cpu.py / test_gpu_remap_pointwise.py: at most 1 % of a family pair's outputs may be unsafe


def test_the_80_level_library_builds_exports_every_symbol_and_reports_its_level_count():
    assert 80 in _lib.NLEV_BUILDS and _lib.so_path(80).endswith("libtransport_se_hip_L80.so")
    so = _lib.build(nlev=80)          # hipcc --offload-arch=gfx950 (up to date after __graft_entry__.build(): no compile)
    assert so == _lib.so_path(80) and os.path.exists(so)
    L80 = _lib.lib(nlev=80)           # (checks tse_nlev())
    missing = [s for s in _lib.SYMBOLS if not hasattr(L80, s)]
    assert not missing, missing
    assert L80.tse_nlev() == 80
    with pytest.raises(RuntimeError, match="built for nlev = 80, not 72"):
        _lib._check_nlev(L80, so, 72)


def _syntax_only(tmp_path, nlev, unit="tse_api.hip"):
    src = os.path.join(ROOT, "transport_se_amd", "csrc", unit)
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-DNLEV=%d" % nlev, src],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path), timeout=600)
    return res.returncode, res.stdout.decode()


@pytest.mark.parametrize("nlev", [88, 96])
def test_every_other_count_above_72_still_fails_to_compile(tmp_path, nlev):
    rc, out = _syntax_only(tmp_path, nlev)
    assert rc != 0 and "static assertion failed" in out and "NLEV <= 72" in out, out[-2000:]


@pytest.mark.parametrize("nlev", [80, 72, 64])
def test_the_built_counts_pass_the_rules(tmp_path, nlev):
    for unit in ("tse_api.hip", "tse_views_api.hip"):   # (the view unit: the level rules of tse_view_kernels.h and tse_view_launch.h)
        rc, out = _syntax_only(tmp_path, nlev, unit)
        assert rc == 0 and "static assertion" not in out, (unit, out[-2000:])


def test_the_80_level_fixtures_are_what_the_formula_gives():
    """the committed files equal the helper's rendering character for character, so every value equals the formula's to the 17 digits
    printed; hyai + hybi strictly increases from eta_top to 1, hybi runs from exactly 0 to exactly 1, every dp0(k) > 0, and HvCoord
    reads them as an 80-level coordinate and refuses mismatched pairs with the reference's message"""
    mid, itf = vl.paths(80)
    for name, text in vl.files(80).items():
        with open(os.path.join(vl.VC, name)) as f:
            assert f.read() == text, name
    hv = HvCoord(mid, itf)
    assert (hv.nlev, hv.nlevp) == (80, 81) and hv.hyai.size == hv.hybi.size == 81 and hv.hyam.size == hv.hybm.size == 80
    ai, bi, am, bm = vl.levels(80)
    for got, want in ((hv.hyai, ai), (hv.hybi, bi), (hv.hyam, am), (hv.hybm, bm)):
        assert (np.abs(got - want) <= vl.ulp_last_digit(want)).all()
    assert np.all(np.diff(hv.etai) > 0) and hv.etai[-1] == 1.0 and abs(hv.etai[0] - np.exp(-vl.Z_TOP / vl.H)) < 1e-16
    assert hv.hybi[0] == 0.0 and hv.hybi[80] == 1.0 and hv.hyai[80] == 0.0 and np.all(np.diff(hv.hybi) > 0)
    assert np.all((hv.etam > hv.etai[:-1]) & (hv.etam < hv.etai[1:]))
    dp0 = np.diff(hv.hyai) * hv.ps0 + np.diff(hv.hybi) * hv.ps0      # prim_advection_mod.F90:818-819
    assert (dp0 > 0).all()
    assert HvCoord(mid, itf, nlev=80).nlev == 80
    with pytest.raises(ValueError, match="Error: hyai input file and HOMME plevp do not match 81 73"):
        HvCoord(mid, os.path.join(DATA, "acme-72i.ascii"))
    with pytest.raises(ValueError, match="Error: hyai input file and HOMME plevp do not match 65 81"):
        HvCoord(vl.paths(64)[0], itf)
    with pytest.raises(ValueError, match="Error: hyai input file and HOMME plevp do not match 73 81"):
        HvCoord(mid, itf, nlev=72)


MEASURED_64 = 2.65e-15   # the largest relative deviation of the formula from the reference-made 64-level files (see below)


def test_the_formula_reproduces_the_reference_made_64_level_files():
    """tests/vcoord_levels.py at 64 levels against 12k_top-64{m,i}.ascii, which the reference made by the same rule.  Measured: 233 of
    the 258 values agree in all 17 printed digits; the largest relative deviation is 2.647e-15 (hyai, where A = eta - B cancels;
    hybi 8.3e-16, hyam 1.5e-15, hybm 4.4e-16) -- one ulp of exp() between the two math libraries, amplified by the two differences of the
    rule.  Asserted: MEASURED_64 relative, plus one unit in the last printed digit of the value."""
    hv = HvCoord(*vl.paths(64))
    worst = 0.0
    for got, want in zip((hv.hyai, hv.hybi, hv.hyam, hv.hybm), vl.levels(64)):
        assert got.shape == want.shape
        d = np.abs(got - want)
        worst = max(worst, float((d[want != 0] / np.abs(want[want != 0])).max()))
        assert (d <= MEASURED_64 * np.abs(want) + vl.ulp_last_digit(want)).all()
        assert np.array_equal(got == 0, want == 0)
    print("formula vs the reference-made 64-level files: largest relative deviation %.4g" % worst)
    assert 0 < worst <= MEASURED_64


@pytest.mark.parametrize("alg", [0, 2])
def test_the_remap_model_lies_within_the_pointwise_bound_at_80_levels(alg):
    """remap_model.remap_q_ppm in fp64 against remap_ld's longdouble value and bound on remap_ld's input families built on the 80-level
    grid (the arrays the GPU test hands to the device): every safe output within the bound, at most 1 % of a (grid family, tracer
    family) pair unsafe, every column's mass; the grid families are what their names say at 80 levels, some column leaving {k, k+1}"""
    assert has_extended_precision(), np.finfo(np.longdouble)
    for qsize in c80.REMAP_QSIZES:
        Q, dp1, dp2 = rl.inputs(80, qsize)
        assert Q.shape == (rl.NELEM, qsize, 80, 4, 4)
        t, safe, kid = rl.remap_q_ppm(Q, dp1, dp2, alg)
        assert t.m == 81          # max(nlev - 1, 55) + 2
        ref = np.stack([rm.remap_q_ppm(Q[e], dp1[e], dp2[e], alg) for e in range(rl.NELEM)])
        _, r = ratio(ref, t)
        assert np.where(safe, r, 0.0).max() <= 1.0, (alg, qsize, float(np.where(safe, r, 0.0).max()))
        wm, _ = rl.column_mass_ratio(ref, Q, t)
        assert wm <= 1.0, (alg, qsize, wm)
        for grid in rl.GRIDS:
            es = [e for e in range(rl.NELEM) if rl.grid_family(e) == grid]
            for fam in rl.TRACERS:
                qs = [q for q in range(qsize) if rl.tracer_family(q) == fam]
                if qs:
                    assert 1.0 - safe[es][:, qs].mean() <= CAP, (alg, qsize, grid, fam)
    off = c80.kid_offsets(dp1, dp2)
    for e in range(rl.NELEM):
        fam = rl.grid_family(e)
        if fam in ("gentle", "identity"):
            assert off[:, e].min() >= 0 and off[:, e].max() <= 1, (fam, e)
        if fam == "squeeze":
            assert off[:, e].max() > 15      # kid(k) far outside {k, k+1}: the generic column loop


@pytest.mark.parametrize("alg", [0, 2])
def test_the_vertical_remap_inputs_of_the_gpu_test_keep_the_cap(alg):
    """the states test_gpu_nlev80.py hands to tse_vertical_remap (remap_ld's families moved by dt*divdp_proj; the grids as k_remap's
    phase 1 forms them, FMAs evaluated exactly): they satisfy the bracket search's precondition, the fp64 model lies within the bound on
    them and at most 1 % of a family pair's outputs are unsafe -- so the cap the GPU test applies is a condition on the inputs"""
    import test_gpu_nlev80 as g80
    hv = c80.hv80()
    for qsize in c80.REMAP_QSIZES:
        Q, dp, dv = g80.vremap_inputs(qsize)
        dp3d, ps, dp2 = g80.vremap_grids(dp, dv, hv)
        rl.check_inputs(dp3d, dp2)
        assert np.abs(dp2.sum(1) + hv.hyai[0] * hv.ps0 - ps).max() <= 1e-13 * ps.max()
        t, safe, kid = rl.remap_q_ppm(Q, dp3d, dp2, alg)
        ref = np.stack([rm.remap_q_ppm(Q[e], dp3d[e], dp2[e], alg) for e in range(rl.NELEM)])
        _, r = ratio(ref, t)
        assert np.where(safe, r, 0.0).max() <= 1.0
        for grid in rl.GRIDS:
            es = [e for e in range(rl.NELEM) if rl.grid_family(e) == grid]
            for fam in rl.TRACERS:
                qs = [q for q in range(qsize) if rl.tracer_family(q) == fam]
                if qs:
                    assert 1.0 - safe[es][:, qs].mean() <= CAP, (alg, qsize, grid, fam, 1.0 - safe[es][:, qs].mean())
    assert c80.kid_offsets(dp3d, dp2).max() > 15 and c80.kid_offsets(dp3d, dp2).min() >= -1
