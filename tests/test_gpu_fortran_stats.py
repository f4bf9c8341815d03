"""-m gpu: stats_view_hip, the Fortran seam's wrapper of tse_stats_view, called from Fortran.

oracle/_ref/dropin/stats_harness (tests/fortran_stats/stats_harness.F90) sets the mesh up with the reference's own routines, calls
cuda_mod_init and then stats_view_hip on device arrays of E3SM's shapes -- time level 2 of v(np,np,2,nlev,3), T(np,np,nlev,3) with a
'true solution' and a weight of the same shape, ps(np,np,3), and one level-fastest array -- each call once with c_null_ptr as the stream and
once on a stream of its own, with and without ref and weight, for element shares and level shares, and dumps what went in and what
came back.  Held: every dump equals HipMod.stats_view on the dumped inputs and geometry in this process, bit for bit -- the marshalling
of the wrapper: argument order, a null ref / weight, per_level, the view structs, and the shape of out in Fortran's memory order
(out(16, [nk,] nf, nelemd) is [e][f]([k])[16]) -- and equals the model."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pyoracle as po
import stats_model as sm
from test_gpu_fortran_views import read_views

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "dropin", "stats_harness")
MPIEXEC = "/opt/conda/bin/mpiexec"
QSIZE, NLEV = 4, 72
built = pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(MPIEXEC)), reason="Fortran stats harness not built")


@pytest.fixture(scope="module")
def run():
    out = tempfile.mkdtemp(prefix="tse_f90stats_")
    stdin = "2 %d\n'%s'\n'%s'\n" % (QSIZE, out, os.path.join(ROOT, "transport_se_amd", "data", "vcoord"))
    res = subprocess.run([MPIEXEC, "-n", "1", HARNESS], input=stdin.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    log = res.stdout.decode()
    assert log.strip().splitlines()[-1].strip().endswith("stats_harness done"), log[-3000:]
    return po.read_static(os.path.join(out, "static_000000_r0000.bin")), read_views(os.path.join(out, "stats_000000_r0000.bin"))


@built
def test_the_wrapper_s_output_is_hipmod_s_and_the_model_s(run):
    import torch
    from transport_se_amd.hip_mod import HipMod
    st, v = run
    elem = dict(Dinv=st["Dinv"], metdet=st["metdet"], rmetdet=st["rmetdet"], spheremp=st["spheremp"], rspheremp=st["rspheremp"],
                putmapP=st["putmap"].astype(np.int32), getmapP=st["getmap"].astype(np.int32), reverse=st["reverse"].astype(np.int32))
    h = HipMod(elem, st["Dvv"], (st["hyai"], st["hybi"], float(st["ps0"])), QSIZE, 1e19, device=0)
    try:
        sp = st["spheremp"]
        V = np.ascontiguousarray(v["in_v"].transpose(0, 2, 1, 3, 4))          # v(np,np,2,nlev,e) -> [e][2][k][j][i]
        T, Tt, dp, ps = v["in_T"][:, None], v["in_Tt"][:, None], v["in_dp"], v["in_ps"][:, None, None]
        LF = np.ascontiguousarray(np.moveaxis(v["in_lf"], -1, -3))            # lf(nlev,np,np,2,e) -> [e][2][k][j][i]
        assert V.shape == (24, 2, NLEV, 4, 4) and LF.shape == V.shape and ps.shape == (24, 1, 1, 4, 4) and float(np.abs(V).max()) <= 20.0
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        dV, dT, dTt, dDP, dPS = dev(V), dev(T), dev(Tt), dev(dp), dev(ps)
        dLF = dev(v["in_lf"])                                                 # as the harness holds it: [e][q][j][i][k]
        cases = {
            "v": (lambda: h.stats_view(dV, "eqkji"), sm.model(V, sp)),
            "v_w_lev": (lambda: h.stats_view(dV, "eqkji", weight=dDP, per_level=True), sm.model(V, sp, None, dp, per_level=True)),
            "T_ref": (lambda: h.stats_view(dT, "eqkji", ref=dTt), sm.model(T, sp, Tt)),
            "T_ref_w_lev": (lambda: h.stats_view(dT, "eqkji", ref=dTt, weight=dDP, per_level=True), sm.model(T, sp, Tt, dp, per_level=True)),
            "ps": (lambda: h.stats_view(dPS, "eqkji"), sm.model(ps, sp)),
            "lf_w": (lambda: h.stats_view(dLF, "eqjik", weight=dDP, weight_axes="ekji"), sm.model(LF, sp, None, dp)),
            "lf_self_lev": (lambda: h.stats_view(dLF, "eqjik", ref=dLF, per_level=True), sm.model(LF, sp, LF, per_level=True)),
        }
        assert {n[:-3] for n in v if n.endswith("_s0")} == set(cases) == {n[:-3] for n in v if n.endswith("_s1")}
        for name, (call, want) in cases.items():
            mine = call()
            for m in (0, 1):
                got = v["%s_s%d" % (name, m)]                                 # out(16, [nk,] nf, e) read as [e][nf]([nk])[16]
                assert got.shape == mine.shape, (name, got.shape, mine.shape)
                assert sm.same(got, mine), (name, m)
            assert sm.same(mine, want), name
        # what distinguishes the calls: a weight that is dropped or a ref that is taken for the weight would show
        assert not v["v_s0"][..., 8:14].any() and v["T_ref_s0"][..., 8:14].all() and not v["lf_self_lev_s0"][..., 8].any()
        assert not sm.same(v["T_ref_w_lev_s0"][..., 14], sm.model(T, sp, per_level=True)[..., 14])
    finally:
        h.close()
