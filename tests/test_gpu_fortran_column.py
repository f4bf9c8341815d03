"""-m gpu: column_view_hip, the Fortran seam's wrapper of tse_column_view, called from Fortran.

oracle/_ref/dropin/column_harness (tests/fortran_column/column_harness.F90) sets the mesh up with the reference's own routines, calls
cuda_mod_init and then column_view_hip on device arrays of E3SM's shapes -- time level 2 of dp3d(np,np,nlev,3), T, vgrad_p and divdp of
the same shape, phis(np,np) -- for the four ops, phi and omega with the pressure formed on the fly and with the p of the pmid call, each
once with c_null_ptr as the stream and once on a stream of its own, and dumps what went in and what came back.  Held: every dump equals
HipMod.column_view on the dumped inputs in this process, bit for bit -- the marshalling of the wrapper: argument order, the absent
views, ptop and rgas by value, the view structs -- and equals the model."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import column_model as cm
import pyoracle as po
from test_gpu_fortran_views import read_views

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "dropin", "column_harness")
MPIEXEC = "/opt/conda/bin/mpiexec"
QSIZE, NLEV = 4, 72
built = pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(MPIEXEC)), reason="Fortran column harness not built")


@pytest.fixture(scope="module")
def run():
    out = tempfile.mkdtemp(prefix="tse_f90column_")
    stdin = "2 %d\n'%s'\n'%s'\n" % (QSIZE, out, os.path.join(ROOT, "transport_se_amd", "data", "vcoord"))
    res = subprocess.run([MPIEXEC, "-n", "1", HARNESS], input=stdin.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    log = res.stdout.decode()
    assert log.strip().splitlines()[-1].strip().endswith("column_harness done"), log[-3000:]
    return po.read_static(os.path.join(out, "static_000000_r0000.bin")), read_views(os.path.join(out, "column_000000_r0000.bin"))


@built
def test_the_wrapper_s_output_is_hipmod_s_and_the_model_s(run):
    import torch
    from transport_se_amd.hip_mod import HipMod
    st, v = run
    elem = dict(Dinv=st["Dinv"], metdet=st["metdet"], rmetdet=st["rmetdet"], spheremp=st["spheremp"], rspheremp=st["rspheremp"],
                putmapP=st["putmap"].astype(np.int32), getmapP=st["getmap"].astype(np.int32), reverse=st["reverse"].astype(np.int32))
    h = HipMod(elem, st["Dvv"], (st["hyai"], st["hybi"], float(st["ps0"])), QSIZE, 1e19, device=0)
    try:
        ptop, rgas = (float(x) for x in v["ptop_rgas"])
        assert ptop == float(st["hyai"][0]) * float(st["ps0"]) and ptop > 0 and rgas == 287.04
        dp, T, vg, div, phis = v["in_dp"], v["in_T"], v["in_vgrad_p"], v["in_divdp"], v["in_phis"]        # [e][k][j][i], [e][j][i]
        E = dp.shape[0]
        assert dp.shape == (E, NLEV, 4, 4) and phis.shape == (E, 4, 4) and float(dp.min()) > 0
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        d = dict(dp=dev(dp), T=dev(T), vg=dev(vg), div=dev(div), phis=dev(phis))
        col = lambda x: np.moveaxis(x, 1, 0)

        def mine(op, nk=NLEV, **kw):
            out = torch.full((E, nk, 4, 4), -7.25, dtype=torch.float64, device="cuda")
            h.column_view(op, out=out, ptop=ptop, rgas=rgas, **kw)
            return out.cpu().numpy()
        pm = cm.model("pmid", ptop, rgas, dp=col(dp))
        pd = dev(np.moveaxis(pm, 0, 1))
        cases = {
            "pint": (mine("pint", NLEV + 1, dp=d["dp"]), cm.model("pint", ptop, rgas, dp=col(dp))),
            "pmid": (mine("pmid", dp=d["dp"]), pm),
            "phi": (mine("phi", dp=d["dp"], a=d["T"], b=d["phis"]), cm.model("phi", ptop, rgas, dp=col(dp), a=col(T), b=phis)),
            "omega": (mine("omega", dp=d["dp"], a=d["vg"], b=d["div"]), cm.model("omega", ptop, rgas, dp=col(dp), a=col(vg), b=col(div))),
            "phi_p": (mine("phi", dp=d["dp"], p=pd, a=d["T"], b=d["phis"]), cm.model("phi", ptop, rgas, dp=col(dp), p=pm, a=col(T), b=phis)),
            "omega_p": (mine("omega", p=pd, a=d["vg"], b=d["div"]), cm.model("omega", ptop, rgas, p=pm, a=col(vg), b=col(div))),
        }
        assert {n[:-3] for n in v if n.endswith("_s0")} == set(cases) == {n[:-3] for n in v if n.endswith("_s1")}
        for name, (got_here, want) in cases.items():
            for m in (0, 1):
                got = v["%s_s%d" % (name, m)]                                 # (np,np,nk,e) read as [e][k][j][i]
                assert got.shape == got_here.shape, (name, got.shape, got_here.shape)
                assert cm.same(got, got_here), (name, m)
            assert cm.same(col(got_here), want), name
        # what distinguishes the calls: phi and omega from the given p are those from the p formed on the fly, and a and b are not swapped
        assert cm.same(v["phi_p_s0"], v["phi_s0"]) and cm.same(v["omega_p_s1"], v["omega_s1"])
        assert not cm.same(cases["omega"][1], cm.model("omega", ptop, rgas, dp=col(dp), a=col(div), b=col(vg)))
    finally:
        h.close()
