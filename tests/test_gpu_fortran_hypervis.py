"""-m gpu: hypervis_view_hip, the Fortran seam's wrapper of tse_hypervis_view, called from Fortran.

oracle/_ref/dropin/hypervis_harness (tests/fortran_hypervis/hypervis_harness.F90) sets the mesh up with the reference's own routines, calls
cuda_mod_init and vector_setup_hip(elem), and then hypervis_view_hip on a device array of E3SM's shapes -- per element T(np,np,nlev,3),
dp3d(np,np,nlev,3) and v(np,np,2,nlev,3) behind one another with gaps; T and dp3d of time level 2 are one scalar view whose q stride is
the distance between the members -- once in place and once into dense out arrays, each with c_null_ptr as the stream and on a stream of
its own, and dumps what went in and the whole array as it came back.  Held: every dump equals HipMod.hypervis_view on the dumped input
and geometry in this process, bit for bit -- the marshalling of the wrapper: argument order, coef by reference, nu_ratio by value, the
optional out views -- the state differs from the input on the views' addresses alone, and with out views it keeps every bit."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dss_view_model as dm
import pyoracle as po
from test_gpu_fortran_views import read_views
from view_common import FakeArray as _Fake

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "dropin", "hypervis_harness")
MPIEXEC = "/opt/conda/bin/mpiexec"
QSIZE, NLEV = 4, 72
built = pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(MPIEXEC)), reason="Fortran hypervis harness not built")


@pytest.fixture(scope="module")
def run():
    out = tempfile.mkdtemp(prefix="tse_f90hypervis_")
    stdin = "2 %d\n'%s'\n'%s'\n" % (QSIZE, out, os.path.join(ROOT, "transport_se_amd", "data", "vcoord"))
    res = subprocess.run([MPIEXEC, "-n", "1", HARNESS], input=stdin.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    log = res.stdout.decode()
    assert log.strip().splitlines()[-1].strip().endswith("hypervis_harness done"), log[-3000:]
    return po.read_static(os.path.join(out, "static_000000_r0000.bin")), read_views(os.path.join(out, "hypervis_000000_r0000.bin"))


@built
def test_the_wrapper_s_output_is_hipmod_s(run):
    import torch
    from transport_se_amd.hip_mod import HipMod
    st, v = run
    elem = dict(Dinv=st["Dinv"], metdet=st["metdet"], rmetdet=st["rmetdet"], spheremp=st["spheremp"], rspheremp=st["rspheremp"],
                putmapP=st["putmap"].astype(np.int32), getmapP=st["getmap"].astype(np.int32), reverse=st["reverse"].astype(np.int32))
    h = HipMod(elem, st["Dvv"], (st["hyai"], st["hybi"], float(st["ps0"])), QSIZE, 1e19, device=0)
    try:
        h.vector_setup(st["D"], v["metinv"], st["mp"])
        ES, oT, oDP, oV = (int(x) for x in v["layout"])
        coef, nu = tuple(float(x) for x in v["coef_nu"][:3]), float(v["coef_nu"][3])
        state = v["in_state"]                                                    # (ES, e) read as [e][ES]
        E = state.shape[0]
        assert state.shape == (E, ES) and E == 24 and nu == 2.5 and len(set(coef)) == 3
        ss, sv = [ES, oDP - oT, 16, 4, 1], [ES, 16, 32, 4, 1]
        bs, bv = oT + 16 * NLEV, oV + 32 * NLEV                                  # time level 2 of each member
        touched = np.zeros(state.shape, dtype=bool)
        touched[:, dm.index(ss[1:], bs, (2, NLEV, 4, 4)).ravel()] = True
        touched[:, dm.index(sv[1:], bv, (2, NLEV, 4, 4)).ravel()] = True
        assert touched.sum() == E * 4 * NLEV * 16 and not (state[touched] == -7.25).any() and (state[:, oDP - 16:oDP] == -7.25).all()

        def views(buf):
            return (_Fake((E, 2, NLEV, 4, 4), ss, buf.data_ptr() + 8 * bs), _Fake((E, 2, NLEV, 4, 4), sv, buf.data_ptr() + 8 * bv))
        # in place
        buf = torch.from_numpy(state.copy()).cuda()
        a, b = views(buf)
        h.hypervis_view(a, "eqkji", b, "eqkji", coef=coef, nu_ratio=nu)
        mine = buf.cpu().numpy()
        assert not dm.same(mine, state) and dm.same(mine[~touched], state[~touched]) and (mine[touched] != state[touched]).mean() > 0.99
        # into out arrays: ten [e][f][k][j][i], vten [e][k][c][j][i]
        buf = torch.from_numpy(state.copy()).cuda()
        a, b = views(buf)
        ten = torch.full((E, 2, NLEV, 4, 4), -7.25, dtype=torch.float64, device="cuda")
        vten = torch.full((E, NLEV, 2, 4, 4), -7.25, dtype=torch.float64, device="cuda")
        h.hypervis_view(a, "eqkji", b, "eqkji", coef=coef, nu_ratio=nu, s_out=ten, v_out=vten, v_out_axes="ekqji")
        assert dm.same(buf.cpu().numpy(), state)
        ten, vten = ten.cpu().numpy(), vten.cpu().numpy()
        assert not (ten == -7.25).any() and not (vten == -7.25).any()
        # the tendencies are what the in-place call added: x + d with one addition
        new_T = mine[:, dm.index(ss[1:], bs, (2, NLEV, 4, 4))]
        assert dm.same(new_T, state[:, dm.index(ss[1:], bs, (2, NLEV, 4, 4))] + ten)
        for m in (0, 1):
            assert dm.same(v["state_s%d" % m], mine), m
            assert dm.same(v["kept_s%d" % m], state), m
            assert dm.same(v["ten_s%d" % m], ten) and dm.same(v["vten_s%d" % m], vten), m
        # the factors are not swapped: another order of coef gives other bits
        buf = torch.from_numpy(state.copy()).cuda()
        a, b = views(buf)
        h.hypervis_view(a, "eqkji", b, "eqkji", coef=(coef[1], coef[0], coef[2]), nu_ratio=nu)
        assert not dm.same(buf.cpu().numpy(), mine)
    finally:
        h.close()
