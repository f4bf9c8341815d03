"""-m gpu: the device-resident route of the Fortran seam, driven from Fortran.

oracle/_ref/dropin/resident_harness (tests/fortran_resident/) sets the mesh up with the reference's own routines and then calls only
cuda_mod_hip.F90's resident entries: dcmip_init_hip, prim_run_subcycle_hip (one rsplit cycle per call, twice) and copy_state_d2h_hip
(Qdp, dp3d, ps_v, Q and lnps from the device).  The state it dumps must be the plain-Fortran reference's
(tests/golden/ref_ne2_dcmip11.npz) to the drop-in harness's bounds, and its Q must be Qdp/dp of its own dumped fields bit for bit."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pyoracle as po
from conftest import record_margin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "dropin", "resident_harness")
MPIEXEC = "/opt/conda/bin/mpiexec"
TOL = 1e-13   # dp3d and ps_v: the drop-in harness's bound (tests/test_gpu_fortran_dropin.py: TOL_DROPIN)
# Qdp: unlike the drop-in harness, whose host evaluates the prescribed winds with the reference's own code, the resident route evaluates
# them on the device (device libm); the suite holds that loop to 10 * TOL_STEP = 5e-12 of this golden after 6 steps
# (test_gpu_parity.py::test_device_dcmip_fields_and_prim_run), and Q formed from it measured 0.97e-13 / 1.42e-13 after 3 / 6 steps
TOL_QDP = 1e-12


def read_q(path):
    """q_<nstep>_r<rank>.bin of the resident harness: Q[ie][q][k][j][i], lnps[ie][j][i], and hyai, hybi, ps0"""
    raw = open(path, "rb").read()
    istep, nelemd, qsize = np.frombuffer(raw, dtype=np.int32, count=3)
    f = np.frombuffer(raw, dtype=np.float64, offset=12)
    hyai, hybi, ps0 = f[:73], f[73:146], f[146]
    per = f[147:].reshape(nelemd, qsize * 72 * 16 + 16)
    return dict(istep=int(istep), Q=per[:, :-16].reshape(nelemd, qsize, 72, 4, 4), lnps=per[:, -16:].reshape(nelemd, 4, 4),
                hyai=hyai, hybi=hybi, ps0=ps0)


@pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(MPIEXEC)), reason="Fortran resident harness not built")
def test_resident_route_from_fortran(gold):
    g = gold("ref_ne2_dcmip11.npz")
    cfg = json.loads(str(g["config"]))
    out = tempfile.mkdtemp(prefix="tse_f90res_")
    stdin = "%d %d %d %r %r %d 1\n'%s'\n'%s'\n" % (cfg["ne"], cfg["qsize"], cfg["nsteps"], cfg["tstep"], cfg["nu_q"], cfg["test"],
                                                 out, os.path.join(ROOT, "transport_se_amd", "data", "vcoord"))
    res = subprocess.run([MPIEXEC, "-n", "1", HARNESS], input=stdin.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    log = res.stdout.decode()
    assert "resident_harness done" in log, log[-3000:]
    assert "hip resident: tracer-DOF-steps/s" in log, log[-3000:]
    for tag, key in (("000003", "qdp_step3"), ("000006", "qdp_step6")):
        st = po.read_state(os.path.join(out, "state_%s_r0000.bin" % tag))
        assert st["istep"] == int(tag)
        err = np.abs(st["qdp"] - g[key]).max() / np.abs(g[key]).max()
        record_margin("fortran_resident %s" % key, err, TOL_QDP)
        assert err < TOL_QDP, (tag, err)
        q = read_q(os.path.join(out, "q_%s_r0000.bin" % tag))
        da = np.diff(q["hyai"])[None, :, None, None]; db = np.diff(q["hybi"])[None, :, None, None]
        dp = (da * q["ps0"]) + (db * st["ps_v"][:, None, :, :])
        assert np.array_equal(q["Q"].view(np.uint64), (st["qdp"] / dp[:, None]).view(np.uint64)), tag
        ref = np.log(st["ps_v"])
        assert (np.abs(q["lnps"] - ref) <= np.spacing(ref)).all(), tag
    s3 = po.read_state(os.path.join(out, "state_000003_r0000.bin"))
    assert np.abs(s3["dp3d"] - g["dp3d_step3"]).max() / np.abs(g["dp3d_step3"]).max() < TOL
    assert np.abs(s3["ps_v"] - g["ps_v_step3"]).max() / 1e5 < TOL
