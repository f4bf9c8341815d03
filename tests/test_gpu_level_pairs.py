"""-m gpu: the level-pair data movement of the DSS-on-read kernels.

In the patch kernels two lanes share a row's loads and stores: each loads points {0,2} or {1,3} of the row for BOTH levels of a pair,
publishes the 16-byte pieces in the block's LDS image and reads its own four values back out of the image behind the barrier
(gather_publish / gather_own); on the way out the pair exchanges halves with bank-masked DPP row shifts (store_row_pair).  What such
code can get wrong is a value that lands at the partner level, at point i +- 1, or that comes from the other (stale) LDS buffer.

So: one tse_advec_tracers_remap_rk2 from a Qdp in which every (element, tracer, level, point) holds a value of its own, at ne = 2 and
ne = 3 (patches with holes, cube corners) and qsize 1, 2, 5 (tracer 0 alone, both roles of a tracer pair, an odd tail), must leave the
bits of the same call with TSE_DSS_ON_READ=0 -- one DSS pass per stage, whose slab kernels are the plain ones (flat blocks, no LDS
image).  On the 72-level library and on the 64- and 80-level ones (a child process each: one library per process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
CASES = [(ne, qsize) for ne in (2, 3) for qsize in (1, 2, 5)]
PARAMS = {2: (1e19, 1800.0), 3: (2e18, 900.0)}   # ne -> (nu_q, dt): hyperviscosity on, so that stage 3 assembles both of its images


def _distinct_q(qsize, n, nlev):
    """mixing ratios in [0.5, 1.5), no two alike"""
    size = qsize * n * nlev * 16
    return (0.5 + np.arange(size, dtype=np.float64) / size).reshape(qsize, n, nlev, 4, 4)


def _both_routes(nlev, ne, qsize):
    """-> Qdp(np1) of one whole tracer step with DSS on read and with one DSS pass per stage, and the Qdp both started from"""
    import vcoord_levels as vl
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.hip_mod import HipMod
    from transport_se_amd.hybvcoord import HvCoord
    nu, dt = PARAMS[ne]
    hv = HvCoord() if nlev == 72 else HvCoord(*vl.paths(nlev))
    topo = cm.topology(ne); geo = cm.geometry(ne, topo)
    d = cm.edge_descriptors(topo)   # one rank: every element, in mesh order
    n = 6 * ne * ne
    elem = dict(Dinv=geo["Dinv"], metdet=geo["metdet"], rmetdet=geo["rmetdet"], spheremp=geo["spheremp"], rspheremp=geo["rspheremp"],
                putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
    h = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), qsize, nu, device=0, schedule=dict(send=d["send"], recv=d["recv"]))
    assert h.nlev == nlev and h.L.tse_nlev() == nlev
    out = {}
    old = os.environ.pop("TSE_DSS_ON_READ", None)
    try:
        for route in ("1", "0"):
            os.environ["TSE_DSS_ON_READ"] = route
            h.dcmip_init(1, geo["lat"], geo["lon"], hv.hyam, hv.hybm); h.dcmip_set_initial(); h.dcmip_step_inputs(0, dt)
            qdp = np.moveaxis(_distinct_q(qsize, n, nlev) * h.fetch("dp", (n, nlev, 4, 4))[None], 0, 1)
            elem["Qdp"] = np.ascontiguousarray(np.stack([qdp, qdp], axis=1))
            h.copy_qdp_h2d(elem, 1); h.copy_qdp_h2d(elem, 2)
            h.advec_tracers_remap_rk2(dt, 1, 2)
            out[route] = h.fetch("qdp", (2, n, qsize, nlev, 4, 4))[1].copy()
        out["in"] = qdp
    finally:
        os.environ.pop("TSE_DSS_ON_READ", None)
        if old is not None:
            os.environ["TSE_DSS_ON_READ"] = old
        h.close()
    return out


def _assert_same_bits(res, nlev, ne, qsize):
    a, b, start = res["1"], res["0"], res["in"]
    assert np.unique(start).size == start.size, "the initial values are not distinct"
    assert a.shape == (6 * ne * ne, qsize, nlev, 4, 4) and np.isfinite(a).all() and not np.array_equal(a, start)
    same = a.view(np.uint64) == b.view(np.uint64)
    if not same.all():
        e, q, k, j, i = (int(x) for x in np.argwhere(~same)[0])
        raise AssertionError("%d levels, ne%d, qsize %d: %d of %d values differ from the per-stage route; first at element %d tracer %d "
                             "level %d point (%d, %d): %r against %r, max difference %.3e"
                             % (nlev, ne, qsize, int((~same).sum()), same.size, e, q, k, j, i, a[e, q, k, j, i], b[e, q, k, j, i],
                                float(np.abs(a - b).max())))


@pytest.mark.parametrize("ne,qsize", CASES)
def test_whole_step_leaves_the_bits_of_the_per_stage_route(ne, qsize):
    _assert_same_bits(_both_routes(72, ne, qsize), 72, ne, qsize)


# ---------------------------------------------------------------------------------------------------------------------------
# the 64- and 80-level libraries: one library per process, every case in one child
def _worker(spec):
    out = {}
    for ne, qsize in CASES:
        for key, x in _both_routes(spec["nlev"], ne, qsize).items():
            out["%d/%d/%s" % (ne, qsize, key)] = x
    np.savez(spec["out"], **out)


def _child_env():
    env = dict(os.environ)
    for k in ("TSE_REMAP_FUSED", "TSE_BOUNDARY_STRIPS", "TSE_DSS_ON_READ", "TSE_LIB", "WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")])
    return env


@pytest.mark.parametrize("nlev", [64, 80])
def test_other_level_counts(tmp_path, nlev):
    from transport_se_amd import _lib
    assert nlev in _lib.NLEV_BUILDS
    path = str(tmp_path / "r.npz")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(dict(nlev=nlev, out=path))], env=_child_env(),
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert res.returncode == 0, res.stdout.decode()[-4000:]
    got = dict(np.load(path))
    for ne, qsize in CASES:
        _assert_same_bits({key: got["%d/%d/%s" % (ne, qsize, key)] for key in ("1", "0", "in")}, nlev, ne, qsize)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    _worker(json.loads(sys.argv[2]))
