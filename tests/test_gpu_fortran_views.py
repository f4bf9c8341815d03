"""-m gpu: every view wrapper of the Fortran seam, called from Fortran.

oracle/_ref/dropin/views_harness (tests/fortran_resident/views_harness.F90) sets the mesh up with the reference's own routines, calls
cuda_mod_init and vector_setup_hip(elem), and then calls view_put_hip, view_get_hip, apply_forcing_hip, apply_forcing_elem_hip,
remap_view_hip, remap_view_status_hip, dss_view_hip, biharmonic_view_hip, vlaplace_view_hip, sphere_op_view_hip, norm_setup_hip,
norm_reference_hip, norm_partials_hip and mix_partials_hip on device arrays of E3SM's shapes (time level 2 of v(np,np,2,nlev,3),
T(np,np,nlev,3), Qdp(np,np,nlev,qsize_d,2), ps(np,np,3); one level-fastest array), every operator once with c_null_ptr as the stream and
once on a stream of its own, and dumps what went in and what came back.  What is held:
 * its geometry is ref_ne2_static.npz's and the fixture's metinv, bit for bit (the same code on the same mesh);
 * its operator inputs are tests/golden/ref_ne2_fieldops.npz's, bit for bit (the same fill module);
 * every call's output has the bits of the same call made through HipMod in this process on the dumped inputs and geometry -- the
   marshalling of each wrapper: argument order, by value or by reference, the view struct, the shifts q-1 / qa-1 / qb-1, the tl of
   derived%FQ, Fortran's memory order of D, metinv and mp;
 * the operator outputs lie within 2 * bound(N, A) of the reference's own Fortran (test_gpu_reference_fieldops.py's bound);
 * the two forcing routes agree with each other and with forcing_model.apply, bit for bit;
 * remap: the bits of HipMod.remap_view, remap_ld's pointwise bound, no refusal for good grids, and one bad element reported by
   remap_view_status_hip (counted from 0) and left with every bit;
 * the norm and mixing partials and sum0 equal norm_model / mixing_model on the dumped Q, bit for bit (q = 2, qa = 1, qb = 2: an
   off-by-one in a shift picks another tracer);
 * on two ranks (two processes on one GPU, the staged exchange through tse_f_exchange) every output, gathered by GlobalId, has the bits
   of the one-rank run."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dss_view_model as dm
import fieldops_ref as fr
import pyoracle as po

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "dropin", "views_harness")
MPIEXEC = "/opt/conda/bin/mpiexec"
QSIZE, NLEV = 4, 72
TAU = np.linspace(0.1, 1.0, 19)
MIX = (0.0, 1.0, 0.9, -0.8)            # xmin, xmax, c0, c2
built = pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(MPIEXEC)), reason="Fortran views harness not built")
# harness record -> case of fieldops_ref.cases (the harness calls vlaplace_view_hip with nu_ratio 2.5: the fixture's second ratio)
OPS = dict(dss_average="dss_average", dss_weak="dss_weak", lap="lap", bih="bih", vlap="vlap_nu1", vbih="vbih_nu1", grad="grad", div="div",
           vor="vor", grad_c0="grad_c0", div_c0="div_c0", vor_c0="vor_c0")
COLLECTIVE = ("dss_average", "dss_weak", "bih", "vbih", "grad_c0", "div_c0", "vor_c0")


def read_views(path):
    """views_000000_r<rank>.bin -> name -> array in C order (Fortran's a(i,j,k) is [k][j][i])"""
    raw = open(path, "rb").read()
    out, o = {}, 0
    while o < len(raw):
        name = raw[o:o + 24].decode().strip(); o += 24
        nd = int(np.frombuffer(raw, "<i4", 1, o)[0]); o += 4
        dims = np.frombuffer(raw, "<i4", nd, o); o += 4 * nd
        n = int(np.prod(dims))
        out[name] = np.frombuffer(raw, "<f8", n, o).reshape(tuple(int(d) for d in dims[::-1])).copy(); o += 8 * n
    return out


def _weights(st):
    from transport_se_amd import diagnostics as dg
    return dg.column_weights(2, st["lat"], st["lon"], dg.level_heights(st["hyam"], st["hybm"]))


def _run(st, nranks):
    out = tempfile.mkdtemp(prefix="tse_f90views_")
    owner, colw, dh = _weights(st)
    with open(os.path.join(out, "weights.bin"), "wb") as f:
        f.write(np.array([owner.shape[0], TAU.size], "<i4").tobytes())
        f.write(np.ascontiguousarray(owner, "<i4").tobytes()); f.write(np.ascontiguousarray(colw, "<f8").tobytes())
        f.write(np.ascontiguousarray(dh, "<f8").tobytes()); f.write(TAU.astype("<f8").tobytes()); f.write(np.array(MIX, "<f8").tobytes())
    stdin = "2 %d\n'%s'\n'%s'\n" % (QSIZE, out, os.path.join(ROOT, "transport_se_amd", "data", "vcoord"))
    res = subprocess.run([MPIEXEC, "-n", str(nranks), HARNESS], input=stdin.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    log = res.stdout.decode()
    assert log.strip().splitlines()[-1].strip().endswith("views_harness done"), log[-3000:]
    return ([po.read_static(os.path.join(out, "static_000000_r%04d.bin" % r)) for r in range(nranks)],
            [read_views(os.path.join(out, "views_000000_r%04d.bin" % r)) for r in range(nranks)])


@pytest.fixture(scope="module")
def gold_pair(gold):
    st, fx = gold("ref_ne2_static.npz"), gold("ref_ne2_fieldops.npz")
    return {k: st[k] for k in st.files}, {k: fx[k] for k in fx.files}


@pytest.fixture(scope="module")
def one(gold_pair):
    sts, vs = _run(gold_pair[0], 1)
    return sts[0], vs[0]


def _scalar(x):
    """s(np,np,nk,e) as dumped -> [e][1][nk][4][4]"""
    return np.ascontiguousarray(x[:, None])


def _vector(x):
    """v(np,np,2,nk,e) as dumped -> [e][2][nk][4][4]"""
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3, 4))


def _field(v, name):
    x = v[name]
    return _scalar(x) if x.ndim == 4 else _vector(x)


def _levfast(x):
    """lf(nlev,np,np,q,e) or lf(nlev,np,np,e) as dumped -> [e][q][k][j][i] or [e][k][j][i]"""
    return np.ascontiguousarray(np.moveaxis(x, -1, -3))


@pytest.fixture(scope="module")
def hip(one):
    from transport_se_amd.hip_mod import HipMod
    st, v = one
    elem = dict(Dinv=st["Dinv"], metdet=st["metdet"], rmetdet=st["rmetdet"], spheremp=st["spheremp"], rspheremp=st["rspheremp"],
                putmapP=st["putmap"].astype(np.int32), getmapP=st["getmap"].astype(np.int32), reverse=st["reverse"].astype(np.int32))
    h = HipMod(elem, st["Dvv"], (st["hyai"], st["hybi"], float(st["ps0"])), QSIZE, 1e19, device=0)
    h.vector_setup(st["D"], v["metinv"], st["mp"])
    yield h
    h.close()


@built
def test_geometry_and_inputs_are_the_fixtures(one, gold_pair):
    st, v = one
    gst, fx = gold_pair
    for k in ("gid", "putmap", "getmap", "reverse", "Dvv", "hyai", "hybi") + fr.GEOMETRY:
        assert np.array_equal(st[k], gst[k]) and (st[k].dtype != np.float64 or dm.same(st[k], gst[k])), k
    assert dm.same(v["metinv"], fx["metinv"]) and np.array_equal(v["gid"], fx["gid"])
    assert dm.same(_field(v, "in_s"), fx["s"]) and dm.same(_field(v, "in_v"), fx["v"])


@built
@pytest.mark.parametrize("name", sorted(OPS))
def test_operator_wrapper(one, hip, gold_pair, name):
    """the wrapper's output == HipMod's on the same inputs, bit for bit, with and without a stream; and within the bound of the reference"""
    from test_gpu_reference_fieldops import _device, _hold
    st, v = one
    gst, fx = gold_pair
    cases = fr.cases(fx)
    c = cases[OPS[name]]
    f = _field(v, "in_s" if c.src in ("s", "dss_average") else "in_v")
    assert c.src != "dss_average"
    want = _device(hip, c.call, f, fx[c.out].shape[1], "dense")
    for m in (0, 1):
        got = _field(v, "%s_s%d" % (name, m))
        assert dm.same(got, want), (name, m, float(np.abs(got - want).max()))
    o = fr.mesh(gst)
    try:
        _, A = c.ld(o, (gst["D"], fx["metinv"], gst["mp"]), fx[c.src], None)
    finally:
        o.close()
    _hold("fortran " + name, "state layout", _field(v, name + "_s0"), fx[c.out], A, c.N)


@built
def test_put_and_get(one):
    st, v = one
    assert dm.same(_levfast(v["get_qdp"]), v["put_qdp"])
    assert dm.same(_levfast(v["get_omega_p"]), v["put_omega_p"])
    assert dm.same(v["get_ps_v"], v["state_ps_v"]) and float(v["state_ps_v"].min()) > 9.0e4


@built
def test_forcing_routes(one):
    import forcing_model as fm
    st, v = one
    a, b = _levfast(v["forcing_elem"]), _levfast(v["forcing_view"])
    res = fm.apply(v["put_qdp"], v["fq"], float(v["forcing_dt"][0]), 0)
    assert (res["branch"] != fm.NOCLIP).any() and (res["branch"] == fm.NOCLIP).any()      # the clip is exercised
    assert dm.same(a, b) and dm.same(a, res["new"])


@built
def test_remap(one, hip):
    import torch
    import remap_ld as rl
    from test_gpu_remap_pointwise import _check
    st, v = one
    Q, dp1, dp2 = v["put_qdp"], v["dp_src"], v["dp_tgt"]
    assert v["remap_good"].tolist() == [0.0, 0.0, 0.0]          # neither good call refused, nothing for the status call to report

    def lib(field, mode):
        t, a, b = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (field, dp1, dp2))
        assert hip.remap_view(t, "eqkji", a, "ekji", b, "ekji", mode=mode, alg=0) == 0
        return t.cpu().numpy()
    assert dm.same(v["remap_mass"], lib(Q, "mass"))
    T = v["put_omega_p"][:, None]
    assert dm.same(v["remap_mean"][:, None], lib(T, "mean"))
    assert dm.same(v["remap_mean"][:, None], lib(T * dp1[:, None], "mass") / dp2[:, None])
    t, safe, kid = rl.remap_q_ppm(Q, dp1, dp2, 0)
    worst = {}
    _check("fortran remap_view_hip", Q.shape[1], v["remap_mass"], Q, t, safe, kid, worst)
    refused, nref, e, col, lev, code, ebad = v["remap_bad_status"].tolist()
    assert (refused, nref, e, code) == (0.0, 1.0, ebad, 1.0) and (col, lev) == (2 * 4 + 1, 4.0), v["remap_bad_status"]
    keep = np.arange(Q.shape[0]) != int(ebad)
    assert dm.same(v["remap_bad"][int(ebad)], Q[int(ebad)]) and dm.same(v["remap_bad"][keep], v["remap_mass"][keep])


@built
def test_norm_and_mixing_partials(one, gold_pair):
    import mixing_model as mm
    import norm_model as nm
    st, v = one
    owner, colw, dh = _weights(gold_pair[0])
    Q = v["state_q"]
    assert not dm.same(Q[:, 0], Q[:, 1]) and not dm.same(Q[:, 1], Q[:, 2])
    dp = (np.diff(st["hyai"]) * st["ps0"])[None, :, None, None] + np.diff(st["hybi"])[None, :, None, None] * v["state_ps_v"][:, None]
    assert dm.same(Q, v["state_qdp"] / dp[:, None])
    q0 = Q[:, 1]                                               # norm_reference_hip(nt = 1, q = 2)
    assert dm.same(v["sum0"], nm.element_sum0(q0, owner))
    avg = float(v["avg"][0])
    # avg is the harness's own input to norm_partials_hip: its sum of the 24 positive shares in Fortran's order, one division
    exact = math.fsum(v["sum0"]) / (NLEV * int(owner.sum()))
    assert abs(avg - exact) <= (owner.shape[0] + 1) * 2.0 ** -53 * exact, (avg, exact)
    assert dm.same(v["norm_partials"], nm.element_partials(q0, q0, owner, colw, dh, avg))
    assert dm.same(v["mix_partials"], mm.element_partials(Q[:, 0], Q[:, 1], owner, colw, dh, *MIX, TAU))   # qa = 1, qb = 2


@built
def test_two_ranks_give_the_bits_of_one(one, gold_pair):
    """two processes on one GPU, the exchange staged through tse_f_exchange: every output of the harness, gathered by GlobalId"""
    st1, v1 = one
    sts, vs = _run(gold_pair[0], 2)
    gid = np.concatenate([s["gid"] for s in sts]) - 1
    assert np.array_equal(np.sort(gid), np.arange(24)) and all(s["send_cycles"].shape[0] > 0 for s in sts)
    for name in sorted(v1):
        if name in ("avg", "norm_partials", "forcing_dt", "remap_good", "remap_bad_status", "remap_bad", "put_qdp", "get_qdp", "put_omega_p", "get_omega_p", "fq",
                    "forcing_elem", "forcing_view", "dp_src", "dp_tgt", "remap_mass", "remap_mean"):
            continue      # scalars, and the fields each rank fills from a seed of its own
        cat = np.concatenate([v[name] for v in vs])
        full = np.empty_like(cat); full[gid] = cat
        assert dm.same(full, v1[name]), name
    # avg is a sum over the ranks in another order than one rank's, and norm_partials_hip depends on it: held to the model with this run's avg
    import norm_model as nm
    owner, colw, dh = _weights(gold_pair[0])
    avg = float(vs[0]["avg"][0])
    assert avg == float(vs[1]["avg"][0]) and abs(avg - float(v1["avg"][0])) <= 2.0 ** -51 * avg
    cat = np.concatenate([v["norm_partials"] for v in vs])
    full = np.empty_like(cat); full[gid] = cat
    assert dm.same(full, nm.element_partials(v1["state_q"][:, 1], v1["state_q"][:, 1], owner, colw, dh, avg))
    for v in vs:
        assert v["remap_good"].tolist() == [0.0, 0.0, 0.0] and v["remap_bad_status"][:3].tolist() == [0.0, 1.0, 1.0]
        assert dm.same(_levfast(v["forcing_elem"]), _levfast(v["forcing_view"]))
    assert set(n[:-3] for n in v1 if n.endswith("_s0")) >= set(COLLECTIVE)
