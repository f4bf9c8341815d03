"""Reference model of the tracer step WITHOUT a limiter (limiter_option = 0; plain numpy over the checker's exported pieces).

The checker (oracle/) applies limiter 8 unconditionally.  This model composes its element operators (Oracle.divergence_sphere,
Oracle.laplace_sphere_wk), its DSS (Oracle.dss) and its state arrays in the reference's operand order for euler_step
(prim_advection_mod.F90:750-960) and leaves out only the limiter line (:880-895 apply limiter_optim_iter_full only under
limiter_option == 8).  `limiter` puts a limiter back per slab; the CPU tests use it with pyoracle.limiter8 to show that the model
differs from the checker's euler_step in nothing else.  The remap is the checker's own vertical_remap on the model's state.

Every function works in place on the Oracle's arrays (o.qdp, o.divdp, o.divdp_proj, o.eta_dot_dpdn, o.omega_p), as the checker does.
"""
import numpy as np

NLEV = 72


def _levels(o, dt, rhs):
    """dp of the stage (:755,847) [e][k][j][i]"""
    return o.dp - (rhs * dt) * o.divdp_proj


def _biharmonic(o, Q, dt):
    """rhs_multiplier 2 (:796-826, viscosity_mod.F90:353-442): -rhs_viss*dt*nu_q*dp0*biharmonic_wk(Q)/spheremp, Q[e][q][k][j][i]"""
    n, qs = o.nelem, o.qsize
    lap = np.empty_like(Q)
    for e in range(n):
        for q in range(qs):
            for k in range(NLEV):
                lap[e, q, k] = o.laplace_sphere_wk(e, Q[e, q, k])
    lap = o.dss(lap.reshape(n, qs * NLEV, 4, 4), 0).reshape(Q.shape)
    out = np.empty_like(Q)
    hyai, hybi = np.asarray(o.hyai), np.asarray(o.hybi)
    ps0 = 1.0e5
    for e in range(n):
        rsp, sp = o.rspheremp[e], o.spheremp[e]
        for q in range(qs):
            for k in range(NLEV):
                lap2 = o.laplace_sphere_wk(e, rsp * lap[e, q, k])
                dp0 = (hyai[k + 1] - hyai[k]) * ps0 + (hybi[k + 1] - hybi[k]) * ps0
                out[e, q, k] = ((((-3.0 * dt) * o.nu_q) * dp0) * lap2) / sp
    return out


def euler_step(o, np1_qdp, n0_qdp, dt, dssopt, rhs_multiplier, limiter=None):
    """euler_step (prim_advection_mod.F90:667-970) on o's state.  dssopt: 1 eta_dot_dpdn, 2 omega_p, 3 divdp_proj.
    limiter: None (limiter_option = 0), or an object with bounds(Q, rhs_multiplier) -- called with Q = Qdp(n0)/dp before the
    advance -- and apply(e, q, k, Qtens, dp_star) -> Qtens, called per slab where the reference calls limiter_optim_iter_full."""
    n, qs = o.nelem, o.qsize
    Qn0 = o.qdp[n0_qdp - 1].copy()
    dpk = _levels(o, dt, rhs_multiplier)
    Q = Qn0 / dpk[:, None]
    if limiter is not None:
        limiter.bounds(Q, rhs_multiplier)
    qb = _biharmonic(o, Q, dt) if rhs_multiplier == 2 else None
    var = {1: o.eta_dot_dpdn, 2: o.omega_p, 3: o.divdp_proj}[dssopt]
    vs1, vs2 = o.vn0[:, :, 0] / dpk, o.vn0[:, :, 1] / dpk
    dp_star = dpk - dt * o.divdp if limiter is not None else None
    out = np.empty_like(Qn0)
    for e in range(n):
        sp = o.spheremp[e]
        for q in range(qs):
            for k in range(NLEV):
                qn0 = Qn0[e, q, k]
                gradQ = np.stack([vs1[e, k] * qn0, vs2[e, k] * qn0])
                qt = o.divergence_sphere(e, gradQ)
                qt = qn0 - dt * qt
                if qb is not None:
                    qt = qt + qb[e, q, k]
                if limiter is not None:
                    qt = limiter.apply(e, q, k, qt, dp_star[e, k])
                out[e, q, k] = sp * qt
    var[:, :NLEV] = o.spheremp[:, None] * var[:, :NLEV]
    out = o.dss(out.reshape(n, qs * NLEV, 4, 4), 0).reshape(out.shape)
    v = o.dss(np.ascontiguousarray(var[:, :NLEV]), 0)
    var[:, :NLEV] = v * o.rspheremp[:, None]
    o.qdp[np1_qdp - 1] = o.rspheremp[:, None, None] * out


def qdp_levels(nstep):
    """(n0_qdp, np1_qdp) of time_mod (qsplit = 1)"""
    return (1, 2) if nstep % 2 == 0 else (2, 1)


def advec_tracers_remap_rk2(o, dt, nstep, limiter=None):
    """Prim_Advec_Tracers_remap_rk2 + qdp_time_avg (prim_advection_mod.F90:579-662) without a limiter"""
    n0, np1 = qdp_levels(nstep)
    for e in range(o.nelem):
        for k in range(NLEV):
            d = o.divergence_sphere(e, o.vn0[e, k])
            o.divdp[e, k] = d
            o.divdp_proj[e, k] = d
    euler_step(o, np1, n0, dt / 2, 3, 0, limiter)
    euler_step(o, np1, np1, dt / 2, 1, 1, limiter)
    euler_step(o, np1, np1, dt / 2, 2, 2, limiter)
    o.qdp[np1 - 1] = (o.qdp[n0 - 1] + 2.0 * o.qdp[np1 - 1]) / 3.0


def prim_run(o, test, tstep, nsub, nstep=0):
    """prim_run_subcycle as the checker's prim_run, without a limiter: rsplit tracer steps, then the checker's vertical_remap.
    Returns (tracer steps done, next nstep); a negative layer thickness raises."""
    done = 0
    for _ in range(nsub):
        np1 = 2
        for _ in range(o.rsplit):
            o.dcmip_step_inputs(test, nstep, tstep)
            advec_tracers_remap_rk2(o, tstep, nstep)
            _, np1 = qdp_levels(nstep)
            nstep += 1
            done += 1
        if o.vertical_remap(tstep * o.rsplit, np1):
            raise RuntimeError("negative layer thickness")
    return done, nstep
