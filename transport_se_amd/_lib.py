"""Loader/builder of libtransport_se_hip.so (in-tree; built by __graft_entry__.build()).

The level count is a build-time setting of the library, as PLEV is of the reference: the default build (NLEV = 72) is
libtransport_se_hip.so, a build for another level count n is libtransport_se_hip_L<n>.so (build(nlev=n), lib(nlev=n)).  The
multiples of 8 from 16 to 72 and 80 compile (csrc/tse_kernels.h names the rules); NLEV_BUILDS are the ones built and tested beside the
default: 64 (the reference's 12k_top-64 grid) and 80 (one remap element per CU; nothing above 80 builds)."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libtransport_se_hip.so")
SRC = [os.path.join(HERE, "csrc", f) for f in ("tse_api.hip", "tse_stage3.hip", "tse_column.hip", "tse_views_api.hip", "tse_tables.cpp", "tse_views.cpp", "tse_kernels.h",
                                             "tse_view_kernels.h", "tse_device.h", "tse_ctx.h", "tse_launch.h", "tse_view_launch.h", "tse_layout.h", "tse_tables.h",
                                             "tse_views.h", "tse_remap_check.h")]
# the translation units in link order and the extra compiler flags of each.  The code objects of the library follow that order: the
# tracer path (tse_api.hip; tse_stage3.hip says why it has a scheduler strategy of its own), then the operators on a resident host's
# arrays (tse_column.hip says why k_column_view has a code object of its own; tse_views_api.hip, the other view kernels, comes last).
# tse_tables.cpp and tse_views.cpp are host C++, which hipcc would otherwise compile as HIP
UNITS = [("tse_api.hip", []), ("tse_stage3.hip", ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]), ("tse_column.hip", []), ("tse_views_api.hip", []),
         ("tse_tables.cpp", ["-x", "c++"]), ("tse_views.cpp", ["-x", "c++"])]
# -fno-honor-nans: value-preserving (no reassociation, no reciprocal tricks); it only lets the compiler drop the
# v_max_f64 x,x "canonicalize" it otherwise puts in front of every fmin/fmax operand (6 per limiter iteration)
CFLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-honor-nans", "-fPIC"]
HDR = os.path.join(os.path.dirname(HERE), "include", "transport_se_hip.h")

EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int)


class InitArgs(C.Structure):
    _fields_ = [
        ("nelemd", C.c_int), ("qsize", C.c_int), ("device", C.c_int), ("nu_q", C.c_double),
        ("limiter_option", C.c_int), ("rsplit", C.c_int),
        ("Dvv", C.c_void_p), ("hyai", C.c_void_p), ("hybi", C.c_void_p), ("ps0", C.c_double),
        ("Dinv", C.c_void_p), ("Dinv_stride", C.c_size_t), ("metdet", C.c_void_p), ("metdet_stride", C.c_size_t),
        ("rmetdet", C.c_void_p), ("rmetdet_stride", C.c_size_t), ("spheremp", C.c_void_p), ("spheremp_stride", C.c_size_t),
        ("rspheremp", C.c_void_p), ("rspheremp_stride", C.c_size_t),
        ("putmapP", C.c_void_p), ("getmapP", C.c_void_p), ("reverse", C.c_void_p),
        ("nsend", C.c_int), ("send_peer", C.c_void_p), ("send_ptrP", C.c_void_p), ("send_lengthP", C.c_void_p),
        ("nrecv", C.c_int), ("recv_peer", C.c_void_p), ("recv_ptrP", C.c_void_p), ("recv_lengthP", C.c_void_p),
        ("exchange", EXCHANGE_FN), ("exchange_user", C.c_void_p),
        ("vert_remap_q_alg", C.c_int),
    ]


class View(C.Structure):
    """tse_view: a strided device view (strides in doubles: element, q, level, j, i)"""
    _fields_ = [("ptr", C.c_void_p), ("stride", C.c_longlong * 5)]


HOOKS_SO = os.path.join(HERE, "libtransport_se_hip_hooks.so")
HOOKS_FLAGS = ["-DTSE_AB_HOOKS"]
DEFAULT_NLEV = 72   # the level count of the default build (csrc/tse_layout.h; TSE_NLEV of the header)
NLEV_BUILDS = (64, 80)   # the other level counts __graft_entry__.build() ships


def so_path(nlev=None):
    """the product library built for `nlev` levels (None: the default build)"""
    if nlev is None or nlev == DEFAULT_NLEV:
        return SO
    return os.path.join(HERE, "libtransport_se_hip_L%d.so" % int(nlev))


def _compile_units(tmp, tag, flags, verbose):
    """start the compiler on every translation unit (they run side by side); returns (objs, [(cmd, Popen)])"""
    objs, procs = [], []
    for name, extra in UNITS:
        obj = os.path.join(tmp, tag + os.path.splitext(name)[0] + ".o")
        cmd = ["hipcc"] + CFLAGS + extra + list(flags) + ["-c", "-o", obj, os.path.join(HERE, "csrc", name)]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd))); objs.append(obj)
    return objs, procs


def _finish(procs):
    """wait for EVERY compile before raising (a compiler left running would write into the temporary directory being removed)"""
    failed = None
    for cmd, p in procs:
        if p.wait() and failed is None:
            failed = subprocess.CalledProcessError(p.returncode, cmd)
    if failed:
        raise failed


def _link(out, objs, verbose):
    cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs + \
          ["-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,/opt/rocm/lib"]   # RCCL: the in-library bndry_exchangeV (tse_comm_init)
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)


def _stale(so):
    newest = max(os.path.getmtime(p) for p in SRC + [HDR])
    return not (os.path.exists(so) and os.path.getmtime(so) >= newest)


def build(force=False, verbose=False, out=None, flags=(), hooks=True, nlev=None):
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU).  Builds the product library and, with hooks=True, its twin with
    -DTSE_AB_HOOKS (libtransport_se_hip_hooks.so: the A/B switches and the fault injection the tests use -- none of which the
    product library contains); all translation units compile side by side.
    nlev: the product library for another level count instead (-DNLEV=<nlev>, so_path(nlev); no hooks twin).  The kernels'
    static_asserts refuse a level count they cannot serve at compile time.
    out/flags: one A/B variant of the same sources instead (tools/ab_build.sh; always with the hooks)."""
    import tempfile
    if nlev is not None and nlev != DEFAULT_NLEV:
        so = so_path(nlev)
        if force or _stale(so):
            with tempfile.TemporaryDirectory() as tmp:
                objs, procs = _compile_units(tmp, "L%d_" % nlev, ["-DNLEV=%d" % nlev], verbose)
                _finish(procs)
                _link(so, objs, verbose)
        return so
    if out is not None:
        with tempfile.TemporaryDirectory() as tmp:
            objs, procs = _compile_units(tmp, "ab_", HOOKS_FLAGS + list(flags), verbose)
            _finish(procs)
            _link(out, objs, verbose)
        return out
    todo = [(so, fl) for so, fl in ((SO, []), (HOOKS_SO, HOOKS_FLAGS)) if (so == SO or hooks) and (force or _stale(so))]
    if not todo:
        return SO
    with tempfile.TemporaryDirectory() as tmp:
        started = [(so,) + _compile_units(tmp, "h_" if fl else "p_", fl, verbose) for so, fl in todo]
        _finish([pr for _, _, procs in started for pr in procs])
        for so, objs, _ in started:
            _link(so, objs, verbose)
    return SO


def source_hash():
    """identifies the kernel sources a committed measurement (profiles/*pmc_traffic*, *l2_dcmip11*) was taken with"""
    import hashlib
    h = hashlib.sha256()
    for f in SRC:
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


_libs = {}

# every symbol include/transport_se_hip.h declares
SYMBOLS = ["tse_init", "tse_finalize", "tse_last_error", "tse_nlev", "tse_synchronize", "tse_copy_qdp_h2d", "tse_copy_qdp_d2h",
           "tse_set_derived", "tse_set_divdp", "tse_get_derived", "tse_advec_tracers_remap_rk2", "tse_compute_divdp", "tse_euler_step",
           "tse_qdp_time_avg", "tse_vertical_remap", "tse_get_qminmax", "tse_dcmip_init", "tse_dcmip_set_initial",
           "tse_dcmip_step_inputs", "tse_prim_run_subcycle", "tse_device_ptr", "tse_kernel_time", "tse_timing", "tse_comm_timing",
           "tse_halo_layout", "tse_halo_minmax_layout", "tse_comm_unique_id", "tse_comm_init", "tse_comm_precheck", "tse_comm_version", "tse_comm_info", "tse_comm_abort",
           "tse_boundary_layout", "tse_patch_layout", "tse_placement", "tse_invalidate_cache", "tse_divergence_sphere", "tse_laplace_sphere_wk", "tse_remap_q_ppm", "tse_host_register", "tse_element_mass", "tse_element_qdiag",
           "tse_state_q", "tse_copy_q_d2h", "tse_copy_lnps_d2h", "tse_norm_setup", "tse_norm_reference", "tse_norm_partials", "tse_mix_partials",
           "tse_view_put", "tse_view_get", "tse_view_plan", "tse_apply_forcing", "tse_apply_forcing_host",
           "tse_remap_view", "tse_remap_view_status", "tse_remap_view_plan", "tse_dss_view", "tse_dss_view_plan",
           "tse_biharmonic_view", "tse_biharmonic_view_plan", "tse_vector_setup", "tse_vlaplace_view", "tse_vlaplace_view_plan",
           "tse_hypervis_view", "tse_hypervis_view_plan",
           "tse_sphere_op_view", "tse_sphere_op_view_plan", "tse_stats_view", "tse_stats_view_plan",
           "tse_column_view", "tse_column_view_plan"]
COMM_ID_BYTES = 128


def lib(path=None, nlev=None):
    """Load the HIP library; raises (never falls back) if it has not been built.  path (or TSE_LIB): another build of the SAME
    sources -- the -DTSE_AB_HOOKS twin (HOOKS_SO: fault injection for the tests, A/B switches) or a tools/ab variant -- never a fallback.
    nlev: the library must be built for this level count (checked with tse_nlev()); a level count other than the default's loads
    so_path(nlev) unless a path is given (TSE_LIB names a default-level build and is not used for it)."""
    if nlev is not None and nlev != DEFAULT_NLEV:
        path = path or so_path(nlev)
    else:
        path = path or os.environ.get("TSE_LIB", SO)
    if path in _libs:
        L = _libs[path]
        _check_nlev(L, path, nlev)
        return L
    if not os.path.exists(path):
        raise RuntimeError("%s is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the product path)" % os.path.basename(path))
    # One HIP runtime and one RCCL per process.  PyTorch (the control plane of the multi-rank driver, and what the benchmark
    # contract synchronises with) loads the ROCm libraries bundled in its wheel by absolute path; a libamdhip64 / librccl that is
    # already in the process under the same SONAME does not stop it, so "library first, torch later" ends with TWO runtimes
    # (device pointers of one unknown to the other: hipErrorNoDevice on the first copy).  The other order is safe: this
    # library's DT_NEEDED entries (libamdhip64.so.7, librccl.so.1) resolve to the copies torch has loaded.  So torch goes first
    # whenever it is installed; tse_comm_version() reports which RCCL that is (bench.py prints it).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, i, d, sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
    L.tse_init.argtypes = [C.POINTER(vp), C.POINTER(InitArgs)]
    L.tse_finalize.argtypes = [vp]; L.tse_finalize.restype = None
    L.tse_last_error.restype = C.c_char_p
    L.tse_nlev.argtypes = []
    L.tse_synchronize.argtypes = [vp]
    L.tse_copy_qdp_h2d.argtypes = [vp, vp, sz, i, i]
    L.tse_copy_qdp_d2h.argtypes = [vp, vp, sz, i, i]
    L.tse_set_derived.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, sz]
    L.tse_set_divdp.argtypes = [vp, vp, sz, vp, sz]
    L.tse_get_derived.argtypes = [vp] + [vp, sz] * 6
    L.tse_advec_tracers_remap_rk2.argtypes = [vp, d, i, i]
    L.tse_compute_divdp.argtypes = [vp]
    L.tse_euler_step.argtypes = [vp, i, i, d, i, i]
    L.tse_qdp_time_avg.argtypes = [vp, i, i, i]
    L.tse_vertical_remap.argtypes = [vp, d, i]
    L.tse_get_qminmax.argtypes = [vp, vp, vp]
    L.tse_dcmip_init.argtypes = [vp, i, vp, vp, vp, vp]
    L.tse_dcmip_set_initial.argtypes = [vp]
    L.tse_dcmip_step_inputs.argtypes = [vp, i, d]
    L.tse_prim_run_subcycle.argtypes = [vp, d, i, C.POINTER(i)]
    L.tse_device_ptr.argtypes = [vp, C.c_char_p, C.POINTER(sz)]; L.tse_device_ptr.restype = vp
    L.tse_kernel_time.argtypes = [vp, C.c_char_p, C.POINTER(d), C.POINTER(C.c_long)]
    L.tse_timing.argtypes = [vp, i]
    L.tse_comm_timing.argtypes = [vp, i]
    L.tse_halo_layout.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    L.tse_halo_minmax_layout.argtypes = [vp, vp, vp]
    L.tse_comm_unique_id.argtypes = [vp]
    L.tse_comm_init.argtypes = [vp, vp, i, i]
    L.tse_comm_precheck.argtypes = [vp, i, i]
    L.tse_comm_version.argtypes = [C.POINTER(i), C.POINTER(i), C.c_char_p, sz]
    L.tse_comm_info.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    L.tse_comm_abort.argtypes = [vp]
    L.tse_boundary_layout.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    L.tse_patch_layout.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    L.tse_placement.argtypes = [vp, C.POINTER(i), C.POINTER(d), C.POINTER(i)]
    L.tse_invalidate_cache.argtypes = [vp]
    L.tse_divergence_sphere.argtypes = [vp, vp, vp]
    L.tse_laplace_sphere_wk.argtypes = [vp, vp, vp]
    L.tse_remap_q_ppm.argtypes = [vp, vp, vp, vp]
    L.tse_host_register.argtypes = [vp, vp, sz]
    L.tse_element_mass.argtypes = [vp, i, vp]
    L.tse_element_qdiag.argtypes = [vp, i, vp, vp, vp, vp]
    L.tse_state_q.argtypes = [vp, i]
    L.tse_copy_q_d2h.argtypes = [vp, vp, sz, i]
    L.tse_copy_lnps_d2h.argtypes = [vp, vp, sz]
    L.tse_norm_setup.argtypes = [vp, vp, vp, vp]
    L.tse_norm_reference.argtypes = [vp, i, i, vp]
    L.tse_norm_partials.argtypes = [vp, i, i, d, vp]
    L.tse_mix_partials.argtypes = [vp, i, i, i, d, d, d, d, vp, i, vp]
    L.tse_view_put.argtypes = [vp, C.c_char_p, i, C.POINTER(View), vp]
    L.tse_view_get.argtypes = [vp, C.c_char_p, i, C.POINTER(View), vp]
    L.tse_view_plan.argtypes = [C.c_char_p, i, i, C.POINTER(View), i, C.POINTER(i), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.tse_apply_forcing.argtypes = [vp, i, d, i, C.POINTER(View), vp, vp]
    L.tse_apply_forcing_host.argtypes = [vp, i, d, i, vp, sz, i, vp]
    L.tse_remap_view.argtypes = [vp, i, i, i, C.POINTER(View), C.POINTER(View), C.POINTER(View), vp]
    L.tse_remap_view_status.argtypes = [vp, C.POINTER(i), C.POINTER(i * 4)]
    L.tse_remap_view_plan.argtypes = [i, i, C.POINTER(View), C.POINTER(View), C.POINTER(View), C.POINTER(i * 3), C.POINTER(C.c_longlong * 3), C.POINTER(C.c_longlong * 3)]
    L.tse_dss_view.argtypes = [vp, i, i, i, C.POINTER(View), vp]
    L.tse_dss_view_plan.argtypes = [i, i, i, C.POINTER(View), C.POINTER(i), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.tse_biharmonic_view.argtypes = [vp, i, i, i, C.POINTER(View), C.POINTER(View), vp]
    L.tse_biharmonic_view_plan.argtypes = [i, i, i, C.POINTER(View), C.POINTER(View), C.POINTER(i * 2), C.POINTER(C.c_longlong * 2), C.POINTER(C.c_longlong * 2)]
    L.tse_vector_setup.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t]
    L.tse_vlaplace_view.argtypes = [vp, i, i, d, C.POINTER(View), C.POINTER(View), vp]
    L.tse_vlaplace_view_plan.argtypes = [i, i, C.POINTER(View), C.POINTER(View), C.POINTER(i * 2), C.POINTER(C.c_longlong * 2), C.POINTER(C.c_longlong * 2)]
    L.tse_hypervis_view.argtypes = [vp, i, i, vp, d] + [C.POINTER(View)] * 4 + [vp]
    L.tse_hypervis_view_plan.argtypes = [i, i, i] + [C.POINTER(View)] * 4 + [C.POINTER(i * 4), C.POINTER(C.c_longlong * 4), C.POINTER(C.c_longlong * 4)]
    L.tse_sphere_op_view.argtypes = [vp, i, i, i, C.POINTER(View), C.POINTER(View), vp]
    L.tse_sphere_op_view_plan.argtypes = [i, i, i, C.POINTER(View), C.POINTER(View), C.POINTER(i * 2), C.POINTER(C.c_longlong * 2), C.POINTER(C.c_longlong * 2)]
    L.tse_stats_view.argtypes = [vp, i, i, i, C.POINTER(View), C.POINTER(View), C.POINTER(View), vp, vp]
    L.tse_stats_view_plan.argtypes = [i, i, i, C.POINTER(View), C.POINTER(View), C.POINTER(View), C.POINTER(i * 3), C.POINTER(C.c_longlong * 3), C.POINTER(C.c_longlong * 3)]
    L.tse_column_view.argtypes = [vp, i, d, d] + [C.POINTER(View)] * 5 + [vp]
    L.tse_column_view_plan.argtypes = [i, i] + [C.POINTER(View)] * 5 + [C.POINTER(i * 5), C.POINTER(C.c_longlong * 5), C.POINTER(C.c_longlong * 5)]
    if hasattr(L, "tse_test_dcmip_point"):   # the -DTSE_AB_HOOKS twin only (HipMod.test_dcmip_point)
        L.tse_test_dcmip_point.argtypes = [vp, i, d, vp, vp]
    _libs[path] = L
    _check_nlev(L, path, nlev)
    return L


def _check_nlev(L, path, nlev):
    if nlev is not None and L.tse_nlev() != nlev:
        raise RuntimeError("%s is built for nlev = %d, not %d" % (os.path.basename(path), L.tse_nlev(), nlev))
