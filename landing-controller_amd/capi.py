"""ctypes binding of the C ABI (include/landing_nlp.h) of liblanding_mi355x.so.

The library is the product: HIP kernels for gfx950 behind plain-C entry points.  This module fails
loudly (ImportError / RuntimeError) when the library is missing or no GPU is usable -- there is no
CPU fallback.  ``load(path)`` lets the CPU test-suite bind the host-emulated build of the same
sources (tests/emu) for logic tests; product code never passes a path.

A new entry point is added to the header, to SIGNATURES below and to a wrapper; tests/test_binding_signatures_cpu.py
fails until the first two agree.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "liblanding_mi355x.so"
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_llp = C.POINTER(C.c_longlong)


class LandingForm(C.Structure):
    _fields_ = [("kin_box", C.c_double * 3), ("kin_z_off", C.c_double), ("comp_eps", C.c_double), ("slip_eps", C.c_double),
                ("run_cost", C.c_int), ("QX", C.c_double * 12), ("Qc", C.c_double * 3), ("Qf", C.c_double * 3),
                ("f_ref", C.c_double * 3), ("p_hip", C.c_double * 12)]


class SolverOpts(C.Structure):
    _fields_ = [("tol", C.c_double), ("max_iter", C.c_int), ("mu_init", C.c_double), ("bound_push", C.c_double),
                ("bound_frac", C.c_double), ("kappa_eps", C.c_double), ("kappa_mu", C.c_double), ("theta_mu", C.c_double),
                ("max_soc", C.c_int), ("max_resets", C.c_int), ("reset_du", C.c_double), ("stage_local_reg", C.c_int), ("sticky_delta", C.c_int), ("restart_period", C.c_int), ("dispatch_order", C.c_int),
                ("delta_init", C.c_double), ("delta_inc_first", C.c_double), ("delta_inc", C.c_double), ("delta_dec", C.c_double),
                ("tau_min", C.c_double), ("alpha_fallback", C.c_double), ("reset_delta", C.c_double), ("clip_k", C.c_int), ("clip_until", C.c_double), ("theta_floor", C.c_double), ("fresh_restart", C.c_int), ("dual_step_cap", C.c_double), ("slack_corr", C.c_double), ("watchdog", C.c_int), ("barrier_smax", C.c_double), ("factor_fp32", C.c_int),
                ("feas_phase", C.c_int), ("feas_rho", C.c_double), ("feas_cert", C.c_double), ("delta_floor", C.c_double), ("jam_clip", C.c_int), ("stag_relief", C.c_int), ("feas_jam", C.c_int), ("feas_stat", C.c_int),
                ("kd_clone_after", C.c_int), ("kd_clone_max", C.c_int), ("kd_clone_iter", C.c_int),
                ("feas_back", C.c_double), ("feas_max", C.c_int), ("feas_delta_dec", C.c_double), ("feas_ret_push", C.c_double), ("feas_ret_mu", C.c_double), ("feas_resume", C.c_int), ("feas_polish", C.c_double)]


class KinodynForm(C.Structure):
    """landing_kinodyn_form of include/landing_nlp.h: the literals of the kinodynamic NLP's constraint set"""
    _fields_ = [("comp_eps", C.c_double), ("slip_eps", C.c_double), ("fk_band", C.c_double), ("kin_box_x0", C.c_double), ("kin_box_y0", C.c_double),
                ("kin_box_y_in", C.c_double), ("kin_box_z_lo", C.c_double), ("kin_box_z_hi", C.c_double), ("tau_max", C.c_double * 3)]


class PipelineOpts(C.Structure):
    """landing_pipeline_opts of include/landing_nlp.h (the drop-state chain): options of the SRBM solve, the refinement and the warm re-solve, the
    refinement's constraint literals, joint limits and joint-angle guess; warm = 0 stops after the refinement"""
    _fields_ = [("srbm", SolverOpts), ("refine", SolverOpts), ("resolve", SolverOpts), ("form", KinodynForm),
                ("jpos_min", C.c_double * 12), ("jpos_max", C.c_double * 12), ("jpos_guess", C.c_double * 3), ("warm", C.c_int)]


class ActuatorModel(C.Structure):
    """landing_actuator_model of include/landing_nlp.h: gear ratios, torque constants, winding resistances and joint torque limits (abad / hip / knee), battery voltage"""
    _fields_ = [("gr", C.c_double * 3), ("kt", C.c_double * 3), ("Rm", C.c_double * 3), ("tau_max", C.c_double * 3), ("battery_v", C.c_double)]


class ActuatorScreen(C.Structure):
    """landing_actuator_screen of include/landing_nlp.h: the limits a member has to hold to be kept (a limit <= 0 is not screened); drive_only = 1 holds
    volt_max against the samples with tau * jvel > 0 only"""
    _fields_ = [("volt_max", C.c_double), ("tau_ratio_max", C.c_double), ("jvel_max", C.c_double), ("drive_only", C.c_int)]


AUDIT_NSUM = 8      # LANDING_AUDIT_NSUM
AUDIT_SUMMARY = ("tau_ratio", "jvel", "volt", "volt_drive", "power_max", "power_min", "n_over", "n_over_drive")      # d_summary's columns


ARGS21 = ["Xref", "Uref", "dt", "q_min", "q_max", "qd_min", "qd_max", "q_init", "qd_init", "q_term_min", "q_term_max",
          "qd_term_min", "qd_term_max", "QN", "x0", "mu", "l_leg_max", "f_max", "mass", "Ib", "Ib_inv"]


ARGS25 = ["Xref", "Uref", "dt", "q_min", "q_max", "qd_min", "qd_max", "q_init", "qd_init", "c_init", "q_term_min", "q_term_max",
          "qd_term_min", "qd_term_max", "QX", "QN", "Qc", "Qf", "x0", "mu", "l_leg_max", "f_max", "mass", "Ib", "Ib_inv"]


class Args25(C.Structure):
    """landing_args25: the 25 solver-function arguments of the reference's N=41 script (analysis/eval_SRBM_CCC.m:72-78), host pointers"""
    _fields_ = [(n, _dp) for n in ARGS25]


class Args21(C.Structure):
    """landing_args21: the reference's 21 solver-function arguments (generate_landingCtrller_IPOPT.m:323-327), host pointers"""
    _fields_ = [(n, _dp) for n in ARGS21]


class RbdModel(C.Structure):
    """landing_rbd_model of include/landing_nlp.h (rbd.quad3d_model fills one)"""
    _fields_ = [("parent", C.c_int * 18), ("jtype", C.c_int * 18), ("E", (C.c_double * 9) * 18), ("r", (C.c_double * 3) * 18),
                ("m", C.c_double * 18), ("h", (C.c_double * 3) * 18), ("I", (C.c_double * 6) * 18),
                ("b_foot", C.c_int * 4), ("foot_r", (C.c_double * 3) * 4), ("l1", C.c_double), ("l2", C.c_double), ("l3", C.c_double), ("l4", C.c_double)]


class KinodynParams(C.Structure):
    """landing_kinodyn_params of include/landing_nlp.h"""
    _fields_ = [("dt", C.c_double * 64), ("mass", C.c_double), ("Ib", C.c_double * 3), ("Ib_inv", C.c_double * 3), ("mu", C.c_double)]


# Entry point -> (restype, argtypes), for every function include/landing_nlp.h declares; load() applies it.  c_void_p: contexts, device addresses
# and streams (a Python integer passes through whole); typed pointers: host arrays and structs.
_vp, _ci, _cd, _ll, _ullp = C.c_void_p, C.c_int, C.c_double, C.c_longlong, C.POINTER(C.c_ulonglong)
_form, _so, _kf, _kp, _po = C.POINTER(LandingForm), C.POINTER(SolverOpts), C.POINTER(KinodynForm), C.POINTER(KinodynParams), C.POINTER(PipelineOpts)
_am, _sc = C.POINTER(ActuatorModel), C.POINTER(ActuatorScreen)
_out5, _out6 = [_dp, _dp, _ip, _ip, _dp], [_dp, _dp, _dp, _ip, _ip, _dp]      # x f [lam_g] status iters kkt, host
_gains = [_cd, _ci, _dp, _cd, _dp, _dp, _dp, _ci]                              # dt_r n Ib3x3 mass Q r_diag F rk4
_chain = _out6 + [_dp, _dp, _ip]                                               # ... pair_in pair_out n_kept
SIGNATURES = {
    # formulation, sizes, patterns, context
    "landing_form_default": (None, [_form]),
    "landing_solver_opts_default": (None, [_so]),
    "landing_solver_opts_warm": (None, [_so]),
    "landing_pattern_jac": (_ci, [_ci, _llp, _llp]),
    "landing_pattern_hess": (_ci, [_ci, _llp, _llp]),
    "landing_pattern_hess_rc": (_ci, [_ci, _llp, _llp]),
    "landing_ctx_np": (_ll, [_vp]),
    "landing_create": (_vp, [_ci, _ci, _form]),
    "landing_destroy": (None, [_vp]),
    "landing_last_error": (C.c_char_p, []),
    "landing_device_count": (_ci, []),
    "landing_kernel_name_sweep": (C.c_char_p, []),
    # function layer and solver of the SRBM NLP
    "landing_eval_batch": (_ci, [_vp, _ci] + [_vp] * 11 + [_vp]),
    "landing_eval_batch_host": (_ci, [_vp, _ci] + [_dp] * 11),
    "landing_eval_hess_rc_batch": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp]),
    "landing_eval_hess_rc_batch_host": (_ci, [_vp, _ci, _dp, _dp, _dp, _dp, _dp]),
    "landing_bounds_batch": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp]),
    "landing_solve_batch": (_ci, [_vp, _ci, _vp, _vp, _so] + [_vp] * 6 + [_vp]),
    "landing_solve_batch_host": (_ci, [_vp, _ci, _dp, _dp, _so] + _out6),
    "landing_pack_args21": (_ci, [_ci, _ci, C.POINTER(Args21), _dp]),
    "landing_solve_args21": (_ci, [_vp, _ci, C.POINTER(Args21), _so] + _out5),
    "landing_solve_21": (_ci, [_vp, _ci] + [_dp] * 21 + [_so] + _out5),
    "landing_pack_args25": (_ci, [_ci, _ci, C.POINTER(Args25), _dp]),
    "landing_solve_args25": (_ci, [_vp, _ci, C.POINTER(Args25), _so] + _out6),
    "landing_mpc_shift": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp, _vp]),
    # several devices from the C boundary
    "landing_multi_create": (_vp, [_ci, _ip, _ci, _form]),
    "landing_multi_destroy": (None, [_vp]),
    "landing_multi_count": (_ci, [_vp]),
    "landing_shard_range": (None, [_ci, _ci, _ci, _ip, _ip]),
    "landing_multi_solve_args21": (_ci, [_vp, _ci, C.POINTER(Args21), _so] + _out6),
    "landing_solve_21_multi": (_ci, [_ip, _ci, _ci, _ci] + [_dp] * 21 + [_so] + _out6),
    "landing_multi_release_cached": (None, []),
    # streaming
    "landing_stream_create": (_vp, [_vp, _ci]),
    "landing_stream_destroy": (None, [_vp]),
    "landing_stream_lanes": (_ci, [_vp]),
    "landing_stream_submit": (_ll, [_vp, _ci, _vp, _vp, _so] + [_vp] * 6 + [_vp]),
    "landing_stream_wait": (_ci, [_vp, _ll, _vp]),
    "landing_stream_sync": (_ci, [_vp, _vp]),
    "landing_solve_stream_host": (_ci, [_vp, _ci, _ci, _ci, _dp, _dp, _so] + _out6),
    # tracking _gains
    "landing_riccati_gains_batch": (_ci, [_vp, _ci, _ci, _vp, _vp, _dp, _cd, _dp, _dp, _dp, _cd, _ci, _vp, _vp, _vp, _vp, _vp]),
    "landing_sample_reference_batch": (_ci, [_vp, _ci, _vp, _vp, _cd, _ci, _vp, _vp, _vp]),
    "landing_tracking_gains_batch": (_ci, [_vp, _ci, _vp, _vp, _vp] + _gains + [_vp] * 6 + [_vp]),
    "landing_tracking_gains_host": (_ci, [_vp, _ci, _dp, _dp, _ip] + _gains + [_dp] * 6),
    # rigid-body routines and the kinodynamic refinement NLP
    "landing_rbd_set_model": (_ci, [_vp, C.POINTER(RbdModel)]),
    "landing_rbd_model_mc3d": (None, [C.POINTER(RbdModel)]),
    "landing_fb_dynamics_batch": (_ci, [_vp, _ci] + [_vp] * 9 + [_cd, _vp]),
    "landing_leg_ik_batch": (_ci, [_vp, _ci, _vp, _vp, _dp, _dp, _ci, _vp, _vp, _vp]),
    "landing_kinodyn_rows_batch": (_ci, [_vp, _ci] + [_vp] * 7 + [_vp]),
    "landing_kinodyn_nlp_dims": (_ci, [_ci, _llp, _llp]),
    "landing_kinodyn_nlp_eval": (_ci, [_vp, _ci, _ci, _vp, _kp, _vp, _vp, _vp]),
    "landing_kinodyn_nlp_hess": (_ci, [_vp, _ci, _ci, _vp, _kp, _vp, _vp, _vp]),
    "landing_kinodyn_form_default": (None, [_kf]),
    "landing_kinodyn_form_knitro": (None, [_kf]),
    "landing_kinodyn_solver_opts_default": (None, [_so]),
    "landing_kinodyn_solver_opts_warm": (None, [_so]),
    "landing_kinodyn_bounds": (_ci, [_ci, _ci, _vp] + [_dp] * 14),
    "landing_kinodyn_solve_batch": (_ci, [_vp, _ci, _ci, _kp] + [_vp] * 4 + [_vp] + [_vp] * 6 + [_vp]),
    "landing_kinodyn_solve_batch_host": (_ci, [_vp, _ci, _ci, _kp, _dp, _dp, _dp, _dp, _vp] + _out6),
    "landing_solve_kinodyn_24": (_ci, [_vp, _ci, _ci, _vp] + [_dp] * 24 + [_vp] + _out6),
    "landing_solve_kinodyn_24_on": (_ci, [_ci, _ci, _ci] + [_dp] * 24 + [_so] + _out6),
    "landing_solve_kinodyn_24_on_form": (_ci, [_ci, _ci, _ci, _kf] + [_dp] * 24 + [_so] + _out6),
    "landing_kinodyn_pattern": (_ci, [_vp, _ci, _ci, _llp, _llp, _llp]),
    "landing_kinodyn_block_nonzeros": (_ci, [_vp, _ip, _ip, C.POINTER(C.c_ubyte)]),
    "landing_kinodyn_casadi_offsets": (_ci, [_ci, _llp]),
    "landing_kinodyn_casadi_bounds": (_ci, [_ci, _vp, _dp, _dp, _dp]),
    "landing_kinodyn_casadi_pattern": (_ci, [_vp, _ci, _ci, C.POINTER(_llp), C.POINTER(_llp), _llp]),
    "landing_kinodyn_casadi_eval_host": (_ci, [_vp, _ci, _dp, _dp, _dp, _dp] + [_dp] * 7),
    "landing_kinodyn_casadi_release": (None, [_vp]),
    # the drop-state _chain and the actuator audit behind it
    "landing_pipeline_opts_default": (None, [_po]),
    "landing_pipeline_final_status": (_ci, [_ci, _ci]),
    "landing_kinodyn_pose_batch": (_ci, [_vp, _ci, _vp, _vp, _po] + [_vp] * 4 + [_vp]),
    "landing_training_pairs_batch": (_ci, [_vp, _ci] + [_vp] * 7 + [_vp]),
    "landing_pipeline_refine_batch": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp, _po] + [_vp] * 10 + [_vp]),
    "landing_pipeline_batch": (_ci, [_vp, _ci, _vp, _vp, _po, _vp] + [_vp] * 10 + [_vp]),
    "landing_pipeline_21": (_ci, [_vp, _ci] + [_dp] * 21 + [_po] + _chain),
    "landing_pipeline_21_on": (_ci, [_ci, _ci, _ci] + [_dp] * 21 + [_po] + _chain),
    "landing_actuator_model_mc3d": (None, [_am]),
    "landing_actuator_screen_default": (None, [_sc]),
    "landing_actuator_audit_batch": (_ci, [_vp, _ci, _vp, _ci, _vp, _am, _sc] + [_vp] * 6 + [_vp]),
    "landing_actuator_audit_host": (_ci, [_vp, _ci, _dp, _ci, _dp, _am, _sc, _dp, _dp, _dp, _dp, _ip, _ip]),
    "landing_pipeline_screened_pairs_batch": (_ci, [_vp, _ci, _vp, _vp, _vp, _am, _sc] + [_vp] * 7 + [_vp]),
    # whole-body SQP
    "landing_wb_backward": (_ci, [_vp, _ci, _ci, _cd, _cd, _vp, _vp, _vp, _vp, _vp, _dp, _dp, _dp, _vp, _vp, _vp, _vp, _vp]),
    "landing_wb_rollout": (_ci, [_vp, _ci, _ci, _ci, _vp, _cd, _vp, _vp, _vp, _vp, _vp, _vp, _dp, _dp, _dp, _vp, _vp, _vp, _vp]),
    "landing_wb_set_integrator": (_ci, [_vp, _ci]),
    "landing_wb_skip_taken": (_ci, [_vp, _vp]),
    "landing_wb_select": (_ci, [_vp, _ci, _ci, _ci] + [_vp] * 10),
    # diagnostics
    "landing_set_profile_buffer": (_ci, [_vp, _vp]),
    "landing_debug_iter_cap": (_ci, [_vp, _ci]),
    "landing_debug_workspace": (_ci, [_vp, C.POINTER(_vp), _ullp]),
    "landing_debug_solver_tables": (_ci, [_vp, _ci, _vp, _ullp]),
    "landing_debug_kd_workspace": (_ci, [_vp, C.POINTER(_vp), _ullp, _ip, _ip]),
    "landing_debug_kd_layout": (_ci, [_ci, _ullp, _ullp, _ullp]),
    "landing_debug_kd_state": (_ci, [_vp, _ci, _dp]),
}
SIGNATURES.update({n: (_ll, [_ci]) for n in ("landing_nx", "landing_ng", "landing_np", "landing_np_ccc", "landing_nnz_jac", "landing_nnz_hess", "landing_nnz_hess_rc",
                                             "landing_sweep_bytes_per_member", "landing_kinodyn_casadi_np")})
# what only the host-emulation build of the same sources exports (tests/emu); bound where present
EMU_HOOKS = {"landing_emu_set_fused": (None, [_ci]), "landing_emu_accept_counts": (_ci, [_ci, _ip]),
             "landing_emu_el_row": (None, [_cd] * 8 + [_dp]),
             "hip_emu_live_blocks": (_ll, []), "hip_emu_fail_alloc": (_ll, [_ll])}


# Sizes the solver kernel's workspace layout is built from (csrc/solver_kernels.hip: RUNC, RIC_STRIDE, RCG, EXIT_REC)
WS_RUNC, WS_RIC_STRIDE, WS_RCG, WS_EXIT_REC = 48, 1200, 36, 8
# ("live" holds live + 2 feas: bit 0 = which instance of the row arrays holds the iterate, bit 1 = the solve ended inside the feasibility phase)
EXIT_RECORD = ("mu", "delta", "alpha", "a_du", "live", "it", "omt", "s_corr")


def workspace_offsets(N, nx=None, ng=None, nnz_jac=None, nnz_hess=None):
    """The layout of one member's block of the solver workspace (landing_debug_workspace): dict name -> (offset, length) in doubles, in the
    order of carve() in csrc/solver_kernels.hip, plus "total" -> the member stride.  x / xt, g / gt and the row arrays with a second instance
    (s, zL, zU, y, sig, rho) swap roles when a first trial point is accepted: "rec" (EXIT_RECORD) says which instance is live at exit."""
    nx = 36 * N + 12 if nx is None else nx
    ng = 104 * N + 12 if ng is None else ng
    nnz_jac = 36 + 385 * (N - 1) + 313 if nnz_jac is None else nnz_jac
    nnz_hess = 177 * N + 12 * (N - 1) + 12 if nnz_hess is None else nnz_hess
    parts = [(n, nx) for n in ("x", "xt", "dx", "gx")] + [(n, ng) for n in ("g", "gt", "s", "ds", "zL", "zU", "y", "yn", "sig", "rho")]
    parts += [("J", nnz_jac), ("H", nnz_hess), ("Hc", N * WS_RUNC), ("ric", (N + 1) * WS_RIC_STRIDE), ("cond", N * WS_RCG)]
    parts += [(n, ng) for n in ("en", "ep", "wn", "wp", "sig2", "rho2", "s2", "zL2", "zU2", "y2")] + [("rec", WS_EXIT_REC)]
    off, out = 0, {}
    for n, sz in parts:
        out[n] = (off, sz)
        off += sz
    out["total"] = off
    return out


def _hip_runtime():
    """the HIP runtime this process has already mapped (torch's own copy when torch is loaded): a second copy would know nothing of the allocations"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    return C.CDLL("libamdhip64.so")


def load(path=None):
    path = path or os.path.join(HERE, LIB_NAME)
    try:  # torch ships its own libamdhip64: it must be the first HIP runtime loaded in the process,
        import torch  # noqa: F401  (otherwise torch.cuda later reports "No HIP GPUs are available")
    except ImportError:
        pass
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with __graft_entry__.build() (hipcc, gfx950). No CPU fallback exists.")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():      # a symbol the library lacks raises here: a broken build
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    lib.emu_hooks = [name for name in EMU_HOOKS if hasattr(lib, name)]      # non-empty: the host emulation, whose device memory is host memory
    for name in lib.emu_hooks:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = EMU_HOOKS[name]
    return lib


def _n(v):
    """a device address or stream held as an integer, 0 = NULL"""
    return v or None


def _ref(v):
    """byref of a struct, None = NULL"""
    return C.byref(v) if v is not None else None


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _pi(a):
    return None if a is None else a.ctypes.data_as(_ip)


def _solve_outputs(B, nx, ng=None):
    """the host outputs of a solve of B members: (dict x f lam_g status iters kkt, their C pointers in that order); ng = None: lam_g = None / NULL"""
    out = dict(x=np.zeros((B, nx)), f=np.zeros(B), lam_g=None if ng is None else np.zeros((B, ng)),
               status=np.zeros(B, np.int32), iters=np.zeros(B, np.int32), kkt=np.zeros((B, 3)))
    return out, [_p(out["x"]), _p(out["f"]), _p(out["lam_g"]), _pi(out["status"]), _pi(out["iters"]), _p(out["kkt"])]


def _block_to_host(lib, ptr, shape, what):
    """host array `shape` of doubles from a block of the library's device memory (host memory under the emulation)"""
    out = np.empty(shape)
    if lib.emu_hooks:
        C.memmove(out.ctypes.data, ptr, out.nbytes)
    else:
        hip = _hip_runtime()
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rc = hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2)      # hipMemcpyDeviceToHost
        if rc != 0:
            raise RuntimeError("hipMemcpy of %s failed (%d)" % (what, rc))
    return out


class SolveStream:
    """landing_stream_* (include/landing_nlp.h): consecutive batches through one context with `lanes` launches in flight.  Device pointers; the caller keeps
    the buffers of a submission alive until it has waited for its ticket."""

    def __init__(self, lib, lanes=2):
        self.L = lib
        self.h = lib.lib.landing_stream_create(lib.ctx, lanes)
        if not self.h:
            raise RuntimeError("landing_stream_create: " + lib.lib.landing_last_error().decode())
        self.lanes = lib.lib.landing_stream_lanes(self.h)

    def submit(self, B, d_p, d_x0, opts, d_x, d_f=0, d_lam_g=0, d_status=0, d_iters=0, d_kkt=0, in_stream=0):
        t = self.L.lib.landing_stream_submit(self.h, B, d_p, d_x0, C.byref(opts), d_x, _n(d_f), _n(d_lam_g), _n(d_status), _n(d_iters), _n(d_kkt), _n(in_stream))
        if t < 0:
            raise RuntimeError("landing_stream_submit: " + self.L.lib.landing_last_error().decode())
        return t

    def wait(self, ticket, stream=0):
        self.L._check(self.L.lib.landing_stream_wait(self.h, ticket, _n(stream)), "landing_stream_wait")

    def sync(self, stream=0):
        self.L._check(self.L.lib.landing_stream_sync(self.h, _n(stream)), "landing_stream_sync")

    def close(self):
        if self.h:
            self.L.lib.landing_stream_destroy(self.h); self.h = None


def _matlab_args(names, struct, args):
    keep, a = [], struct()
    B = np.asarray(args["x0"]).shape[-1] if np.asarray(args["x0"]).ndim > 1 else 1
    for n in names:
        v = args.get(n)
        if v is None:
            setattr(a, n, None)
            continue
        buf = np.ascontiguousarray(np.asarray(v, float).reshape((-1, B), order="F").T)     # [B, n] member-major
        keep.append(buf)
        setattr(a, n, buf.ctypes.data_as(_dp))
    return a, keep, B


def matlab_args21(N, args):
    """dict of the 21 arguments as MATLAB would hold them for a batch of B members -- arrays whose LAST axis is the batch
    (Xref [12, N+1, B], dt [1, N, B], 6-vectors [6, B], x0 [nx, B], scalars [1, B] ...) -- flattened column-major into the
    member-major host buffers the C ABI takes.  Returns (Args21, keep-alive list, B)."""
    return _matlab_args(ARGS21, Args21, args)


def matlab_args25(N, args):
    """the same for the 25 arguments of the N=41 script (c_init may be missing: inactive)"""
    return _matlab_args(ARGS25, Args25, args)


class LandingLib:
    """Thin object wrapper: one context per (N, device)."""

    def __init__(self, N, device=0, kin_box=None, lib_path=None, run_cost=None, ccc_params=False):
        self.lib = load(lib_path)
        self.N = N
        form = LandingForm()
        self.lib.landing_form_default(C.byref(form))
        if kin_box is not None:
            for i in range(3):
                form.kin_box[i] = kin_box[i]
        if run_cost is not None:      # dict(QX=[12], Qc=[3], Qf=[3], f_ref=[3]): generate_quadruped_SRBM_CCC.m:81-89
            form.run_cost = 1
            for i in range(12):
                form.QX[i] = run_cost["QX"][i]
            for i in range(3):
                form.Qc[i] = run_cost["Qc"][i]; form.Qf[i] = run_cost["Qf"][i]; form.f_ref[i] = run_cost.get("f_ref", (0, 0, 0))[i]
        if ccc_params:                # the N=41 script's own parameter vector: weights and force reference are entries of p (run_cost = 2)
            form.run_cost = 2
        self.form = form
        self.ctx = self.lib.landing_create(N, device, C.byref(form))
        if not self.ctx:
            raise RuntimeError("landing_create failed: " + self.lib.landing_last_error().decode())
        self.nx, self.ng, self.np_ = self.lib.landing_nx(N), self.lib.landing_ng(N), self.lib.landing_ctx_np(self.ctx)
        self.nnz_jac, self.nnz_hess = self.lib.landing_nnz_jac(N), self.lib.landing_nnz_hess(N)

    def close(self):
        if self.ctx:
            self.lib.landing_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.landing_last_error().decode()}")

    def default_opts(self):
        o = SolverOpts()
        self.lib.landing_solver_opts_default(C.byref(o))
        return o

    def warm_opts(self):
        o = SolverOpts()
        self.lib.landing_solver_opts_warm(C.byref(o))
        return o

    def mpc_shift_device(self, B, d_x_prev, d_state, d_p, d_x0, stream=0):
        self._check(self.lib.landing_mpc_shift(self.ctx, B, d_x_prev, d_state, d_p, d_x0, _n(stream)), "landing_mpc_shift")

    def pattern_jac(self):
        ci = np.zeros(self.nx + 1, np.int64); r = np.zeros(self.nnz_jac, np.int64)
        self._check(self.lib.landing_pattern_jac(self.N, ci.ctypes.data_as(_llp), r.ctypes.data_as(_llp)), "pattern_jac")
        return ci, r

    def pattern_hess(self):
        ci = np.zeros(self.nx + 1, np.int64); r = np.zeros(self.nnz_hess, np.int64)
        self._check(self.lib.landing_pattern_hess(self.N, ci.ctypes.data_as(_llp), r.ctypes.data_as(_llp)), "pattern_hess")
        return ci, r

    def pattern_hess_rc(self):
        """pattern of the Lagrangian Hessian of the running-cost formulation: casadi_s4 + 18 N diagonals"""
        n = self.lib.landing_nnz_hess_rc(self.N)
        ci = np.zeros(self.nx + 1, np.int64); r = np.zeros(n, np.int64)
        self._check(self.lib.landing_pattern_hess_rc(self.N, ci.ctypes.data_as(_llp), r.ctypes.data_as(_llp)), "pattern_hess_rc")
        return ci, r

    def hess_rc_host(self, x, p, lam_f, lam_g):
        x = np.ascontiguousarray(np.atleast_2d(x), float); p = np.ascontiguousarray(np.atleast_2d(p), float)
        lam_g = np.ascontiguousarray(np.atleast_2d(lam_g), float)
        lam_f = None if lam_f is None else np.ascontiguousarray(np.atleast_1d(lam_f), float)
        h = np.full((x.shape[0], self.lib.landing_nnz_hess_rc(self.N)), np.nan)
        self._check(self.lib.landing_eval_hess_rc_batch_host(self.ctx, x.shape[0], _p(x), _p(p), _p(lam_f), _p(lam_g), _p(h)), "landing_eval_hess_rc_batch_host")
        return h

    def workspace_offsets(self):
        return workspace_offsets(self.N, self.nx, self.ng, self.nnz_jac, self.nnz_hess)

    def _workspace(self):
        """landing_debug_workspace: (address of the solver workspace or None, doubles per member)"""
        ptr = C.c_void_p(); st = C.c_ulonglong()
        self._check(self.lib.landing_debug_workspace(self.ctx, C.byref(ptr), C.byref(st)), "landing_debug_workspace")
        return ptr.value, int(st.value)

    def workspace_stride(self):
        """doubles per member of the solver workspace, as the library lays it out"""
        return self._workspace()[1]

    def debug_workspace(self, B):
        """landing_debug_workspace: the blocks of the first B members of the last solve as a host array [B, stride] (diagnostic; the caller has
        synchronised with that solve -- the host entry points have).  Slice a row with workspace_offsets()."""
        ptr, stride = self._workspace()
        if not ptr:
            raise RuntimeError("landing_debug_workspace: no solve has run in this context")
        return _block_to_host(self.lib, ptr, (B, stride), "the solver workspace")

    def solver_tables(self):
        """landing_debug_solver_tables: the tables the solver kernel reads, as the context holds them -- dict of ctab, ccomb, rterm (uint64),
        ctype (int32) and the ints c_ml, c_mid, rlen.  Builds them when no solve has run in this context."""
        out = {}
        for which, (name, dt) in enumerate((("ctab", np.uint64), ("ccomb", np.uint64), ("ctype", np.int32), ("rterm", np.uint64), ("scalars", np.int32))):
            n = C.c_ulonglong()
            self._check(self.lib.landing_debug_solver_tables(self.ctx, which, None, C.byref(n)), "landing_debug_solver_tables")
            out[name] = np.empty(n.value // np.dtype(dt).itemsize, dt)
            self._check(self.lib.landing_debug_solver_tables(self.ctx, which, out[name].ctypes.data, C.byref(n)), "landing_debug_solver_tables")
        out["c_ml"], out["c_mid"], out["rlen"] = (int(v) for v in out.pop("scalars"))
        return out

    # ---- host-pointer entry points (numpy in / numpy out) --------------------------------------
    def eval_host(self, x, p, lam_f=None, lam_g=None, want=("f", "g", "grad_f", "jac", "hess", "grad_gamma_x", "grad_gamma_p")):
        x = np.ascontiguousarray(np.atleast_2d(x), float); p = np.ascontiguousarray(np.atleast_2d(p), float)
        B = x.shape[0]
        if lam_g is not None:
            lam_g = np.ascontiguousarray(np.atleast_2d(lam_g), float)
        if lam_f is not None:
            lam_f = np.ascontiguousarray(np.atleast_1d(lam_f), float)
        shapes = dict(f=(B,), g=(B, self.ng), grad_f=(B, self.nx), jac=(B, self.nnz_jac), hess=(B, self.nnz_hess),
                      grad_gamma_x=(B, self.nx), grad_gamma_p=(B, self.np_))
        out = {k: (np.full(shapes[k], np.nan) if k in want else None) for k in shapes}
        rc = self.lib.landing_eval_batch_host(self.ctx, B, _p(x), _p(p), _p(lam_f), _p(lam_g), _p(out["f"]), _p(out["g"]),
                                              _p(out["grad_f"]), _p(out["jac"]), _p(out["hess"]), _p(out["grad_gamma_x"]),
                                              _p(out["grad_gamma_p"]))
        self._check(rc, "landing_eval_batch_host")
        return {k: v for k, v in out.items() if v is not None}

    def solve_host(self, p, x0, opts=None):
        p = np.ascontiguousarray(np.atleast_2d(p), float); x0 = np.ascontiguousarray(np.atleast_2d(x0), float)
        B = p.shape[0]
        opts = opts or self.default_opts()
        out, ptrs = _solve_outputs(B, self.nx, self.ng)
        self._check(self.lib.landing_solve_batch_host(self.ctx, B, _p(p), _p(x0), C.byref(opts), *ptrs), "landing_solve_batch_host")
        return out

    def solve_stream_host(self, p, x0, opts=None, chunk=1024, lanes=2):
        """landing_solve_stream_host: any number of members, cut into chunks that go through a stream of `lanes` launches in flight"""
        p = np.ascontiguousarray(np.atleast_2d(p), float); x0 = np.ascontiguousarray(np.atleast_2d(x0), float)
        B = p.shape[0]
        opts = opts or self.default_opts()
        out, ptrs = _solve_outputs(B, self.nx, self.ng)
        self._check(self.lib.landing_solve_stream_host(self.ctx, B, chunk, lanes, _p(p), _p(x0), C.byref(opts), *ptrs), "landing_solve_stream_host")
        return out

    def stream(self, lanes=2):
        """landing_stream_create on this context: SolveStream with submit / wait / sync / close"""
        return SolveStream(self, lanes)

    def pack_args21(self, args):
        """p [B, np] from the 21 MATLAB-shaped arguments (landing_pack_args21; host only)"""
        a, keep, B = matlab_args21(self.N, args)
        p = np.zeros((B, self.np_))
        self._check(self.lib.landing_pack_args21(self.N, B, C.byref(a), _p(p)), "landing_pack_args21")
        return p

    def solve_args21(self, args, opts=None, spelled_out=False):
        """the reference's solver-function call, batched: args = dict of the 21 MATLAB-shaped arrays (batch = last axis)"""
        a, keep, B = matlab_args21(self.N, args)
        opts = opts or self.default_opts()
        out, ptrs = _solve_outputs(B, self.nx)
        del out["lam_g"], ptrs[2]      # (this entry point has no multiplier output)
        if spelled_out:
            rc = self.lib.landing_solve_21(self.ctx, B, *[getattr(a, n) for n in ARGS21], C.byref(opts), *ptrs)
        else:
            rc = self.lib.landing_solve_args21(self.ctx, B, C.byref(a), C.byref(opts), *ptrs)
        self._check(rc, "landing_solve_args21")
        return out

    def solve_args25(self, args, opts=None):
        """the N=41 script's solver-function call, batched: args = dict of its 25 MATLAB-shaped arrays (batch = last axis)"""
        a, keep, B = matlab_args25(self.N, args)
        opts = opts or self.default_opts()
        out, ptrs = _solve_outputs(B, self.nx, self.ng)
        self._check(self.lib.landing_solve_args25(self.ctx, B, C.byref(a), C.byref(opts), *ptrs), "landing_solve_args25")
        return out

    def solve_args21_multi(self, args, devices, opts=None, one_call=False, want_lam=True):
        """the reference's solver-function call sharded over a device list from the C boundary (landing_multi_solve_args21 /
        landing_solve_21_multi): contiguous shards, one host thread + context per entry of `devices` (an index may repeat)"""
        a, keep, B = matlab_args21(self.N, args)
        opts = opts or self.default_opts()
        out, ptrs = _solve_outputs(B, self.nx, self.ng if want_lam else None)
        dev = (C.c_int * len(devices))(*devices)
        if one_call:
            rc = self.lib.landing_solve_21_multi(dev, len(devices), self.N, B, *[getattr(a, n) for n in ARGS21], C.byref(opts), *ptrs)
        else:
            m = self.lib.landing_multi_create(self.N, dev, len(devices), C.byref(self.form))
            if not m:
                raise RuntimeError("landing_multi_create: " + self.lib.landing_last_error().decode())
            try:
                rc = self.lib.landing_multi_solve_args21(m, B, C.byref(a), C.byref(opts), *ptrs)
            finally:
                self.lib.landing_multi_destroy(m)
        self._check(rc, "landing_multi_solve_args21")
        return out

    def riccati_gains_device(self, B, n, d_xref, d_fref, Ib3x3, mass, Q, r_diag, F, dt, rk4=False, d_P=0, d_K=0, d_A=0, d_B=0, stream=0):
        """landing_riccati_gains_batch: VBL linearisation + Riccati tracking gains along B sampled trajectories (device pointers)"""
        Ib3x3 = np.ascontiguousarray(Ib3x3, float); Q = np.ascontiguousarray(Q, float); F = np.ascontiguousarray(F, float); r = np.ascontiguousarray(r_diag, float)
        rc = self.lib.landing_riccati_gains_batch(self.ctx, B, n, d_xref, d_fref, _p(Ib3x3), float(mass), _p(Q), _p(r), _p(F), float(dt), int(bool(rk4)),
                                                  _n(d_P), _n(d_K), _n(d_A), _n(d_B), _n(stream))
        self._check(rc, "landing_riccati_gains_batch")

    def sample_reference_device(self, B, d_x, d_p, dt_r, n, d_xref=0, d_fref=0, stream=0):
        """landing_sample_reference_batch: B solutions (solver layout) onto the uniform Riccati grid of n points, step dt_r, each member along the
        time grid its own p carries (device pointers).  The last interval is never entered: points past the second-to-last knot extrapolate."""
        rc = self.lib.landing_sample_reference_batch(self.ctx, B, _n(d_x), _n(d_p), float(dt_r), int(n), _n(d_xref), _n(d_fref), _n(stream))
        self._check(rc, "landing_sample_reference_batch")

    def tracking_gains_device(self, B, d_x, d_p, dt_r, n, Ib3x3, mass, Q, r_diag, F, rk4=False, d_status=0, d_P=0, d_K=0, d_A=0, d_B=0, d_xref=0, d_fref=0, stream=0):
        """landing_tracking_gains_batch: resampling + Riccati tracking gains of a solved batch on one stream (device pointers).  With d_status,
        members that did not converge get zeros; d_xref / d_fref = 0 keeps the sampled reference in the context."""
        Ib3x3 = np.ascontiguousarray(Ib3x3, float); Q = np.ascontiguousarray(Q, float); F = np.ascontiguousarray(F, float); r = np.ascontiguousarray(r_diag, float)
        rc = self.lib.landing_tracking_gains_batch(self.ctx, B, _n(d_x), _n(d_p), _n(d_status), float(dt_r), int(n), _p(Ib3x3), float(mass), _p(Q), _p(r), _p(F),
                                                   int(bool(rk4)), _n(d_P), _n(d_K), _n(d_A), _n(d_B), _n(d_xref), _n(d_fref), _n(stream))
        self._check(rc, "landing_tracking_gains_batch")

    def tracking_gains_host(self, x, p, dt_r, n, Ib3x3, mass, Q, r_diag, F, rk4=False, status=None, want=("K",)):
        """landing_tracking_gains_host: numpy in / numpy out; want: any of P, K, A, B, xref, fref"""
        x = np.ascontiguousarray(np.atleast_2d(x), float); p = np.ascontiguousarray(np.atleast_2d(p), float)
        B = x.shape[0]
        status = None if status is None else np.ascontiguousarray(status, np.int32)
        Ib3x3 = np.ascontiguousarray(Ib3x3, float); Q = np.ascontiguousarray(Q, float); F = np.ascontiguousarray(F, float); r = np.ascontiguousarray(r_diag, float)
        shapes = dict(P=(B, n, 24, 24), K=(B, n, 12, 24), A=(B, n, 24, 24), B=(B, n, 24, 12), xref=(B, n, 24), fref=(B, n, 12))
        out = {k: (np.full(shapes[k], np.nan) if k in want else None) for k in shapes}
        rc = self.lib.landing_tracking_gains_host(self.ctx, B, _p(x), _p(p), _pi(status), float(dt_r), int(n), _p(Ib3x3),
                                                  float(mass), _p(Q), _p(r), _p(F), int(bool(rk4)), *[_p(out[k]) for k in ("P", "K", "A", "B", "xref", "fref")])
        self._check(rc, "landing_tracking_gains_host")
        return {k: v for k, v in out.items() if v is not None}

    # ---- device-pointer entry points (integers = device addresses, e.g. torch tensor.data_ptr()) --
    def eval_device(self, B, d_x, d_p, d_lam_f=0, d_lam_g=0, d_f=0, d_g=0, d_grad_f=0, d_jac=0, d_hess=0, d_ggx=0, d_ggp=0, stream=0):
        rc = self.lib.landing_eval_batch(self.ctx, B, d_x, d_p, _n(d_lam_f), _n(d_lam_g), _n(d_f), _n(d_g),
                                         _n(d_grad_f), _n(d_jac), _n(d_hess), _n(d_ggx), _n(d_ggp), _n(stream))
        self._check(rc, "landing_eval_batch")

    def bounds_device(self, B, d_p, d_lbg, d_ubg, stream=0):
        self._check(self.lib.landing_bounds_batch(self.ctx, B, d_p, d_lbg, d_ubg, _n(stream)), "landing_bounds_batch")

    def solve_device(self, B, d_p, d_x0, opts, d_x, d_f=0, d_lam_g=0, d_status=0, d_iters=0, d_kkt=0, stream=0):
        rc = self.lib.landing_solve_batch(self.ctx, B, d_p, d_x0, C.byref(opts), d_x, _n(d_f), _n(d_lam_g),
                                          _n(d_status), _n(d_iters), _n(d_kkt), _n(stream))
        self._check(rc, "landing_solve_batch")
