"""Host side of the floating-base rigid-body routines: the reference's 'quad3D' Mini-Cheetah tree
(utilities_general/dynamics-utilities/get_robot_model.m:134-234 with the 'mc3D' parameters of get_robot_params.m:50-115)
in the compact form the HIP kernels use -- Xtree = plux(E, r), link inertia = (mass, m*com, rotational inertia about the
link origin) -- and the ctypes binding of landing_rbd_set_model / landing_fb_dynamics_batch / landing_kinodyn_rows_batch."""
import ctypes as C

import numpy as np

from . import constants as K


class RbdModel(C.Structure):
    _fields_ = [("parent", C.c_int * 18), ("jtype", C.c_int * 18), ("E", (C.c_double * 9) * 18), ("r", (C.c_double * 3) * 18),
                ("m", C.c_double * 18), ("h", (C.c_double * 3) * 18), ("I", (C.c_double * 6) * 18),
                ("b_foot", C.c_int * 4), ("foot_r", (C.c_double * 3) * 4), ("l1", C.c_double), ("l2", C.c_double), ("l3", C.c_double), ("l4", C.c_double)]


def _rbi(m, com, rot):
    """(m, h, Ibar about the origin): spatialInertia.m restated in compact form"""
    com = np.asarray(com, float); c = K._skew(com)
    Ibar = np.asarray(rot, float) + m * (c @ c.T)
    return m, m * com, np.array([Ibar[0, 0], Ibar[0, 1], Ibar[0, 2], Ibar[1, 1], Ibar[1, 2], Ibar[2, 2]])


def _flip_y_rbi(m, h, I6):
    """flipAlongAxis(I, 'Y') (get_robot_model.m:852-889): mirror the link through the x-z plane"""
    return m, h * np.array([1, -1, 1.0]), I6 * np.array([1, -1, 1, 1, -1, 1.0])


def quad3d_model():
    M = RbdModel()
    abad = _rbi(0.54, [0, 0.036, 0], 1e-6 * np.array([[381, 58, 0.45], [58, 560, 0.95], [0.45, 0.95, 444]]))
    hip = _rbi(0.634, [0, 0.016, -0.02], 1e-6 * np.array([[1983, 245, 13], [245, 2103, 1.5], [13, 1.5, 408]]))
    knee = _rbi(0.064, [0, 0, -0.061], 1e-6 * np.array([[6, 0, 0], [0, 248, 0], [0, 0, 245.0]]))
    body = _rbi(3.3, [0, 0, 0], 1e-6 * np.diag([11253.0, 36203.0, 42673.0]))
    zero = (0.0, np.zeros(3), np.zeros(6))
    abad_loc, hip_loc, knee_loc, foot_loc = np.array([0.19, 0.049, 0.0]), np.array([0, 0.062, 0.0]), np.array([0, 0, -0.209]), np.array([0, 0, -0.195])
    side = np.array([[1, 1, -1, -1], [-1, 1, -1, 1], [1, 1, 1, 1]], float)
    rzpi = np.array([[np.cos(np.pi), np.sin(np.pi), 0], [-np.sin(np.pi), np.cos(np.pi), 0], [0, 0, 1.0]])
    bodies = [(i, t, np.eye(3), np.zeros(3), zero) for i, t in zip(range(6), (3, 4, 5, 0, 1, 2))]     # Px Py Pz Rx Ry Rz
    bodies[5] = (5, 2, np.eye(3), np.zeros(3), body)
    leg_side = -1
    for leg in range(4):
        s = side[:, leg]
        links = [abad, hip, knee] if leg_side > 0 else [_flip_y_rbi(*abad), _flip_y_rbi(*hip), _flip_y_rbi(*knee)]
        n0 = len(bodies)
        bodies.append((6, 0, np.eye(3), s * abad_loc, links[0]))
        bodies.append((n0 + 1, 1, rzpi, s * hip_loc, links[1]))           # plux(rz(pi), 0) * plux(1, r) = plux(rz(pi), r)
        bodies.append((n0 + 2, 1, np.eye(3), s * knee_loc, links[2]))
        M.b_foot[leg] = n0 + 3
        for j in range(3):
            M.foot_r[leg][j] = (s * foot_loc)[j]
        leg_side = -leg_side
    for i, (pa, jt, E, r, (m, h, I6)) in enumerate(bodies):
        M.parent[i] = pa; M.jtype[i] = jt; M.m[i] = m
        for j in range(9): M.E[i][j] = E.flatten()[j]
        for j in range(3): M.r[i][j] = r[j]; M.h[i][j] = h[j]
        for j in range(6): M.I[i][j] = I6[j]
    M.l1, M.l2, M.l3, M.l4 = 0.062, 0.209, 0.195, 0.004                       # get_foot_jacobians_mc.m:5-8
    return M


TAU_MAX = np.tile(np.array([6.0, 6.0, 9.33]) * 3.0, 4)     # model.gr .* motorTauMax (get_robot_model.m:236-240, get_robot_params.m:103-108)
JPOS_MIN = np.tile([-np.pi / 3, -np.pi / 2, 0.0], 4)       # landing_optimization.m:246-247
JPOS_MAX = np.tile([np.pi / 3, np.pi / 2, 3 * np.pi / 4], 4)


class KinodynParams(C.Structure):
    """landing_kinodyn_params of include/landing_nlp.h"""
    _fields_ = [("dt", C.c_double * 64), ("mass", C.c_double), ("Ib", C.c_double * 3), ("Ib_inv", C.c_double * 3), ("mu", C.c_double)]


class Rbd:
    """binds the three entry points on an existing LandingLib (its context owns the uploaded model)"""

    def __init__(self, lib, model=None):
        """model: an RbdModel to upload instead of quad3d_model() (any tree landing_rbd_set_model takes; include/landing_nlp.h states what needs the quadruped's numbering)"""
        self.L = lib
        vp = C.c_void_p
        lib.lib.landing_rbd_set_model.argtypes = [vp, C.POINTER(RbdModel)]
        lib.lib.landing_fb_dynamics_batch.argtypes = [vp, C.c_int] + [vp] * 9 + [C.c_double, vp]
        lib.lib.landing_kinodyn_rows_batch.argtypes = [vp, C.c_int] + [vp] * 7 + [vp]
        dp = C.POINTER(C.c_double)
        lib.lib.landing_leg_ik_batch.argtypes = [vp, C.c_int, vp, vp, dp, dp, C.c_int, vp, vp, vp]
        lib.lib.landing_kinodyn_nlp_dims.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        lib.lib.landing_kinodyn_nlp_eval.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(KinodynParams), vp, vp, vp]
        lib.lib.landing_kinodyn_nlp_hess.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(KinodynParams), vp, vp, vp]
        ip = C.POINTER(C.c_int)
        lib.lib.landing_kinodyn_solve_batch_host.argtypes = [vp, C.c_int, C.c_int, C.POINTER(KinodynParams), dp, dp, dp, dp, vp, dp, dp, dp, ip, ip, dp]
        lib.lib.landing_kinodyn_solve_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(KinodynParams)] + [vp] * 4 + [vp] + [vp] * 6 + [vp]
        self.model = quad3d_model() if model is None else model
        lib._check(lib.lib.landing_rbd_set_model(lib.ctx, C.byref(self.model)), "landing_rbd_set_model")

    def fb_dynamics(self, npts, d_q, d_qd, d_tau=0, d_f_foot=0, d_H=0, d_C=0, d_qdd=0, d_A=0, d_Hinv=0, fd_h=0.0, stream=0):
        """fd_h = 0: exact linearisation (forward-mode tangents of the inverse dynamics); fd_h > 0: central differences with that step"""
        n = lambda v: v or None
        self.L._check(self.L.lib.landing_fb_dynamics_batch(self.L.ctx, npts, d_q, d_qd, n(d_tau), n(d_f_foot), n(d_H), n(d_C), n(d_qdd), n(d_A), n(d_Hinv), fd_h, n(stream)),
                      "landing_fb_dynamics_batch")

    def kinodyn_rows(self, npts, d_q6, d_c, d_f, d_jpos, d_fk=0, d_fk_err=0, d_tau=0, stream=0):
        n = lambda v: v or None
        self.L._check(self.L.lib.landing_kinodyn_rows_batch(self.L.ctx, npts, d_q6, n(d_c), n(d_f), d_jpos, n(d_fk), n(d_fk_err), n(d_tau), n(stream)), "landing_kinodyn_rows_batch")

    def kinodyn_nlp_dims(self, N):
        nx, ng = C.c_longlong(), C.c_longlong()
        self.L._check(self.L.lib.landing_kinodyn_nlp_dims(N, C.byref(nx), C.byref(ng)), "landing_kinodyn_nlp_dims")
        return nx.value, ng.value

    @staticmethod
    def _kd_params(N, dt, mass, Ib, Ib_inv, mu):
        prm = KinodynParams()
        for k in range(N):
            prm.dt[k] = float(dt[k])
        prm.mass = float(mass); prm.mu = float(mu)
        for i in range(3):
            prm.Ib[i] = float(Ib[i]); prm.Ib_inv[i] = float(Ib_inv[i])
        return prm

    def kinodyn_nlp_eval(self, B, N, d_x, dt, mass, Ib, Ib_inv, mu, d_g=0, d_jac=0, stream=0):
        """function layer of the kinodynamic refinement NLP (include/landing_nlp.h): g [B, ng] and / or the Jacobian blocks [B, N, 141, 72]"""
        prm = self._kd_params(N, dt, mass, Ib, Ib_inv, mu)
        n = lambda v: v or None
        self.L._check(self.L.lib.landing_kinodyn_nlp_eval(self.L.ctx, B, N, d_x, C.byref(prm), n(d_g), n(d_jac), n(stream)), "landing_kinodyn_nlp_eval")

    def kinodyn_nlp_hess(self, B, N, d_x, dt, mass, Ib, Ib_inv, mu, d_lam_g, d_hess, stream=0):
        """Hessian blocks of lam_g' g per interval [B, N, 72, 72] (include/landing_nlp.h)"""
        prm = self._kd_params(N, dt, mass, Ib, Ib_inv, mu)
        self.L._check(self.L.lib.landing_kinodyn_nlp_hess(self.L.ctx, B, N, d_x, C.byref(prm), d_lam_g, d_hess, stream or None), "landing_kinodyn_nlp_hess")

    def kinodyn_default_opts(self):
        from .capi import SolverOpts
        o = SolverOpts()
        self.L.lib.landing_kinodyn_solver_opts_default(C.byref(o))
        return o

    def kinodyn_warm_opts(self):
        """landing_kinodyn_solver_opts_warm: the re-solve from a previous solution"""
        from .capi import SolverOpts
        o = SolverOpts()
        self.L.lib.landing_kinodyn_solver_opts_warm(C.byref(o))
        return o

    def kinodyn_solve_host(self, N, lbg, ubg, cost, x0, dt, mass, Ib, Ib_inv, mu, opts=None):
        """landing_kinodyn_solve_batch_host: B kinodynamic refinement NLPs (host arrays [B, ng], [B, ng], [B, 24], [B, nx]) -> dict"""
        lbg = np.ascontiguousarray(np.atleast_2d(lbg), float); ubg = np.ascontiguousarray(np.atleast_2d(ubg), float)
        cost = np.ascontiguousarray(np.atleast_2d(cost), float); x0 = np.ascontiguousarray(np.atleast_2d(x0), float)
        B = x0.shape[0]; nx, ng = self.kinodyn_nlp_dims(N)
        assert x0.shape == (B, nx) and lbg.shape == (B, ng) and ubg.shape == (B, ng) and cost.shape == (B, 24)
        prm = self._kd_params(N, dt, mass, Ib, Ib_inv, mu)
        x = np.zeros((B, nx)); f = np.zeros(B); lam = np.zeros((B, ng)); st = np.zeros(B, np.int32); it = np.zeros(B, np.int32); kkt = np.zeros((B, 3))
        dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int); P = lambda a: a.ctypes.data_as(dp)
        rc = self.L.lib.landing_kinodyn_solve_batch_host(self.L.ctx, B, N, C.byref(prm), P(lbg), P(ubg), P(cost), P(x0), C.byref(opts) if opts is not None else None,
                                                         P(x), P(f), P(lam), st.ctypes.data_as(ip), it.ctypes.data_as(ip), P(kkt))
        self.L._check(rc, "landing_kinodyn_solve_batch_host")
        return dict(x=x, f=f, lam_g=lam, status=st, iters=it, kkt=kkt)

    def kinodyn_solve_device(self, B, N, d_lbg, d_ubg, d_cost, d_x0, dt, mass, Ib, Ib_inv, mu, opts, d_x, d_f=0, d_lam=0, d_status=0, d_iters=0, d_kkt=0, stream=0):
        prm = self._kd_params(N, dt, mass, Ib, Ib_inv, mu)
        n = lambda v: v or None
        rc = self.L.lib.landing_kinodyn_solve_batch(self.L.ctx, B, N, C.byref(prm), d_lbg, d_ubg, d_cost, d_x0, C.byref(opts) if opts is not None else None,
                                                    d_x, n(d_f), n(d_lam), n(d_status), n(d_iters), n(d_kkt), n(stream))
        self.L._check(rc, "landing_kinodyn_solve_batch")

    ARGS24 = ("Xref", "Uref", "dt", "q_min", "q_max", "qd_min", "qd_max", "q_init", "qd_init", "c_init", "q_term_min", "q_term_max", "qd_term_min",
              "qd_term_max", "QN", "x0", "jpos_min", "jpos_max", "kin_box", "mu", "l_leg_max", "mass", "Ib", "Ib_inv")

    def kinodyn_solve_24(self, N, args, opts=None, form=None):
        """landing_solve_kinodyn_24: the reference's 24-argument solver function (generate_landingCtrller_KNITRO.m:373-377), `args` = dict name ->
        MATLAB-shaped array (column-major, batch = last axis; Uref may be None)"""
        dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int)
        keep = []
        def conv(name):
            v = args.get(name)
            if v is None:
                return None
            a = np.asfortranarray(np.asarray(v, float)); keep.append(a)
            return a.ctypes.data_as(dp)
        ptrs = [conv(n) for n in self.ARGS24]
        B = int(np.asarray(args["x0"]).reshape(48 * N + 12, -1, order="F").shape[1])
        nx, ng = self.kinodyn_nlp_dims(N)
        x = np.zeros((B, nx)); f = np.zeros(B); lam = np.zeros((B, ng)); st = np.zeros(B, np.int32); it = np.zeros(B, np.int32); kkt = np.zeros((B, 3))
        P = lambda a: a.ctypes.data_as(dp)
        fn = self.L.lib.landing_solve_kinodyn_24
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [dp] * 24 + [C.c_void_p, dp, dp, dp, ip, ip, dp]
        rc = fn(self.L.ctx, N, B, C.byref(form) if form is not None else None, *ptrs, C.byref(opts) if opts is not None else None,
                P(x), P(f), P(lam), st.ctypes.data_as(ip), it.ctypes.data_as(ip), P(kkt))
        self.L._check(rc, "landing_solve_kinodyn_24")
        return dict(x=x, f=f, lam_g=lam, status=st, iters=it, kkt=kkt)

    # ---- the drop-state chain: SRBM solve -> refinement -> warm re-solve (include/landing_nlp.h landing_pipeline_*; device pointers are integers) ----
    def pipeline_opts(self):
        """landing_pipeline_opts_default"""
        from .capi import PipelineOpts
        o = PipelineOpts()
        self.L.lib.landing_pipeline_opts_default(C.byref(o))
        return o

    def kinodyn_pose_device(self, B, d_p, d_x_srbm, d_lbg, d_ubg, d_cost, d_x0, opts=None, stream=0):
        """landing_kinodyn_pose_batch: member b's refinement problem from its SRBM p and x*"""
        self.L._check(self.L.lib.landing_kinodyn_pose_batch(self.L.ctx, B, d_p, d_x_srbm, C.byref(opts) if opts is not None else None, d_lbg, d_ubg, d_cost, d_x0,
                                                            stream or None), "landing_kinodyn_pose_batch")

    def training_pairs_device(self, B, d_p, d_x_kd, d_status_final, d_in, d_out, d_index, d_count, stream=0):
        """landing_training_pairs_batch: the converged members' training columns, compacted in member order"""
        self.L._check(self.L.lib.landing_training_pairs_batch(self.L.ctx, B, d_p, d_x_kd, d_status_final, d_in, d_out, d_index, d_count, stream or None),
                      "landing_training_pairs_batch")

    # ---- actuator audit of refined trajectories (include/landing_nlp.h landing_actuator_*; csrc/actuator_kernels.hip) ----
    def actuator_model(self):
        """landing_actuator_model_mc3d"""
        from .capi import ActuatorModel
        m = ActuatorModel()
        self.L.lib.landing_actuator_model_mc3d(C.byref(m))
        return m

    def actuator_screen(self, **limits):
        """landing_actuator_screen_default (volt_max = 24, drive_only = 1, the other limits off), fields overridden by keyword"""
        from .capi import ActuatorScreen
        s = ActuatorScreen()
        self.L.lib.landing_actuator_screen_default(C.byref(s))
        for k, v in limits.items():
            if k not in dict(ActuatorScreen._fields_):
                raise TypeError("landing_actuator_screen has no field %r" % k)
            setattr(s, k, v)
        return s

    def actuator_audit_device(self, B, d_dt, dt_stride, d_x_kd, d_summary, d_where, d_ok, model=None, screen=None, d_tau=0, d_jvel=0, d_volt=0, stream=0):
        """landing_actuator_audit_batch: device pointers (integers); d_dt + b * dt_stride is member b's grid (0: one grid for all)"""
        n = lambda v: v or None
        ref = lambda v: C.byref(v) if v is not None else None
        self.L._check(self.L.lib.landing_actuator_audit_batch(self.L.ctx, B, n(d_dt), dt_stride, n(d_x_kd), ref(model), ref(screen), n(d_tau), n(d_jvel), n(d_volt),
                                                              n(d_summary), n(d_where), n(d_ok), n(stream)), "landing_actuator_audit_batch")

    def actuator_audit(self, x_kd, dt, model=None, screen=None, full=True):
        """landing_actuator_audit_host: numpy x [B, 48N+12] (the refinement's layout) and dt [N] (one grid) or [B, N] -> dict of summary [B, 8]
        (capi.AUDIT_SUMMARY), where [B, 4], ok [B] and, with full, tau / jvel / volt [B, N, 12]"""
        from .capi import AUDIT_NSUM
        N = self.L.N
        x = np.ascontiguousarray(np.atleast_2d(x_kd), float); dt = np.ascontiguousarray(dt, float)
        B = x.shape[0]
        assert x.shape == (B, 48 * N + 12) and dt.shape in ((N,), (B, N))
        mk = lambda: np.zeros((B, N, 12)) if full else None
        tau, jvel, volt = mk(), mk(), mk()
        summ, where, ok = np.zeros((B, AUDIT_NSUM)), np.zeros((B, 4), np.int32), np.zeros(B, np.int32)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        P = lambda a: None if a is None else a.ctypes.data_as(dp)
        ref = lambda v: C.byref(v) if v is not None else None
        rc = self.L.lib.landing_actuator_audit_host(self.L.ctx, B, P(dt), N if dt.ndim == 2 else 0, P(x), ref(model), ref(screen), P(tau), P(jvel), P(volt), P(summ),
                                                    where.ctypes.data_as(ip), ok.ctypes.data_as(ip))
        self.L._check(rc, "landing_actuator_audit_host")
        out = dict(summary=summ, where=where, ok=ok)
        if full:
            out.update(tau=tau, jvel=jvel, volt=volt)
        return out

    def screened_pairs(self, B, d_p, d_x_kd, d_status3, d_summary, d_where, d_ok, d_in, d_out, d_index, d_count, model=None, screen=None, stream=0):
        """landing_pipeline_screened_pairs_batch: the chain's pair writer behind the screen (device pointers): the members with final status 0 AND ok"""
        n = lambda v: v or None
        ref = lambda v: C.byref(v) if v is not None else None
        self.L._check(self.L.lib.landing_pipeline_screened_pairs_batch(self.L.ctx, B, n(d_p), n(d_x_kd), n(d_status3), ref(model), ref(screen), n(d_summary), n(d_where),
                                                                       n(d_ok), n(d_in), n(d_out), n(d_index), n(d_count), n(stream)), "landing_pipeline_screened_pairs_batch")

    def pipeline_refine_device(self, B, d_p, d_x_srbm, opts, d_x, d_f, d_status, d_iters, d_kkt, d_lam=0, d_in=0, d_out=0, d_index=0, d_count=0,
                               d_srbm_status=0, d_srbm_iters=0, stream=0):
        """landing_pipeline_refine_batch: pose, refinement, warm re-solve, final choice, pairs behind SRBM solutions already on the device"""
        n = lambda v: v or None
        self.L._check(self.L.lib.landing_pipeline_refine_batch(self.L.ctx, B, d_p, d_x_srbm, n(d_srbm_status), n(d_srbm_iters), C.byref(opts) if opts is not None else None,
                                                               d_x, d_f, n(d_lam), d_status, d_iters, d_kkt, n(d_in), n(d_out), n(d_index), n(d_count), n(stream)),
                      "landing_pipeline_refine_batch")

    def pipeline_device(self, B, d_p, d_x0, opts, d_x, d_f, d_status, d_iters, d_kkt, d_lam=0, d_in=0, d_out=0, d_index=0, d_count=0, d_x_srbm=0, stream=0):
        """landing_pipeline_batch: the SRBM solve and the chain above on one stream"""
        n = lambda v: v or None
        self.L._check(self.L.lib.landing_pipeline_batch(self.L.ctx, B, d_p, d_x0, C.byref(opts) if opts is not None else None, n(d_x_srbm), d_x, d_f, n(d_lam),
                                                        d_status, d_iters, d_kkt, n(d_in), n(d_out), n(d_index), n(d_count), n(stream)), "landing_pipeline_batch")

    def pipeline_21(self, args, opts=None, want_lam=False):
        """landing_pipeline_21: the 21 MATLAB-shaped SRBM arguments (batch = last axis) -> the refined, re-solved batch and its training pairs (host arrays)"""
        from .capi import ARGS21, matlab_args21
        a, keep, B = matlab_args21(self.L.N, args)
        N = self.L.N; nxk, ngk = 48 * N + 12, 48 + 141 * (N - 1) + 117
        x = np.zeros((B, nxk)); f = np.zeros(B); lam = np.zeros((B, ngk)) if want_lam else None; st = np.zeros((B, 3), np.int32); it = np.zeros((B, 3), np.int32)
        kkt = np.zeros((B, 3)); pin = np.zeros((B, 9)); pout = np.zeros((B, nxk)); kept = C.c_int(0)
        dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int); P = lambda v: None if v is None else v.ctypes.data_as(dp)
        rc = self.L.lib.landing_pipeline_21(self.L.ctx, B, *[getattr(a, n) for n in ARGS21], C.byref(opts) if opts is not None else None, P(x), P(f), P(lam),
                                            st.ctypes.data_as(ip), it.ctypes.data_as(ip), P(kkt), P(pin), P(pout), C.byref(kept))
        self.L._check(rc, "landing_pipeline_21")
        m = kept.value
        return dict(x=x, f=f, lam_g=lam, status=st, iters=it, kkt=kkt, pair_in=pin[:m].T.copy(), pair_out=pout[:m].T.copy(), n_kept=m)

    def kinodyn_bounds(self, N, B, q_init, qd_init, c_init, q_min, q_term_min, q_term_max, qd_term_min, qd_term_max, jpos_min, jpos_max, kin_box, l_leg_max):
        """landing_kinodyn_bounds (pure host code): arrays [B, n] -> lbg, ubg [B, ng]"""
        dp = C.POINTER(C.c_double)
        a = [np.ascontiguousarray(v, float) for v in (q_init, qd_init, c_init, q_min, q_term_min, q_term_max, qd_term_min, qd_term_max, jpos_min, jpos_max, kin_box, l_leg_max)]
        ng = 48 + 141 * (N - 1) + 117
        lb = np.zeros((B, ng)); ub = np.zeros((B, ng))
        fn = self.L.lib.landing_kinodyn_bounds
        fn.argtypes = [C.c_int, C.c_int, C.c_void_p] + [dp] * 14
        self.L._check(fn(N, B, None, *[v.ctypes.data_as(dp) for v in a], lb.ctypes.data_as(dp), ub.ctypes.data_as(dp)), "landing_kinodyn_bounds")
        return lb, ub

    # ---- CasADi-external face of the kinodynamic NLP (include/landing_nlp.h, round 6): what landingCtrller_KNITRO_mi355x.so forwards to
    def kinodyn_casadi_np(self, N):
        fn = self.L.lib.landing_kinodyn_casadi_np; fn.restype = C.c_longlong; fn.argtypes = [C.c_int]
        return int(fn(N))

    def kinodyn_casadi_pattern(self, N, which):
        lp = C.POINTER(C.c_longlong)
        ci, r, nnz = lp(), lp(), C.c_longlong()
        fn = self.L.lib.landing_kinodyn_casadi_pattern
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(lp), C.POINTER(lp), lp]
        self.L._check(fn(self.L.ctx, N, which, C.byref(ci), C.byref(r), C.byref(nnz)), "landing_kinodyn_casadi_pattern")
        nx = 48 * N + 12
        return np.array(ci[:nx + 1], np.int64), np.array(r[:nnz.value], np.int64)

    def kinodyn_casadi_bounds(self, N, p):
        dp = C.POINTER(C.c_double)
        p = np.ascontiguousarray(p, float); ng = 48 + 141 * (N - 1) + 117
        lb, ub = np.zeros(ng), np.zeros(ng)
        fn = self.L.lib.landing_kinodyn_casadi_bounds
        fn.argtypes = [C.c_int, C.c_void_p, dp, dp, dp]
        self.L._check(fn(N, None, p.ctypes.data_as(dp), lb.ctypes.data_as(dp), ub.ctypes.data_as(dp)), "landing_kinodyn_casadi_bounds")
        return lb, ub

    def kinodyn_casadi_eval(self, N, x, p, lam_f=1.0, lam_g=None, want=("f", "g", "grad_f", "jac", "hess", "ggx", "ggp")):
        """landing_kinodyn_casadi_eval_host: one problem, host arrays; returns a dict of the requested outputs (jac / hess as CCS nonzeros)"""
        dp = C.POINTER(C.c_double)
        nx, ng, npar = 48 * N + 12, 48 + 141 * (N - 1) + 117, self.kinodyn_casadi_np(N)
        x = np.ascontiguousarray(x, float); p = np.ascontiguousarray(p, float)
        assert x.shape == (nx,) and p.shape == (npar,)
        nj, nh = (len(self.kinodyn_casadi_pattern(N, w)[1]) for w in (0, 1))
        size = dict(f=1, g=ng, grad_f=nx, jac=nj, hess=nh, ggx=nx, ggp=npar)
        out = {k: np.zeros(size[k]) for k in want}
        ptr = lambda k: out[k].ctypes.data_as(dp) if k in out else None
        lf = C.c_double(lam_f)
        lg = np.ascontiguousarray(lam_g, float) if lam_g is not None else None
        fn = self.L.lib.landing_kinodyn_casadi_eval_host
        fn.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, dp] + [dp] * 7
        self.L._check(fn(self.L.ctx, N, x.ctypes.data_as(dp), p.ctypes.data_as(dp), C.byref(lf), lg.ctypes.data_as(dp) if lg is not None else None,
                         *[ptr(k) for k in ("f", "g", "grad_f", "jac", "hess", "ggx", "ggp")]), "landing_kinodyn_casadi_eval_host")
        if "f" in out:
            out["f"] = float(out["f"][0])
        return out

    def kinodyn_pattern(self, N, which):
        """landing_kinodyn_pattern: CCS (colind, row) of jac_g_x (which = 0) or triu(hess_gamma_x_x) (which = 1)"""
        nx = 48 * N + 12
        colind = np.zeros(nx + 1, np.int64); nnz = C.c_longlong()
        lp = C.POINTER(C.c_longlong)
        fn = self.L.lib.landing_kinodyn_pattern
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, lp, lp, lp]
        self.L._check(fn(self.L.ctx, N, which, colind.ctypes.data_as(lp), None, C.byref(nnz)), "landing_kinodyn_pattern")
        row = np.zeros(nnz.value, np.int64)
        self.L._check(fn(self.L.ctx, N, which, colind.ctypes.data_as(lp), row.ctypes.data_as(lp), C.byref(nnz)), "landing_kinodyn_pattern")
        return colind, row

    def kinodyn_block_nonzeros(self):
        """landing_kinodyn_block_nonzeros: the solver's table of the structural non-zeros of a Jacobian block's inequality rows -> ((rows, cols) of a middle interval,
        (rows, cols) of the last one); rows count from the top of the 141 x 72 block"""
        n0, n1 = C.c_int(), C.c_int(); buf = np.zeros(2 * 1280, np.uint8)
        fn = self.L.lib.landing_kinodyn_block_nonzeros
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)]
        self.L._check(fn(self.L.ctx, C.byref(n0), C.byref(n1), buf.ctypes.data_as(C.POINTER(C.c_ubyte))), "landing_kinodyn_block_nonzeros")
        e = buf[:2 * (n0.value + n1.value)].reshape(-1, 2).astype(int)
        return (e[:n0.value, 0], e[:n0.value, 1]), (e[n0.value:, 0], e[n0.value:, 1])

    # ---- diagnostics: the workspace the refinement solve leaves behind (include/landing_nlp.h landing_debug_kd_*) ----
    KD_LAYOUT = ("x", "dx", "g", "s", "ds", "zL", "zU", "y", "yn", "sig", "rho", "gc")
    KD_STATE = ("mu", "delta", "delta_last", "alpha", "a_du", "it", "nfact", "nreset", "last_reset_it", "feas", "status", "pending", "omt", "s_corr", "done", "reg_it")
    KD_GC = 60 * 60 + 60

    def kinodyn_workspace_layout(self, N):
        """landing_debug_kd_layout: dict name -> (offset, length) in doubles inside a member's block, plus "state" -> offset of the iteration state and
        "total" -> the member stride"""
        off = (C.c_ulonglong * len(self.KD_LAYOUT))(); so = C.c_ulonglong(); st = C.c_ulonglong()
        fn = self.L.lib.landing_debug_kd_layout
        fn.argtypes = [C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
        self.L._check(fn(N, off, C.byref(so), C.byref(st)), "landing_debug_kd_layout")
        nx, ng = 48 * N + 12, 48 + 141 * (N - 1) + 117
        size = dict(x=nx, dx=nx, gc=N * self.KD_GC)
        out = {n: (int(o), size.get(n, ng)) for n, o in zip(self.KD_LAYOUT, off)}
        out["state"] = int(so.value); out["total"] = int(st.value)
        return out

    def kinodyn_debug_workspace(self, B):
        """landing_debug_kd_workspace: the blocks of the first B members of the last refinement solve as a host array [B, stride] (the caller has
        synchronised with that solve -- the host entry point has).  Slice a row with kinodyn_workspace_layout()."""
        ptr = C.c_void_p(); st = C.c_ulonglong(); n = C.c_int(); nb = C.c_int()
        fn = self.L.lib.landing_debug_kd_workspace
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ulonglong), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self.L._check(fn(self.L.ctx, C.byref(ptr), C.byref(st), C.byref(n), C.byref(nb)), "landing_debug_kd_workspace")
        if B > nb.value:
            raise ValueError("the last refinement solve had %d member blocks" % nb.value)
        out = np.empty((B, st.value))
        if hasattr(self.L.lib, "landing_emu_set_fused"):      # host emulation: the workspace is host memory
            C.memmove(out.ctypes.data, ptr.value, out.nbytes)
        else:
            from .capi import _hip_runtime
            hip = _hip_runtime()
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            rc = hip.hipMemcpy(out.ctypes.data, ptr.value, out.nbytes, 2)      # hipMemcpyDeviceToHost
            if rc != 0:
                raise RuntimeError("hipMemcpy of the refinement solver's workspace failed (%d)" % rc)
        return out, n.value

    def kinodyn_debug_state(self, member):
        """landing_debug_kd_state: the member's iteration scalars after the last refinement solve, dict by KD_STATE"""
        out = (C.c_double * len(self.KD_STATE))()
        fn = self.L.lib.landing_debug_kd_state
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        self.L._check(fn(self.L.ctx, member, out), "landing_debug_kd_state")
        return dict(zip(self.KD_STATE, out))

    def leg_ik(self, npts, d_q6, d_c, d_jpos, d_res=0, iters=12, jmin=None, jmax=None, stream=0):
        jmin = np.ascontiguousarray(JPOS_MIN[:3] if jmin is None else jmin, float); jmax = np.ascontiguousarray(JPOS_MAX[:3] if jmax is None else jmax, float)
        dp = C.POINTER(C.c_double)
        self.L._check(self.L.lib.landing_leg_ik_batch(self.L.ctx, npts, d_q6, d_c, jmin.ctypes.data_as(dp), jmax.ctypes.data_as(dp), iters, d_jpos, d_res or None, stream or None),
                      "landing_leg_ik_batch")

    def kinodynamic_screen(self, N, x_star, kin_tol=0.01):
        """SRBM solutions x* [B, nx] (device tensor) -> per member: worst FK residual after IK, worst torque ratio |tau| / tau_max and
        whether every stage satisfies the FK band and the torque limits of landing_optimization.m:165-171,186-187"""
        import torch
        B = x_star.shape[0]; nX = 12 * (N + 1); n = B * N
        X = x_star[:, :nX].reshape(B, N + 1, 12); U = x_star[:, nX:].reshape(B, N, 24)
        q6 = X[:, :N, :6].reshape(n, 6).contiguous(); c = U[:, :, :12].reshape(n, 12).contiguous(); f = U[:, :, 12:].reshape(n, 12).contiguous()
        mk = lambda *s: torch.zeros(*s, device=x_star.device, dtype=torch.float64)
        jp, res, tau, err = mk(n, 12), mk(n, 4), mk(n, 12), mk(n, 12)
        st = torch.cuda.current_stream().cuda_stream
        self.leg_ik(n, q6.data_ptr(), c.data_ptr(), jp.data_ptr(), res.data_ptr(), stream=st)
        self.kinodyn_rows(n, q6.data_ptr(), c.data_ptr(), f.data_ptr(), jp.data_ptr(), 0, err.data_ptr(), tau.data_ptr(), stream=st)
        ratio = (tau.abs() / torch.as_tensor(TAU_MAX, device=x_star.device)).reshape(B, N * 12).max(dim=1).values
        fk_bad = err.abs().reshape(B, N * 12).max(dim=1).values
        return dict(jpos=jp.reshape(B, N, 12), fk_err_max=fk_bad, torque_ratio_max=ratio, feasible=(fk_bad <= kin_tol) & (ratio <= 1.0))
