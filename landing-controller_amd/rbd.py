"""Host side of the floating-base rigid-body routines: the reference's 'quad3D' Mini-Cheetah tree
(utilities_general/dynamics-utilities/get_robot_model.m:134-234 with the 'mc3D' parameters of get_robot_params.m:50-115)
in the compact form the HIP kernels use -- Xtree = plux(E, r), link inertia = (mass, m*com, rotational inertia about the
link origin) -- and the wrappers of the landing_rbd_* / landing_kinodyn_* / landing_pipeline_* / landing_actuator_* entry points (their
signatures and the struct mirrors RbdModel / KinodynParams are declared in capi.py)."""
import ctypes as C

import numpy as np

from . import constants as K
from .capi import (ARGS21, AUDIT_NSUM, ActuatorModel, ActuatorScreen, KinodynParams, PipelineOpts, RbdModel, SolverOpts,
                   _block_to_host, _llp, _n, _p, _pi, _ref, _solve_outputs, matlab_args21)
from .kinodyn import dims as kinodyn_dims


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


class Rbd:
    """binds the three entry points on an existing LandingLib (its context owns the uploaded model)"""

    def __init__(self, lib, model=None):
        """model: an RbdModel to upload instead of quad3d_model() (any tree landing_rbd_set_model takes; include/landing_nlp.h states what needs the quadruped's numbering)"""
        self.L = lib
        self.model = quad3d_model() if model is None else model
        lib._check(lib.lib.landing_rbd_set_model(lib.ctx, C.byref(self.model)), "landing_rbd_set_model")

    def fb_dynamics(self, npts, d_q, d_qd, d_tau=0, d_f_foot=0, d_H=0, d_C=0, d_qdd=0, d_A=0, d_Hinv=0, fd_h=0.0, stream=0):
        """fd_h = 0: exact linearisation (forward-mode tangents of the inverse dynamics); fd_h > 0: central differences with that step"""
        self.L._check(self.L.lib.landing_fb_dynamics_batch(self.L.ctx, npts, d_q, d_qd, _n(d_tau), _n(d_f_foot), _n(d_H), _n(d_C), _n(d_qdd), _n(d_A), _n(d_Hinv), fd_h, _n(stream)),
                      "landing_fb_dynamics_batch")

    def kinodyn_rows(self, npts, d_q6, d_c, d_f, d_jpos, d_fk=0, d_fk_err=0, d_tau=0, stream=0):
        self.L._check(self.L.lib.landing_kinodyn_rows_batch(self.L.ctx, npts, d_q6, _n(d_c), _n(d_f), d_jpos, _n(d_fk), _n(d_fk_err), _n(d_tau), _n(stream)), "landing_kinodyn_rows_batch")

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
        self.L._check(self.L.lib.landing_kinodyn_nlp_eval(self.L.ctx, B, N, d_x, C.byref(prm), _n(d_g), _n(d_jac), _n(stream)), "landing_kinodyn_nlp_eval")

    def kinodyn_nlp_hess(self, B, N, d_x, dt, mass, Ib, Ib_inv, mu, d_lam_g, d_hess, stream=0):
        """Hessian blocks of lam_g' g per interval [B, N, 72, 72] (include/landing_nlp.h)"""
        prm = self._kd_params(N, dt, mass, Ib, Ib_inv, mu)
        self.L._check(self.L.lib.landing_kinodyn_nlp_hess(self.L.ctx, B, N, d_x, C.byref(prm), d_lam_g, d_hess, _n(stream)), "landing_kinodyn_nlp_hess")

    def kinodyn_default_opts(self):
        o = SolverOpts()
        self.L.lib.landing_kinodyn_solver_opts_default(C.byref(o))
        return o

    def kinodyn_warm_opts(self):
        """landing_kinodyn_solver_opts_warm: the re-solve from a previous solution"""
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
        out, ptrs = _solve_outputs(B, nx, ng)
        rc = self.L.lib.landing_kinodyn_solve_batch_host(self.L.ctx, B, N, C.byref(prm), _p(lbg), _p(ubg), _p(cost), _p(x0), _ref(opts), *ptrs)
        self.L._check(rc, "landing_kinodyn_solve_batch_host")
        return out

    def kinodyn_solve_device(self, B, N, d_lbg, d_ubg, d_cost, d_x0, dt, mass, Ib, Ib_inv, mu, opts, d_x, d_f=0, d_lam=0, d_status=0, d_iters=0, d_kkt=0, stream=0):
        prm = self._kd_params(N, dt, mass, Ib, Ib_inv, mu)
        rc = self.L.lib.landing_kinodyn_solve_batch(self.L.ctx, B, N, C.byref(prm), d_lbg, d_ubg, d_cost, d_x0, _ref(opts),
                                                    d_x, _n(d_f), _n(d_lam), _n(d_status), _n(d_iters), _n(d_kkt), _n(stream))
        self.L._check(rc, "landing_kinodyn_solve_batch")

    ARGS24 = ("Xref", "Uref", "dt", "q_min", "q_max", "qd_min", "qd_max", "q_init", "qd_init", "c_init", "q_term_min", "q_term_max", "qd_term_min",
              "qd_term_max", "QN", "x0", "jpos_min", "jpos_max", "kin_box", "mu", "l_leg_max", "mass", "Ib", "Ib_inv")

    def kinodyn_solve_24(self, N, args, opts=None, form=None):
        """landing_solve_kinodyn_24: the reference's 24-argument solver function (generate_landingCtrller_KNITRO.m:373-377), `args` = dict name ->
        MATLAB-shaped array (column-major, batch = last axis; Uref may be None)"""
        keep = [None if args.get(n) is None else np.asfortranarray(np.asarray(args[n], float)) for n in self.ARGS24]
        nx, ng = self.kinodyn_nlp_dims(N)
        B = int(np.asarray(args["x0"]).reshape(nx, -1, order="F").shape[1])
        out, ptrs = _solve_outputs(B, nx, ng)
        rc = self.L.lib.landing_solve_kinodyn_24(self.L.ctx, N, B, _ref(form), *[_p(a) for a in keep], _ref(opts), *ptrs)
        self.L._check(rc, "landing_solve_kinodyn_24")
        return out

    # ---- the drop-state chain: SRBM solve -> refinement -> warm re-solve (include/landing_nlp.h landing_pipeline_*; device pointers are integers) ----
    def pipeline_opts(self):
        """landing_pipeline_opts_default"""
        o = PipelineOpts()
        self.L.lib.landing_pipeline_opts_default(C.byref(o))
        return o

    def kinodyn_pose_device(self, B, d_p, d_x_srbm, d_lbg, d_ubg, d_cost, d_x0, opts=None, stream=0):
        """landing_kinodyn_pose_batch: member b's refinement problem from its SRBM p and x*"""
        self.L._check(self.L.lib.landing_kinodyn_pose_batch(self.L.ctx, B, d_p, d_x_srbm, _ref(opts), d_lbg, d_ubg, d_cost, d_x0,
                                                            _n(stream)), "landing_kinodyn_pose_batch")

    def training_pairs_device(self, B, d_p, d_x_kd, d_status_final, d_in, d_out, d_index, d_count, stream=0):
        """landing_training_pairs_batch: the converged members' training columns, compacted in member order"""
        self.L._check(self.L.lib.landing_training_pairs_batch(self.L.ctx, B, d_p, d_x_kd, d_status_final, d_in, d_out, d_index, d_count, _n(stream)),
                      "landing_training_pairs_batch")

    # ---- actuator audit of refined trajectories (include/landing_nlp.h landing_actuator_*; csrc/actuator_kernels.hip) ----
    def actuator_model(self):
        """landing_actuator_model_mc3d"""
        m = ActuatorModel()
        self.L.lib.landing_actuator_model_mc3d(C.byref(m))
        return m

    def actuator_screen(self, **limits):
        """landing_actuator_screen_default (volt_max = 24, drive_only = 1, the other limits off), fields overridden by keyword"""
        s = ActuatorScreen()
        self.L.lib.landing_actuator_screen_default(C.byref(s))
        for k, v in limits.items():
            if k not in dict(ActuatorScreen._fields_):
                raise TypeError("landing_actuator_screen has no field %r" % k)
            setattr(s, k, v)
        return s

    def actuator_audit_device(self, B, d_dt, dt_stride, d_x_kd, d_summary, d_where, d_ok, model=None, screen=None, d_tau=0, d_jvel=0, d_volt=0, stream=0):
        """landing_actuator_audit_batch: device pointers (integers); d_dt + b * dt_stride is member b's grid (0: one grid for all)"""
        self.L._check(self.L.lib.landing_actuator_audit_batch(self.L.ctx, B, _n(d_dt), dt_stride, _n(d_x_kd), _ref(model), _ref(screen), _n(d_tau), _n(d_jvel), _n(d_volt),
                                                              _n(d_summary), _n(d_where), _n(d_ok), _n(stream)), "landing_actuator_audit_batch")

    def actuator_audit(self, x_kd, dt, model=None, screen=None, full=True):
        """landing_actuator_audit_host: numpy x [B, 48N+12] (the refinement's layout) and dt [N] (one grid) or [B, N] -> dict of summary [B, 8]
        (capi.AUDIT_SUMMARY), where [B, 4], ok [B] and, with full, tau / jvel / volt [B, N, 12]"""
        N = self.L.N
        x = np.ascontiguousarray(np.atleast_2d(x_kd), float); dt = np.ascontiguousarray(dt, float)
        B = x.shape[0]
        assert x.shape == (B, kinodyn_dims(N)[0]) and dt.shape in ((N,), (B, N))
        mk = lambda: np.zeros((B, N, 12)) if full else None
        tau, jvel, volt = mk(), mk(), mk()
        summ, where, ok = np.zeros((B, AUDIT_NSUM)), np.zeros((B, 4), np.int32), np.zeros(B, np.int32)
        rc = self.L.lib.landing_actuator_audit_host(self.L.ctx, B, _p(dt), N if dt.ndim == 2 else 0, _p(x), _ref(model), _ref(screen), _p(tau), _p(jvel), _p(volt), _p(summ),
                                                    _pi(where), _pi(ok))
        self.L._check(rc, "landing_actuator_audit_host")
        out = dict(summary=summ, where=where, ok=ok)
        if full:
            out.update(tau=tau, jvel=jvel, volt=volt)
        return out

    def screened_pairs(self, B, d_p, d_x_kd, d_status3, d_summary, d_where, d_ok, d_in, d_out, d_index, d_count, model=None, screen=None, stream=0):
        """landing_pipeline_screened_pairs_batch: the chain's pair writer behind the screen (device pointers): the members with final status 0 AND ok"""
        self.L._check(self.L.lib.landing_pipeline_screened_pairs_batch(self.L.ctx, B, _n(d_p), _n(d_x_kd), _n(d_status3), _ref(model), _ref(screen), _n(d_summary), _n(d_where),
                                                                       _n(d_ok), _n(d_in), _n(d_out), _n(d_index), _n(d_count), _n(stream)), "landing_pipeline_screened_pairs_batch")

    def pipeline_refine_device(self, B, d_p, d_x_srbm, opts, d_x, d_f, d_status, d_iters, d_kkt, d_lam=0, d_in=0, d_out=0, d_index=0, d_count=0,
                               d_srbm_status=0, d_srbm_iters=0, stream=0):
        """landing_pipeline_refine_batch: pose, refinement, warm re-solve, final choice, pairs behind SRBM solutions already on the device"""
        self.L._check(self.L.lib.landing_pipeline_refine_batch(self.L.ctx, B, d_p, d_x_srbm, _n(d_srbm_status), _n(d_srbm_iters), _ref(opts),
                                                               d_x, d_f, _n(d_lam), d_status, d_iters, d_kkt, _n(d_in), _n(d_out), _n(d_index), _n(d_count), _n(stream)),
                      "landing_pipeline_refine_batch")

    def pipeline_device(self, B, d_p, d_x0, opts, d_x, d_f, d_status, d_iters, d_kkt, d_lam=0, d_in=0, d_out=0, d_index=0, d_count=0, d_x_srbm=0, stream=0):
        """landing_pipeline_batch: the SRBM solve and the chain above on one stream"""
        self.L._check(self.L.lib.landing_pipeline_batch(self.L.ctx, B, d_p, d_x0, _ref(opts), _n(d_x_srbm), d_x, d_f, _n(d_lam),
                                                        d_status, d_iters, d_kkt, _n(d_in), _n(d_out), _n(d_index), _n(d_count), _n(stream)), "landing_pipeline_batch")

    def pipeline_21(self, args, opts=None, want_lam=False):
        """landing_pipeline_21: the 21 MATLAB-shaped SRBM arguments (batch = last axis) -> the refined, re-solved batch and its training pairs (host arrays)"""
        a, keep, B = matlab_args21(self.L.N, args)
        nxk, ngk = kinodyn_dims(self.L.N)
        x = np.zeros((B, nxk)); f = np.zeros(B); lam = np.zeros((B, ngk)) if want_lam else None; st = np.zeros((B, 3), np.int32); it = np.zeros((B, 3), np.int32)
        kkt = np.zeros((B, 3)); pin = np.zeros((B, 9)); pout = np.zeros((B, nxk)); kept = C.c_int(0)
        rc = self.L.lib.landing_pipeline_21(self.L.ctx, B, *[getattr(a, n) for n in ARGS21], _ref(opts), _p(x), _p(f), _p(lam), _pi(st), _pi(it), _p(kkt),
                                            _p(pin), _p(pout), C.byref(kept))
        self.L._check(rc, "landing_pipeline_21")
        m = kept.value
        return dict(x=x, f=f, lam_g=lam, status=st, iters=it, kkt=kkt, pair_in=pin[:m].T.copy(), pair_out=pout[:m].T.copy(), n_kept=m)

    def kinodyn_bounds(self, N, B, q_init, qd_init, c_init, q_min, q_term_min, q_term_max, qd_term_min, qd_term_max, jpos_min, jpos_max, kin_box, l_leg_max):
        """landing_kinodyn_bounds (pure host code): arrays [B, n] -> lbg, ubg [B, ng]"""
        a = [np.ascontiguousarray(v, float) for v in (q_init, qd_init, c_init, q_min, q_term_min, q_term_max, qd_term_min, qd_term_max, jpos_min, jpos_max, kin_box, l_leg_max)]
        ng = kinodyn_dims(N)[1]
        lb = np.zeros((B, ng)); ub = np.zeros((B, ng))
        self.L._check(self.L.lib.landing_kinodyn_bounds(N, B, None, *[_p(v) for v in a], _p(lb), _p(ub)), "landing_kinodyn_bounds")
        return lb, ub

    # ---- CasADi-external face of the kinodynamic NLP (include/landing_nlp.h, round 6): what landingCtrller_KNITRO_mi355x.so forwards to
    def kinodyn_casadi_np(self, N):
        return int(self.L.lib.landing_kinodyn_casadi_np(N))

    def kinodyn_casadi_pattern(self, N, which):
        ci, r, nnz = _llp(), _llp(), C.c_longlong()
        self.L._check(self.L.lib.landing_kinodyn_casadi_pattern(self.L.ctx, N, which, C.byref(ci), C.byref(r), C.byref(nnz)), "landing_kinodyn_casadi_pattern")
        nx = kinodyn_dims(N)[0]
        return np.array(ci[:nx + 1], np.int64), np.array(r[:nnz.value], np.int64)

    def kinodyn_casadi_bounds(self, N, p):
        p = np.ascontiguousarray(p, float); ng = kinodyn_dims(N)[1]
        lb, ub = np.zeros(ng), np.zeros(ng)
        self.L._check(self.L.lib.landing_kinodyn_casadi_bounds(N, None, _p(p), _p(lb), _p(ub)), "landing_kinodyn_casadi_bounds")
        return lb, ub

    def kinodyn_casadi_eval(self, N, x, p, lam_f=1.0, lam_g=None, want=("f", "g", "grad_f", "jac", "hess", "ggx", "ggp")):
        """landing_kinodyn_casadi_eval_host: one problem, host arrays; returns a dict of the requested outputs (jac / hess as CCS nonzeros)"""
        (nx, ng), npar = kinodyn_dims(N), self.kinodyn_casadi_np(N)
        x = np.ascontiguousarray(x, float); p = np.ascontiguousarray(p, float)
        assert x.shape == (nx,) and p.shape == (npar,)
        nj, nh = (len(self.kinodyn_casadi_pattern(N, w)[1]) for w in (0, 1))
        size = dict(f=1, g=ng, grad_f=nx, jac=nj, hess=nh, ggx=nx, ggp=npar)
        out = {k: np.zeros(size[k]) for k in want}
        lf = C.c_double(lam_f)
        lg = np.ascontiguousarray(lam_g, float) if lam_g is not None else None
        self.L._check(self.L.lib.landing_kinodyn_casadi_eval_host(self.L.ctx, N, _p(x), _p(p), C.byref(lf), _p(lg),
                                                                  *[_p(out.get(k)) for k in ("f", "g", "grad_f", "jac", "hess", "ggx", "ggp")]), "landing_kinodyn_casadi_eval_host")
        if "f" in out:
            out["f"] = float(out["f"][0])
        return out

    def kinodyn_pattern(self, N, which):
        """landing_kinodyn_pattern: CCS (colind, row) of jac_g_x (which = 0) or triu(hess_gamma_x_x) (which = 1)"""
        colind = np.zeros(kinodyn_dims(N)[0] + 1, np.int64); nnz = C.c_longlong()
        fn = self.L.lib.landing_kinodyn_pattern
        self.L._check(fn(self.L.ctx, N, which, colind.ctypes.data_as(_llp), None, C.byref(nnz)), "landing_kinodyn_pattern")
        row = np.zeros(nnz.value, np.int64)
        self.L._check(fn(self.L.ctx, N, which, colind.ctypes.data_as(_llp), row.ctypes.data_as(_llp), C.byref(nnz)), "landing_kinodyn_pattern")
        return colind, row

    def kinodyn_block_nonzeros(self):
        """landing_kinodyn_block_nonzeros: the solver's table of the structural non-zeros of a Jacobian block's inequality rows -> ((rows, cols) of a middle interval,
        (rows, cols) of the last one); rows count from the top of the 141 x 72 block"""
        n0, n1 = C.c_int(), C.c_int(); buf = np.zeros(2 * 1280, np.uint8)
        self.L._check(self.L.lib.landing_kinodyn_block_nonzeros(self.L.ctx, C.byref(n0), C.byref(n1), buf.ctypes.data_as(C.POINTER(C.c_ubyte))), "landing_kinodyn_block_nonzeros")
        e = buf[:2 * (n0.value + n1.value)].reshape(-1, 2).astype(int)
        return (e[:n0.value, 0], e[:n0.value, 1]), (e[n0.value:, 0], e[n0.value:, 1])

    # ---- diagnostics: the workspace the refinement solve leaves behind (include/landing_nlp.h landing_debug_kd_*) ----
    KD_LAYOUT = ("x", "dx", "g", "s", "ds", "zL", "zU", "y", "yn", "sig", "rho", "gc", "en", "ep", "wn", "wp")
    KD_STATE = ("mu", "delta", "delta_last", "alpha", "a_du", "it", "nfact", "nreset", "last_reset_it", "feas", "status", "pending", "omt", "s_corr", "done", "reg_it")
    KD_GC = 60 * 60 + 60

    def kinodyn_workspace_layout(self, N):
        """landing_debug_kd_layout: dict name -> (offset, length) in doubles inside a member's block, plus "state" -> offset of the iteration state and
        "total" -> the member stride"""
        off = (C.c_ulonglong * len(self.KD_LAYOUT))(); so = C.c_ulonglong(); st = C.c_ulonglong()
        self.L._check(self.L.lib.landing_debug_kd_layout(N, off, C.byref(so), C.byref(st)), "landing_debug_kd_layout")
        nx, ng = kinodyn_dims(N)
        size = dict(x=nx, dx=nx, gc=N * self.KD_GC)
        out = {n: (int(o), size.get(n, ng)) for n, o in zip(self.KD_LAYOUT, off)}
        out["state"] = int(so.value); out["total"] = int(st.value)
        return out

    def kinodyn_debug_workspace(self, B):
        """landing_debug_kd_workspace: the blocks of the first B members of the last refinement solve as a host array [B, stride] (the caller has
        synchronised with that solve -- the host entry point has).  Slice a row with kinodyn_workspace_layout()."""
        ptr = C.c_void_p(); st = C.c_ulonglong(); n = C.c_int(); nb = C.c_int()
        self.L._check(self.L.lib.landing_debug_kd_workspace(self.L.ctx, C.byref(ptr), C.byref(st), C.byref(n), C.byref(nb)), "landing_debug_kd_workspace")
        if B > nb.value:
            raise ValueError("the last refinement solve had %d member blocks" % nb.value)
        out = _block_to_host(self.L.lib, ptr.value, (B, st.value), "the refinement solver's workspace")
        return out, n.value

    def kinodyn_debug_state(self, member):
        """landing_debug_kd_state: the member's iteration scalars after the last refinement solve, dict by KD_STATE"""
        out = (C.c_double * len(self.KD_STATE))()
        self.L._check(self.L.lib.landing_debug_kd_state(self.L.ctx, member, out), "landing_debug_kd_state")
        return dict(zip(self.KD_STATE, out))

    def leg_ik(self, npts, d_q6, d_c, d_jpos, d_res=0, iters=12, jmin=None, jmax=None, stream=0):
        jmin = np.ascontiguousarray(JPOS_MIN[:3] if jmin is None else jmin, float); jmax = np.ascontiguousarray(JPOS_MAX[:3] if jmax is None else jmax, float)
        self.L._check(self.L.lib.landing_leg_ik_batch(self.L.ctx, npts, d_q6, d_c, _p(jmin), _p(jmax), iters, d_jpos, _n(d_res), _n(stream)),
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
