"""TEST INFRASTRUCTURE: the reference's actuator look at a refined trajectory, restated in numpy from its .m files, and the summary / where / ok
rules of include/landing_nlp.h (landing_actuator_audit_batch) written from the header's text.  It shares nothing with the kernels.

utilities_landing/plot_results.m:12-39:
    torque(leg, i)  = J_f{leg}' * (-rpyToRotMat_xyz(rpy_i)' * f_star(leg, i))
    joint_vel(:, 1:N-2) = diff(jpos_star, 1, 2) ./ dt_val(1:N-2)      (N = number of knots there: the last of the N-1 columns stays 0)
    v(:, i) = torque ./ gr ./ (1.5 kt) .* Rm + joint_vel .* gr .* kt * 2
rx / ry / rz: spatial_v2's coordinate rotations; rpyToRotMat_xyz.m:2: R_body_to_world = rx(r)' * ry(p)' * rz(y)';
get_foot_jacobians_mc.m:12-24 with l_1 .. l_4 = 0.062, 0.209, 0.195, 0.004 (:5-8 from get_robot_params.m's hip / knee / foot locations);
model.gr / kt / Rm / tauMax / batteryV: get_robot_model.m:237-242 from get_robot_params.m:109-115."""
import numpy as np

GR = np.array([6.0, 6.0, 9.33])
KT = np.array([0.05, 0.05, 0.05])
RM = np.array([0.173, 0.173, 0.173])
TAU_MAX = GR * 3.0
BATTERY_V = 24.0
L1, L2, L3, L4 = 0.062, 0.209, 0.195, 0.004
SIDE_SIGN = (-1.0, 1.0, -1.0, 1.0)
PRODUCTION_DT = np.array([0.05] + [0.02] * 15 + [0.05, 0.05, 0.1, 0.2])      # landing_optimization.m's grid for N = 20 intervals
SUMMARY = ("tau_ratio", "jvel", "volt", "volt_drive", "power_max", "power_min", "n_over", "n_over_drive")


def rx(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[1, 0, 0], [0, c, s], [0, -s, c]])


def ry(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])


def rz(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])


def rpy_to_rot_xyz(rpy):
    return rx(rpy[0]).T @ ry(rpy[1]).T @ rz(rpy[2]).T


def foot_jacobians(q):
    out = []
    for leg in range(4):
        q1, q2, q3 = q[3 * leg:3 * leg + 3]
        s1, s2, s3 = np.sin(q1), np.sin(q2), np.sin(q3)
        c1, c2, c3 = np.cos(q1), np.cos(q2), np.cos(q3)
        c23 = c2 * c3 - s2 * s3; s23 = s2 * c3 + c2 * s3
        sg = SIDE_SIGN[leg]
        out.append(np.array([[0, L3 * c23 + L2 * c2, L3 * c23],
                             [L3 * c1 * c23 + L2 * c1 * c2 - (L1 + L4) * s1 * sg, -L3 * s1 * s23 - L2 * s1 * s2, -L3 * s1 * s23],
                             [L3 * s1 * c23 + L2 * c2 * s1 + (L1 + L4) * sg * c1, L3 * c1 * s23 + L2 * c1 * s2, L3 * c1 * s23]]))
    return out


def split(N, x):
    """x = [X(:) (12 x (N+1)); jpos(:) (12 x N); U(:) (24 x N)], column-major -> X [12, N+1], jpos [12, N], U [24, N]"""
    nX, nJ = 12 * (N + 1), 12 * N
    return x[:nX].reshape(12, N + 1, order="F"), x[nX:nX + nJ].reshape(12, N, order="F"), x[nX + nJ:].reshape(24, N, order="F")


def pack(X, J, U):
    return np.concatenate([X.flatten(order="F"), J.flatten(order="F"), U.flatten(order="F")])


def actuator_data(N, x, dt, gr=GR, kt=KT, Rm=RM):
    """-> tau, jvel, volt [N, 12] of one member (plot_results.m:12-39; knot-major as the library stores them)"""
    X, jpos, U = split(N, np.asarray(x, float))
    f = U[12:24]
    tau = np.zeros((12, N))
    for i in range(N):
        Rwb = rpy_to_rot_xyz(X[3:6, i]).T
        Jf = foot_jacobians(jpos[:, i])
        for leg in range(4):
            idx = slice(3 * leg, 3 * leg + 3)
            tau[idx, i] = Jf[leg].T @ (-Rwb @ f[idx, i])
    jvel = np.zeros((12, N))
    if N > 1:
        jvel[:, :N - 1] = np.diff(jpos, axis=1) / np.asarray(dt, float)[:N - 1]
    g, k, r = np.tile(gr, 4)[:, None], np.tile(kt, 4)[:, None], np.tile(Rm, 4)[:, None]
    volt = tau / g / (1.5 * k) * r + jvel * g * k * 2.0
    return tau.T.copy(), jvel.T.copy(), volt.T.copy()


def _peak(values, mask):
    """largest value among the masked samples and its flat index, the lowest index among equals; (0, -1) when there is none.  NaN samples are
    left out (no comparison with a NaN holds)."""
    best, at = 0.0, -1
    for i, (v, m) in enumerate(zip(values.reshape(-1), mask.reshape(-1))):
        if m and not np.isnan(v) and (at < 0 or v > best):
            best, at = float(v), i
    return best, at


def summarise(tau, jvel, volt, tau_max=TAU_MAX, battery_v=BATTERY_V):
    """the header's d_summary [8] and d_where [4] of one member"""
    with np.errstate(invalid="ignore"):
        power = tau * jvel
        drive = power > 0
        av = np.abs(volt)
        ratio = np.abs(tau) / np.tile(tau_max, 4)[None, :]
        every = np.ones(av.shape, bool)
        pv, iv = _peak(av, every)
        pd, idr = _peak(av, drive)
        fin = lambda a: a[~np.isnan(a)]
        s = [max(fin(ratio), default=0.0), max(fin(np.abs(jvel)), default=0.0), pv, pd, max(fin(power), default=-np.inf), min(fin(power), default=np.inf),
             float((av > battery_v).sum()), float(((av > battery_v) & drive).sum())]
    w = [iv // 12 if iv >= 0 else -1, iv % 12 if iv >= 0 else -1, idr // 12 if idr >= 0 else -1, idr % 12 if idr >= 0 else -1]
    return np.array(s, float), np.array(w, np.int32)


def is_ok(summary, finite, volt_max=24.0, tau_ratio_max=0.0, jvel_max=0.0, drive_only=1):
    ok = bool(finite)
    if volt_max > 0:
        ok = ok and summary[3 if drive_only else 2] <= volt_max
    if tau_ratio_max > 0:
        ok = ok and summary[0] <= tau_ratio_max
    if jvel_max > 0:
        ok = ok and summary[1] <= jvel_max
    return int(ok)


def audit(N, x, dt, screen=None, gr=GR, kt=KT, Rm=RM, tau_max=TAU_MAX, battery_v=BATTERY_V):
    """batch x [B, 48N+12], dt [N] or [B, N]; screen: dict of volt_max, tau_ratio_max, jvel_max, drive_only (default: the library's default) ->
    dict of tau, jvel, volt [B, N, 12], summary [B, 8], where [B, 4], ok [B]"""
    x = np.atleast_2d(np.asarray(x, float)); dt = np.asarray(dt, float)
    B = x.shape[0]
    out = dict(tau=[], jvel=[], volt=[], summary=[], where=[], ok=[])
    for b in range(B):
        d = dt[b] if dt.ndim == 2 else dt
        with np.errstate(invalid="ignore", divide="ignore"):
            t, v, u = actuator_data(N, x[b], d, gr, kt, Rm)
        s, w = summarise(t, v, u, tau_max, battery_v)
        finite = np.isfinite(x[b]).all() and np.isfinite(d[:N]).all() and np.isfinite(t).all() and np.isfinite(v).all() and np.isfinite(u).all()
        for k, a in zip(("tau", "jvel", "volt", "summary", "where", "ok"), (t, v, u, s, w, is_ok(s, finite, **(screen or {})))):
            out[k].append(a)
    return {k: np.array(v, np.int32 if k in ("where", "ok") else float) for k, v in out.items()}


# ---- the inputs the CPU and GPU tests share ----------------------------------------------------------------------------------------------------
STORED = ("a", "b", "m", "g", "kd0", "kd1", "kd2")


def stored_solutions(golden):
    """the seven refined trajectories kept as fixtures (N = 20), in the order of STORED -> x [7, 972]: n1_kinodyn_solutions a / b, n1_kinodyn_multipliers
    m (the reference's production prevSoln) / g, the three members of n1_kd_solved"""
    import os
    rows = []
    for name, tags in (("n1_kinodyn_solutions.npz", "ab"), ("n1_kinodyn_multipliers.npz", "mg")):
        with np.load(os.path.join(golden, name)) as d:
            rows += [pack(d["X_" + t], d["J_" + t], d["U_" + t]) for t in tags]
    with np.load(os.path.join(golden, "n1_kd_solved.npz")) as d:
        rows += list(d["x"])
    return np.array(rows)


def random_states(N, B, seed):
    """B random members: pitch up to +-60 deg, roll / yaw up to +-30 deg, different joint angles on every leg inside the joint limits, forces of both
    signs -> x [B, 48N+12]"""
    rng = np.random.default_rng(seed)
    xs = []
    for _ in range(B):
        X = rng.normal(size=(12, N + 1))
        X[3] = rng.uniform(-np.pi / 6, np.pi / 6, N + 1); X[4] = rng.uniform(-np.pi / 3, np.pi / 3, N + 1); X[5] = rng.uniform(-np.pi / 6, np.pi / 6, N + 1)
        lo, hi = np.tile([-np.pi / 3, -np.pi / 2, 0.0], 4)[:, None], np.tile([np.pi / 3, np.pi / 2, 3 * np.pi / 4], 4)[:, None]
        J = rng.uniform(lo, hi, size=(12, N))
        U = np.concatenate([rng.normal(size=(12, N)), rng.uniform(-60.0, 120.0, size=(12, N))])
        xs.append(pack(X, J, U))
    return np.array(xs)


def random_dt(N, B, seed):
    """B different non-uniform grids [B, N]"""
    return np.random.default_rng(seed).uniform(0.01, 0.2, size=(B, N))


def assert_matches(got, ref, tol=1e-12):
    """tau / jvel / volt and the summary's values to tol * max(1, |ref|_inf) (the project's function-layer tolerance); counts, where and ok equal"""
    for k in ("tau", "jvel", "volt"):
        if k in got and got[k] is not None:
            err = np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
            assert err <= tol, (k, err)
    gs, rs = got["summary"], ref["summary"]
    for j in range(6):
        fin = np.isfinite(rs[:, j])
        assert np.array_equal(gs[~fin, j], rs[~fin, j]), (SUMMARY[j], gs[:, j], rs[:, j])
        if fin.any():
            err = np.abs(gs[fin, j] - rs[fin, j]).max() / max(1.0, np.abs(rs[fin, j]).max())
            assert err <= tol, (SUMMARY[j], err)
    assert np.array_equal(gs[:, 6:], rs[:, 6:]), (gs[:, 6:], rs[:, 6:])
    assert np.array_equal(got["where"], ref["where"]), (got["where"], ref["where"])
    assert np.array_equal(got["ok"], ref["ok"]), (got["ok"], ref["ok"])
