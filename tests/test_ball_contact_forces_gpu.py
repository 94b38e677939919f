"""Contact forces of the ball scene on the GPU (`tacex_fem_ball_contact_forces` -> `UipcSim.contact_forces` -> `BallContactForces` ->
`VisionTactileSensorUIPC.contact_wrench`) against the NumPy reference of tests/ball_contact_forces_ref.py, which is built from the pieces of
oracle/abd_oracle.py alone: every term at once, a mollified edge-edge pair, no contact, the solver's balance after real steps, batch
independence, reset / kinematic body / refusals / list overflow, and the sensor's camera frame."""
import numpy as np
import pytest
import torch

import ball_contact_forces_ref as R

pytestmark = pytest.mark.gpu

REFP = np.array([[0.001, 0.002, 0.02], [-0.002, 0.001, 0.015], [0.0, 0.0, 0.0], [0.003, -0.001, 0.01]])
FRIC_SLOTS = [3, 4, 5, 32, 33, 38, 39]
NORMAL_SLOTS = [0, 1, 2, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 34, 35, 36, 37, 40, 41, 42]


def _y(sim, b):
    return np.concatenate([sim.x[b].cpu().numpy(), sim.q[b].cpu().numpy()], 0)


def _dev(ys, V):
    x = torch.from_numpy(np.stack([y[:V] for y in ys])).cuda()
    q = torch.from_numpy(np.stack([y[V:] for y in ys])).cuda()
    return x, q


def _vertex_check(vf, out, what):
    scale = max(np.abs(out["record"][R.FORCE_SLOTS]).max(), np.abs(out["vertex"]).max())
    err = np.abs(vf - out["vertex"]).max()
    print(f"{what}: per-vertex forces max |diff| {err:.3e} of largest force entry {scale:.3e}")
    assert err <= 1e-9 * scale, (what, err, scale)


def test_every_term_vs_reference():
    """Pairs of all three kinds, the ground under the ball, sticking (env 0) and slipping (env 1) lagged friction of every contact, previous
    states handed over explicitly: every force slot and the per-vertex forces to 1e-9 of the largest force entry, counts and flags exact,
    distances to 1e-12; `friction=False` leaves the normal slots alone and zeroes the friction slots."""
    sim, sc, cons, back = R.build()
    V = sc.V
    ys, yps = zip(*[R.issue_states(_y(sim, b), b) for b in range(2)])
    x, q = _dev(ys, V)
    xp, qp = _dev(yps, V)
    refp = torch.from_numpy(REFP[:2]).cuda()
    w = sim._ball_contact_forces(x, q, refp, True, True, xp, qp)
    w0 = sim.contact_forces(x=x, q=q, ref_points=refp, per_vertex=True, friction=False)
    rec, rec0, vf, vf0 = w.record.cpu().numpy(), w0.record.cpu().numpy(), w.vertex_forces.cpu().numpy(), w0.vertex_forces.cpu().numpy()
    eps = sc.eps_v * sc.dt
    for b in range(2):
        out = R.ball_forces_ref(sc, ys[b], lag_state=yps[b], ref=REFP[b])
        assert (out["record"][16:19] >= 1).all() and out["record"][36] >= 1 and len(out["slid"]) > 0  # three kinds, the ground, lagged contacts
        assert (out["slid"] < eps).any() if b == 0 else (out["slid"] > eps).any()                     # both friction branches
        R.compare(rec[b], out["record"], 1e-9, f"env {b}")
        _vertex_check(vf[b], out, f"env {b}")
        out0 = R.ball_forces_ref(sc, ys[b], ref=REFP[b])
        R.compare(rec0[b], out0["record"], 1e-9, f"env {b}, friction=False")
        _vertex_check(vf0[b], out0, f"env {b}, friction=False")
        assert np.all(rec0[b, FRIC_SLOTS] == 0.0) and np.abs(rec[b, FRIC_SLOTS]).max() > 0.0
        scale = np.abs(out["record"][R.FORCE_SLOTS]).max()
        assert np.allclose(rec0[b, NORMAL_SLOTS], rec[b, NORMAL_SLOTS], rtol=1e-12, atol=1e-12 * scale)
    # the body's torque about p, from the reference's forces on the surface points' rows: sum_k c_k x G_k
    for b in range(2):
        tot = sum(R.ball_forces_ref(sc, ys[b], lag_state=yps[b], ref=REFP[b])[k] for k in ("barrier", "ground", "friction_pairs", "friction_ground"))
        tq = np.cross(ys[b][V + 1:], tot[V + 1:]).sum(0)
        assert np.abs(w.body_torque[b].cpu().numpy() - tq).max() <= 1e-9 * np.abs(tq).max()
        assert np.abs(w.body_force[b].cpu().numpy() - tot[V]).max() <= 1e-9 * np.abs(tot[V]).max()


def test_mollified_edge_edge_pair_and_switch():
    """A pad edge laid nearly parallel over a ball edge (the construction of tests/test_fem_ball_gpu.py): the pair is mollified (m < 1), its
    own gradient term is part of the forces; with `tacex_fem_set_edge_edge(ctx, 0)` no kind-2 pair is counted and the record is the
    reference's without that kind."""
    from tacex_amd import _lib

    sim, sc, cons, back = R.build(press=3.5e-4)
    V = sc.V
    y = [_y(sim, b) for b in range(2)]
    ee = sc.pairs(y[0])[2]
    assert len(ee[0]) > 0
    k = int(np.argmin(ee[3]))
    pe, be = sc.pad_edges[ee[0][k]], sc.ball_edges[ee[1][k]]
    xb = sc.ball.points(y[0][V:])
    e2 = xb[be[1]] - xb[be[0]]
    u2 = e2 / np.linalg.norm(e2)
    nn = ee[4][k] - (ee[4][k] @ u2) * u2
    nn /= np.linalg.norm(nn)
    mid = xb[be[0]] + 0.5 * e2 + 0.4 * sc.dhat * nn
    L = np.linalg.norm(y[0][pe[1]] - y[0][pe[0]])
    skew = 0.01 * L * np.cross(u2, nn)
    y[0][pe[0]] = mid - 0.3 * L * u2 - skew
    y[0][pe[1]] = mid + 0.3 * L * u2 + skew
    yp = [yy.copy() for yy in y]
    for b in range(2):
        yp[b][V] += np.array([2e-6, -1e-6, 0.0])  # (the body slid: the mollified pair's friction carries its mollifier in lam)
    x, q = _dev(y, V)
    xp, qp = _dev(yp, V)
    refp = torch.from_numpy(REFP[:2]).cuda()
    out = [R.ball_forces_ref(sc, y[b], lag_state=yp[b], ref=REFP[b]) for b in range(2)]
    assert (out[0]["mol"][out[0]["active"]] < 1.0).any() and sc._pair_rows(y[0])[6] is not None
    w = sim._ball_contact_forces(x, q, refp, True, True, xp, qp)
    for b in range(2):
        R.compare(w.record[b].cpu().numpy(), out[b]["record"], 1e-9, f"mollified, env {b}")
        _vertex_check(w.vertex_forces[b].cpu().numpy(), out[b], f"mollified, env {b}")
    assert out[0]["record"][18] >= 1
    _lib.check(sim._lib.tacex_fem_set_edge_edge(sim._handle, 0), "tacex_fem_set_edge_edge")
    sc.edge_edge = False
    w = sim._ball_contact_forces(x, q, refp, True, True, xp, qp)
    for b in range(2):
        o = R.ball_forces_ref(sc, y[b], lag_state=yp[b], ref=REFP[b])
        assert float(w.record[b, 18]) == 0.0 and o["record"][18] == 0
        R.compare(w.record[b].cpu().numpy(), o["record"], 1e-9, f"edge-edge off, env {b}")
        _vertex_check(w.vertex_forces[b].cpu().numpy(), o, f"edge-edge off, env {b}")
    assert np.abs(w.record[0].cpu().numpy()[:3] - out[0]["record"][:3]).max() > 1e-6 * np.abs(out[0]["record"][:3]).max()  # the kind mattered


def test_no_contact_reports_zeros():
    """The pad lifted 2 d_hat beyond the ball's zone, the ball above the ground's: every force slot zero, counts 0, the smallest distances
    +inf, the centre of pressure = the reference points handed in."""
    sim, sc, cons, back = R.build(press=-1e-3, ground_gap=1.5)
    refp = torch.from_numpy(REFP[:2]).cuda()
    w = sim.contact_forces(ref_points=refp, per_vertex=True)
    rec = w.record.cpu().numpy()
    assert np.all(rec[:, [k for k in R.FORCE_SLOTS if not 12 <= k <= 14]] == 0.0) and np.all(rec[:, R.COUNT_SLOTS] == 0.0)
    assert np.all(np.isposinf(rec[:, R.DIST_SLOTS])) and np.array_equal(rec[:, 12:15], REFP[:2])
    assert float(w.vertex_forces.abs().max()) == 0.0
    for b in range(2):
        R.compare(rec[b], R.ball_forces_ref(sc, _y(sim, b), ref=REFP[b])["record"], 1e-9, f"no contact, env {b}")


def test_after_real_steps_the_record_is_what_the_solver_balanced():
    """`FemBallScene` solved tightly (the configuration of tests/test_fem_ball_gpu.py's stationarity test): after a step, dt^2 times the
    body's generalised contact force from `contact_forces()` - friction from the step's workspace, no explicit previous state - equals the
    body rows' remainder S (q - q~) + dt^2 ortho'(q) (inertia and orthogonality alone, no pair code) to 1e-5 of the largest pair force; and
    the record is the reference's with the lag of the state the step started from, to 1e-9."""
    from oracle.abd_oracle import AffineBody, BallScene
    from oracle.fem_oracle import FemModel
    from tacex_amd.uipc.gelpad_scene import FemBallScene
    from tacex_amd.uipc.uipc_sim import UipcSimCfg

    cfg = UipcSimCfg(device="cuda:0")
    cfg.newton.velocity_tol, cfg.newton.transrate_tol, cfg.linear_system.tol_rate, cfg.linear_system.max_iter = 1e-7, 1e-6, 1e-12, 4000
    t = FemBallScene(2, "cuda:0", max_newton_iter=200, cfg=cfg, ball_density=1e5)
    sim, pad, ball = t.sim, t.gelpad, t.ball
    with pytest.raises(ValueError):
        sim.contact_forces(friction=True)  # no step yet: nothing to take the lag from
    m = FemModel.build(pad.points, pad.tets, youngs=pad.cfg.constitution_cfg.youngs_modulus * 1e6, poisson=pad.cfg.constitution_cfg.poisson_rate,
                       density=pad.cfg.mass_density, dt=cfg.dt, strength=1000.0)
    osc = BallScene(m, pad.surface_triangles(), pad.surface_vertex_areas(), AffineBody(ball.points, ball.tris, density=1e5), dhat=cfg.contact.d_hat,
                    ground_height=cfg.ground_height, resistance=cfg.contact.default_contact_resistance)
    osc.mu, osc.eps_v = cfg.contact.default_friction_ratio, cfg.contact.eps_velocity
    V, dt = osc.V, cfg.dt
    worst, checked = 0.0, 0
    for i in range(10):
        y_n = [_y(sim, b) for b in range(2)]
        qv_n = sim.qv.cpu().numpy()
        t.step(i)
        info = sim.check_step()
        assert info["newton_iters"].max() < 200 and int(sim.step_info[:, 2].max()) == 0, (i, info)
        w = t.contact_forces(per_vertex=True)
        rec = w.record.cpu().numpy()
        for b in range(2):
            y = _y(sim, b)
            out = R.ball_forces_ref(osc, y, lag_state=y_n[b])
            R.compare(rec[b], out["record"], 1e-9, f"step {i}, env {b}")
            _vertex_check(w.vertex_forces[b].cpu().numpy(), out, f"step {i}, env {b}")
            qt = y_n[b][V:] + dt * qv_n[b]
            qt[0] += dt**2 * np.asarray(cfg.gravity)
            rem = osc.ball.S @ (y[V:] - qt) + dt**2 * osc.ball.ortho(y[V:])[1]
            lams = _pair_lams(osc, y)
            scale = dt**2 * np.abs(lams).max() if len(lams) else 0.0
            err = np.abs(dt**2 * rec[b, 20:32].reshape(4, 3) - rem).max()
            print(f"step {i}, env {b}: |dt^2 G - remainder| {err:.3e}, largest pair force x dt^2 {scale:.3e}, pairs {rec[b, 10]:.0f}, lagged friction |f| {np.abs(rec[b, 3:6]).max():.3e}")
            if scale < 1e-6:  # (a pair that has only just entered the zone pushes with less than the round-off of the pad's elastic forces)
                continue
            checked += 1
            worst = max(worst, err / scale)
            assert err <= 1e-5 * scale, (i, b, err, scale)
        if checked >= 4:
            break
    assert checked >= 2
    print(f"worst |dt^2 G - remainder| / pair force: {worst:.2e}")


def _pair_lams(osc, y):
    from oracle.fem_oracle import barrier

    _, _, w, d, _, mol, _ = osc._pair_rows(y)
    return osc.kappa * w * mol * barrier(d / osc.dhat)[1] / osc.dhat


def test_batch_independence_and_state_arguments():
    """Four different states in one batch of four = four batches of one, to 1e-12 of the largest force (list slots are handed out with
    atomics: round-off, not bits), counts exact; `contact_forces(x=sim.x, q=sim.q)` is `contact_forces()`."""
    sim, sc, cons, back = R.build(B=4)
    V = sc.V
    rest = _y(sim, 0)
    ys, yps = [], []
    for b in range(4):
        y, yp = R.issue_states(rest, b % 2)
        if b >= 2:
            rng = np.random.default_rng(20 + b)
            y = y + 1e-5 * rng.standard_normal(y.shape)
            yp = yp + 1e-5 * rng.standard_normal(y.shape)
        ys.append(y); yps.append(yp)
    x, q = _dev(ys, V)
    xp, qp = _dev(yps, V)
    refp = torch.from_numpy(REFP).cuda()
    w = sim._ball_contact_forces(x, q, refp, True, True, xp, qp)
    rec = w.record.cpu().numpy()
    assert len({tuple(r[:3]) for r in rec}) == 4 and np.all(rec[:, 10] > 0)
    for b in range(4):
        one = sim._ball_contact_forces(x[b:b + 1], q[b:b + 1], refp[b:b + 1], True, True, xp[b:b + 1], qp[b:b + 1])
        r1 = one.record[0].cpu().numpy()
        scale = np.abs(rec[b, R.FORCE_SLOTS]).max()
        err = np.abs(r1[R.FORCE_SLOTS] - rec[b, R.FORCE_SLOTS]).max()
        print(f"env {b}: batch of four vs batch of one {err / scale:.2e} of the largest force")
        assert err <= 1e-12 * scale
        assert np.array_equal(r1[R.COUNT_SLOTS], rec[b, R.COUNT_SLOTS]) and np.allclose(r1[R.DIST_SLOTS], rec[b, R.DIST_SLOTS], rtol=1e-12, atol=0)
        assert float((one.vertex_forces[0] - w.vertex_forces[b]).abs().max()) <= 1e-12 * scale
    a, c = sim.contact_forces(per_vertex=True), sim.contact_forces(x=sim.x, q=sim.q, per_vertex=True)
    scale = float(a.record[:, R.FORCE_SLOTS].abs().max())
    assert scale > 0 and float((a.record - c.record)[:, R.FORCE_SLOTS].abs().max()) <= 1e-12 * scale
    assert float((a.vertex_forces - c.vertex_forces).abs().max()) <= 1e-12 * scale


def test_reset_clears_the_friction_reference_of_the_env():
    """After `sim.reset([1])` env 1 reports zero friction and the reference's normal part at the reset state, env 0 is unchanged; after the
    next step env 1 reports friction again.  The scene starts with the pad's face and the ground just inside the barrier zones (0.98 d_hat),
    so the reset state has contacts and the step that follows has lagged ones."""
    sim, sc, cons, back = R.build(press=1e-5, ground_gap=0.98)
    for _ in range(2):
        sim.step(max_newton_iter=64)
    assert torch.isfinite(sim.x).all() and torch.isfinite(sim.q).all()
    wa = sim.contact_forces()
    ra = wa.record.cpu().numpy()
    assert np.abs(ra[:, FRIC_SLOTS]).max(1).min() > 0.0  # both envs report friction (friction=None: the cfg's, after a step)
    sim.reset([1])
    wb = sim.contact_forces(friction=True)
    rb = wb.record.cpu().numpy()
    assert np.all(rb[1, FRIC_SLOTS] == 0.0)
    out = R.ball_forces_ref(sc, _y(sim, 1))
    assert out["record"][10] > 0 and out["record"][36] > 0
    R.compare(rb[1], out["record"], 1e-9, "reset env")
    scale = np.abs(ra[0, R.FORCE_SLOTS]).max()
    assert np.abs(rb[0, R.FORCE_SLOTS] - ra[0, R.FORCE_SLOTS]).max() <= 1e-12 * scale and np.array_equal(rb[0, R.COUNT_SLOTS], ra[0, R.COUNT_SLOTS])
    y_n = _y(sim, 1)
    sim.step(max_newton_iter=64)
    rc = sim.contact_forces().record.cpu().numpy()
    assert np.abs(rc[1, FRIC_SLOTS]).max() > 0.0
    R.compare(rc[1], R.ball_forces_ref(sc, _y(sim, 1), lag_state=y_n)["record"], 1e-9, "reset env, one step later")


def test_kinematic_body_follows_the_steps_rule():
    """The scene of `test_kinematic_body_is_fixed_within_a_step_and_dents_the_pad`, the caller lifting the ball and moving it sideways before
    each of two steps: the reported friction is what the second step balanced - the lag taken against the body where that step had it, the
    pad rows sliding from the step's start positions, the body rows from where the body stood when the FIRST step ended - so the record is
    the reference's with that lag and sliding reference; the pad is pushed upward, more where the ball rose further.  Moving the body after
    the step adds that motion to the sliding."""
    sim, sc, cons, back = R.build(press=-1e-5, ground_gap=4.0, shift=(0.0008, 0.0005), kinematic=True)
    lift = torch.tensor([1.0, 0.5], device="cuda", dtype=torch.float64)
    for k in range(2):
        q_last = sim.q.cpu().numpy().copy()  # where the body stood when the previous step ended
        sim.q[:, 0, 2] += 1e-4 * lift
        sim.q[:, 0, 0] += 4e-6 * lift
        sim.q[:, 0, 1] -= 2e-6
        x_n = sim.x.cpu().numpy().copy()
        sim.step(max_newton_iter=64)
    info = sim.check_step()
    assert len(info["line_search_failed_envs"]) == 0 and info["newton_iters"].max() < 64, info
    w = sim.contact_forces(per_vertex=True)
    rec = w.record.cpu().numpy()
    qn = sim.q.cpu().numpy()
    lag = [np.concatenate([x_n[b], qn[b]], 0) for b in range(2)]       # (a kinematic body does not move in the step: q of the step = q now)
    slide = [np.concatenate([x_n[b], q_last[b]], 0) for b in range(2)]
    for b in range(2):
        out = R.ball_forces_ref(sc, _y(sim, b), lag_state=lag[b], slide_ref=slide[b])
        still = R.ball_forces_ref(sc, _y(sim, b), lag_state=lag[b])
        assert out["record"][10] > 0 and np.abs(out["record"][3:6] - still["record"][3:6]).max() > 1e-6 * np.abs(out["record"][3:6]).max()  # the body's motion is in the friction
        R.compare(rec[b], out["record"], 1e-9, f"kinematic, env {b}")
        _vertex_check(w.vertex_forces[b].cpu().numpy(), out, f"kinematic, env {b}")
    f = w.force.cpu().numpy()
    assert f[0, 2] > f[1, 2] > 0.0, f
    q_moved = sim.q.clone()
    q_moved[:, 0, 0] += 2e-6
    q_moved[:, 0, 1] -= 1e-6
    w2 = sim.contact_forces(q=q_moved)
    for b in range(2):
        y = np.concatenate([sim.x[b].cpu().numpy(), q_moved[b].cpu().numpy()], 0)
        R.compare(w2.record[b].cpu().numpy(), R.ball_forces_ref(sc, y, lag_state=lag[b], slide_ref=slide[b])["record"], 1e-9, f"kinematic, body moved, env {b}")
    assert float((w2.record[:, 3:6] - w.record[:, 3:6]).abs().max()) > 0.0


def test_refusals():
    """Refused with the documented error: friction before any step, friction for fewer envs than the step had, the C call without previous
    states or the step's workspace, one previous state alone, a context without a body (whose own call names this one)."""
    from tacex_amd import _lib
    from tacex_amd.uipc import UipcObject, UipcObjectCfg, UipcSim, UipcSimCfg
    from tacex_amd.uipc.uipc_object import gelpad_box_mesh

    sim, sc, cons, back = R.build(press=-2e-5, ground_gap=1.02)
    lib, h = sim._lib, sim._handle
    with pytest.raises(ValueError, match="after a step"):
        sim.contact_forces(friction=True)
    rec = torch.empty((2, 44), dtype=torch.float64, device="cuda")
    args = lambda ws, xp, qp, fr, B: (h, _lib.ptr(sim.x), _lib.ptr(sim.q), ws, xp, qp, 0, fr, _lib.ptr(rec), 0, B, sim._stream())  # noqa: E731
    assert lib.tacex_fem_ball_contact_forces(*args(_lib.ptr(sim._ball_ws), 0, 0, 1, 2)) == 2 and b"last tacex_fem_ball_step" in lib.tacex_last_error()
    assert lib.tacex_fem_ball_contact_forces(*args(0, 0, 0, 1, 2)) == 2
    assert lib.tacex_fem_ball_contact_forces(*args(0, _lib.ptr(sim.x), 0, 1, 2)) == 2 and b"go together" in lib.tacex_last_error()
    assert lib.tacex_fem_ball_contact_forces(*args(0, 0, 0, 0, 2)) == 0  # without friction nothing else is needed
    sim.step(max_newton_iter=64)
    assert lib.tacex_fem_ball_contact_forces(*args(_lib.ptr(sim._ball_ws), 0, 0, 1, 2)) == 0
    assert lib.tacex_fem_ball_contact_forces(*args(_lib.ptr(sim._ball_ws), 0, 0, 1, 1)) == 2 and b"last tacex_fem_ball_step" in lib.tacex_last_error()
    with pytest.raises(ValueError, match="after a step"):
        sim.contact_forces(x=sim.x[:1], q=sim.q[:1], friction=True)
    assert tuple(sim.contact_forces(x=sim.x[:1], q=sim.q[:1]).record.shape) == (1, 44)  # (friction=None: off for fewer envs)
    torch.cuda.synchronize()
    # a context without a body
    P, T = gelpad_box_mesh(4, 5, 2)
    plain = UipcSim(UipcSimCfg(device="cuda:0"), num_envs=1)
    UipcObject(UipcObjectCfg(mesh_points=P, mesh_tets=T), plain)
    plain.setup_sim()
    q1 = torch.zeros((1, 4, 3), dtype=torch.float64, device="cuda")
    r1 = torch.empty((1, 44), dtype=torch.float64, device="cuda")
    assert lib.tacex_fem_ball_contact_forces(plain._handle, _lib.ptr(plain.x), _lib.ptr(q1), 0, 0, 0, 0, 0, _lib.ptr(r1), 0, 1, plain._stream()) == 2
    assert b"no affine body" in lib.tacex_last_error()
    r16 = torch.empty((2, 16), dtype=torch.float64, device="cuda")
    assert lib.tacex_fem_contact_forces(h, _lib.ptr(sim.x), 0, 0, 0, _lib.ptr(r16), 0, 2, sim._stream()) == 2
    assert b"tacex_fem_ball_contact_forces" in lib.tacex_last_error()


def test_candidate_list_overflow_is_flagged_and_finite():
    """The scene of `test_candidate_list_overflow_is_flagged_not_fatal` (a barrier zone of 6 mm around a level-3 ball, two steps).  The step
    lists candidates at 2.8 d_hat and overflows there; this kernel culls at d_hat, where the scene's own states hold a few dozen candidates
    (flags 0).  With the ball lifted by 0.8 d_hat into the pad's zone (gap 0.22 d_hat, no penetration) 570 of its 1920 edges fall inside the
    candidates' box: the list of 512 clamps, the record's flag slot is 16 in every env, everything stays finite, nothing is written behind
    the outputs."""
    from tacex_amd.uipc.gelpad_scene import FemBallScene

    sc = FemBallScene(3, "cuda:0", max_newton_iter=3, level=3, d_hat=6e-3)
    for i in range(2):
        sc.step(i)
    assert torch.equal(sc.contact_forces().flags, torch.zeros(3, dtype=torch.float64, device="cuda:0"))
    q = sc.sim.q.clone()
    q[:, 0, 2] += 0.8 * 6e-3
    guard = torch.full((4096,), 7.25, dtype=torch.float64, device="cuda:0")
    w = sc.contact_forces(q=q, per_vertex=True)
    w2 = sc.contact_forces(q=q, per_vertex=True)
    torch.cuda.synchronize()
    for r in (w, w2):
        assert torch.equal(r.flags, torch.full((3,), 16.0, dtype=torch.float64, device="cuda:0"))
        assert torch.isfinite(r.record[:, :37]).all() and torch.isfinite(r.record[:, 38:42]).all() and torch.isfinite(r.vertex_forces).all()  # (37, 42: +inf, no ground contact)
        assert float(r.num_contacts.min()) > 0
    assert bool((guard == 7.25).all())


def test_sensor_frame():
    """`VisionTactileSensorUIPC.contact_wrench()` on a ball scene = the world-frame `contact_forces(ref_points=cam_pos)` rotated on the host
    with the camera rotation, to 1e-12; `ManiSkillSimulator.contact_wrench()` hands the same result on."""
    from tacex_amd import GelSightSensor, GelSightSensorCfg
    from tacex_amd.simulation_approaches.fem_based import ManiSkillSimulatorCfg
    from tacex_amd.uipc.gelpad_scene import FemBallScene
    from tacex_amd.uipc.uipc_sim import BallContactForces

    B = 2
    scene = FemBallScene(B, "cuda:0")
    cam = np.array(scene.camera_pose()[0])
    qc = np.array([0.05, 0.98, -0.1, 0.15]); qc /= np.linalg.norm(qc)
    mcfg = ManiSkillSimulatorCfg(tactile_img_res=(320, 240), device="cuda:0", camera_pos_w=tuple(cam), camera_quat_w_ros=tuple(qc))
    cfg = GelSightSensorCfg(num_envs=B, data_types=["marker_motion"], optical_sim_cfg=None, marker_motion_sim_cfg=mcfg,
                            sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(320, 240)), device="cuda:0")
    cfg.compute_indentation_depth_class = "marker_motion_sim"
    s = GelSightSensor(cfg, gelpad_obj=scene.gelpad)
    s.compute_indentation_depth_func = None
    s.initialize()
    plugin = s.marker_motion_simulator
    for i in range(8):
        scene.step(i)
    w = scene.contact_forces(ref_points=torch.from_numpy(np.repeat(cam[None], B, 0)), per_vertex=True)
    c = plugin.marker_motion_sim.contact_wrench(per_vertex=True)
    c2 = plugin.contact_wrench(per_vertex=True)
    assert isinstance(c, BallContactForces) and isinstance(c2, BallContactForces)
    ww, wx, wy, wz = qc
    Rm = np.array([[1 - 2 * (wy * wy + wz * wz), 2 * (wx * wy - wz * ww), 2 * (wx * wz + wy * ww)],
                   [2 * (wx * wy + wz * ww), 1 - 2 * (wx * wx + wz * wz), 2 * (wy * wz - wx * ww)],
                   [2 * (wx * wz - wy * ww), 2 * (wy * wz + wx * ww), 1 - 2 * (wx * wx + wy * wy)]])
    rw, rc, rc2 = w.record.cpu().numpy(), c.record.cpu().numpy(), c2.record.cpu().numpy()
    print(f"sensor frame: pairs {rw[:, 10]}, ground contacts of the ball {rw[:, 36]}, largest force entry {np.abs(rw[:, :9]).max():.3e}")
    assert rw[:, 10].max() > 0 and np.abs(rw[:, 20:32]).max() > 0  # pairs somewhere
    vec = [k for k in R.FORCE_SLOTS if not 12 <= k <= 14]
    scale = np.abs(rw[:, vec]).max()
    want = rw.copy()
    for k in (0, 3, 6, 20, 23, 26, 29, 32, 38):
        want[:, k:k + 3] = rw[:, k:k + 3] @ Rm  # R^T v, as rows
    want[:, 12:15] = (rw[:, 12:15] - cam) @ Rm
    for got in (rc, rc2):
        assert np.abs(got[:, vec] - want[:, vec]).max() <= 1e-12 * scale, np.abs(got[:, vec] - want[:, vec]).max()
        assert np.abs(got[:, 12:15] - want[:, 12:15]).max() <= 1e-12 * np.abs(want[:, 12:15]).max()
        assert np.array_equal(got[:, R.COUNT_SLOTS + R.DIST_SLOTS], rw[:, R.COUNT_SLOTS + R.DIST_SLOTS])
    vw = w.vertex_forces.cpu().numpy() @ Rm
    assert np.abs(c.vertex_forces.cpu().numpy() - vw).max() <= 1e-12 * scale
    # the body's torque about its origin is a vector like the others
    assert np.abs(c.body_torque.cpu().numpy() - w.body_torque.cpu().numpy() @ Rm).max() <= 1e-12 * scale
