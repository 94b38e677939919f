"""NumPy reference of `tacex_fem_ball_contact_forces` (csrc/fem_ball_contact_forces.h): the contact forces of the ball scene per state row
and the (44,) record derived from them, built from the pieces of oracle/abd_oracle.py alone - `BallScene._pair_rows`, `_ground`,
`friction_lag`, `_fric`, `barrier`, `friction_f0`, `AffineBody.to_q` - with no physics of its own.  A force on a state row is what
`BallScene.gradient` adds for the term, divided by -dt^2 (tests/test_ball_contact_forces.py pins that).  Also the scene builder the GPU
tests share (tests/test_fem_ball_gpu.py `_build`, copied)."""
import numpy as np

SLOTS = 44


def oracle_scene(mesh=(6, 8, 2), R=0.006, level=1, press=4e-4, ground_gap=0.6, density=1e3, shift=(0.0005, 0.0005), dhat=5e-4, gh=0.001):
    """`BallScene` of tests/test_fem_ball_gpu.py `_build` without the device side: (scene, rest state (V + 4, 3), world pad points, tets, ball mesh)."""
    from oracle.abd_oracle import AffineBody, BallScene
    from oracle.fem_oracle import FemModel
    from tacex_amd.uipc import UipcObject, UipcObjectCfg, UipcSim, UipcSimCfg
    from tacex_amd.uipc.gelpad_scene import icosphere
    from tacex_amd.uipc.uipc_object import gelpad_box_mesh

    P, T = gelpad_box_mesh(*mesh)
    size = P.max(0) - P.min(0)
    Pw = P * np.array([1.0, -1.0, -1.0]) + np.array([-size[0] / 2 + shift[0], size[1] / 2 + shift[1], 0.0])
    zc = gh + dhat * ground_gap + R
    Pw[:, 2] += zc + R + (dhat - press) - Pw[:, 2].min()
    cfg = UipcSimCfg(device="cuda:0")
    cfg.contact.d_hat, cfg.ground_height = dhat, gh
    pad = UipcObject(UipcObjectCfg(mesh_points=Pw, mesh_tets=T), UipcSim(cfg, num_envs=1))  # (host side only: surface triangles and areas)
    vb, tb = icosphere(R, level)
    m = FemModel.build(Pw, T, youngs=pad.cfg.constitution_cfg.youngs_modulus * 1e6, poisson=pad.cfg.constitution_cfg.poisson_rate,
                       density=pad.cfg.mass_density, dt=cfg.dt, strength=1000.0)
    sc = BallScene(m, pad.surface_triangles(), pad.surface_vertex_areas(), AffineBody(vb, tb, density=density), dhat=dhat, ground_height=gh,
                   resistance=cfg.contact.default_contact_resistance)
    sc.mu, sc.eps_v = cfg.contact.default_friction_ratio, cfg.contact.eps_velocity
    rest = np.concatenate([Pw, np.array([[0.0, 0.0, zc]]), np.eye(3)], 0)
    return sc, rest, Pw, T, (vb, tb)


def build(B=2, mesh=(6, 8, 2), R=0.006, level=1, press=4e-4, ground_gap=0.6, density=1e3, shift=(0.0005, 0.0005), dhat=5e-4, gh=0.001,
          velocity_tol=None, tol_rate=None, transrate_tol=None, kinematic=False):
    """tests/test_fem_ball_gpu.py `_build`: the same scene twice, `UipcSim` (HIP) and `BallScene` (oracle).  kinematic: the body of
    `test_kinematic_body_is_fixed_within_a_step_and_dents_the_pad` (the oracle scene has no such switch: its terms are the same)."""
    import torch

    from oracle.abd_oracle import AffineBody, BallScene
    from oracle.fem_oracle import FemModel
    from tacex_amd.uipc import UipcObject, UipcObjectCfg, UipcSim, UipcSimCfg
    from tacex_amd.uipc.gelpad_scene import icosphere
    from tacex_amd.uipc.uipc_object import gelpad_box_mesh

    P, T = gelpad_box_mesh(*mesh)
    size = P.max(0) - P.min(0)
    Pw = P * np.array([1.0, -1.0, -1.0]) + np.array([-size[0] / 2 + shift[0], size[1] / 2 + shift[1], 0.0])
    zc = gh + dhat * ground_gap + R
    Pw[:, 2] += zc + R + (dhat - press) - Pw[:, 2].min()
    cfg = UipcSimCfg(device="cuda:0")
    cfg.contact.d_hat, cfg.ground_height = dhat, gh
    if velocity_tol is not None:
        cfg.newton.velocity_tol = velocity_tol
    if transrate_tol is not None:
        cfg.newton.transrate_tol = transrate_tol
    if tol_rate is not None:
        cfg.linear_system.tol_rate = tol_rate
        cfg.linear_system.max_iter = 4000
    sim = UipcSim(cfg, num_envs=B)
    pad = UipcObject(UipcObjectCfg(mesh_points=Pw, mesh_tets=T), sim)
    vb, tb = icosphere(R, level)
    UipcObject(UipcObjectCfg(mesh_points=vb, mesh_tris=tb, mass_density=density, init_pos=(0.0, 0.0, zc),
                             constitution_cfg=UipcObjectCfg.AffineBodyConstitutionCfg(kinematic=bool(kinematic))), sim)
    sim.setup_sim(constraint_strength_ratio=1000.0)
    back = np.where(Pw[:, 2] > Pw[:, 2].max() - 1e-12)[0]
    sim.set_constraints(back, torch.from_numpy(np.repeat(Pw[None, back], B, 0)).cuda())
    m = FemModel.build(Pw, T, youngs=pad.cfg.constitution_cfg.youngs_modulus * 1e6, poisson=pad.cfg.constitution_cfg.poisson_rate,
                       density=pad.cfg.mass_density, dt=cfg.dt, strength=1000.0)
    sc = BallScene(m, pad.surface_triangles(), pad.surface_vertex_areas(), AffineBody(vb, tb, density=density), dhat=dhat, ground_height=gh,
                   resistance=cfg.contact.default_contact_resistance)
    if cfg.contact.enable_friction:  # one default contact model for every pair of surfaces (US:192-201)
        sc.mu, sc.eps_v = cfg.contact.default_friction_ratio, cfg.contact.eps_velocity
    cons = np.zeros(len(Pw))
    cons[back] = 1.0
    return sim, sc, cons, back


def issue_states(rest, b):
    """State and previous state of env b of the every-term case: y = rest + 2e-5 N(0,1) from default_rng(5 + b), env 1 with 1e-3 N on its three
    affine rows too; y_prev = y + 2e-6 N with the body's p row moved by (s, -s/2, 0), s = 3e-5 (env 0: every contact sticks) / 3e-4 (env 1:
    every contact slips)."""
    V = len(rest) - 4
    rng = np.random.default_rng(5 + b)
    y = rest + 2e-5 * rng.standard_normal((V + 4, 3))
    if b == 1:
        y[V + 1:] += 1e-3 * rng.standard_normal((3, 3))
    yp = y + 2e-6 * rng.standard_normal((V + 4, 3))
    s = 3e-5 if b == 0 else 3e-4
    yp[V] += np.array([s, -s / 2, 0.0])
    return y, yp


def _pair_kinds(rows, V):
    """Pair kind from the row pattern of `_pair_rows`: 0 = one pad row then the ball's, 1 = the ball's rows first, 2 = two pad rows first."""
    return np.where(rows[:, 0] >= V, 1, np.where(rows[:, 1] >= V, 0, 2))


def ball_forces_ref(sc, y, lag_state=None, slide_ref=None, ref=None):
    """Forces at the state y (V + 4, 3) of `BallScene` sc, per state row, and the record.

    lag_state: the state the lagged friction contacts are taken at (None: no friction); slide_ref: the state sliding is measured from
    (None: lag_state).  Returns a dict: `barrier`, `ground`, `friction_pairs`, `friction_ground` (V + 4, 3) forces on the state rows,
    `vertex` (V, 3) their sum on the pad rows, `record` (44,), `slid` (K,) |u| of the lagged contacts."""
    from oracle.fem_oracle import barrier
    from oracle.abd_oracle import friction_f0

    V, dh, kap = sc.V, sc.dhat, sc.kappa
    ref = np.zeros(3) if ref is None else np.asarray(ref, np.float64)
    rec = np.zeros(SLOTS)
    # ---- pairs at y ----
    rows, coef, w, d, n, mol, X = sc._pair_rows(y)
    kind = _pair_kinds(rows, V) if len(w) else np.zeros(0, np.int64)
    act = (d < dh) & (w * mol > 0)
    lam = np.where(act, -kap * w * mol * barrier(d / dh)[1] / dh, 0.0)
    fb = np.zeros_like(y)
    for r in range(8):
        np.add.at(fb, rows[:, r], (lam * coef[:, r])[:, None] * n)
    if X is not None:
        k, xr, xv = X
        sb = kap * w[k] * barrier(d[k] / dh)[0]
        for r in range(6):
            np.add.at(fb, xr[:, r], -sb[:, None] * xv[:, r])
    # pad-side closest point of every pair: its pad rows' coefficients times the vertices (kind 1 carries them negated)
    cp = np.zeros((len(w), 3))
    for r in range(8):
        on = (rows[:, r] < V) & (coef[:, r] != 0.0)
        cp[on] += coef[on, r, None] * y[rows[on, r]]
    cp[kind == 1] *= -1.0
    # ---- ground at y ----
    fg = np.zeros_like(y)
    _, gz_pad, _, gap_pad = sc._ground(y[:V], sc.pad_area)
    fg[:V, 2] = -gz_pad / sc.dt**2
    xb = sc.ball.points(y[V:])
    _, gz_b, _, gap_b = sc._ground(xb, sc.ball.area)
    fbz = np.zeros((len(xb), 3))
    fbz[:, 2] = -gz_b / sc.dt**2
    fg[V:] = sc.ball.to_q(fbz)
    on_pad = (gap_pad > 0) & (gap_pad < dh)
    on_b = (gap_b > 0) & (gap_b < dh)
    # ---- lagged friction ----
    ffp, ffg = np.zeros_like(y), np.zeros_like(y)
    slid = np.zeros(0)
    if lag_state is not None and sc.mu > 0.0:
        y0 = lag_state if slide_ref is None else slide_ref
        keep = sc._lag
        sc._lag = sc.friction_lag(lag_state)[:4] + (y0,)
        f = sc._fric(y)
        sc._lag = keep
        if f is not None:
            frows, fcoef, flam, u, _ = f
            slid = np.linalg.norm(u, axis=1)
            a = friction_f0(slid, sc.eps_v * sc.dt)[1]
            npairs = len(sc._pair_rows(lag_state)[2])  # (friction_lag lists the pairs first, then the ground contacts of pad and ball)
            is_pair = np.arange(len(flam)) < npairs
            for r in range(8):
                c = (-sc.mu * flam * a * fcoef[:, r])[:, None] * u
                np.add.at(ffp, frows[is_pair, r], c[is_pair])
                np.add.at(ffg, frows[~is_pair, r], c[~is_pair])
            gfr = np.zeros((len(flam), 3))  # the ground contacts' friction per contact, split by body
            gfr[~is_pair] = (-sc.mu * flam * a)[~is_pair, None] * u[~is_pair]
            g_pad = ~is_pair & (frows[:, 0] < V)
            g_ball = ~is_pair & (frows[:, 0] >= V)
            rec[38:40] = gfr[g_pad, :2].sum(0)
            rec[32:34] = gfr[g_ball, :2].sum(0)
    # ---- record ----
    rec[0:3] = fb[:V].sum(0)
    rec[3:6] = ffp[:V].sum(0)
    rec[6:9] = np.cross(y[:V] - ref, fb[:V] + ffp[:V]).sum(0)
    rec[9] = lam.sum()
    rec[10] = act.sum()
    rec[11] = 0.0
    rec[12:15] = ref + (lam[:, None] * (cp - ref)).sum(0) / lam.sum() if lam.sum() > 0 else ref
    rec[15] = d[act].min() if act.any() else np.inf
    for k in range(3):
        rec[16 + k] = (act & (kind == k)).sum()
    rec[20:32] = (fb[V:] + ffp[V:] + fg[V:] + ffg[V:]).reshape(12)
    rec[34] = fbz[:, 2].sum()
    rec[35] = fbz[on_b, 2].sum()
    rec[36] = on_b.sum()
    rec[37] = gap_b[on_b].min() if on_b.any() else np.inf
    rec[40] = fg[:V, 2].sum()
    rec[41] = on_pad.sum()
    rec[42] = gap_pad[on_pad].min() if on_pad.any() else np.inf
    return {"barrier": fb, "ground": fg, "friction_pairs": ffp, "friction_ground": ffg, "vertex": (fb + fg + ffp + ffg)[:V], "record": rec,
            "slid": slid, "mol": mol, "active": act, "kind": kind}


FORCE_SLOTS = list(range(0, 10)) + list(range(12, 15)) + list(range(20, 36)) + list(range(38, 41))  # newtons (12..14: metres)
COUNT_SLOTS = [10, 11, 16, 17, 18, 19, 36, 41, 43]
DIST_SLOTS = [15, 37, 42]


def compare(rec, ref, tol=1e-9, what=""):
    """The issue's comparison of a kernel record with the reference's: every force slot to `tol` of the largest force entry, counts and
    flags exact, distances to 1e-12 relative; the centre of pressure (metres) to `tol` of its own size.  Prints the figures first."""
    rec, ref = np.asarray(rec, np.float64), np.asarray(ref, np.float64)
    fs = [k for k in FORCE_SLOTS if not 12 <= k <= 14]
    scale = np.abs(ref[fs]).max()
    err = np.abs(rec[fs] - ref[fs]).max()
    cop = np.abs(rec[12:15] - ref[12:15]).max()
    print(f"{what}: force slots max |diff| {err:.3e} of largest {scale:.3e} ({err / max(scale, 1e-300):.2e}), centre of pressure diff {cop:.2e} m")
    assert err <= tol * scale, (what, err, scale)
    assert cop <= tol * max(np.abs(ref[12:15]).max(), 1e-3), (what, cop)
    assert np.array_equal(rec[COUNT_SLOTS], ref[COUNT_SLOTS]), (what, rec[COUNT_SLOTS], ref[COUNT_SLOTS])
    for k in DIST_SLOTS:
        if np.isinf(ref[k]):
            assert rec[k] == ref[k], (what, k, rec[k])
        else:
            assert abs(rec[k] - ref[k]) <= 1e-12 * abs(ref[k]), (what, k, rec[k], ref[k])
