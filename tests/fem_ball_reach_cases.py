"""Cases of the ball scene beyond its first family of states (a flat pad OVER an icosphere of level 1), as plain NumPy with no GPU code:
the pad BESIDE the body with its face inside the ground's barrier zone, a cube with flat faces under the pad (exactly parallel edge-edge
pairs), bodies of 12 and 162 vertices, and the pad pressed onto the ground over three steps.  tests/test_fem_ball_reach_cases.py asserts
on the CPU, with the oracle alone, what tests/test_fem_ball_reach_gpu.py relies on; `gpu_sim` builds the same scene as a `UipcSim` from the
same arrays.  Every mesh goes through the product's own helpers (`UipcObject.surface_triangles`, `.tris`, `surface_vertex_areas`)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

DHAT, GH, MESH = 5e-4, 0.001, (6, 8, 2)
TIGHT = dict(velocity_tol=1e-6, transrate_tol=1e-5, tol_rate=1e-12)  # both solvers tight: the step comparisons' setting
CAP = 60
X_TOL, A_TOL = 2e-8, 2e-7  # step bounds of test_step_vs_oracle_step_from_outside_every_barrier_zone: twice the Newton tolerance times dt
# back-face drives per step [m]: pad-on-ground env 0 straight down, env 1 down and along x (the face slides over the ground)
GROUND_DRIVES = ((0.0, 0.0, -1e-4), (5e-5, 0.0, -8e-5))
# the four scenarios of the large-batch ball step: depths per step of the standard over-the-ball step scene (two are the existing test's)
BATCH_DEPTHS = (5e-5, 8e-5, 3e-5, 6.5e-5)


@dataclass
class Case:
    name: str
    Pw: np.ndarray          # (V,3) pad rest points, world
    T: np.ndarray           # (Tn,4) pad tets
    body_pts: np.ndarray    # body mesh in its own frame
    body_tris: np.ndarray   # outward surface triangles (the product's)
    body_tets: np.ndarray | None
    centre: tuple
    density: float
    sc: object              # oracle BallScene
    rest: np.ndarray        # (V+4,3)
    cons: np.ndarray        # (V,) 1.0 on the constrained back face
    back: np.ndarray
    face: np.ndarray        # the pad's contact-face vertices
    y: list = field(default_factory=list)    # state rows per env
    yt: list = field(default_factory=list)   # predictor state per env
    yp: list = field(default_factory=list)   # friction reference state per env
    aim: np.ndarray | None = None            # (B,V,3)

    @property
    def V(self):
        return len(self.Pw)


def _face_down_pad(mesh=MESH):
    """The pad of `_build` (tests/test_fem_ball_gpu.py) turned face-down: x in [0, sx], y in [-sy, 0], z in [-sz, 0], contact face at z-min."""
    from tacex_amd.uipc.uipc_object import gelpad_box_mesh

    P, T = gelpad_box_mesh(*mesh)
    return P * np.array([1.0, -1.0, -1.0]), T, P.max(0) - P.min(0)


def place_over(vb, press, ground_gap, shift, mesh=MESH):
    """`_build`'s placement: the pad centred over the body's axis (plus shift), its face `d_hat - press` above the body's TOP, the body's
    lowest point ground_gap * d_hat above the ground.  Top and bottom are the mesh's own (an icosahedron of level 0 has an edge, 0.85 R up,
    where the finer spheres have a vertex at R; for those this is `_build` to the last bit)."""
    Pf, T, size = _face_down_pad(mesh)
    zc = GH + DHAT * ground_gap - vb[:, 2].min()
    Pw = Pf + np.array([-size[0] / 2 + shift[0], size[1] / 2 + shift[1], 0.0])
    Pw[:, 2] += zc + vb[:, 2].max() + (DHAT - press) - Pw[:, 2].min()
    return Pw, T, (0.0, 0.0, zc)


def place_beside(vb, R, side_gap, face_gap, ball_gap, yshift=0.0007, mesh=MESH):
    """The second placement: the pad BESIDE the body.  Its -x side face stands side_gap * d_hat from the sphere of radius R around the body's
    axis, its contact face face_gap * d_hat above the ground; the body's lowest point ball_gap * d_hat above the ground."""
    Pf, T, size = _face_down_pad(mesh)
    zc = GH + DHAT * ball_gap - vb[:, 2].min()
    Pw = Pf + np.array([R + side_gap * DHAT, size[1] / 2 + yshift, 0.0])
    Pw[:, 2] += GH + face_gap * DHAT - Pw[:, 2].min()
    return Pw, T, (0.0, 0.0, zc)


def _scene(name, Pw, T, centre, density, body_pts, body_tris=None, body_tets=None):
    from oracle.abd_oracle import AffineBody, BallScene
    from oracle.fem_oracle import FemModel
    from tacex_amd.uipc import UipcObject, UipcObjectCfg
    from tacex_amd.uipc.uipc_sim import UipcSimCfg

    cfg = UipcSimCfg(device="cuda:0")
    pad = UipcObject(UipcObjectCfg(mesh_points=Pw, mesh_tets=T))
    body = UipcObject(UipcObjectCfg(mesh_points=body_pts, mesh_tris=body_tris, mesh_tets=body_tets, mass_density=density,
                                    constitution_cfg=UipcObjectCfg.AffineBodyConstitutionCfg()))
    m = FemModel.build(Pw, T, youngs=pad.cfg.constitution_cfg.youngs_modulus * 1e6, poisson=pad.cfg.constitution_cfg.poisson_rate,
                       density=pad.cfg.mass_density, dt=cfg.dt, strength=1000.0)
    sc = BallScene(m, pad.surface_triangles(), pad.surface_vertex_areas(), AffineBody(body.points, body.tris, density=density), dhat=DHAT,
                   ground_height=GH, resistance=cfg.contact.default_contact_resistance)
    assert cfg.contact.enable_friction
    sc.mu, sc.eps_v = cfg.contact.default_friction_ratio, cfg.contact.eps_velocity
    back = np.where(Pw[:, 2] > Pw[:, 2].max() - 1e-12)[0]
    face = np.where(Pw[:, 2] < Pw[:, 2].min() + 1e-12)[0]
    cons = np.zeros(len(Pw))
    cons[back] = 1.0
    rest = np.concatenate([Pw, np.asarray(centre, np.float64)[None], np.eye(3)], 0)
    return Case(name, Pw, T, body.points, body.tris, body_tets, tuple(centre), density, sc, rest, cons, back, face)


def _term_states(c, seed, noise=(2e-5, 2e-5), affine=(0.0, 1e-3), slide=(3e-5, 3e-4), slide_affine=(1e-3, 2e-2), valid_reference=False):
    """Two envs of the every-term recipe of `test_energy_and_gradient_of_the_step_potential_vs_oracle`: y = rest + noise * N(0,1) (env 1 with
    its affine rows stretched and sheared too), a predictor 1e-5 N away, aims 1e-5 off, and a friction reference `slide` away - 3e-5 in env 0
    and 3e-4 in env 1, either side of eps_velocity * dt = 1e-4 (stick / slip).  valid_reference: the reference is itself a state with every
    gap > 0 (the force record takes its LAG there, `ball_terms` only measures sliding from it): 2e-6 N away with the pad moved `slide`
    along y - along its own side face and the ground - where plain noise of 3e-4 would put face vertices under the ground."""
    V = c.V
    rng = np.random.default_rng(seed)
    c.y, c.yt, c.yp = [], [], []
    for b in range(2):
        y = c.rest + noise[b] * rng.standard_normal((V + 4, 3))
        y[V + 1:] += affine[b] * rng.standard_normal((3, 3))
        c.y.append(y)
    c.yt = [y + 1e-5 * rng.standard_normal(y.shape) for y in c.y]
    for b in range(2):
        if valid_reference:
            yp = c.y[b] + 2e-6 * rng.standard_normal(c.y[b].shape)
            yp[:V, 1] += slide[b]
        else:
            yp = c.y[b] + slide[b] * rng.standard_normal(c.y[b].shape)
        yp[V + 1:] = c.y[b][V + 1:] + slide_affine[b] * rng.standard_normal((3, 3))
        c.yp.append(yp)
    c.aim = np.repeat(c.Pw[None], 2, 0) + 1e-5
    return c


@functools.lru_cache(maxsize=None)
def beside(R=0.002, level=1):
    """`beside-R2` / `beside-R3-l2`: the pad beside the ball, every one of its 63 face vertices inside the ground's barrier zone (0.6 d_hat up),
    its -x side 0.3 d_hat from the ball's sphere: pairs of all three kinds on the pad's side face and edge, the ground under pad and ball."""
    from tacex_amd.uipc.gelpad_scene import icosphere

    vb, tb = icosphere(R, level)
    Pw, T, centre = place_beside(vb, R, 0.3, 0.6, 0.6)
    c = _scene("beside-R2" if level == 1 else "beside-R3-l2", Pw, T, centre, 1e3, vb, body_tris=tb)
    return _term_states(c, 5 + level, valid_reference=True)


def cube_mesh(size=0.006):
    from tacex_amd.uipc.uipc_object import gelpad_box_mesh

    Pb, Tb = gelpad_box_mesh(2, 2, 2, size=(size,) * 3)
    return Pb - size / 2, Tb


@functools.lru_cache(maxsize=None)
def cube_parallel():
    """`cube-parallel`: a 6 mm cube (27-vertex tet mesh, its boundary faces oriented outward by `UipcObject`) under the pad at 0.6 d_hat, the pad
    shifted by the irregular (0.31, 0.47) mm so that no pad vertex sits over a diagonal of the cube's triangles (where two region
    classifications tie).  Env 0 is the rest placement: pad edges and cube edges are EXACTLY parallel (Ericson's den = 0, |e_a x e_b|^2 = 0,
    mollifier 0, the unit vector between the closest points arbitrary).  Env 1 is 2e-5 N(0,1) away: the same pairs nearly parallel, their
    mollifiers strictly between 0 and 1.  The friction references keep env 0's pairs exactly parallel (the body's p row moved, as
    tests/ball_contact_forces_ref.py `issue_states` does) - the force record takes its lag there."""
    Pb, Tb = cube_mesh()
    Pw, T, centre = place_over(Pb, 0.4 * DHAT, 0.6, (0.00031, 0.00047))
    c = _scene("cube-parallel", Pw, T, centre, 1e3, Pb, body_tets=Tb)
    V = c.V
    rng = np.random.default_rng(31)
    c.y = [c.rest.copy(), c.rest + 2e-5 * rng.standard_normal((V + 4, 3))]
    c.yt = [y + 1e-5 for y in c.y]
    c.yp = [y.copy() for y in c.y]
    for b, s in enumerate((3e-5, 3e-4)):
        c.yp[b][V] += np.array([s, -s / 2, 0.0])
    c.yp[1][:V] += 2e-6 * rng.standard_normal((V, 3))
    c.aim = np.repeat(c.Pw[None], 2, 0) + 1e-5
    return c


L2_PRESSES = tuple(1e-5 * k for k in range(20, 49, 2))  # the candidates `over-l2` picks its press from
L2_PRESS = 4.2e-4


@functools.lru_cache(maxsize=None)
def over(level, press=None):
    """`over-l0` / `over-l2`: `_build`'s placement with the icosphere of R = 6 mm at level 0 (12 vertices: fewer than a wave; its top is an edge
    along y, exactly parallel to the pad's y edges) and level 2 (162 vertices / 320 triangles / 480 edges).  Level 2 takes the press of
    `L2_PRESSES` at which the oracle lists the most pairs in the two states without a gap <= 0 (the CPU test repeats the scan)."""
    from tacex_amd.uipc.gelpad_scene import icosphere

    vb, tb = icosphere(0.006, level)
    if press is None:
        press = 4e-4 if level == 0 else L2_PRESS
    Pw, T, centre = place_over(vb, press, 0.6, (0.0005, 0.0005))
    c = _scene(f"over-l{level}", Pw, T, centre, 1e3, vb, body_tris=tb)
    return _term_states(c, 40 + level)


@functools.lru_cache(maxsize=None)
def over_step(level=1):
    """The standard over-the-ball step scene (`test_step_vs_oracle_step_from_outside_every_barrier_zone`: press -2e-5, the ball 1.02 d_hat above
    the ground, density 1e5, shift (0.8, 0.5) mm), with the ball of the given level."""
    from tacex_amd.uipc.gelpad_scene import icosphere

    vb, tb = icosphere(0.006, level)
    Pw, T, centre = place_over(vb, -2e-5, 1.02, (0.0008, 0.0005))
    return _scene(f"over-step-l{level}", Pw, T, centre, 1e5, vb, body_tris=tb)


@functools.lru_cache(maxsize=None)
def pad_on_ground():
    """`pad-on-ground`: the pad's face 1.02 d_hat above the ground, the ball (R = 2 mm, density 1e5) 4 d_hat from the pad's side - out of reach;
    the back face is driven `GROUND_DRIVES` per step, so the face is pressed into the ground's zone (env 1: and dragged along x).  (The
    side-contact placement of `beside` is not stepped: there the oracle's first step runs into its cap of 60 iterations - the ball is shot
    sideways - which is a property of the scene.)"""
    from tacex_amd.uipc.gelpad_scene import icosphere

    vb, tb = icosphere(0.002, 1)
    Pw, T, centre = place_beside(vb, 0.002, 4.0, 1.02, 0.6)
    return _scene("pad-on-ground", Pw, T, centre, 1e5, vb, body_tris=tb)


def step_aims(c, drive, k):
    """(V,3) aims of step k (0-based) for a back face driven `drive` (3,) per step."""
    return c.Pw + (k + 1) * np.asarray(drive, np.float64)


@functools.lru_cache(maxsize=None)
def oracle_steps(case_fn, args, drive, nsteps, friction=True):
    """`BallScene.step` from rest, both solvers tight, `nsteps` steps of the back face driven `drive` per step: [(y, v, info)] per step.
    Computed once per scenario and shared (the results are not to be modified)."""
    c = case_fn(*args)
    sc = c.sc
    mu = sc.mu
    y, v, out = c.rest.copy(), np.zeros_like(c.rest), []
    try:
        if not friction:
            sc.mu = 0.0
        for k in range(nsteps):
            y, v, io = sc.step(y, v, c.cons, step_aims(c, drive, k), gravity=(0.0, 0.0, -9.8), max_newton=CAP, velocity_tol=TIGHT["velocity_tol"],
                               transrate_tol=TIGHT["transrate_tol"], pcg_max_iter=4000, pcg_tol_rate=TIGHT["tol_rate"])
            out.append((y, v, io))
    finally:
        sc.mu, sc._lag = mu, None
    return out


def pad_ground_gaps(c, y):
    """Gaps of the pad's contact-face vertices to the ground."""
    return y[c.face, 2] - c.sc.gh


def counts(c, y):
    """(pairs per kind (3,), pad surface vertices inside the ground's zone, body vertices inside it, smallest pair gap, smallest ground gap)."""
    sc = c.sc
    k = sc.pairs(y)
    gp = sc._ground(y[:c.V], sc.pad_area)[3]
    gb = sc._ground(sc.ball.points(y[c.V:]), sc.ball.area)[3]
    dmin = min([float(kk[3].min()) for kk in k if len(kk[3])] or [np.inf])
    return (np.array([len(kk[0]) for kk in k]), int(((gp > 0) & (gp < sc.dhat)).sum()), int(((gb > 0) & (gb < sc.dhat)).sum()), dmin,
            float(min(gp.min(), gb.min())))


def penetrates(c, y):
    """True when a pad surface vertex lies inside the (convex) body or a body vertex inside a pad tet: the unsigned pair distances alone
    cannot tell a state that has passed through the surface from one in front of it."""
    sc, V = c.sc, c.V
    xb = sc.ball.points(y[V:])
    a, b, cc = (xb[sc.ball.tris[:, k]] for k in range(3))
    n = np.cross(b - a, cc - a)
    inside_body = ((y[sc.pad_sv][:, None, :] - a[None]) * n[None]).sum(-1).max(1) <= 0.0
    p = y[:V][c.T]                                             # (Tn,4,3)
    M = np.linalg.inv((p[:, 1:] - p[:, :1]).transpose(0, 2, 1))  # barycentric coordinates of every body vertex in every tet
    lam = np.einsum("tij,vtj->vti", M, xb[:, None, :] - p[None, :, 0])
    inside_pad = ((lam >= 0.0).all(-1) & (lam.sum(-1) <= 1.0)).any()
    return bool(inside_body.any() or inside_pad)


def lagged(sc, y, yp):
    """Sets the scene's lag the way `tacex_fem_ball_terms(x_prev, q_prev)` takes it - forces, normals and weights of the state itself,
    sliding measured from yp - and returns |u| per lagged contact and the number of pair contacts among them (the ground's follow)."""
    sc._lag = sc.friction_lag(y)[:4] + (yp,)
    f = sc._fric(y)
    return (np.linalg.norm(f[3], axis=1) if f is not None else np.zeros(0)), len(sc._pair_rows(y)[2])


def gpu_sim(c, B=2, tight=False):
    """The case's scene as a `UipcSim` (HIP) from the same arrays - the role of `_build` in tests/test_fem_ball_gpu.py."""
    import torch

    from tacex_amd.uipc import UipcObject, UipcObjectCfg, UipcSim, UipcSimCfg

    cfg = UipcSimCfg(device="cuda:0")
    cfg.contact.d_hat, cfg.ground_height = DHAT, GH
    if tight:
        cfg.newton.velocity_tol, cfg.newton.transrate_tol = TIGHT["velocity_tol"], TIGHT["transrate_tol"]
        cfg.linear_system.tol_rate, cfg.linear_system.max_iter = TIGHT["tol_rate"], 4000
    sim = UipcSim(cfg, num_envs=B)
    UipcObject(UipcObjectCfg(mesh_points=c.Pw, mesh_tets=c.T), sim)
    body = UipcObject(UipcObjectCfg(mesh_points=c.body_pts, mesh_tris=None if c.body_tets is not None else c.body_tris, mesh_tets=c.body_tets,
                                    mass_density=c.density, init_pos=c.centre, constitution_cfg=UipcObjectCfg.AffineBodyConstitutionCfg()), sim)
    assert np.array_equal(body.tris, c.body_tris)
    sim.setup_sim(constraint_strength_ratio=1000.0)
    sim.set_constraints(c.back, torch.from_numpy(np.repeat(c.Pw[None, c.back], B, 0)).cuda())
    return sim


def oracle_terms(c, b, friction=True, edge_edge=True):
    """(energy, gradient) of env b's state in the oracle, with the lag `tacex_fem_ball_terms` takes (`lagged`) or frictionless."""
    sc = c.sc
    mu = sc.mu
    try:
        sc.edge_edge = bool(edge_edge)
        if friction:
            lagged(sc, c.y[b], c.yp[b])
        else:
            sc.mu, sc._lag = 0.0, None
        return sc.energy(c.y[b], c.yt[b], c.cons, c.aim[b]), sc.gradient(c.y[b], c.yt[b], c.cons, c.aim[b])
    finally:
        sc.mu, sc._lag, sc.edge_edge = mu, None, True


def gpu_terms(sim, c, friction=True):
    """`UipcSim.ball_terms` at the case's states: (energy (2,), gradient (2, V + 4, 3), step_info (2, 4)) as NumPy."""
    import torch

    V = c.V
    dev = lambda ys, lo, hi: torch.from_numpy(np.stack([y[lo:hi] for y in ys])).cuda()  # noqa: E731
    sim.aim_position.copy_(torch.from_numpy(c.aim).cuda())
    kw = dict(x_prev=dev(c.yp, 0, V), q_prev=dev(c.yp, V, V + 4)) if friction else {}
    E, g, si = sim.ball_terms(dev(c.y, 0, V), dev(c.y, V, V + 4), dev(c.yt, 0, V), dev(c.yt, V, V + 4), **kw)
    torch.cuda.synchronize()
    return E.cpu().numpy(), g.cpu().numpy(), si.cpu().numpy()


def gpu_steps(c, drives, nsteps, before_step=None):
    """`nsteps` tight steps of a `UipcSim` with one env per row of `drives` (B,3), the back face's aims moved by its row per step:
    (sim, [(states (B, V + 4, 3), step_info (B, 4), check_step() dict)] per step).  before_step(sim, k) runs ahead of step k."""
    import torch

    sim = gpu_sim(c, len(drives), tight=True)
    D = torch.from_numpy(np.asarray(drives, np.float64)).cuda()
    aim0 = sim.aim_position.clone()
    out = []
    for k in range(nsteps):
        if before_step is not None:
            before_step(sim, k)
        sim.aim_position.copy_(aim0 + (k + 1) * D[:, None, :])
        sim.step(max_newton_iter=CAP)
        info = sim.check_step()
        out.append((np.concatenate([sim.x.cpu().numpy(), sim.q.cpu().numpy()], 1), sim.step_info.cpu().numpy().copy(), info))
    return sim, out
