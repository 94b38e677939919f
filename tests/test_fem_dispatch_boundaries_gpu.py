"""GPU tests of every Newton kernel route at the vertex counts where the dispatch switches (`launch_newton` and `ball_lds_ok` in
csrc/fem_kernels.hip), one pad on each side of each boundary, with the route the step took read back (`UipcSim.newton_route`).

Every LDS budget there is a CU's 160 KB LESS the kernel's static __shared__ (256 B for `fem_newton_lds_kernel`, 3 472 B for the streaming
`fem_newton_kernel`, 18 768 B for `fem_ball_newton_kernel<512>`): a pad whose dynamic LDS fits the 160 KB but not what the static part
leaves takes the next route - or, in the ball scene, which has none, gets the descriptive refusal - instead of a failed launch.

Each gelpad case checks one Newton iteration against the float64 oracle (`newton_step_contact`, tolerances of
test_fem_gpu.py::test_newton_step_c4_mesh_vs_oracle), then one tightly solved full step against the plain incremental potential (the bound
of test_fem_physics_gpu.py), and that no step flag is raised.  Also here: the kinematic body's friction reference across a per-env reset.
"""
import numpy as np
import pytest
import torch

from test_fem_ball_gpu import _build, _y
from test_fem_physics_gpu import TIGHT_VTOL, WIDE_TOL

pytestmark = pytest.mark.gpu


def _box_scene(cells, B=2, deterministic=False, friction=True, mesh_indenter=None, gap=0.0009, strength=1000.0):
    """The C4 scene of test_fem_gpu.py (`_c4_scene`) on a `gelpad_box_mesh(*cells)` pad of the same physical size: back face constrained and
    sheared differently per env, a sphere (or `mesh_indenter` = (vertices, triangles) at the sphere's pose) over the front-face vertex nearest
    the middle (odd cell counts have none AT the middle: a sphere there misses d_hat on the coarse pads), `gap` from it for env 0, 0.1 mm less
    for env 1."""
    from oracle.fem_oracle import ContactModel, FemModel
    from tacex_amd.uipc import UipcObject, UipcObjectCfg, UipcSim, UipcSimCfg
    from tacex_amd.uipc.uipc_object import gelpad_box_mesh

    P, T = gelpad_box_mesh(*cells)
    cfg = UipcSimCfg(device="cuda:0")
    cfg.linear_system.deterministic = deterministic
    cfg.contact.enable_friction = friction
    sim = UipcSim(cfg, num_envs=B)
    gel = UipcObject(UipcObjectCfg(mesh_points=P, mesh_tets=T), sim)
    sim.setup_sim(constraint_strength_ratio=strength)
    m = FemModel.build(P, T, youngs=gel.cfg.constitution_cfg.youngs_modulus * 1e6, poisson=gel.cfg.constitution_cfg.poisson_rate,
                       density=gel.cfg.mass_density, dt=sim.cfg.dt, strength=strength)
    back = np.where(P[:, 2] < 1e-12)[0]
    aim = np.repeat(P[None], B, 0)
    aim[:, :, 0] += 0.0002 * (1 + np.arange(B))[:, None]  # every env sheared differently
    sim.set_constraints(back, torch.from_numpy(aim[:, back]).cuda())
    cons = np.zeros(len(P)); cons[back] = 1.0
    top, size = P[:, 2].max(), P.max(0)
    face = np.where(P[:, 2] > top - 1e-12)[0]
    mid = P[face[np.argmin(np.hypot(P[face, 0] - size[0] / 2, P[face, 1] - size[1] / 2))]]
    ind = np.zeros((B, 8)); ind[:, 0] = 1.0
    ind[:, 1], ind[:, 2], ind[:, 4] = mid[0], mid[1], 0.004
    ind[:, 3] = top + 0.004 + gap - 1e-4 * np.arange(B)  # (default: gaps of 0.9, 0.8 mm - inside d_hat = 1 mm)
    if mesh_indenter is not None:
        sim.set_indenter_mesh(*mesh_indenter)
        ind[:, 0], ind[:, 4] = 4.0, 0.0
        ind[:, 5:8] = [[0.2, 0.1, -0.3], [0.0, 0.0, 0.0]][:B]  # the pose matters: the facets are not symmetric
        ind[:, 3] -= 1e-4  # (the facets lie inside the sphere: a little closer)
    sim.set_contact_indenters(torch.from_numpy(ind))
    area = gel.surface_vertex_areas()
    kappa = sim.cfg.contact.default_contact_resistance * 1e9 * sim.cfg.contact.d_hat
    cms = [ContactModel(area, ind[b].copy(), sim.cfg.contact.d_hat, kappa, sim.cfg.dt, mesh=mesh_indenter) for b in range(B)]
    return sim, m, P, cons, aim, cms, area


def _plain_gradient(sim, m, area, x_end, x_n, v_n, ind_now, ind_prev, b, mesh=None):
    """test_fem_physics_gpu.py::_plain_gradient with the indenter's mesh: the gradient of IPC's plain incremental potential of env b at x_end
    and the largest contact force on a vertex (both dt^2-scaled), friction lagged from the previous configuration (Li et al. 2020, 5.4)."""
    from oracle.fem_oracle import ContactModel, FrictionModel

    cfg = sim.cfg
    dt = cfg.dt
    kappa = cfg.contact.default_contact_resistance * 1e9 * cfg.contact.d_hat
    cons = sim.is_constrained[b].cpu().numpy().astype(np.float64)
    aim = sim.aim_position[b].cpu().numpy()
    xt = x_n + dt * v_n + dt * dt * np.asarray(cfg.gravity, np.float64)
    cm = ContactModel(area, ind_now, cfg.contact.d_hat, kappa, dt, mesh=mesh)
    g = m.gradient(x_end, xt, cons, aim) + cm.gradient(x_end)
    scale = np.abs(cm.gradient(x_end)).max()
    if cfg.contact.enable_friction:
        fr = FrictionModel(ContactModel(area, ind_prev, cfg.contact.d_hat, kappa, dt, mesh=mesh), x_n, ind_now[1:4] - ind_prev[1:4],
                           cfg.contact.default_friction_ratio, cfg.contact.eps_velocity)
        if fr.lam.max() > 0.0:
            g = g + fr.gradient(x_end)
    return g, scale


def _chains(sim):
    from oracle.fem_oracle import chain_tables

    return chain_tables(sim.vertex_chains, sim._obj.num_verts)


STREAM = 512  # block size of the streaming kernel
# (cells, vertices, deterministic, friction in the full step, route (threads, lds_mode)); lds_mode -1 = CU-resident
ROUTES = [
    ((7, 7, 3), 256, False, True, (256, -1)),
    ((4, 12, 3), 260, False, True, (512, -1)),
    ((7, 15, 3), 512, False, True, (512, -1)),
    ((8, 18, 2), 513, False, True, (768, -1)),
    ((8, 18, 2), 513, True, True, (STREAM, 0)),  # the deterministic switch beyond 512 vertices: fixed-order gathers through memory
    ((10, 16, 3), 748, False, False, (768, -1)),  # 163 312 B of dynamic LDS: fits next to the 256 B static
    ((9, 24, 2), 750, False, False, (STREAM, 2)),  # 163 744 B: 96 B under 160 KB, over it with the static 256 B
    ((13, 16, 3), 952, False, True, (STREAM, 2)),  # 21 V doubles = 159 936 B next to 3 472 B static
    ((11, 19, 3), 960, False, True, (STREAM, 1)),  # 21 V doubles = 161 280 B: fits 160 KB alone, not with the static part
    ((21, 24, 3), 2200, False, True, (STREAM, 1)),  # 9 V doubles = 158 400 B
    ((23, 30, 2), 2232, False, True, (STREAM, 0)),  # 9 V doubles = 160 704 B: 160 KB alone, not with the static part
]


def _route_case(cells, V, deterministic, friction, route, mesh_indenter=None):
    from oracle.fem_oracle import newton_step_contact

    B = 2
    resident = route[1] == -1
    # (1) one Newton iteration from the rest state against the oracle.  The streaming kernel has no vertex chains and no edge snap
    #     (test_fem_gpu.py::test_streaming_newton_kernel_steps_simple_axle_with_sphere_contact): its oracle runs without them.  Both PCGs
    #     run to r.z <= 1e-20 r0.z0 (a residual of 1e-10): at the C4 tests' 1e-12 the finer pads (952, 2200, 2232 vertices) stop where the
    #     energy after the step still differs by 1e-4 - 3e-3 relative between two stopping iterations - a comparison of where each solve
    #     happened to stop, not of the kernel.
    sim, m, P, cons, aim, cms, area = _box_scene(cells, B, deterministic=deterministic, friction=friction, mesh_indenter=mesh_indenter)
    assert len(P) == V and sim.newton_route is None
    sim.cfg.linear_system.max_iter, sim.cfg.linear_system.tol_rate = 3000, 1e-20
    sim.x_tilde = sim.x.clone()
    st = sim.newton_step().cpu().numpy().copy()
    assert sim.newton_route == route, (sim.newton_route, route)
    assert sim.newton_kernel_resident is resident
    x = sim.x.cpu().numpy()
    worst = 0.0
    for b in range(B):
        xo, so = newton_step_contact(m, cms[b], P.copy(), P, cons, aim[b], pcg_max_iter=3000, pcg_tol_rate=1e-20, coarse=sim.coarse_space,
                                     chains=_chains(sim) if resident else None, edge=resident)
        assert abs(st[b, 0] - so[0]) <= 1e-6 * abs(so[0]) + 1e-20, (b, st[b], so)
        assert abs(st[b, 1] - so[1]) <= 1e-5 * abs(so[1]) + 1e-20, (b, st[b], so)
        assert st[b, 2] == so[2], (b, st[b], so)  # the same step: the line search cut it as often
        assert abs(st[b, 3] - so[3]) <= 0.05 * so[3] + 2, (b, st[b], so)  # PCG iterations (summation order differs)
        d = np.abs(x[b] - xo).max()
        assert d <= 1e-6 * np.ptp(P), (b, d)
        worst = max(worst, d)
    assert np.abs(x[0] - x[1]).max() > 1e-5  # the envs really differ
    # (2) one tightly solved full step (friction where the row has it) is a stationary point of the plain incremental potential.  The
    #     indenter starts deeper (0.5 / 0.4 mm): at 0.9 mm the pad sags out of the barrier zone within the step and there is no contact
    #     force left to measure the gradient against.
    sim, m, P, cons, aim, cms, area = _box_scene(cells, B, deterministic=deterministic, friction=friction, mesh_indenter=mesh_indenter, gap=0.0005)
    sim.cfg.newton.velocity_tol = TIGHT_VTOL
    sim.cfg.linear_system.max_iter, sim.cfg.linear_system.tol_rate = 6000, 1e-12
    x_n, v_n = sim.x.cpu().numpy().copy(), sim.v.cpu().numpy().copy()
    ind = sim.contact_indenters.cpu().numpy().copy()
    sim.step(max_newton_iter=200)
    assert sim.newton_route == route, (sim.newton_route, route)
    info = sim.check_step()
    flags = sim.step_info[:, 2].cpu().numpy()
    assert (flags == 0).all() and info["newton_iters"].max() < 200, info  # (3) no step flag of any kind
    x_end = sim.x.cpu().numpy()
    ratio = 0.0
    for b in range(B):
        g, scale = _plain_gradient(sim, m, area, x_end[b], x_n[b], v_n[b], ind[b], ind[b], b, mesh=mesh_indenter)  # (first step: no indenter motion)
        assert scale > 0.0, b  # in contact
        assert np.abs(g).max() <= WIDE_TOL * scale, (b, np.abs(g).max(), scale)
        ratio = max(ratio, np.abs(g).max() / scale)
    print(f"{V} vertices {cells}: route {route}, oracle |dx| {worst:.2e} m ({worst / np.ptp(P):.1e} ptp), |grad| / contact force {ratio:.2e}")


@pytest.mark.parametrize("cells,V,deterministic,friction,route", ROUTES,
                         ids=[f"{c[1]}{'-det' if c[2] else ''}-{c[4][0]}t{'' if c[4][1] < 0 else f'-lds{c[4][1]}'}" for c in ROUTES])
def test_newton_route_at_vertex_count_boundary_vs_oracle(cells, V, deterministic, friction, route):
    _route_case(cells, V, deterministic, friction, route)


def test_mesh_indenter_on_the_512_vertex_resident_kernel_vs_oracle():
    """The largest pad the MESH=true CU-resident kernel takes (a triangle-mesh indenter runs only the 512-thread variant)."""
    from tacex_amd.uipc.indenter_meshes import icosphere

    _route_case((7, 15, 3), 512, False, True, (512, -1), mesh_indenter=icosphere(0.004, 2))


def test_ball_scene_at_693_vertices_vs_oracle_step():
    """The largest gelpad box of this family that fits the ball kernel (693 vertices: 144 432 B of dynamic LDS next to 18 768 B static):
    two tight steps against `BallScene.step`, with the bounds of test_fem_ball_gpu.py::test_step_vs_oracle_step_from_outside_every_barrier_zone."""
    sim, sc, cons, back = _build(B=2, mesh=(10, 20, 2), press=-2e-5, ground_gap=1.02, density=1e5, shift=(0.0008, 0.0005), velocity_tol=1e-6,
                                 transrate_tol=1e-5, tol_rate=1e-12)
    V = sc.V
    assert V == 693
    yo = [_y(sim, b) for b in range(2)]
    vo = [np.zeros_like(yo[0]) for _ in range(2)]
    aim0 = sim.aim_position.clone()
    depth = np.array([5e-5, 8e-5])
    worst = [0.0, 0.0]
    for k in range(2):
        aim = aim0.clone()
        aim[:, :, 2] -= torch.from_numpy(depth * (k + 1)).cuda()[:, None]
        sim.aim_position.copy_(aim)
        sim.step(max_newton_iter=60)
        assert sim.newton_route == (512, -1)
        info = sim.check_step()
        assert int(sim.step_info[:, 2].max()) == 0 and info["newton_iters"].max() < 60, info
        for b in range(2):
            yo[b], vo[b], io = sc.step(yo[b], vo[b], cons, aim[b].cpu().numpy(), gravity=sim.cfg.gravity, max_newton=60, velocity_tol=1e-6,
                                       transrate_tol=1e-5, pcg_max_iter=4000, pcg_tol_rate=1e-12)
            assert io[0] < 60 and int(io[2]) == 0
            yk = _y(sim, b)
            worst[0] = max(worst[0], np.abs(yk[:V + 1] - yo[b][:V + 1]).max())
            worst[1] = max(worst[1], np.abs(yk[V + 1:] - yo[b][V + 1:]).max())
            assert np.abs(yk[:V + 1] - yo[b][:V + 1]).max() <= 2e-8, (k, b, np.abs(yk[:V + 1] - yo[b][:V + 1]).max())
            assert np.abs(yk[V + 1:] - yo[b][V + 1:]).max() <= 2e-7, (k, b)
    kinds = sc.pairs(_y(sim, 1))
    assert len(kinds[0][0]) + len(kinds[1][0]) >= 1  # the pad touched the ball
    print(f"693-vertex ball scene: worst |dx| pad + translation {worst[0]:.2e} m, affine rows {worst[1]:.2e}")


@pytest.mark.parametrize("mesh,V", [((9, 13, 4), 700), ((10, 12, 4), 715)])
def test_ball_scene_refuses_a_pad_beyond_its_lds_and_leaves_the_state_alone(mesh, V):
    """Pads whose ball-kernel state (208 V + 288 B) fits 160 KB but not next to the kernel's 18 768 B of static LDS: the step is refused with
    the descriptive message before anything is launched - x, v, q and qv are bit for bit what they were."""
    sim, sc, cons, back = _build(B=2, mesh=mesh)
    assert sc.V == V
    sim.v.normal_(0.0, 1e-3)
    sim.qv.normal_(0.0, 1e-3)
    before = [t.clone() for t in (sim.x, sim.v, sim.q, sim.qv)]
    with pytest.raises(ValueError, match="160 KB of LDS"):
        sim.step()
    with pytest.raises(ValueError, match="160 KB of LDS"):
        sim.ball_terms()
    torch.cuda.synchronize()
    for a, t in zip(before, (sim.x, sim.v, sim.q, sim.qv)):
        assert torch.equal(a, t)


def _kinematic_scene(B):
    """The scene of test_fem_ball_gpu.py::test_kinematic_body_is_fixed_within_a_step_and_dents_the_pad, with the pad's face INSIDE the ball's
    barrier zone at the start (0.6 d_hat): a reset env is in contact, so friction sees whatever body motion its first step is told of."""
    from tacex_amd.uipc import UipcObject, UipcObjectCfg, UipcSim, UipcSimCfg
    from tacex_amd.uipc.gelpad_scene import icosphere
    from tacex_amd.uipc.uipc_object import gelpad_box_mesh

    R, dhat, gh = 0.006, 5e-4, 0.001
    P, T = gelpad_box_mesh(6, 8, 2)
    size = P.max(0) - P.min(0)
    Pw = P * np.array([1.0, -1.0, -1.0]) + np.array([-size[0] / 2 + 0.0008, size[1] / 2 + 0.0005, 0.0])
    zc = gh + 0.002 + R
    Pw[:, 2] += zc + R + 0.6 * dhat - Pw[:, 2].min()
    cfg = UipcSimCfg(device="cuda:0")
    cfg.contact.d_hat, cfg.ground_height = dhat, gh
    cfg.newton.velocity_tol, cfg.newton.transrate_tol = 1e-6, 1e-5
    cfg.linear_system.tol_rate, cfg.linear_system.max_iter = 1e-12, 4000
    sim = UipcSim(cfg, num_envs=B)
    UipcObject(UipcObjectCfg(mesh_points=Pw, mesh_tets=T), sim)
    vb, tb = icosphere(R, 1)
    UipcObject(UipcObjectCfg(mesh_points=vb, mesh_tris=tb, init_pos=(0.0, 0.0, zc),
                             constitution_cfg=UipcObjectCfg.AffineBodyConstitutionCfg(kinematic=True)), sim)
    sim.setup_sim(constraint_strength_ratio=1000.0)
    back = np.where(Pw[:, 2] > Pw[:, 2].max() - 1e-12)[0]
    sim.set_constraints(back, torch.from_numpy(np.repeat(Pw[None, back], B, 0)).cuda())
    assert sim.cfg.contact.enable_friction
    return sim


def test_kinematic_body_reset_clears_its_friction_reference():
    """A kinematic body's friction slides relative to where the body stood at the end of the previous step.  After `reset(env_ids)` the reset
    env's body is back at q0, and its first step must see no body motion, like the first step of a fresh scene: the ball is lifted into the
    pad and slid sideways for four steps (0.2 mm), env 1 is reset and stepped once with the body held still - it must match a fresh
    scene's first step to the tight solves' 2e-8 m; env 0 is untouched by the reset.  Measured before the reset cleared the reference:
    the stale 0.2 mm slide moved the reset pad by up to 0.23 mm (2.25e-4 m) in its first step, against the 2e-8 m bound."""
    B = 2
    sim = _kinematic_scene(B)
    for k in range(4):
        sim.q[:, 0, 2] += 5e-5 * torch.tensor([1.0, 0.5], device="cuda", dtype=torch.float64)  # the caller moves the body: up into the pad ...
        sim.q[:, 0, 0] += 5e-5  # ... and sideways
        sim.step(max_newton_iter=64)
        info = sim.check_step()
        assert int(sim.step_info[:, 2].max()) == 0 and info["newton_iters"].max() < 64, (k, info)
    keep = [t[0].clone() for t in (sim.x, sim.v, sim.q, sim.qv)]
    sim.reset([1])
    for a, t in zip(keep, (sim.x, sim.v, sim.q, sim.qv)):
        assert torch.equal(a, t[0])  # env 0 untouched
    assert torch.equal(sim.q[1], sim._q0) and float(sim.qv[1].abs().max()) == 0.0
    sim.step(max_newton_iter=64)  # the body held still
    assert int(sim.step_info[:, 2].max()) == 0 and int(sim.step_info[:, 0].max()) < 64
    fresh = _kinematic_scene(B)
    fresh.step(max_newton_iter=64)
    assert int(fresh.step_info[:, 2].max()) == 0 and int(fresh.step_info[:, 0].max()) < 64
    d = float((sim.x[1] - fresh.x[1]).abs().max())
    assert d <= 2e-8, d
    assert torch.equal(sim.q[1], fresh.q[1])
    face_lift = float((fresh.x[1, :, 2] - torch.from_numpy(sim._obj.points).cuda()[:, 2]).abs().max())
    assert face_lift > 1e-6  # the barrier acted in that first step: the reset env really is in contact
