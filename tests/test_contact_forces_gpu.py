"""Contact forces and net wrench of the gelpad on the GPU (`tacex_fem_contact_forces` -> `UipcSim.contact_forces` ->
`VisionTactileSensorUIPC.contact_wrench`): the kernel against the float64 oracle's barrier and friction terms (through the record
restatement of tests/contact_forces_ref.py), against the library's own gradient, on a solved scene (force balance), with the mesh and
material libraries (bit for bit against uniform scenes) and in the sensor's camera frame."""
import numpy as np
import pytest
import torch

import contact_forces_ref as ref

pytestmark = pytest.mark.gpu

# 90 vertices (three of the kernel's four waves hold nothing), exactly 256 (one full stride), 495 (two strides, the second partial)
PADS = [(4, 5, 2), (3, 7, 7), (8, 10, 4)]
DISP = np.array([2e-5, -1e-5, -5e-5])
ACTIVE_495 = [10, 99, 0, 7]  # active vertices per env on the 495-vertex pad, from the oracle alone


def _inputs(mesh):
    """Pad, the four indenters of tests/test_fem_gpu.py::_contact_setup (the sphere with radius 20 mm) and the perturbed states."""
    from oracle.fem_oracle import box_tet_mesh

    P, Tt = box_tet_mesh(*mesh)
    top = P[:, 2].max()
    fr = np.where(P[:, 2] > top - 1e-12)[0]
    vc = fr[np.argmin(np.hypot(P[fr, 0] - P[:, 0].mean(), P[fr, 1] - P[:, 1].mean()))]
    cx, cy = P[vc, 0], P[vc, 1]
    ind = np.zeros((4, 8))
    ind[0] = [1, cx, cy, top + 0.02 + 0.0004, 0.02, 0, 0, 1]               # sphere of 20 mm, lowest point 0.4 mm above the pad
    ind[1] = [2, cx, cy, top + 0.0006, 0, 0, 0, -1.0]                       # half-space coming down from above
    ind[2] = [0, 0, 0, 0, 0, 0, 0, 0]                                       # no indenter
    ind[3] = [3, cx, cy, top + 0.003 + 0.0005, 0.003, 0.008, 0.0, 0.0]      # lying capsule
    x = P[None] + 2e-5 * np.random.default_rng(2).normal(size=(4,) + P.shape)
    return P, Tt, ind, x


def _sim(P, Tt, B, friction_lag=None, friction_ratio=None, gel=None):
    from tacex_amd.uipc import UipcObject, UipcObjectCfg, UipcSim, UipcSimCfg

    cfg = UipcSimCfg(device="cuda:0")
    cfg.linear_system.coarse_grid = None
    cfg.linear_system.vertex_chains = None
    if friction_lag is not None:
        cfg.contact.friction_lag = friction_lag
    if friction_ratio is not None:
        cfg.contact.default_friction_ratio = friction_ratio
    sim = UipcSim(cfg, num_envs=B)
    ocfg = UipcObjectCfg(mesh_points=P, mesh_tets=Tt)
    if gel is not None:
        ocfg.constitution_cfg = UipcObjectCfg.StableNeoHookeanCfg(youngs_modulus=gel.youngs_modulus, poisson_rate=gel.poisson_rate)
        ocfg.mass_density = gel.mass_density
    obj = UipcObject(ocfg, sim)
    sim.setup_sim(constraint_strength_ratio=100.0)
    back = np.where(P[:, 2] < 1e-12)[0]
    sim.set_constraints(back, torch.from_numpy(P[back]).cuda()[None].repeat(B, 1, 1))
    return sim, obj


def _consts(sim):
    c = sim.cfg.contact
    return c.d_hat, c.default_contact_resistance * 1e9 * c.d_hat, sim.cfg.dt


def _extent(P):
    return float(np.linalg.norm(P.max(0) - P.min(0)))


def _check_record(got, want, f_v, x, refp, extent, what):
    """Bounds: every component of the force sums within 1e-10 sum |f_v|, torque 1e-10 sum |r_v| |f_v|, area and count exact, centre of pressure 1e-10
    of the pad's extent; sum lam like a sum."""
    fs = np.linalg.norm(f_v, axis=1).sum()  # (|f_v| the vector's length: a component that is round-off in every vertex has no scale of its own)
    assert np.all(np.abs(got[0:3] + got[3:6] - want[0:3] - want[3:6]) <= 1e-10 * fs + 1e-300), (what, got[0:6], want[0:6])
    tb = 1e-10 * (np.linalg.norm(x - refp, axis=1) * np.linalg.norm(f_v, axis=1)).sum()
    assert np.all(np.abs(got[6:9] - want[6:9]) <= tb + 1e-300), (what, got[6:9], want[6:9], tb)
    assert abs(got[9] - want[9]) <= 1e-10 * want[9] + 1e-300, (what, got[9], want[9])
    assert got[11] == want[11], (what, got[11], want[11])
    assert got[10] == want[10], (what, got[10], want[10])  # exact: the restatement adds in the kernel's order
    assert np.all(np.abs(got[12:15] - want[12:15]) <= 1e-10 * extent), (what, got[12:15], want[12:15])


@pytest.mark.parametrize("mesh", PADS, ids=lambda m: "pad%dx%dx%d" % m)
def test_normal_part_vs_oracle(mesh):
    """Per-vertex forces against -ContactModel.gradient / dt^2 within 1e-10 of the largest entry per env (the bound of
    test_contact_energy_gradient_vs_oracle for the same term); the record within the bounds of `_check_record`, about a reference point
    off every axis; min_gap equal to contact_gaps().amin(1) bit for bit; the env without an indenter all zeros and +inf."""
    P, Tt, ind, x = _inputs(mesh)
    assert len(P) == {(4, 5, 2): 90, (3, 7, 7): 256, (8, 10, 4): 495}[mesh]
    sim, obj = _sim(P, Tt, 4)
    sim.set_contact_indenters(torch.from_numpy(ind))
    area = obj.surface_vertex_areas()
    dhat, kappa, dt = _consts(sim)
    refp = np.array([[0.004, -0.003, 0.011], [0.03, 0.02, -0.01], [-0.01, 0.0, 0.002], [0.01, 0.012, 0.05]])
    xd = torch.from_numpy(x).cuda()
    w = sim.contact_forces(x=xd, ref_points=torch.from_numpy(refp), per_vertex=True, friction=False)
    rec, vf = w.record.cpu().numpy(), w.vertex_forces.cpu().numpy()
    gaps = sim.contact_gaps(xd).amin(1).cpu().numpy()
    counts = []
    for b in range(4):
        f_n, d = ref.normal_forces(area, ind[b], dhat, kappa, dt, x[b])
        want = ref.wrench_record(x[b], f_n, np.zeros_like(f_n), area, d, dhat, refp[b])
        counts.append(int(want[11]))
        print(f"{mesh} env {b}: active {int(want[11])}, per-vertex error {np.abs(vf[b] - f_n).max():.2e} of largest entry {np.abs(f_n).max():.2e}, "
              f"record error {np.abs(rec[b, :15] - want[:15]).max():.2e}")
        assert np.abs(vf[b] - f_n).max() <= 1e-10 * np.abs(f_n).max(), b
        assert np.all(vf[b][area == 0] == 0) and np.all(rec[b, 3:6] == 0)
        _check_record(rec[b], want, f_n, x[b], refp[b], _extent(P), (mesh, b))
        assert rec[b, 15] == gaps[b], (b, rec[b, 15], gaps[b])  # bit for bit
        assert (np.isinf(want[15]) and np.isinf(rec[b, 15])) or abs(rec[b, 15] - want[15]) <= 1e-12 * _extent(P)
    if mesh == (8, 10, 4):
        assert counts == ACTIVE_495, counts
    assert counts[0] > 0 and counts[1] > 0 and counts[3] > 0
    assert np.all(rec[2, 0:12] == 0) and np.array_equal(rec[2, 12:15], refp[2]) and rec[2, 15] == np.inf and np.all(vf[2] == 0)
    assert np.array_equal(w.normal_force.cpu().numpy(), rec[:, 0:3]) and np.array_equal(w.min_gap.cpu().numpy(), rec[:, 15])
    # without contact indenters: zeros and +inf without a launch; origin as the reference point by default
    w0 = sim.contact_forces(x=xd, friction=False)
    np.testing.assert_array_equal(w0.record[:, 0:6].cpu().numpy(), rec[:, 0:6])
    sim.set_contact_indenters(None)
    wn = sim.contact_forces(x=xd, per_vertex=True)
    assert np.all(wn.record[:, :15].cpu().numpy() == 0) and np.all(np.isinf(wn.min_gap.cpu().numpy())) and np.all(wn.vertex_forces.cpu().numpy() == 0)


@pytest.mark.parametrize("mesh", PADS, ids=lambda m: "pad%dx%dx%d" % m)
def test_vertex_forces_equal_the_librarys_own_contact_gradient(mesh):
    """-(gradient with indenters - gradient without) / dt^2 of the existing `sim.gradient()` equals `vertex_forces`: 1e-10 of the largest
    entry plus the 1e-12 |g0| round-off term of test_contact_energy_gradient_vs_oracle (the difference of two full gradients)."""
    P, Tt, ind, x = _inputs(mesh)
    sim, obj = _sim(P, Tt, 4)
    dt = sim.cfg.dt
    sim.x = torch.from_numpy(x).cuda()
    sim.x_tilde = sim.x.clone()
    g0 = sim.gradient().cpu().numpy()
    sim.set_contact_indenters(torch.from_numpy(ind))
    g1 = sim.gradient().cpu().numpy()
    vf = sim.contact_forces(per_vertex=True, friction=False).vertex_forces.cpu().numpy()
    for b in range(4):
        want = -(g1[b] - g0[b]) / dt**2
        err = np.abs(vf[b] - want).max()
        print(f"{mesh} env {b}: {err:.2e} against largest entry {np.abs(want).max():.2e}")
        assert err <= 1e-10 * np.abs(want).max() + 1e-12 * np.abs(g0[b]).max() / dt**2, b
    assert np.abs(vf[[0, 1, 3]]).max() > 0 and np.all(vf[2] == 0)


def _friction_case(mesh, rng_seed=3):
    """One real step from x with the indenters moved by DISP since the step before, and the evaluation state x_e: the step's start
    positions plus, per vertex, an offset of length U(0, 3 eps_velocity dt) in a random direction of the plane tangential to the lagged
    normal (the vertical where the vertex has none)."""
    P, Tt, ind, x = _inputs(mesh)
    rng = np.random.default_rng(rng_seed)
    n = np.zeros_like(x)
    from oracle.fem_oracle import contact_distance

    for b in range(4):
        n[b] = contact_distance(ind[b], x[b])[1]
    n[np.linalg.norm(n, axis=-1) < 0.5] = [0.0, 0.0, 1.0]
    t = rng.normal(size=x.shape)
    t -= (t * n).sum(-1, keepdims=True) * n
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    x_e = x + rng.uniform(0.0, 3 * 0.01 * 0.01, size=x.shape[:2])[..., None] * t
    return P, Tt, ind, x, x_e


def _step_twice(sim, ind, x, newton=2):
    """indenters at `ind`, one step; back to x at rest, indenters at ind + DISP, one step: the workspace holds x_prev = x and disp = DISP"""
    xd = torch.from_numpy(x).cuda()
    sim.x.copy_(xd); sim.v.zero_()
    sim.set_contact_indenters(torch.from_numpy(ind))
    sim.step(max_newton_iter=newton)
    sim.x.copy_(xd); sim.v.zero_()
    sim.contact_indenters[:, 1:4] += torch.from_numpy(DISP).cuda()
    sim.step(max_newton_iter=newton)
    assert len(sim.check_step()["penetrating_envs"]) == 0


@pytest.mark.parametrize("mesh", PADS, ids=lambda m: "pad%dx%dx%d" % m)
def test_friction_part_vs_oracle(mesh):
    """IPC's lag: friction forces at x_e against -FrictionModel(ContactModel(area, ind_prev ...), x_prev, disp, mu, eps_v).gradient(x_e) / dt^2,
    per vertex within 1e-10 of the largest entry per env, the record within `_check_record`'s bounds; every env with an indenter has
    sticking AND slipping lagged vertices - asserted in full on the 495-vertex pad; on the two smaller pads an env whose indenter touches
    ONE vertex (the 20 mm sphere on the 90-vertex pad) cannot show both and is let through: a deviation from "every env" forced by the
    fixed indenters.  `friction=True` under the capped lag raises ValueError, and so it does before a step has run."""
    P, Tt, ind, x, x_e = _friction_case(mesh)
    sim, obj = _sim(P, Tt, 4)
    area = obj.surface_vertex_areas()
    dhat, kappa, dt = _consts(sim)
    mu, eps_v = sim.cfg.contact.default_friction_ratio, sim.cfg.contact.eps_velocity
    sim.set_contact_indenters(torch.from_numpy(ind))
    with pytest.raises(ValueError):
        sim.contact_forces(friction=True)  # no step yet: nothing to lag from
    assert np.all(sim.contact_forces().friction_force.cpu().numpy() == 0)  # friction=None: not evaluated before a step
    _step_twice(sim, ind, x)
    ind_now = ind.copy(); ind_now[:, 1:4] += DISP
    np.testing.assert_array_equal(sim.contact_indenters.cpu().numpy(), ind_now)
    xd = torch.from_numpy(x_e).cuda()
    refp = np.array([[0.004, -0.003, 0.011]] * 4)
    wt = sim.contact_forces(x=xd, ref_points=torch.from_numpy(refp), per_vertex=True)  # friction=None: on (ipc, a step has run)
    wn = sim.contact_forces(x=xd, ref_points=torch.from_numpy(refp), per_vertex=True, friction=False)
    rec, vft, vfn = wt.record.cpu().numpy(), wt.vertex_forces.cpu().numpy(), wn.vertex_forces.cpu().numpy()
    np.testing.assert_array_equal(rec[:, 0:3], wn.record[:, 0:3].cpu().numpy())
    np.testing.assert_array_equal(sim.contact_forces(x=xd, ref_points=torch.from_numpy(refp), friction=True).record.cpu().numpy(), rec)
    # the friction part is a function of what the step stored: an indenter moved (away) after the step changes the normal part alone
    sim.contact_indenters[:, 1:4] += torch.tensor([1e-4, 5e-5, 1e-4], dtype=torch.float64, device="cuda")
    moved = sim.contact_forces(x=xd, ref_points=torch.from_numpy(refp)).record.cpu().numpy()
    assert np.array_equal(moved[:, 3:6], rec[:, 3:6]) and not np.array_equal(moved[[0, 1, 3], 0:3], rec[[0, 1, 3], 0:3])
    sim.contact_indenters.copy_(torch.from_numpy(ind_now))
    for b in range(4):
        f_f, fr = ref.friction_forces(area, ind[b], dhat, kappa, dt, x[b], DISP, mu, eps_v, x_e[b])
        f_n, d = ref.normal_forces(area, ind_now[b], dhat, kappa, dt, x_e[b])
        assert not np.any((area > 0) & (d <= 0))
        got = vft[b] - vfn[b]
        lagged = fr.lam > 0
        y = fr._u(x_e[b])[1]
        stick, slip = int((lagged & (y < fr.eps)).sum()), int((lagged & (y >= fr.eps)).sum())
        print(f"{mesh} env {b}: lagged vertices sticking {stick} slipping {slip}; per-vertex error {np.abs(got - f_f).max():.2e} of largest entry "
              f"{np.abs(f_f).max():.2e}; sum error {np.abs(rec[b, 3:6] - f_f.sum(0)).max():.2e}")
        if ind[b, 0] > 0:
            # (both regimes in every env with an indenter - where it has two lagged vertices to show them with: the sphere touches the
            #  90-vertex pad with one)
            assert lagged.sum() >= 1 and ((stick >= 1 and slip >= 1) or (lagged.sum() < 2 and mesh != (8, 10, 4))), (b, stick, slip)
            assert np.abs(f_f).max() > 0
        else:
            assert np.all(rec[b, 0:12] == 0) and np.all(vft[b] == 0)
        assert np.abs(got - f_f).max() <= 1e-10 * np.abs(f_f).max() + 1e-15 * np.abs(f_n).max(), b  # (got is a difference of two totals)
        assert np.all(np.abs(rec[b, 3:6] - f_f.sum(0)) <= 1e-10 * np.linalg.norm(f_f, axis=1).sum() + 1e-300), b
        want = ref.wrench_record(x_e[b], f_n, f_f, area, d, dhat, refp[b])
        _check_record(rec[b], want, f_n + f_f, x_e[b], refp[b], _extent(P), (mesh, b))
    # the capped lag is refused, on the host
    sim2, _ = _sim(P, Tt, 4, friction_lag="capped")
    _step_twice(sim2, ind, x)
    with pytest.raises(ValueError):
        sim2.contact_forces(x=xd, friction=True)
    w2 = sim2.contact_forces(x=xd)  # friction=None: the normal part alone
    np.testing.assert_array_equal(w2.record[:, 0:3].cpu().numpy(), rec[:, 0:3])
    assert np.all(w2.friction_force.cpu().numpy() == 0)


def test_library_refuses_what_it_cannot_report():
    """The C entry point itself: friction under lag mode 0, without a workspace, with another workspace or env count is refused with a
    message (2 -> ValueError); contact disabled or friction ratio 0 give valid zeros."""
    from tacex_amd import _lib

    P, Tt, ind, x = _inputs(PADS[0])
    sim, _ = _sim(P, Tt, 4, friction_ratio=0.0)
    _step_twice(sim, ind, x)
    lib, h = sim._lib, sim._handle
    rec = torch.full((4, 16), -1.0, dtype=torch.float64, device="cuda")
    st = sim._stream()

    def call(ws, fric, B=4, out=rec):
        return lib.tacex_fem_contact_forces(h, _lib.ptr(sim.x), _lib.ptr(ws) if ws is not None else 0, 0, fric, _lib.ptr(out), 0, B, st)

    assert call(sim._ws, 1) == 0 and np.all(rec[:, 3:6].cpu().numpy() == 0) and np.abs(rec[:, 0:3].cpu().numpy()).max() > 0  # ratio 0
    assert call(None, 1) == 2 and b"workspace" in lib.tacex_last_error()
    assert call(torch.empty_like(sim._ws), 1) == 2 and b"last tacex_fem_step" in lib.tacex_last_error()
    assert call(sim._ws, 1, B=3) == 2
    assert lib.tacex_fem_contact_forces(h, _lib.ptr(sim.x), 0, 0, 0, 0, 0, 4, st) == 2  # no record to write
    _lib.check(lib.tacex_fem_set_friction_lag(h, 0), "set_friction_lag")
    assert call(sim._ws, 1) == 2 and b"lag" in lib.tacex_last_error()
    assert call(sim._ws, 0) == 0
    sim.set_contact_indenters(None)
    assert call(sim._ws, 1) == 0  # contact disabled: zeros
    r = rec.cpu().numpy()
    assert np.all(r[:, :15] == 0) and np.all(np.isinf(r[:, 15]))


def test_force_balance_on_a_solved_scene_and_reset():
    """The rolling scene of tests/test_fem_physics_gpu.py::_scene, tight tolerances, IPC's lag, 8 steps.  At every step's end and for every
    env in contact the contact forces balance the pad's other forces: `vertex_forces` dt^2 EQUALS the oracle's non-contact gradient
    (`FemModel.gradient`; a force on the pad is minus the gradient of its potential, so the stationary point g_other + g_contact +
    g_friction = 0 reads g_other - dt^2 f = 0) within that file's stationarity bound GRAD_TOL[d_hat] of the largest barrier-gradient entry.
    The summed force pushes the pad down, and |friction| <= mu sum lam.  After `reset([1])` env 1 reports zero friction - and, its
    indenter put clear of the pad as a task does at a reset, zero normal force - until it steps again; the other envs are unchanged bit
    for bit."""
    from oracle.fem_oracle import ContactModel, FemModel
    from test_fem_physics_gpu import GRAD_TOL, TIGHT_VTOL, _scene

    B, d_hat = 3, 1e-3
    fem = _scene(B, d_hat=d_hat, velocity_tol=TIGHT_VTOL, tol_rate=1e-12, friction_lag="ipc")
    sim, obj = fem.sim, fem.gelpad
    cc = obj.cfg.constitution_cfg
    m = FemModel.build(obj.points, obj.tets, youngs=cc.youngs_modulus * 1e6, poisson=cc.poisson_rate, density=obj.cfg.mass_density, dt=sim.cfg.dt,
                       strength=1000.0)
    area = obj.surface_vertex_areas()
    dhat, kappa, dt = _consts(sim)
    mu = sim.cfg.contact.default_friction_ratio
    g = np.asarray(sim.cfg.gravity, np.float64)
    in_contact, with_friction, worst = 0, 0, 0.0
    for i in range(8):
        x_n, v_n = sim.x.cpu().numpy().copy(), sim.v.cpu().numpy().copy()
        fem.step(i)
        info = sim.check_step()
        assert len(info["penetrating_envs"]) == 0 and len(info["line_search_failed_envs"]) == 0 and info["newton_iters"].max() < 200, (i, info)
        w = fem.contact_forces(per_vertex=True)
        rec, vf = w.record.cpu().numpy(), w.vertex_forces.cpu().numpy()
        x_end, ind_now = sim.x.cpu().numpy(), fem.ind.cpu().numpy()
        cons, aim = sim.is_constrained.cpu().numpy().astype(np.float64), sim.aim_position.cpu().numpy()
        for b in range(B):
            scale = np.abs(ContactModel(area, ind_now[b], dhat, kappa, dt).gradient(x_end[b])).max()
            if not scale > 0.0:
                continue
            in_contact += 1
            go = m.gradient(x_end[b], x_n[b] + dt * v_n[b] + dt * dt * g, cons[b], aim[b])
            res = np.abs(go - vf[b] * dt**2).max()
            worst = max(worst, res / scale)
            fz, ff, sl = rec[b, 2] + rec[b, 5], np.linalg.norm(rec[b, 3:6]), rec[b, 9]
            with_friction += ff > 0
            print(f"step {i} env {b}: |g_other - dt^2 f| {res:.3e} = {res / scale:.2e} of the largest barrier-gradient entry; force z {fz:.4e} N, "
                  f"|friction| {ff:.4e} N, mu sum lam {mu * sl:.4e} N, contacts {int(rec[b, 11])}")
            assert res <= GRAD_TOL[d_hat] * scale, (i, b, res, scale)
            assert fz < 0, (i, b, fz)
            assert ff <= mu * sl, (i, b, ff, mu * sl)
    print(f"worst balance residual {worst:.2e} of the largest barrier-gradient entry over {in_contact} env-steps in contact")
    assert in_contact >= 16 and with_friction >= 8
    # reset of env 1
    before = fem.contact_forces(per_vertex=True)
    sim.reset(env_ids=[1])
    after = fem.contact_forces(per_vertex=True)
    rb, ra = before.record.cpu().numpy(), after.record.cpu().numpy()
    assert np.abs(rb[1, 3:6]).max() > 0  # (env 1 did report friction)
    assert np.all(ra[1, 3:6] == 0)
    for b in (0, 2):
        assert np.array_equal(ra[b], rb[b]) and np.array_equal(after.vertex_forces[b].cpu().numpy(), before.vertex_forces[b].cpu().numpy())
    fem.ind[1, 3] += 2 * d_hat  # the task lifts the reset env's indenter clear of the pad
    lifted = fem.contact_forces(per_vertex=True)
    rl = lifted.record.cpu().numpy()
    assert np.all(rl[1, 0:12] == 0) and np.all(lifted.vertex_forces[1].cpu().numpy() == 0) and rl[1, 15] > d_hat
    for b in (0, 2):
        assert np.array_equal(rl[b], rb[b])
    fem.reset_indenters([1])
    fem.step(8)
    again = fem.contact_forces().record.cpu().numpy()
    assert again[1, 9] > 0 and np.all(np.isfinite(again))


def test_mesh_and_material_libraries_bit_for_bit_against_uniform_scenes():
    """A batch mixing two indenter meshes (icosphere levels 1 and 2) and three materials with different friction ratios: every env's record
    and per-vertex forces, friction included, equal those of a uniform B = 1 scene of its mesh and material (built with the API from
    before the libraries) bit for bit; a repeated call is bit-identical."""
    from tacex_amd.uipc import GelMaterialCfg
    from tacex_amd.uipc.indenter_meshes import icosphere

    P, Tt, ind4, x4, x_e4 = _friction_case(PADS[2])
    top, cx, cy = P[:, 2].max(), ind4[0, 1], ind4[0, 2]  # over a vertex of the face: the barrier is per vertex
    meshes = [icosphere(0.004, 1), icosphere(0.0035, 2)]
    mats = [GelMaterialCfg(youngs_modulus=1e-2, poisson_rate=0.49, mass_density=1000.0, friction_ratio=0.5),
            GelMaterialCfg(youngs_modulus=5e-3, poisson_rate=0.45, mass_density=1100.0, friction_ratio=0.2),
            GelMaterialCfg(youngs_modulus=5e-2, poisson_rate=0.40, mass_density=900.0, friction_ratio=1.0)]
    mesh_ids, mat_ids = [0, 1, 1, 0, 1], [0, 1, 2, 2, 0]
    B = len(mesh_ids)
    x, x_e = x4[[0, 1, 2, 3, 0]], x_e4[[0, 1, 2, 3, 1]]
    ind = np.zeros((B, 8))
    for b, k in enumerate(mesh_ids):
        ind[b] = [4.0, cx + 3e-4 * b, cy, top + 0.0004 - meshes[k][0][:, 2].min(), 0.0, 0.0, 0.0, 0.3 * b]
    refp = np.array([[0.004, -0.003, 0.011]] * B)

    def forces(sim, rows, xs, xes, rp):
        _step_twice(sim, rows, xs, newton=1)
        a = sim.contact_forces(x=torch.from_numpy(xes).cuda(), ref_points=torch.from_numpy(rp), per_vertex=True)
        b2 = sim.contact_forces(x=torch.from_numpy(xes).cuda(), ref_points=torch.from_numpy(rp), per_vertex=True)
        ra, va = a.record.cpu().numpy(), a.vertex_forces.cpu().numpy()
        assert np.array_equal(ra, b2.record.cpu().numpy()) and np.array_equal(va, b2.vertex_forces.cpu().numpy())  # repeated: bit-identical
        return ra, va

    sim, _ = _sim(P, Tt, B)
    sim.set_materials(mats, mat_ids)
    sim.set_indenter_meshes(meshes, mesh_ids)
    rec, vf = forces(sim, ind, x, x_e, refp)
    assert np.all(rec[:, 11] > 0) and np.all(np.linalg.norm(rec[:, 3:6], axis=1) > 0)
    for b in range(B):
        one, _ = _sim(P, Tt, 1, friction_ratio=mats[mat_ids[b]].friction_ratio, gel=mats[mat_ids[b]])
        one.set_indenter_mesh(*meshes[mesh_ids[b]])
        r1, v1 = forces(one, ind[b:b + 1], x[b:b + 1], x_e[b:b + 1], refp[b:b + 1])
        assert np.array_equal(r1[0], rec[b]), (b, r1[0], rec[b])
        assert np.array_equal(v1[0], vf[b]), b
    # envs 0 and 4 share state and mesh placement rule but not the material... and 2 / 3 the material but not the mesh: the ids matter
    assert not np.array_equal(rec[2, 3:6], rec[3, 3:6])


def test_sensor_frame():
    """`VisionTactileSensorUIPC.contact_wrench()` = the world-frame `contact_forces(ref_points=cam_pos)` rotated and translated with the camera
    pose in NumPy, to 1e-12 relative; `ManiSkillSimulator.contact_wrench()` hands the same result on."""
    from tacex_amd import GelSightSensor, GelSightSensorCfg
    from tacex_amd.simulation_approaches.fem_based import ManiSkillSimulatorCfg
    from tacex_amd.uipc.gelpad_scene import FemGelpad

    B = 3
    cam = np.array([0.008, 0.012625, -0.024])
    q = np.array([0.98, 0.05, -0.1, 0.15]); q /= np.linalg.norm(q)
    fem = FemGelpad(B, "cuda:0", motion="rolling")
    mcfg = ManiSkillSimulatorCfg(tactile_img_res=(320, 240), device="cuda:0", camera_pos_w=tuple(cam), camera_quat_w_ros=tuple(q))
    cfg = GelSightSensorCfg(num_envs=B, data_types=["marker_motion"], optical_sim_cfg=None, marker_motion_sim_cfg=mcfg,
                            sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(320, 240)), device="cuda:0")
    cfg.compute_indentation_depth_class = "marker_motion_sim"
    s = GelSightSensor(cfg, gelpad_obj=fem.gelpad)
    s.compute_indentation_depth_func = None
    s.initialize()
    plugin = s.marker_motion_simulator
    for i in range(3):
        fem.step(i)
    w = fem.contact_forces(ref_points=torch.from_numpy(np.repeat(cam[None], B, 0)), per_vertex=True)
    c = plugin.marker_motion_sim.contact_wrench(per_vertex=True)
    c2 = plugin.contact_wrench(per_vertex=True)
    assert np.array_equal(c.record.cpu().numpy(), c2.record.cpu().numpy()) and np.array_equal(c.vertex_forces.cpu().numpy(), c2.vertex_forces.cpu().numpy())
    ww, wx, wy, wz = q
    R = np.array([[1 - 2 * (wy * wy + wz * wz), 2 * (wx * wy - wz * ww), 2 * (wx * wz + wy * ww)],
                  [2 * (wx * wy + wz * ww), 1 - 2 * (wx * wx + wz * wz), 2 * (wy * wz - wx * ww)],
                  [2 * (wx * wz - wy * ww), 2 * (wy * wz + wx * ww), 1 - 2 * (wx * wx + wy * wy)]])
    rw, rc = w.record.cpu().numpy(), c.record.cpu().numpy()
    assert np.all(rw[:, 11] > 0) and np.linalg.norm(rw[:, 3:6], axis=1).min() > 0
    for name, sl in ref.SLOTS.items():
        if name == "centre_of_pressure":
            want = (rw[:, sl] - cam) @ R  # R^T (p - cam), as rows
        elif isinstance(sl, slice):
            want = rw[:, sl] @ R
        else:
            want = rw[:, sl]
        got = getattr(c, name).cpu().numpy()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), name
    np.testing.assert_allclose(c.force.cpu().numpy(), (rw[:, 0:3] + rw[:, 3:6]) @ R, rtol=0, atol=1e-12 * np.abs(rw[:, 0:6]).max())
    want_v = w.vertex_forces.cpu().numpy() @ R
    assert np.abs(c.vertex_forces.cpu().numpy() - want_v).max() <= 1e-12 * np.abs(want_v).max()
    # the camera looks along its z axis at the pad: the same vectors the surface vertices are taken to the camera frame with
    xs = plugin.marker_motion_sim.get_surface_vertices_camera().cpu().numpy()
    np.testing.assert_allclose(xs, (fem.sim.x.cpu().numpy()[:, plugin.marker_motion_sim.surf_vertex_ids] - cam) @ R, rtol=0, atol=1e-14)
