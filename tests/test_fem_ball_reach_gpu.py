"""GPU: `fem_ball_newton_kernel`, `fem_ball_contact_forces_kernel` and `fem_env_order_kernel` beyond the first family of states of
tests/test_fem_ball_gpu.py, against oracle/abd_oracle.py at the bounds those tests already use (energy 1e-10 relative, gradient 1e-9 of its
largest entry, steps 2e-8 m / 2e-7, force records 1e-9): the pad's own ground contact (the record's slots 38-42 are pinned here), a body
with flat faces (exactly parallel edge-edge pairs), bodies of 12 and 162 vertices, the 256-thread instantiation, and the env order of
batches above 256 (ball step) and above 1 024 envs (gelpad step).  The cases are tests/fem_ball_reach_cases.py; what they must hold is
asserted on the CPU in tests/test_fem_ball_reach_cases.py.  PARITY UNPINNED like every FEM row."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ball_contact_forces_ref as R
import fem_ball_reach_cases as K

pytestmark = pytest.mark.gpu

REFP = np.array([[0.001, 0.002, 0.02], [-0.002, 0.001, 0.015]])


def _check_terms(c, E, g, si, friction, what, edge_edge=True):
    """Kernel terms of both envs against the oracle's: finite first, then energy to 1e-10 relative and the gradient of all V + 4 rows to 1e-9
    of its largest entry; no flag.  Returns the oracle's energies."""
    assert np.isfinite(E).all(), (what, E)
    assert np.isfinite(g).all(), (what, np.argwhere(~np.isfinite(g))[:8])
    assert int(si[:, 2].max()) == 0, (what, si)
    Eos = []
    for b in range(2):
        Eo, go = K.oracle_terms(c, b, friction, edge_edge)
        ee, eg = abs(E[b] - Eo) / abs(Eo), np.abs(g[b] - go).max() / np.abs(go).max()
        print(f"{c.name} {what} env {b}: |E - E_oracle| / |E_oracle| = {ee:.2e} (bound 1e-10), max |g - g_oracle| / max |g_oracle| = {eg:.2e} (bound 1e-9)")
        assert ee <= 1e-10, (what, b, E[b], Eo)
        assert eg <= 1e-9, (what, b, eg)
        Eos.append(Eo)
    return Eos


def _step_dev(c, yk, yo):
    V = c.V
    return float(np.abs(yk[:V + 1] - yo[:V + 1]).max()), float(np.abs(yk[V + 1:] - yo[V + 1:]).max())


def _check_step(c, yk, yo, what):
    dx, da = _step_dev(c, yk, yo)
    print(f"{c.name} {what}: pad and translation rows {dx:.2e} m (bound {K.X_TOL:.0e}), affine rows {da:.2e} (bound {K.A_TOL:.0e})")
    assert dx <= K.X_TOL and da <= K.A_TOL, (what, dx, da)


def _clean(info, what):
    assert len(info["penetrating_envs"]) == 0 and len(info["line_search_failed_envs"]) == 0 and len(info["pair_list_overflow_envs"]) == 0, (what, info)
    assert info["newton_iters"].max() < K.CAP and info["newton_iters"].min() >= 1, (what, info)


def _dev(ys, V):
    return (torch.from_numpy(np.stack([y[:V] for y in ys])).cuda(), torch.from_numpy(np.stack([y[V:] for y in ys])).cuda())


def _forces_vs_reference(sim, c, what):
    """The (44,) record and the per-vertex forces of both envs against `ball_forces_ref`, lag taken at the friction reference state."""
    V = c.V
    x, q = _dev(c.y, V)
    xp, qp = _dev(c.yp, V)
    w = sim._ball_contact_forces(x, q, torch.from_numpy(REFP).cuda(), True, True, xp, qp)
    rec, vf = w.record.cpu().numpy(), w.vertex_forces.cpu().numpy()
    assert np.isfinite(vf).all() and np.isfinite(rec[:, R.FORCE_SLOTS]).all(), what
    outs = []
    for b in range(2):
        out = R.ball_forces_ref(c.sc, c.y[b], lag_state=c.yp[b], ref=REFP[b])
        R.compare(rec[b], out["record"], 1e-9, f"{c.name} {what} env {b}")
        scale = max(np.abs(out["record"][R.FORCE_SLOTS]).max(), np.abs(out["vertex"]).max())
        err = np.abs(vf[b] - out["vertex"]).max()
        print(f"{c.name} {what} env {b}: per-vertex forces max |diff| {err:.3e} of largest force entry {scale:.3e}")
        assert err <= 1e-9 * scale, (what, b, err, scale)
        outs.append(out)
    return rec, outs


# ---- 1. terms with the pad in the ground's zone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["beside-R2", "beside-R3-l2"])
def test_terms_with_the_pad_inside_the_grounds_zone_vs_oracle(which):
    """The pad beside the ball, all 63 face vertices inside the ground's barrier zone: energy and gradient with lagged friction (stick in env 0,
    slip in env 1 - on the pad's ground contacts too) and without.  The oracle's gradient WITHOUT `_ground(x, pad_area)` lies more than
    1e-3 of the largest entry from the kernel's: a kernel that dropped the pad's ground term would fail the comparison."""
    c = K.beside() if which == "beside-R2" else K.beside(0.003, 2)
    sim = K.gpu_sim(c)
    for friction in (True, False):
        E, g, si = K.gpu_terms(sim, c, friction)
        _check_terms(c, E, g, si, friction, "friction" if friction else "frictionless")
        for b in range(2):
            _, go = K.oracle_terms(c, b, friction)
            go[:c.V, 2] -= c.sc._ground(c.y[b][:c.V], c.sc.pad_area)[1]
            assert np.abs(g[b] - go).max() > 1e-3 * np.abs(go).max()


# ---- 2. the force record with the pad on the ground -----------------------------------------------------------------------------------
def test_force_record_with_the_pad_on_the_ground_vs_reference():
    """`beside-R2`: the whole record and the per-vertex forces; slots 38:41 (the ground's friction and normal force on the pad) are non-zero,
    slot 41 counts the pad vertices inside the ground's zone (63) and slot 42 is their smallest gap - the slots every other test of the
    record sees as 0 / +inf."""
    c = K.beside()
    sim = K.gpu_sim(c)
    rec, outs = _forces_vs_reference(sim, c, "pad on the ground")
    for b in range(2):
        n_zone = K.counts(c, c.y[b])[1]
        assert (rec[b, 38:41] != 0.0).all(), rec[b, 38:43]
        assert rec[b, 41] == n_zone == 63
        gaps = K.pad_ground_gaps(c, c.y[b])
        assert np.isfinite(rec[b, 42]) and abs(rec[b, 42] - gaps.min()) <= 1e-12 * gaps.min()
        assert rec[b, 40] > 0.0  # the ground pushes the pad up


# ---- 3. steps with the pad pressed onto the ground ------------------------------------------------------------------------------------
def test_steps_with_the_pad_pressed_onto_the_ground_vs_oracle_step():
    """`pad-on-ground`: three tight steps, env 0 driven straight down, env 1 down and along x.  Every step within the step bounds of the
    oracle's, clean, every face vertex above the ground and all 63 inside its zone at the end (kernel and oracle alike); env 1's face is
    held back by the ground's friction: the kernel's end state lies within the bound of the frictional oracle run and further than 10 x
    the bound from the frictionless one."""
    c = K.pad_on_ground()
    ref = [K.oracle_steps(K.pad_on_ground, (), d, 3) for d in K.GROUND_DRIVES]
    sim, out = K.gpu_steps(c, K.GROUND_DRIVES, 3)
    for k, (yk, si, info) in enumerate(out):
        _clean(info, k)
        for b in range(2):
            _check_step(c, yk[b], ref[b][k][0], f"step {k} env {b}")
            assert (K.pad_ground_gaps(c, yk[b]) > 0).all()
    for b in range(2):
        for y in (out[-1][0][b], ref[b][-1][0]):
            gaps = K.pad_ground_gaps(c, y)
            assert ((gaps > 0) & (gaps < K.DHAT)).sum() == 63
    free = K.oracle_steps(K.pad_on_ground, (), K.GROUND_DRIVES[1], 3, False)
    away = _step_dev(c, out[-1][0][1], free[-1][0])[0]
    print(f"pad-on-ground env 1: {away:.3e} m from the frictionless oracle run (must exceed {10 * K.X_TOL:.0e})")
    assert away > 10 * K.X_TOL


# ---- 4. flat body: exactly parallel edge-edge pairs -----------------------------------------------------------------------------------
def test_flat_body_with_exactly_parallel_edge_pairs_vs_oracle():
    """`cube-parallel`: env 0 holds 12 edge-edge pairs whose mollifier is exactly 0 (den = 0 in the segment-segment routine, no defined
    direction between the closest points), env 1 the same pairs nearly parallel (0 < m < 1).  Energy and gradient are finite - asserted
    before the comparison, so a NaN is reported as one - and the oracle's, with and without friction; the force record likewise; and with
    `tacex_fem_set_edge_edge(ctx, 0)` the terms are the oracle's without that pair kind, at another energy."""
    from tacex_amd import _lib

    c = K.cube_parallel()
    sim = K.gpu_sim(c)
    on = None
    for friction in (True, False):
        E, g, si = K.gpu_terms(sim, c, friction)
        on = _check_terms(c, E, g, si, friction, "friction" if friction else "frictionless")
    _forces_vs_reference(sim, c, "flat body")
    _lib.check(sim._lib.tacex_fem_set_edge_edge(sim._handle, 0), "tacex_fem_set_edge_edge")
    c.sc.edge_edge = False
    try:
        E, g, si = K.gpu_terms(sim, c, False)
        off = _check_terms(c, E, g, si, False, "edge-edge off", edge_edge=False)
    finally:
        c.sc.edge_edge, c.sc._rows_memo = True, None
    for b in range(2):
        assert off[b] < on[b] * (1 - 1e-6) and abs(E[b] - on[b]) > 1e-6 * abs(on[b])  # the edge-edge barrier energy is gone


# ---- 5. body sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
def test_body_sizes_terms_and_moments_vs_oracle(level):
    """Icospheres of 12 vertices (fewer than a wave) and of 162 vertices / 320 triangles / 480 edges: terms with and without friction, and
    the body's moments against `AffineBody.S` / `.kv` at rtol 1e-12."""
    c = K.over(level)
    assert len(c.body_pts) == (12 if level == 0 else 162) and len(c.sc.ball_edges) == (30 if level == 0 else 480)
    sim = K.gpu_sim(c)
    for friction in (True, False):
        E, g, si = K.gpu_terms(sim, c, friction)
        _check_terms(c, E, g, si, friction, "friction" if friction else "frictionless")
    S, kv = (C.c_double * 16)(), C.c_double()
    from tacex_amd import _lib
    _lib.check(sim._lib.tacex_fem_ball_moments(sim._handle, S, C.byref(kv)), "moments")
    assert np.allclose(np.array(S).reshape(4, 4), c.sc.ball.S, rtol=1e-12, atol=1e-22)
    assert kv.value == pytest.approx(c.sc.ball.kv, rel=1e-12)


def test_step_of_the_twelve_vertex_body_vs_oracle_step():
    """One tight step of the standard over-the-ball step scene with the icosahedron (the oracle converges there: the CPU test says so)."""
    c = K.over_step(0)
    drive = (0.0, 0.0, -K.BATCH_DEPTHS[0])
    (yo, vo, io), = K.oracle_steps(K.over_step, (0,), drive, 1)
    sim, out = K.gpu_steps(c, [drive, drive], 1)
    _clean(out[0][2], "l0")
    for b in range(2):
        _check_step(c, out[0][0][b], yo, f"env {b}")


# ---- 6. the 256-thread instantiation ---------------------------------------------------------------------------------------------------
_CHILD = r'''
import sys
sys.path[:0] = [REPO, REPO + "/tests"]
import numpy as np
import fem_ball_reach_cases as K

res = {}
for c in (K.beside(), K.cube_parallel()):
    sim = K.gpu_sim(c)
    E, g, si = K.gpu_terms(sim, c, True)
    res[c.name + "__E"], res[c.name + "__g"], res[c.name + "__si"] = E, g, si
for tag, c, drives in (("ground", K.pad_on_ground(), K.GROUND_DRIVES), ("over", K.over_step(1), [(0.0, 0.0, -d) for d in K.BATCH_DEPTHS[:2]])):
    sim, out = K.gpu_steps(c, drives, 1)
    res[tag + "__y"], res[tag + "__si"], res[tag + "__route"] = out[0][0], out[0][1], np.array(sim.newton_route)
np.savez(sys.argv[1], **res)
'''


def test_the_256_thread_instantiation_vs_oracle(tmp_path):
    """`fem_ball_newton_kernel<256>` (TACEX_BALL_NT=256, read once per process: a child process runs it): the terms of `beside-R2` and
    `cube-parallel`, the first step of `pad-on-ground` and the first step of the standard over-the-ball step test, each against the oracle
    at the bounds of the 512-thread tests; the child reports the route (256, -1).  Any library error ends the child at once (non-zero exit)."""
    from conftest import REPO

    script, out = tmp_path / "ball_nt256.py", tmp_path / "nt256.npz"
    script.write_text(f"REPO = {str(REPO)!r}\n" + _CHILD)
    r = subprocess.run([sys.executable, str(script), str(out)], env=dict(os.environ, TACEX_BALL_NT="256"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = np.load(out)
    for c in (K.beside(), K.cube_parallel()):
        _check_terms(c, res[c.name + "__E"], res[c.name + "__g"], res[c.name + "__si"], True, "256 threads")
    for tag, c, fn, args, drives in (("ground", K.pad_on_ground(), K.pad_on_ground, (), K.GROUND_DRIVES),
                                     ("over", K.over_step(1), K.over_step, (1,), [(0.0, 0.0, -d) for d in K.BATCH_DEPTHS[:2]])):
        assert tuple(res[tag + "__route"]) == (256, -1)
        si = res[tag + "__si"]
        assert (si[:, 2] == 0).all() and si[:, 0].max() < K.CAP and si[:, 0].min() >= 1, si
        for b, d in enumerate(drives):
            _check_step(c, res[tag + "__y"][b], K.oracle_steps(fn, args, tuple(d), 3 if tag == "ground" else 2)[0][0], f"256 threads, first step, env {b}")


# ---- 7. large batches: the env order -----------------------------------------------------------------------------------------------------
SPECIAL_KEYS = (0.0, 1.0, 2046.0, 2047.0, 2048.0, 50000.0, 1e300, -5.0, float("nan"))


def _crafted_step_info(B, block, seed):
    """(B,4) step_info rows as "whatever the previous step left" whose key [:,3] + 6 [:,0] takes the special values - both sides of the clamp
    at 2 047, far beyond it, negative, NaN - a block of `block` envs sharing one key (a bucket larger than a wave, filled by atomics), and
    scattered keys for the rest, so that the order is far from index order."""
    rng = np.random.default_rng(seed)
    si = np.zeros((B, 4))
    keys = rng.integers(0, 3000, B).astype(np.float64)
    keys[:len(SPECIAL_KEYS)] = SPECIAL_KEYS
    keys[len(SPECIAL_KEYS):len(SPECIAL_KEYS) + block] = 777.0
    keys = keys[rng.permutation(B)]
    newton = np.where(np.isfinite(keys) & (keys >= 60) & (keys < 1e5), rng.integers(0, 10, B), 0).astype(np.float64)  # split the key over both columns
    si[:, 0], si[:, 3] = newton, keys - 6.0 * newton
    assert np.array_equal(np.sort(si[:, 3] + 6.0 * si[:, 0]), np.sort(keys), equal_nan=True)
    return si


def test_ball_step_of_260_envs_in_crafted_order_vs_oracle_step():
    """B = 260: the smallest batch above the switch of 256 (fem_kernels.hip) that is no multiple of 64, where the ball step takes its envs in
    the order `fem_env_order_kernel` gives.  Env b runs scenario b % 4 - four depths of the standard over-the-ball step scene, which need
    different iteration counts - and after every step lies within the step bounds of the oracle's state of its scenario (the oracle runs once
    per scenario).  Before the second step the step_info rows are overwritten with crafted work counts, so the order is far from index
    order: a duplicated or missing index would leave one env unstepped (or stepped by two workgroups at once).  Two steps, not three: the
    oracle's four scenarios cost about 5 s per pair of steps."""
    c = K.over_step(1)
    B = 260
    drives = [(0.0, 0.0, -K.BATCH_DEPTHS[b % 4]) for b in range(B)]
    ref = [K.oracle_steps(K.over_step, (1,), (0.0, 0.0, -d), 2) for d in K.BATCH_DEPTHS]
    assert len({int(r[0][2][0]) for r in ref}) > 1  # different iteration counts

    def craft(sim, k):
        if k == 1:
            sim.step_info.copy_(torch.from_numpy(_crafted_step_info(B, 200, 7)).cuda())

    sim, out = K.gpu_steps(c, drives, 2, before_step=craft)
    assert sim.newton_route == (512, -1)
    for k, (yk, si, info) in enumerate(out):
        _clean(info, k)
        assert (si[:, 2] == 0).all() and np.isfinite(si).all()
        worst = np.array([_step_dev(c, yk[b], ref[b % 4][k][0]) for b in range(B)]).max(0)
        print(f"ball step of {B} envs, step {k}: worst env {worst[0]:.2e} m (bound {K.X_TOL:.0e}), affine rows {worst[1]:.2e} (bound {K.A_TOL:.0e}); "
              f"Newton iterations per scenario {[int(si[s, 0]) for s in range(4)]}")
        assert worst[0] <= K.X_TOL and worst[1] <= K.A_TOL, (k, worst)
        assert np.abs(yk[0] - yk[1]).max() > 10 * K.X_TOL  # the scenarios differ


def _gel_scene(B, deterministic=True):
    """`_box_scene` (tests/test_fem_dispatch_boundaries_gpu.py) on `gelpad_box_mesh(5, 6, 3)` (168 vertices), env b running scenario
    b % 5: sphere presses with gaps of 0.9, 0.8, 0.7, 0.6 mm and differently sheared back faces, and one env with no indenter (kind 0)."""
    from oracle.fem_oracle import ContactModel, FemModel
    from tacex_amd.uipc import UipcObject, UipcObjectCfg, UipcSim, UipcSimCfg
    from tacex_amd.uipc.uipc_object import gelpad_box_mesh

    P, T = gelpad_box_mesh(5, 6, 3)
    cfg = UipcSimCfg(device="cuda:0")
    cfg.linear_system.deterministic = deterministic
    cfg.newton.velocity_tol = 2e-3
    cfg.linear_system.max_iter, cfg.linear_system.tol_rate = 600, 1e-12
    sim = UipcSim(cfg, num_envs=B)
    gel = UipcObject(UipcObjectCfg(mesh_points=P, mesh_tets=T), sim)
    sim.setup_sim(constraint_strength_ratio=1000.0)
    s = np.arange(B) % 5
    back = np.where(P[:, 2] < 1e-12)[0]
    aim = np.repeat(P[None], B, 0)
    aim[:, :, 0] += 0.0002 * (1 + s)[:, None]
    sim.set_constraints(back, torch.from_numpy(aim[:, back]).cuda())
    cons = np.zeros(len(P)); cons[back] = 1.0
    top, size = P[:, 2].max(), P.max(0)
    face = np.where(P[:, 2] > top - 1e-12)[0]
    mid = P[face[np.argmin(np.hypot(P[face, 0] - size[0] / 2, P[face, 1] - size[1] / 2))]]
    ind = np.zeros((B, 8))
    ind[:, 0] = (s < 4).astype(np.float64)
    ind[:, 1], ind[:, 2], ind[:, 4] = mid[0], mid[1], 0.004
    ind[:, 3] = top + 0.004 + 0.0009 - 1e-4 * s
    sim.set_contact_indenters(torch.from_numpy(ind))
    m = FemModel.build(P, T, youngs=gel.cfg.constitution_cfg.youngs_modulus * 1e6, poisson=gel.cfg.constitution_cfg.poisson_rate,
                       density=gel.cfg.mass_density, dt=cfg.dt, strength=1000.0)
    kappa = cfg.contact.default_contact_resistance * 1e9 * cfg.contact.d_hat
    cms = [ContactModel(gel.surface_vertex_areas(), ind[b].copy(), cfg.contact.d_hat, kappa, cfg.dt) for b in range(min(B, 4))]
    return sim, m, P, cons, aim, cms


@pytest.mark.parametrize("deterministic", [True, False])
def test_gelpad_step_of_1100_envs_in_crafted_order_is_its_five_scenarios(deterministic):
    """B = 1 100 - more than the 1 024 threads of `fem_env_order_kernel`, so its strided loops run twice - on the CU-resident Newton kernel:
    env b runs scenario b % 5 over three steps.  Before the second and third steps the large batch's step_info rows are overwritten with
    crafted keys (0, 1, 2 046, 2 047, 2 048, 50 000, 1e300, -5, NaN, a block of 300 envs sharing one key).

    deterministic: x, v and step_info of env b are BIT-equal to env b % 5 of a 5-env scene stepped the same way (deterministic sweeps are
    bit-identical between runs; the order decides only WHEN an env runs, as the kernel's comment promises).  The deterministic switch runs
    this pad on the 512-thread variant - route (512, -1): `launch_newton` keeps the 256-thread variant for the atomic sweeps - so the
    256-thread route (256, -1) is the second case, atomic sweeps: their summation order depends on timing, two runs of one scenario both
    stop inside the Newton tolerance (2e-3 m/s here) and lie about 1e-6 m apart (measured; the oracle's first step lies as far from the
    kernel's), so an env agrees with its scenario within twice the Newton tolerance times dt per step taken - the bound of
    `test_step_c4_vs_oracle_step_and_convergence_rule` for two solves that stop on the tolerance - with the same flags and iteration counts
    within one; an env the order left out keeps its crafted step_info row and fails that.
    The 5-env scene's first step is also the oracle's `fem_step` at the bounds of `test_step_c4_vs_oracle_step_and_convergence_rule`, so the
    twin is not the only reference."""
    from oracle.fem_oracle import chain_tables, fem_step

    B = 1100
    route = (512, -1) if deterministic else (256, -1)
    twin, m, P, cons, aim, cms = _gel_scene(5, deterministic)
    ind = twin.contact_indenters
    log, inds = [], []
    for k in range(3):
        gap = twin.contact_gaps().amin(1)
        ind[:4, 3] -= 0.3 * gap[:4]
        ind[:4, 1] += 2e-5
        inds.append(ind.clone())
        twin.step(max_newton_iter=40)
        info = twin.check_step()
        assert twin.newton_route == route and twin.newton_kernel_resident is True
        assert len(info["line_search_failed_envs"]) == 0 and info["newton_iters"].max() < 40 and info["newton_iters"].min() >= 1, info
        log.append((twin.x.clone(), twin.v.clone(), twin.step_info.clone()))
        if k == 0:
            x, v = twin.x.cpu().numpy(), twin.v.cpu().numpy()
            fr = (twin.cfg.contact.default_friction_ratio, twin.cfg.contact.eps_velocity, np.zeros(3))
            for b in range(4):
                cms[b].ind[1:4] = ind[b, 1:4].cpu().numpy()
                xo, vo, io = fem_step(m, cms[b], P.copy(), np.zeros_like(P), cons, aim[b], gravity=twin.cfg.gravity, max_newton=40, velocity_tol=2e-3,
                                      pcg_max_iter=600, pcg_tol_rate=1e-12, coarse=twin.coarse_space, chains=chain_tables(twin.vertex_chains, len(P)),
                                      friction=fr, friction_lag="ipc")
                assert abs(int(info["newton_iters"][b]) - int(io[0])) <= 1, (b, info["newton_iters"], io)
                tol = 1e-4 * np.ptp(P) if info["newton_iters"][b] == io[0] else 2 * 2e-3 * twin.cfg.dt
                print(f"5-env twin, first step, env {b}: max |x - x_oracle| {np.abs(x[b] - xo).max():.2e} m (bound {tol:.1e})")
                assert np.abs(x[b] - xo).max() <= tol and np.abs(v[b] - vo).max() <= tol / twin.cfg.dt, b
    assert len({float(log[-1][2][s, 3]) for s in range(5)}) > 1  # the scenarios cost different amounts of work
    big = _gel_scene(B, deterministic)[0]
    sel = torch.arange(B, device="cuda") % 5
    for k in range(3):
        big.contact_indenters.copy_(inds[k][sel])
        if k > 0:
            big.step_info.copy_(torch.from_numpy(_crafted_step_info(B, 300, 11 + k)).cuda())
        big.step(max_newton_iter=40)
        torch.cuda.synchronize()
        assert big.newton_route == route
        xs, vs, sis = log[k]
        if deterministic:
            bad = (~((big.x == xs[sel]).flatten(1).all(1) & (big.v == vs[sel]).flatten(1).all(1) & (big.step_info == sis[sel]).all(1))).nonzero().flatten()
            print(f"gelpad step of {B} envs (deterministic), step {k}: {len(bad)} envs differ from their scenario in some bit (must be 0)")
        else:
            assert bool((big.step_info[:, 2] == sis[sel][:, 2]).all()) and bool(((big.step_info[:, 0] - sis[sel][:, 0]).abs() <= 1).all())
            bound = 2 * 2e-3 * big.cfg.dt * (k + 1)
            dev = (big.x - xs[sel]).abs().flatten(1).amax(1)
            bad = (dev > bound).nonzero().flatten()
            print(f"gelpad step of {B} envs (atomic sweeps, 256 threads), step {k}: worst env {float(dev.max()):.2e} m from its scenario (bound {bound:.1e})")
        assert len(bad) == 0, (k, bad[:16].tolist())
