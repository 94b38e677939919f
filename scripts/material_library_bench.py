"""Material-library timing and calibration on the C4 pad (FemGelpad's breathing scene, 512 envs, hipEvents around every step, warm-up first).

  --nolib          ms per FEM step with NO library set.  Uses only what existed before the library, so `--repo DIR` can point it at a
                   checkout of an older commit (with its own built libtacex_hip.so): run it alternately on both trees for an A/B.
  --stationarity   per material of the test set, a UNIFORM scene (no library): worst |gradient of the plain incremental potential| /
                   contact force over 16 tight rolling steps, on the C4 pad and the 550-vertex pad - the figures behind the bounds of
                   tests/test_material_library_gpu.py.  Old API only as well (`--repo`).
  (default)        library of one against no library; K = 5 (the test set), 64 and 512 materials (log-uniform E in [2e3, 2e5] Pa, ids =
                   env index mod K) against uniform scenes of the softest, the default and the stiffest material, with the mean Newton /
                   PCG iterations per env and step."""
import argparse
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=str(Path(__file__).resolve().parent.parent))
ap.add_argument("--envs", type=int, default=512)
ap.add_argument("--steps", type=int, default=42)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--reps", type=int, default=1)
ap.add_argument("--nolib", action="store_true")
ap.add_argument("--stationarity", action="store_true")
ap.add_argument("--k", default="1,5,64,512")
a = ap.parse_args()
sys.path.insert(0, a.repo)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacex_amd.uipc import gelpad_scene  # noqa: E402
from tacex_amd.uipc.uipc_object import UipcObjectCfg  # noqa: E402
from tacex_amd.uipc.uipc_sim import UipcSimCfg  # noqa: E402

TEST_SET = [(1e4, 0.49, 1000.0, 0.5), (5e3, 0.45, 1100.0, 0.2), (5e4, 0.40, 900.0, 1.0), (2e5, 0.30, 1200.0, 0.8), (2e3, 0.49, 1000.0, 0.05)]


def uniform_scene(B, mat=None, cfg=None, **kw):
    """FemGelpad with ONE material for all envs through the API from before the library: the gelpad object's cfg and the scene's friction."""
    cfg = cfg if cfg is not None else UipcSimCfg(device="cuda:0")
    if mat is None:
        return gelpad_scene.FemGelpad(B, "cuda:0", cfg=cfg, **kw)
    E, nu, rho, f = mat
    cfg.contact.default_friction_ratio = f
    orig = gelpad_scene.UipcObjectCfg

    def with_material(**okw):
        return orig(constitution_cfg=UipcObjectCfg.StableNeoHookeanCfg(youngs_modulus=E / 1e6, poisson_rate=nu), mass_density=rho, **okw)

    gelpad_scene.UipcObjectCfg = with_material
    try:
        return gelpad_scene.FemGelpad(B, "cuda:0", cfg=cfg, **kw)
    finally:
        gelpad_scene.UipcObjectCfg = orig


def time_scene(fem, steps, warmup):
    for i in range(warmup):
        fem.step(i)
    torch.cuda.synchronize()
    ms, newton, pcg, flagged = [], 0.0, 0.0, 0
    per_env = torch.zeros((fem.B, 2), dtype=torch.float64, device="cuda")
    for i in range(warmup, warmup + steps):
        fem.step(i)
        ms.append(fem.fem_ms_last())
        si = fem.sim.step_info
        per_env += si[:, [0, 3]]
        flagged += int(((si[:, 2].long() & 3) != 0).sum())
    per_env = (per_env / steps).cpu().numpy()
    return float(np.mean(ms)), float(np.median(ms)), per_env, flagged


def fmt(r):
    return f"{r[0]:.3f} ms (median {r[1]:.3f}; Newton {r[2][:, 0].mean():.2f}, PCG {r[2][:, 1].mean():.1f} per env and step; envs flagged 1|2: {r[3]})"


def stationarity():
    from oracle.fem_oracle import ContactModel, FemModel, FrictionModel

    for mesh, name in (((8, 10, 4), "C4 pad"), ((9, 10, 4), "550-vertex pad")):
        out = []
        for k, mat in enumerate(TEST_SET):
            cfg = UipcSimCfg(device="cuda:0")
            cfg.newton.velocity_tol = 1e-7
            cfg.linear_system.tol_rate = 1e-12
            B = 6
            fem = uniform_scene(B, mat, cfg, max_newton_iter=200, motion="rolling", d_hat=1e-3, friction_lag="ipc", mesh=mesh)
            sim, obj = fem.sim, fem.gelpad
            c = obj.cfg.constitution_cfg
            m = FemModel.build(obj.points, obj.tets, youngs=c.youngs_modulus * 1e6, poisson=c.poisson_rate, density=obj.cfg.mass_density, dt=sim.cfg.dt,
                               strength=1000.0)
            area = obj.surface_vertex_areas()
            cc = sim.cfg.contact
            kappa = cc.default_contact_resistance * 1e9 * cc.d_hat
            worst, ind_prev, n, bad, iters = 0.0, None, 0, 0, 0
            for i in range(16):
                x_n, v_n = sim.x.cpu().numpy().copy(), sim.v.cpu().numpy().copy()
                fem.step(i)
                info = sim.check_step(raise_on_penetration=False)
                bad += len(info["penetrating_envs"]) + len(info["line_search_failed_envs"])
                iters = max(iters, int(info["newton_iters"].max()))
                x_end, ind_now = sim.x.cpu().numpy(), fem.ind.cpu().numpy().copy()
                if ind_prev is None:
                    ind_prev = ind_now
                for b in range(B):
                    cons, aim = sim.is_constrained[b].cpu().numpy().astype(np.float64), sim.aim_position[b].cpu().numpy()
                    xt = x_n[b] + sim.cfg.dt * v_n[b] + sim.cfg.dt**2 * np.asarray(sim.cfg.gravity, np.float64)
                    cm = ContactModel(area, ind_now[b], cc.d_hat, kappa, sim.cfg.dt)
                    g = m.gradient(x_end[b], xt, cons, aim) + cm.gradient(x_end[b])
                    scale = np.abs(cm.gradient(x_end[b])).max()
                    fr = FrictionModel(ContactModel(area, ind_prev[b], cc.d_hat, kappa, sim.cfg.dt), x_n[b], ind_now[b, 1:4] - ind_prev[b, 1:4],
                                       mat[3], cc.eps_velocity)
                    if fr.lam.max() > 0.0:
                        g = g + fr.gradient(x_end[b])
                    if scale > 0.0:
                        n += 1
                        worst = max(worst, np.abs(g).max() / scale)
                ind_prev = ind_now
            print(f"{name}, route {sim.newton_route}, material {k} {mat}: worst |grad| / contact force {worst:.3e} over {n} env-steps in contact; "
                  f"flagged (1|2) env-steps {bad}, most Newton iterations {iters}", flush=True)
            out.append(worst)
        print(f"{name}: ratios {['%.2e' % w for w in out]}", flush=True)


def main():
    B = a.envs
    print(f"tree {a.repo}, {B} envs, {a.steps} timed steps after {a.warmup}", flush=True)
    if a.stationarity:
        return stationarity()
    if a.nolib:
        for r in range(a.reps):
            print(f"  no library: {fmt(time_scene(uniform_scene(B), a.steps, a.warmup))}", flush=True)
        return
    from tacex_amd.uipc import GelMaterialCfg

    def cfgs(mats):
        return [GelMaterialCfg(youngs_modulus=E / 1e6, poisson_rate=nu, mass_density=rho, friction_ratio=f) for E, nu, rho, f in mats]

    print(f"  no library:             {fmt(time_scene(uniform_scene(B), a.steps, a.warmup))}", flush=True)
    for k in (int(s) for s in a.k.split(",")):
        if k == 1:
            mats = TEST_SET[:1]
        elif k == 5:
            mats = TEST_SET
        else:
            rng = np.random.default_rng(k)
            mats = [(float(E), float(rng.uniform(0.3, 0.49)), float(rng.uniform(900, 1200)), float(rng.uniform(0.05, 1.0)))
                    for E in np.exp(np.linspace(np.log(2e3), np.log(2e5), k))]
        ids = np.arange(B) % k
        fem = gelpad_scene.FemGelpad(B, "cuda:0", materials=cfgs(mats), material_ids=ids)
        r = time_scene(fem, a.steps, a.warmup)
        bad = len(fem.sim.check_step(raise_on_penetration=False)["bad_material_id_envs"])
        print(f"  library of {k:3d}:         {fmt(r)}; bad ids {bad}", flush=True)
        if k == 5:
            for m in range(5):
                sel = ids == m
                print(f"      material {m} {TEST_SET[m]}: Newton {r[2][sel, 0].mean():.2f}, PCG {r[2][sel, 1].mean():.1f} per env and step")
        if k > 1:
            E = np.array([m[0] for m in mats])
            for what, m in (("softest", mats[int(E.argmin())]), ("default", TEST_SET[0]), ("stiffest", mats[int(E.argmax())])):
                print(f"      uniform, {what:8s} {fmt(time_scene(uniform_scene(B, m), a.steps, a.warmup))}", flush=True)
        del fem
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
