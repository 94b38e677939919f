"""Time of a `UipcSim.contact_forces()` call against `contact_gaps()` - the same loop over the vertices, one distance evaluation per vertex
instead of two contact evaluations and one friction evaluation - on the C4 scene: 512 envs, the 8 x 10 x 4 pad (495 vertices), FemGelpad's
sphere, then the same scene with a 320-triangle mesh indenter (icosphere level 2) in its place.  hipEvents around `--calls` calls in a row,
the variants alternating over `--reps` rounds after a warm-up; the scene's FEM step is timed beside them for scale.

  --out FILE   also write the table as markdown."""
import argparse
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=str(Path(__file__).resolve().parent.parent))
ap.add_argument("--envs", type=int, default=512)
ap.add_argument("--steps", type=int, default=12, help="FEM steps before the timing (the pad is pressed and sliding: the scene in contact)")
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
sys.path.insert(0, a.repo)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacex_amd.uipc.gelpad_scene import FemGelpad  # noqa: E402
from tacex_amd.uipc.indenter_meshes import icosphere  # noqa: E402


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3  # us per call


def scene(B, mesh):
    fem = FemGelpad(B, "cuda:0", motion="rolling")
    if mesh:
        v, t = icosphere(fem.R, 2)
        assert len(t) == 320
        fem.sim.set_indenter_mesh(v, t)
        fem.ind[:, 0] = 4.0   # the same centre; a kind-4 row reads (radius, n) as (offset, rotation vector): none of either
        fem.ind[:, 4:8] = 0.0
    for i in range(a.steps):
        fem.step(i)
    torch.cuda.synchronize()
    info = fem.sim.check_step(raise_on_penetration=False)
    return fem, info


def main():
    B = a.envs
    rows = []
    for mesh in (False, True):
        fem, info = scene(B, mesh)
        sim = fem.sim
        variants = {
            "contact_gaps()": lambda: sim.contact_gaps(),
            "contact_forces(friction=False)": lambda: sim.contact_forces(friction=False),
            "contact_forces()": lambda: sim.contact_forces(),
            "contact_forces(per_vertex=True)": lambda: sim.contact_forces(per_vertex=True),
        }
        w = sim.contact_forces()
        nc = w.num_contacts.cpu().numpy()
        assert np.abs(w.friction_force.cpu().numpy()).max() > 0  # friction really is evaluated
        for fn in variants.values():
            timed(fn, 20)
        us = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                us[k].append(timed(fn, a.calls))
        step_ms = []
        for i in range(a.steps, a.steps + 8):
            fem.step(i)
            step_ms.append(fem.fem_ms_last())
        name = "320-triangle mesh" if mesh else "sphere"
        base = float(np.median(us["contact_gaps()"]))
        for k, v in us.items():
            rows.append((name, k, float(np.median(v)), float(min(v)), float(max(v)), float(np.median(v)) / base))
        rows.append((name, "FEM step (for scale)", float(np.median(step_ms)) * 1e3, float(min(step_ms)) * 1e3, float(max(step_ms)) * 1e3,
                     float(np.median(step_ms)) * 1e3 / base))
        print(f"{name}: {B} envs, active vertices per env mean {nc.mean():.1f} (max {int(nc.max())}), penetrating envs {len(info['penetrating_envs'])}", flush=True)
        del fem
        torch.cuda.empty_cache()
    lines = ["| indenter | call | median us | min | max | x contact_gaps |", "|---|---|---|---|---|---|"]
    lines += [f"| {n} | {k} | {m:.1f} | {lo:.1f} | {hi:.1f} | {r:.2f} |" for n, k, m, lo, hi, r in rows]
    print("\n".join(lines), flush=True)
    if a.out:
        head = (f"# contact_forces() against contact_gaps(), C4 scene\n\n{B} envs, 8 x 10 x 4 pad (495 vertices), rolling contact after {a.steps} steps; "
                f"{a.calls} calls per timing between two hipEvents, {a.reps} alternating rounds (median, min, max of the rounds), one MI355X.  "
                f"A call includes its output allocation (`torch.empty`) and the ctypes call, like `contact_gaps()`.\n\n")
        Path(a.out).write_text(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
