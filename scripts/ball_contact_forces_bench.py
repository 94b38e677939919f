"""Time of a `UipcSim.contact_forces()` call on the ball scene (`FemBallScene`: the 8 x 10 x 4 pad over the level-2 ball on the ground, what
bench.py's c4_ball entry steps) next to a step of the same scene: 512 envs, hipEvents around `--calls` calls in a row, the three variants
(without friction, with friction, with per-vertex forces) alternating over `--reps` rounds after a warm-up; then one press-and-release
period of steps, each between two hipEvents, for scale (tacex_fem_ball_step's kernels are those of the parent commit).

  --out FILE   also write the table as markdown."""
import argparse
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=str(Path(__file__).resolve().parent.parent))
ap.add_argument("--envs", type=int, default=512)
ap.add_argument("--steps", type=int, default=10, help="FEM steps before the timing (step 10 is the press peak: every env in contact)")
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
sys.path.insert(0, a.repo)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacex_amd.uipc.gelpad_scene import FemBallScene  # noqa: E402


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3  # us per call


def main():
    B = a.envs
    scene = FemBallScene(B, "cuda:0")
    sim = scene.sim
    for i in range(a.steps + 1):
        scene.step(i)
    torch.cuda.synchronize()
    info = sim.check_step(raise_on_penetration=False)
    variants = {
        "contact_forces(friction=False)": lambda: sim.contact_forces(friction=False),
        "contact_forces()": lambda: sim.contact_forces(),
        "contact_forces(per_vertex=True)": lambda: sim.contact_forces(per_vertex=True),
    }
    w = sim.contact_forces()
    rec = w.record.cpu().numpy()
    assert np.abs(rec[:, 3:6]).max() > 0 and int(rec[:, 11].max()) == 0  # friction really is evaluated, no list overflowed
    for fn in variants.values():
        timed(fn, 20)
    us = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():
            us[k].append(timed(fn, a.calls))
    step_us = []
    for i in range(a.steps + 1, a.steps + 22):  # one period of the press
        step_us.append(timed(lambda: scene.step(i), 1))
    step = float(np.median(step_us))
    rows = [(k, float(np.median(v)), float(min(v)), float(max(v)), float(np.median(v)) / step) for k, v in us.items()]
    rows.append(("FEM step (one period, for scale)", step, float(min(step_us)), float(max(step_us)), 1.0))
    print(f"{B} envs: active pairs per env mean {rec[:, 10].mean():.1f} (max {int(rec[:, 10].max())}), kinds {rec[:, 16:19].mean(0).round(1)}, "
          f"ground contacts of the ball mean {rec[:, 36].mean():.1f}, flagged envs {len(info['pair_list_overflow_envs'])}", flush=True)
    lines = ["| call | median us | min | max | x step |", "|---|---|---|---|---|"]
    lines += [f"| {k} | {m:.1f} | {lo:.1f} | {hi:.1f} | {r:.3f} |" for k, m, lo, hi, r in rows]
    print("\n".join(lines), flush=True)
    if a.out:
        head = (f"# contact_forces() on the ball scene against a step of it\n\n{B} envs, `FemBallScene` (8 x 10 x 4 pad, 495 vertices; level-2 ball, 162 "
                f"vertices / 320 triangles / 480 edges; ground), after {a.steps + 1} steps (press peak); {a.calls} calls per timing between two "
                f"hipEvents, {a.reps} alternating rounds (median, min, max of the rounds), one MI355X.  A call includes its output allocation "
                f"(`torch.empty`) and the ctypes call.  Active pairs per env: mean {rec[:, 10].mean():.1f}, max {int(rec[:, 10].max())}.\n\n")
        Path(a.out).write_text(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
