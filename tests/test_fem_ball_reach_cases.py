"""CPU, oracle alone: the cases of tests/fem_ball_reach_cases.py hold what tests/test_fem_ball_reach_gpu.py relies on - a case that lost
its teeth fails here and not silently there.  These are conditions on the INPUTS; the oracle is the only thing that decides."""
import numpy as np
import pytest

import fem_ball_reach_cases as K

TERM_CASES = {"beside-R2": lambda: K.beside(), "beside-R3-l2": lambda: K.beside(0.003, 2), "cube-parallel": K.cube_parallel,
              "over-l0": lambda: K.over(0), "over-l2": lambda: K.over(2)}
FORCE_CASES = ("beside-R2", "cube-parallel")
PAD_IN_ZONE = {"beside-R2": 63, "beside-R3-l2": 63, "cube-parallel": 0, "over-l0": 0, "over-l2": 0}


@pytest.mark.parametrize("name", list(TERM_CASES))
def test_term_case_holds_what_the_gpu_test_relies_on(name):
    """Per env: every pair kind has >= 1 active pair, the pad's face vertices inside the ground's zone are all 63 (beside) or none, every pair
    and ground gap is > 0 and nothing has passed through a surface, and the oracle's gradient - friction lag included - agrees with a
    central difference of its energy along two random directions to 1e-6 relative."""
    c = TERM_CASES[name]()
    sc, V = c.sc, c.V
    assert len(c.face) == 63 and (sc.pad_area[c.face] > 0).all()
    rng = np.random.default_rng(3)
    for b in range(2):
        y, yt, yp = c.y[b], c.yt[b], c.yp[b]
        n, in_pad, in_ball, dmin, gmin = K.counts(c, y)
        print(f"{name} env {b}: pairs {n}, pad / body vertices in the ground's zone {in_pad} / {in_ball}, smallest pair gap {dmin / K.DHAT:.3f} d_hat, "
              f"smallest ground gap {gmin / K.DHAT:.3f} d_hat")
        assert (n >= 1).all() and in_ball >= 1
        assert in_pad == PAD_IN_ZONE[name]
        zone = (K.pad_ground_gaps(c, y) > 0) & (K.pad_ground_gaps(c, y) < K.DHAT)
        assert zone.sum() == PAD_IN_ZONE[name]  # (the face's, not some other surface vertex's)
        assert dmin > 0 and gmin > 0 and not K.penetrates(c, y)
        if name in FORCE_CASES:  # the force record takes its lag at the friction reference: a state like the others
            assert K.counts(c, yp)[3] > 0 and K.counts(c, yp)[4] > 0 and not K.penetrates(c, yp) and K.counts(c, yp)[0].sum() >= 1
        try:
            K.lagged(sc, y, yp)
            g = sc.gradient(y, yt, c.cons, c.aim[b])
            assert np.isfinite(g).all() and np.isfinite(sc.energy(y, yt, c.cons, c.aim[b]))
            for _ in range(2):
                d = rng.standard_normal(y.shape)
                h = 1e-8
                fd = (sc.energy(y + h * d, yt, c.cons, c.aim[b]) - sc.energy(y - h * d, yt, c.cons, c.aim[b])) / (2 * h)
                an = float((g * d).sum())
                print(f"    directional derivative {an:.9e}, central difference {fd:.9e}: {abs(fd - an) / abs(an):.1e} relative")
                assert abs(fd - an) <= 1e-6 * abs(an)
        finally:
            sc._lag = None


def test_cube_pairs_are_exactly_parallel_at_rest_and_nearly_parallel_when_perturbed():
    c = K.cube_parallel()
    m0, m1 = c.sc.pairs(c.y[0])[2][7], c.sc.pairs(c.y[1])[2][7]
    assert (m0 == 0.0).sum() >= 8 and ((m0 == 0.0) | (m0 == 1.0)).all()
    assert ((m1 > 0.0) & (m1 < 1.0)).sum() >= 1
    assert (c.sc.pairs(c.yp[0])[2][7] == 0.0).sum() >= 8  # the force record's lag state keeps them exactly parallel


def test_beside_r2_has_both_friction_branches_on_the_pads_ground_contacts_and_on_the_pairs():
    c = K.beside()
    sc, eps = c.sc, c.sc.eps_v * c.sc.dt
    try:
        slid = [K.lagged(sc, c.y[b], c.yp[b]) for b in range(2)]
        pad_ground = []
        for b, (s, npairs) in enumerate(slid):
            rows = sc._lag[0]
            pad_ground.append(s[npairs:][rows[npairs:, 0] < c.V])
            assert len(pad_ground[-1]) == 63
        pg, pr = np.concatenate(pad_ground), np.concatenate([s[:n] for s, n in slid])
        assert (pg < eps).any() and (pg > eps).any()
        assert (pr < eps).any() and (pr > eps).any()
        assert (slid[0][0] < eps).any() and (slid[1][0] > eps).any()
    finally:
        sc._lag = None


def test_over_l2_press_lists_the_most_pairs_of_its_candidates():
    """`L2_PRESS` is the first candidate of `L2_PRESSES` with the most pairs (both envs together) among those where nothing has passed through
    a surface - beyond it the unsigned distances grow again although the state is invalid."""
    best, best_n = None, -1
    for p in K.L2_PRESSES:
        c = K.over(2, p)
        if any(K.penetrates(c, y) for y in c.y):
            continue
        n = sum(int(K.counts(c, y)[0].sum()) for y in c.y)
        if n > best_n:
            best, best_n = p, n
    assert best == pytest.approx(K.L2_PRESS, rel=1e-12)


def test_pad_on_ground_steps_converge_with_the_face_inside_the_zone():
    """Three oracle steps per env: below the cap of 60 with flag 0, all 63 face vertices inside the ground's zone after every step (and above
    the ground), the ball out of reach; env 1's face slides by more than eps_velocity * dt in at least one step, and friction holds it back
    afterwards (the frictionless run of the same drive ends further than 10 x the step bound away)."""
    c = K.pad_on_ground()
    assert K.counts(c, c.rest)[1] == 0  # starts outside (1.02 d_hat)
    eps = c.sc.eps_v * c.sc.dt
    slid = 0.0
    for b, drive in enumerate(K.GROUND_DRIVES):
        out = K.oracle_steps(K.pad_on_ground, (), drive, 3)
        prev = c.rest
        for y, v, io in out:
            assert io[0] < K.CAP and int(io[2]) == 0, (b, io)
            gaps = K.pad_ground_gaps(c, y)
            assert ((gaps > 0) & (gaps < K.DHAT)).sum() == 63
            assert K.counts(c, y)[0].sum() == 0
            if b == 1:
                slid = max(slid, float(np.hypot(*(y[c.face, :2] - prev[c.face, :2]).T).max()))
            prev = y
        print(f"pad-on-ground env {b}: Newton iterations {[int(o[2][0]) for o in out]}")
    assert slid > eps
    free = K.oracle_steps(K.pad_on_ground, (), K.GROUND_DRIVES[1], 3, False)
    sep = np.abs(free[-1][0][:c.V + 1] - out[-1][0][:c.V + 1]).max()
    print(f"frictionless vs frictional end state of env 1: {sep:.3e} m")
    assert sep > 10 * K.X_TOL


def test_over_l0_step_converges_in_the_oracle():
    c = K.over_step(0)
    (y, v, io), = K.oracle_steps(K.over_step, (0,), (0.0, 0.0, -K.BATCH_DEPTHS[0]), 1)
    assert io[0] < K.CAP and int(io[2]) == 0 and not K.penetrates(c, y)
