"""CPU: the NumPy reference of the ball scene's contact forces (tests/ball_contact_forces_ref.py) against the oracle's own gradient, the
`BallContactForces` dataclass against the header's record table, and the argument checks that need no device."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ball_contact_forces_ref as R


@pytest.fixture(scope="module")
def scene():
    sc, rest, *_ = R.oracle_scene()
    return sc, rest


def test_scene_is_the_issues(scene):
    sc, _ = scene
    assert (sc.V, len(sc.pad.tets), len(sc.pad_sv), len(sc.pad_edges)) == (189, 576, 154, 456)
    assert (len(sc.ball.X), len(sc.ball.tris), len(sc.ball_edges)) == (42, 80, 120)


@pytest.mark.parametrize("b", [0, 1])
def test_reference_is_the_oracle_gradient_over_minus_dt2(scene, b):
    """forces = -(gradient(kappa, mu) - gradient(kappa = 0, mu = 0)) / dt^2 on the every-term states, to 1e-12 of the largest entry (measured
    5.6e-16 / 3.0e-16); the pair forces on the pad rows and the body's p row cancel to 1e-12 of the largest (measured 3.4e-16 / 1.6e-16);
    and the states hold what the GPU test relies on: all three pair kinds, a ground contact, sticking (env 0) and slipping (env 1)."""
    sc, rest = scene
    V = sc.V
    y, yp = R.issue_states(rest, b)
    out = R.ball_forces_ref(sc, y, lag_state=yp, ref=np.array([0.001, 0.002, 0.003]))
    rec = out["record"]
    assert tuple(rec[16:19]) == ((2, 2, 12) if b == 0 else (2, 1, 9)) and len(out["slid"]) == (17 if b == 0 else 21)
    eps = sc.eps_v * sc.dt
    assert (out["slid"] < eps).all() if b == 0 else (out["slid"] > eps).all()
    assert rec[36] == 1 and 1.0e-4 < rec[15] < 1.2e-4
    yt = y + 1e-5 * np.random.default_rng(11).standard_normal(y.shape)
    cons, aim = np.zeros(V), y[:V] + 1e-5
    kappa, mu = sc.kappa, sc.mu
    try:
        sc._lag = sc.friction_lag(yp)
        g1 = sc.gradient(y, yt, cons, aim)
        sc.kappa, sc.mu, sc._rows_memo = 0.0, 0.0, None
        g0 = sc.gradient(y, yt, cons, aim)
    finally:
        sc.kappa, sc.mu, sc._lag, sc._rows_memo = kappa, mu, None, None
    F = -(g1 - g0) / sc.dt**2
    tot = out["barrier"] + out["ground"] + out["friction_pairs"] + out["friction_ground"]
    err = np.abs(F - tot).max() / np.abs(F).max()
    pairs = out["barrier"]
    bal = np.abs(pairs[:V].sum(0) + pairs[V]).max() / np.abs(pairs).max()
    print(f"env {b}: reference vs gradient {err:.2e}, pair force balance {bal:.2e}")
    assert err <= 1e-12 and bal <= 1e-12
    assert np.array_equal(out["vertex"], tot[:V])
    # the record's sums are those of the rows
    assert np.allclose(rec[20:32].reshape(4, 3), tot[V:], rtol=1e-14, atol=0)
    assert np.allclose(rec[0:3] + rec[3:6], (pairs + out["friction_pairs"])[:V].sum(0), rtol=1e-14, atol=0)


def test_dataclass_properties_are_the_headers_slots():
    from conftest import REPO
    from tacex_amd import _lib
    from tacex_amd.uipc.uipc_sim import BallContactForces, ContactForces

    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+tacex_fem_ball_contact_forces\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["tacex_fem_ball_contact_forces"][1]) == 12
    assert "record_dev (num_envs, 44) f64" in hdr
    kh = (REPO / "tacex_amd" / "csrc" / "fem_ball_contact_forces.h").read_text()
    assert re.search(r"kBallForceSlots\s*=\s*44", kh)
    rec = torch.arange(88, dtype=torch.float64).reshape(2, 44)
    q = torch.zeros((2, 4, 3), dtype=torch.float64)
    q[:, 1:] = torch.eye(3, dtype=torch.float64)
    w = BallContactForces(rec, None, q)
    sl = {"normal_force": slice(0, 3), "friction_force": slice(3, 6), "torque": slice(6, 9), "normal_magnitude": 9, "num_contacts": 10, "flags": 11,
          "centre_of_pressure": slice(12, 15), "min_gap": 15, "num_pairs_by_kind": slice(16, 19), "body_force": slice(20, 23),
          "ground_force_on_body": slice(32, 35), "ground_contacts_body": slice(35, 38), "ground_force_on_pad": slice(38, 41),
          "ground_contacts_pad": slice(41, 43)}
    for name, s in sl.items():
        assert torch.equal(getattr(w, name), rec[:, s]), name
    assert torch.equal(w.force, rec[:, 0:3] + rec[:, 3:6])
    assert torch.equal(w.body_generalized_force, rec[:, 20:32].reshape(2, 4, 3))
    G = rec[:, 23:32].reshape(2, 3, 3)
    assert torch.equal(w.body_torque, torch.cross(q[:, 1:], G, dim=-1).sum(1))
    # the pad side carries ContactForces' names where a counterpart exists (contact_area has none: slot 10 counts pairs here)
    shared = [n for n in vars(ContactForces) if isinstance(vars(ContactForces)[n], property) and n != "contact_area"]
    assert shared and all(isinstance(vars(BallContactForces).get(n), property) for n in shared)
    with pytest.raises(ValueError):
        BallContactForces(rec).body_torque


def test_refusals_that_need_no_device():
    from tacex_amd import _lib
    from tacex_amd.uipc.uipc_sim import UipcSim, UipcSimCfg

    lib = _lib.load_library()
    assert lib.tacex_fem_ball_contact_forces(None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) == 2
    assert b"tacex_fem_ball_contact_forces" in lib.tacex_last_error() and b"null" in lib.tacex_last_error()
    # the Python layer's own checks come before any library call: a sim that was never set up on a device is enough
    sim = UipcSim.__new__(UipcSim)
    sim.cfg, sim.num_envs, sim.device = UipcSimCfg(device="cuda:0"), 2, torch.device("cpu")
    sim._obj, sim._body, sim._ball_friction_ref = SimpleNamespace(num_verts=5), object(), False
    sim.x, sim.q = torch.zeros((2, 5, 3), dtype=torch.float64), torch.zeros((2, 4, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="x must be"):
        sim.contact_forces(x=torch.zeros((3, 5, 3)))
    with pytest.raises(ValueError, match="x must be"):
        sim.contact_forces(x=torch.zeros((2, 4, 3)))
    with pytest.raises(ValueError, match="q must be"):
        sim.contact_forces(q=torch.zeros((1, 4, 3)))
    with pytest.raises(ValueError, match="go together"):
        sim._ball_contact_forces(None, None, None, False, None, x_prev=torch.zeros((2, 5, 3)))
    with pytest.raises(ValueError, match="after a step"):
        sim.contact_forces(friction=True)  # no step yet
    sim._ball_friction_ref = True
    with pytest.raises(ValueError, match="after a step"):
        sim.contact_forces(x=sim.x[:1], q=sim.q[:1], friction=True)  # fewer envs than the step had
    sim._body = None
    with pytest.raises(ValueError, match="affine body"):
        sim.contact_forces(q=sim.q)
