"""Gel memory on the CPU: the ABI (symbol, refusals before any GPU call), profile validation, the coefficient table against a float64
restatement, and the NumPy restatement of the contract (tests/gel_memory_ref.py) against the model's closed forms: identity, hold then
release, time subdivision, the bound by the deepest past press and the return to exactly zero."""
import math
import re

import numpy as np
import pytest
from conftest import REPO
from gel_memory_ref import DT, F32, GelMemoryRef, closed_form, coefficient_row, rest_plane, sequence, table

ULP32 = 2.0 ** -24


def _lib_and_module():
    from tacex_amd import _lib

    return _lib.load_library(), _lib


def test_symbol_declared_exported_and_bound():
    lib, _lib = _lib_and_module()
    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = re.search(r"tacex_gel_memory\s*\(([^)]*)\)", txt)
    assert decl, "tacex_gel_memory is not declared in include/tacex_hip.h"
    assert hasattr(lib, "tacex_gel_memory") and "tacex_gel_memory" in _lib.SIGNATURES
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["tacex_gel_memory"][1]) == 17
    assert lib.tacex_abi_version() == int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == 20


def test_the_translation_unit_is_built_without_fp_contraction():
    from tacex_amd import _build

    assert "gel_memory.hip" in _build.SOURCES and (REPO / "tacex_amd" / "csrc" / "gel_memory.hip").exists()
    assert "-ffp-contract=off" in _build.FILE_FLAGS["gel_memory.hip"]


def test_exported_from_the_package():
    import tacex_amd

    assert {"GelMemoryProfile", "TactileGelMemory"} <= set(tacex_amd.__all__)
    assert tacex_amd.TactileGelMemory.__module__ == "tacex_amd.gel_memory"
    assert hasattr(tacex_amd.GelSightSensor, "set_gel_memory")
    for name in ("apply", "reset", "randomize", "imprint"):
        assert callable(getattr(tacex_amd.TactileGelMemory, name)), name


# arguments of a valid call (the pointers are never dereferenced: every case below is refused before any GPU call)
_OK = dict(hm=0x1000, state=0x2000, live=0x3000, coef=0x4000, P=1, ids=None, z0=28.5, gh=0.0045, gd=0.024, fmin=0x5000, ind=0x6000,
           rows=None, B=1, H=4, W=8, K=1)


@pytest.mark.parametrize("change, word", [
    (dict(hm=None), b"hm_mm_dev"), (dict(state=None), b"state_dev"), (dict(live=None), b"live_dev"), (dict(coef=None), b"coef_dev"),
    (dict(fmin=None), b"frame_min_dev"), (dict(ind=None), b"indent_mm_dev"),
    (dict(K=0), b"terms"), (dict(K=3), b"terms"), (dict(K=-1), b"terms"), (dict(P=0), b"num_profiles"),
    (dict(B=0), b"num_frames"), (dict(B=-1), b"num_frames"), (dict(H=0), b"height"), (dict(H=-3), b"height"), (dict(W=0), b"width"),
    (dict(W=-5), b"width"), (dict(hm=0x1004), b"aligned"), (dict(state=0x2008), b"aligned"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_refusals_return_2_and_name_the_argument(change, word):
    lib, _lib = _lib_and_module()
    a = dict(_OK, **change)
    rc = lib.tacex_gel_memory(a["hm"], a["state"], a["live"], a["coef"], a["P"], a["ids"], a["z0"], a["gh"], a["gd"], a["fmin"], a["ind"],
                              a["rows"], a["B"], a["H"], a["W"], a["K"], None)
    assert rc == 2
    msg = lib.tacex_last_error()
    assert b"tacex_gel_memory" in msg and word in msg, msg
    with pytest.raises(ValueError):
        _lib.check(rc, "tacex_gel_memory")


def test_profile_validation():
    from tacex_amd import GelMemoryProfile, TactileGelMemory

    GelMemoryProfile().row(DT)
    GelMemoryProfile(tau_s=(0.0, 0.0), weight=(0.5, 0.5), floor_mm=0.0).row(DT)  # tau == 0 and w1 + w2 == 1 are allowed
    for bad in (dict(tau_s=(-0.1, 0.0)), dict(tau_s=(0.1, -1.0)), dict(weight=(-0.1, 0.2)), dict(weight=(0.2, -0.1)),
                dict(weight=(0.6, 0.5)), dict(floor_mm=-1e-6), dict(tau_s=(0.1,)), dict(weight=(0.1, 0.2, 0.3)),
                dict(tau_s=(float("nan"), 0.0)), dict(weight=(float("inf"), 0.0))):
        with pytest.raises(ValueError):
            GelMemoryProfile(**bad).row(DT)
    for dt in (0.0, -0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            GelMemoryProfile().row(dt)
    # the model refuses the same before it looks at the device
    ok = [GelMemoryProfile()]
    for args in ((0, (8, 4), ok), (2, (8, 0), ok), (2, (8, 4), []), (2, (8, 4), [np.zeros(8)]),
                 (2, (8, 4), [GelMemoryProfile(weight=(0.9, 0.2))])):
        with pytest.raises(ValueError):
            TactileGelMemory(*args, device="cuda")
    with pytest.raises(ValueError):
        TactileGelMemory(2, (8, 4), ok, terms=3, device="cuda")
    with pytest.raises(ValueError):
        TactileGelMemory(2, (8, 4), ok, dt=0.0, device="cuda")


def test_coefficient_table_against_float64():
    from tacex_amd import GelMemoryProfile, TactileGelMemory

    cases = [((0.05, 0.4), (0.5, 0.3), 1e-4), ((0.0, 0.02), (0.25, 0.75), 0.0), ((1e-3, 10.0), (0.0, 1.0), 2e-3)]
    for dt in (DT, 1 / 240.0, 0.5):
        got = TactileGelMemory.coefficient_table([GelMemoryProfile(t, w, f) for t, w, f in cases], dt)
        assert got.dtype == np.float32 and got.shape == (3, 8)
        for row, (tau, w, f) in zip(got, cases):
            a = [np.exp(-np.float64(dt) / np.float64(t)) if t > 0 else np.float64(0) for t in tau]
            want = np.array([a[0], (1 - a[0]) * w[0], a[1], (1 - a[1]) * w[1], f, 0, 0, 0], np.float64).astype(np.float32)
            assert np.array_equal(row.view(np.uint32), want.view(np.uint32)), (dt, tau, row, want)
            assert np.array_equal(row, coefficient_row(tau, w, f, dt))
    assert got[1, 0] == 0 and got[1, 1] == np.float32(0.25)  # tau == 0: a = 0, c = w


# -- the restatement against the model's closed forms -----------------------------------------------------------------------------------
def _flat(H, W, d):
    """A map pressed d mm below the rest plane everywhere except the first row (at the far plane)."""
    z0 = rest_plane()
    m = np.full((1, H, W), F32(z0 - F32(d)), F32)
    m[0, 0] = F32(29.0)
    return m


def test_identity_profile_returns_the_input_bits():
    seq = sequence(30, 40)
    for K in (1, 2):
        zero = np.zeros((1, 8), F32)
        for ids in ([0, 0, 0], [5, -1, 1]):  # the all-zero row, and ids outside the table
            ref = GelMemoryRef(3, 30, 40, K, zero, ids)
            for hm in seq:
                out = ref.step(hm)
                assert np.array_equal(out.view(np.uint32), hm.view(np.uint32))
                assert not ref.state.any() and not ref.live.any()


@pytest.mark.parametrize("K", [1, 2])
def test_hold_then_release_matches_the_closed_form(K):
    n, j, d0 = 5, 7, 0.4
    tau, w = (0.05, 0.4), (0.5, 0.3)
    row = coefficient_row(tau, w, 0.0, DT)  # floor_mm = 0: nothing is flushed
    ref = GelMemoryRef(1, 4, 8, K, row[None], [0])
    press, free = _flat(4, 8, d0), np.full((1, 4, 8), F32(29.0), F32)
    d0 = float(rest_plane() - press[0, 1, 0])  # the penetration the map really holds
    for _ in range(n):
        ref.step(press)
    for _ in range(j):
        out = ref.step(free)
    a = [math.exp(-DT / t) for t in tau[:K]]
    want = closed_form(d0, w[:K], a, n, j)
    got = ref.imprint()[0, 1:].astype(np.float64)
    bound = 3 * (n + j) * ULP32
    print(f"K={K}: closed form {want:.9e}, restatement {got[0, 0]:.9e}, relative error {abs(got[0, 0] - want) / want:.3e} (bound {bound:.3e})")
    assert (np.abs(got - want) <= bound * want).all()
    assert not ref.imprint()[0, 0].any()  # the row that was never pressed
    # the released map shows the imprint below the rest plane, nowhere lifted
    z0 = rest_plane()
    assert np.array_equal(out[0, 1:], (z0 - ref.imprint()[0, 1:]).astype(F32)) and (out <= free).all()
    assert ref.live[0] == 1


@pytest.mark.parametrize("K", [1, 2])
def test_time_subdivision(K):
    tau, w, d0 = (0.05, 0.4), (0.5, 0.3), 0.4
    press = _flat(4, 8, d0)
    one = GelMemoryRef(1, 4, 8, K, coefficient_row(tau, w, 0.0, DT)[None], [0])
    two = GelMemoryRef(1, 4, 8, K, coefficient_row(tau, w, 0.0, DT / 2)[None], [0])
    one.step(press)
    two.step(press)
    two.step(press)
    a, b = one.imprint()[0, 1:].astype(np.float64), two.imprint()[0, 1:].astype(np.float64)
    bound = 3 * (1 + 2) * ULP32  # three roundings per step, three steps
    print(f"K={K}: one step {a[0, 0]:.9e}, two half steps {b[0, 0]:.9e}, relative difference {abs(a[0, 0] - b[0, 0]) / a[0, 0]:.3e} (bound {bound:.3e})")
    assert (a > 0).all() and (np.abs(a - b) <= bound * a).all()


@pytest.mark.parametrize("K", [1, 2])
def test_imprint_never_deeper_than_the_deepest_past_press(K):
    H, W = 30, 40
    seq = sequence(H, W)
    ref = GelMemoryRef(3, H, W, K, table(), [0, 1, 0])
    z0 = rest_plane()
    deepest = np.zeros((3, H, W), F32)
    for hm in list(seq) + list(seq):
        deepest = np.maximum(deepest, np.maximum(z0 - hm, F32(0)))
        out = ref.step(hm)
        assert (ref.imprint() <= deepest).all()
        assert (out <= hm).all() and (out >= z0 - deepest).all()


@pytest.mark.parametrize("K", [1, 2])
def test_state_returns_to_exactly_zero(K):
    tau, w, floor, d0, n = (0.02, 0.03), (0.5, 0.3), 1e-4, 0.4, 4
    row = coefficient_row(tau, w, floor, DT)
    ref = GelMemoryRef(1, 4, 8, K, row[None], [0])
    press, free = _flat(4, 8, d0), np.full((1, 4, 8), F32(29.0), F32)
    d0 = float(rest_plane() - press[0, 1, 0])
    for _ in range(n):
        ref.step(press)
    # branch k is flushed at the first release step j with w_k d0 (1 - a_k^n) a_k^j < floor; the state is zero when the last branch is
    counts = []
    for k in range(K):
        a = float(row[2 * k])
        m0 = closed_form(d0, [w[k]], [a], n, 0)
        j = max(1, math.floor(math.log(float(F32(floor)) / m0) / math.log(a)) + 1)
        assert m0 * a ** (j - 1) > floor * (1 + 1e-4) and m0 * a ** j < floor * (1 - 1e-4), "the count must not hinge on rounding"
        counts.append(j)
    steps = max(counts)
    print(f"K={K}: branches flushed after {counts} release steps")
    for _ in range(steps - 1):
        ref.step(free)
    assert ref.state.any() and ref.live[0] == 1
    out = ref.step(free)
    assert not ref.state.any() and ref.live[0] == 0
    assert np.array_equal(out.view(np.uint32), free.view(np.uint32))
    # and from here on the frame is dead: nothing changes
    out = ref.step(free)
    assert not ref.state.any() and ref.live[0] == 0 and np.array_equal(out, free)
