"""GPU: the Taxim shading bin by bin - every table record, every bin edge, every ending of a render, and the wave-uniform shortcuts
of the streaming tail at their thresholds - against the float64 oracle, record for record (100 %, not the 99 % of the parity protocol,
which is made for the reference's noisy flat regions and lets a wrong record or a shifted edge pass).

The inputs and the rule that says which pixels must agree come from tests/taxim_bin_cases.py (checked on the CPU by
tests/test_taxim_bin_cases.py): the lattice goes straight into `shade_kernel`, facets and composites through `render_direct` on the
streaming tail, the LDS-tiled tail and the shade-alone ending.  Every case prints the records / pixels it asserted, the share the
margin rule left out and the largest RGB error."""
import numpy as np
import pytest
import torch

import taxim_bin_cases as bc
import taxim_route_cases as rc
from parity import rgb_rel_err

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4  # parity.rgb_rel_err, the project's tolerance


@pytest.fixture(scope="module")
def calib_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("bin_calib")


@pytest.fixture(scope="module")
def lattice(calib_dir):
    from oracle.taxim_oracle import TaximOracle
    from tacex_amd.simulation_approaches.gpu_taxim.sim import Taxim

    return (Taxim(calib_folder=calib_dir, backend="hip", device="cuda:0"), TaximOracle(calib_dir, bc.LATTICE_SHAPE, "direct"),
            TaximOracle(calib_dir, bc.LATTICE_SHAPE, "fft32"))


def _shade(tx, Z):
    rgb, idx = tx.shade(torch.from_numpy(np.ascontiguousarray(Z)).cuda(), return_bins=True)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy().astype(np.int64)
    return rgb.cpu().numpy(), idx[..., 0], idx[..., 1]


def _assert_replicated(im, idd):
    """Rows 0 / H-1 and columns 0 / W-1 carry the bins of the clamped pixel (replicate padding of the gradient maps)."""
    H, W = im.shape[-2:]
    yy, xx = np.clip(np.arange(H), 1, H - 2), np.clip(np.arange(W), 1, W - 2)
    for a in (im, idd):
        np.testing.assert_array_equal(a, a[:, yy][:, :, xx])


def _mismatches(what, where, im, idd, m, limit=8):
    """Printed before a failing bin assertion: the offending (t, dir), the kernel's bins and the oracle's."""
    bad = np.argwhere(where & ((im != m["im"]) | (idd != m["idd"])))
    for f, y, x in bad[:limit]:
        print(f"  {what}: frame {f} pixel ({y}, {x}) t {np.tan(m['mag'][f, y, x]):.9g} dir {m['dir'][f, y, x]:.9g} rad = bins "
              f"{m['mag'][f, y, x] / bc.X_BINR:.6f} / {(m['dir'][f, y, x] + np.pi) / bc.Y_BINR:.6f}: kernel ({im[f, y, x]}, {idd[f, y, x]}) "
              f"oracle ({m['im'][f, y, x]}, {m['idd'][f, y, x]})")
    return len(bad)


# ---- a. shade_kernel on the lattice ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.FAMILIES)
def test_shade_kernel_lattice(name, lattice):
    tx, od, _ = lattice
    fam = bc.family(name, bc.LATTICE_SHAPE, bc.grad_scales(od.p, bc.LATTICE_SHAPE))
    Z, s = fam["Z"], fam["sites"]
    m = bc.margins(od, Z)
    rgb, im, idd = _shade(tx, Z)
    c = (s[:, 0], s[:, 1], s[:, 2])
    centre = bc.site_mask(Z.shape, s)
    other = ~centre & m["compare"]
    left_out = max(float((~m["compare"][f][~centre[f]]).mean()) for f in range(len(Z)))
    err = rgb_rel_err(rgb, m["rgb"]).max(-1)
    n_bad = _mismatches(name + " centre", centre, im, idd, m) + _mismatches(name + " other", other, im, idd, m)
    print(f"lattice {name}: {len(s)} records asserted at their centres, {int(other.sum())} other pixels compared, margin rule left out "
          f"{left_out:.3%} of a frame's non-centre pixels at the most; largest RGB error centres {err[c].max():.2e} others {err[other].max():.2e}; "
          f"{n_bad} bin mismatches")
    assert len(s) == 15376 and m["compare"][c].all()
    assert np.array_equal(im[c], fam["im"]) and np.array_equal(idd[c], fam["idd"]), "a centre is not on its record"
    assert err[c].max() <= RGB_TOL
    assert left_out < 0.02
    assert np.array_equal(im[other], m["im"][other]) and np.array_equal(idd[other], m["idd"][other])
    assert err[other].max() <= RGB_TOL
    _assert_replicated(im, idd)


def test_shade_kernel_special_points(lattice):
    """Axis-aligned directions (exactly on a bin edge), t = 1 (on a magnitude edge), diagonals, zero, 1e-12 and 1e3 per quadrant:
    the bins of the reference's float32 formula, restated in NumPy float32.  t^2 < FLT_MIN: the flat record (taxim_device.h,
    shade_dir_bin) - the reference would compute a direction from a denormal."""
    tx, od, of = lattice
    H, W = bc.LATTICE_SHAPE
    names, Z, s = bc.special_frames(od.p, bc.LATTICE_SHAPE)
    ref_rgb, mag32, dir32, im32, idd32 = of.shade(Z, True)
    flat_rgb = od.shade(np.zeros((1, H, W), np.float32))[0]
    rgb, im, idd = _shade(tx, Z)
    worst, wrong = 0.0, []
    for (f, y, x) in s:
        n = names[f]
        want = bc.FLAT if n.startswith("tiny") else (int(im32[f, y, x]), int(idd32[f, y, x]))
        want_rgb = flat_rgb[y, x] if n.startswith("tiny") else ref_rgb[f, y, x]
        got = (int(im[f, y, x]), int(idd[f, y, x]))
        e = float(rgb_rel_err(rgb[f, y, x], want_rgb).max())
        worst = max(worst, e)
        if got != want or e > RGB_TOL:
            wrong.append(n)
            print(f"  special '{n}' at ({y}, {x}): kernel {got}, float32 restatement {want} (grad_mag {mag32[f, y, x]!r} = bin "
                  f"{np.float32(mag32[f, y, x]) / np.float32(bc.X_BINR)!r}, grad_dir {dir32[f, y, x]!r}); RGB error {e:.2e}")
    print(f"special points: {len(names)} points at {len(s)} sites; largest RGB error {worst:.2e}; wrong: {sorted(set(wrong))}")
    assert not wrong
    _assert_replicated(im, idd)


# ---- b / c / d. every ending of a render -----------------------------------------------------------------------------------------------
def _endings(case):
    """(name, tail mode, with frames): the streaming tail, the LDS-tiled tail (mode 2, z_out / mask_out) - or shade alone."""
    return [("stream", 1, False), ("tiled", 2, True)] if case.n_fused else [("shade", 1, False)]


def _taxim(case, folder):
    from tacex_amd.simulation_approaches.gpu_taxim.sim import Taxim

    tx = Taxim(calib_folder=folder, backend="hip", device="cuda:0")
    routes = tx.level_routes(case.shape)
    assert routes == {"ksize": list(case.ksize), "levels": case.level_routes, "tail": case.tail, "tail_frames": case.tail_frames}, routes
    return tx


def _render_endings(tx, case, hm, press):
    """RGB (NHWC, NumPy) per ending; the route is read back before every render."""
    B, (H, W) = hm.shape[0], case.shape
    out = {}
    for name, mode, frames in _endings(case):
        tx.set_fused_tail(case.shape, mode)
        assert tx.level_routes(case.shape)["tail_frames" if frames else "tail"] == name
        rgb = torch.empty((B, H, W, 3), device="cuda")
        z = torch.empty((B, H, W), device="cuda") if frames else None
        mk = torch.empty((B, H, W), dtype=torch.uint8, device="cuda") if frames else None
        tx.render_direct(hm, False, press, out=rgb, z_out=z, mask_out=mk)
        torch.cuda.synchronize()
        out[name] = rgb
    tx.set_fused_tail(case.shape, 1)
    return out


def _deform_and_bins(tx, case, ref):
    """The HIP path's own deformed gel within bc.z_tolerance of the oracle's, and the bins `shade_kernel` gives for it."""
    hm, press = torch.from_numpy(ref["hm"].copy()).cuda(), torch.from_numpy(ref["press"].copy()).cuda()
    tx.set_fused_tail(case.shape, 1)
    Z, M = tx.deform(hm, press)
    torch.cuda.synchronize()
    assert bool(M.bool().all()), "the whole frame in contact"
    z_err = np.abs(Z.cpu().numpy().astype(np.float64) - ref["Z"]).max(axis=(1, 2))
    tol = bc.z_tolerance(ref["Z"])  # 1e-5 mm; 4 ulp32 of max |Z| where a facet spans more than 100 mm (1e-5 mm is below one ulp there)
    _, idx = tx.shade(Z, return_bins=True)
    idx = idx.cpu().numpy().astype(np.int64)
    return hm, press, z_err, tol, idx[..., 0], idx[..., 1]


@pytest.mark.parametrize("name", bc.FACET_CASES)
def test_facets_every_ending(name, calib_dir, calib_tmp):
    """372 facets per case - every magnitude bin, every direction bin at magnitude bin 0 (the streaming tail's LDS records) and at
    magnitude bin 1 (its first gathered record): bins equal the target on every interior pixel, RGB of every ending within 1e-4 of the
    float64 oracle there, streaming and tiled RGB bit-equal."""
    case = rc.BY_NAME[name]
    ref = bc.reference(case, "facets", calib_dir, calib_tmp)
    tx = _taxim(case, ref["folder"])
    inter, m = ref["interior"], ref["m"]
    hm, press, z_err, tol, im, idd = _deform_and_bins(tx, case, ref)
    where = np.broadcast_to(inter, im.shape)
    n_bad = _mismatches(name, where, im, idd, m)
    rgbs = _render_endings(tx, case, hm, press)
    errs = {k: float(rgb_rel_err(v.cpu().numpy(), m["rgb"])[:, inter].max()) for k, v in rgbs.items()}
    print(f"facets {name}: {len(ref['im'])} records asserted on {int(where.sum())} interior pixels, margin rule left out "
          f"{(~m['compare'][:, inter]).mean():.3%}; {n_bad} bin mismatches; max |Z - Zo| {z_err.max():.3e} mm (worst ratio to its bound "
          f"{(z_err / tol).max():.2f}); largest RGB error " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert (z_err <= tol).all()
    assert np.array_equal(im[:, inter], np.broadcast_to(ref["im"][:, None], im[:, inter].shape))
    assert np.array_equal(idd[:, inter], np.broadcast_to(ref["idd"][:, None], idd[:, inter].shape))
    assert max(errs.values()) <= RGB_TOL, errs
    if case.n_fused:
        assert torch.equal(rgbs["stream"], rgbs["tiled"]), "streaming and tiled RGB must be bit-equal"


def test_magnitude_shortcut_where_it_is_taken(calib_dir, calib_tmp):
    """The streaming tail skips the magnitude evaluation of a row segment whose gradients all lie below the first magnitude-bin edge.
    A frame in contact everywhere never takes that path (bc.row_threshold_frames); here a dent in an untouched gel puts ONE pixel of a
    row 4 tau_mag above the edge (it alone must make the wave evaluate, and carries bin 1) or the whole row 4 tau_mag below it."""
    case = rc.BY_NAME[bc.ROW_CASE]
    ref = bc.reference(case, "rows", calib_dir, calib_tmp)
    tx = _taxim(case, ref["folder"])
    m = ref["m"]
    hm, press = torch.from_numpy(ref["hm"].copy()).cuda(), torch.from_numpy(ref["press"].copy()).cuda()
    Z, M = tx.deform(hm, press)
    np.testing.assert_array_equal(M.cpu().numpy().astype(bool), ref["M"])
    z_err = float(np.abs(Z.cpu().numpy().astype(np.float64) - ref["Z"]).max())
    _, idx = tx.shade(Z, return_bins=True)
    idx = idx.cpu().numpy().astype(np.int64)
    im, idd = idx[..., 0], idx[..., 1]
    cmp_ = m["compare"]
    n_bad = _mismatches("rows", cmp_, im, idd, m)
    rgbs = _render_endings(tx, case, hm, press)
    errs = {k: rgb_rel_err(v.cpu().numpy(), m["rgb"]).max(-1) for k, v in rgbs.items()}
    probe = {k: max(float(e[f, y, int(m["mag"][f, y].argmax())]) for f, (y, _) in enumerate(ref["rows"])) for k, e in errs.items()}
    print(f"rows {case.name}: {len(ref['rows'])} frames, {int(cmp_.sum())} pixels compared, margin rule left out {(~cmp_).mean():.3%} (a gel "
          f"that is almost flat: tau_dir grows with 1 / t); {n_bad} bin mismatches; max |Z - Zo| {z_err:.3e} mm; largest RGB error "
          + ", ".join(f"{k} {e[cmp_].max():.2e} (probed pixels {probe[k]:.2e})" for k, e in errs.items()))
    assert z_err <= 1e-5
    assert np.array_equal(im[cmp_], m["im"][cmp_]) and np.array_equal(idd[cmp_], m["idd"][cmp_])
    for f, (y, side) in enumerate(ref["rows"]):
        x = int(m["mag"][f, y].argmax())
        assert cmp_[f, y, x] and im[f, y, x] == (1 if side > 0 else 0)
    assert max(float(e[cmp_].max()) for e in errs.values()) <= RGB_TOL
    assert torch.equal(rgbs["stream"], rgbs["tiled"]), "streaming and tiled RGB must be bit-equal"


@pytest.mark.parametrize("name", bc.FACET_CASES)
def test_shortcuts_at_their_thresholds(name, calib_dir, calib_tmp):
    """Facets 4 tau_mag below and above the first magnitude-bin edge in 8 directions (bin 0 below - the streaming tail's skipped
    magnitude evaluation and LDS records -, bin 1 above), and composite frames that put one facet lane group into a wave that is flat
    everywhere else (half frames; 4-column strips at a lane-group boundary and at the seam column): compared pixels carry the oracle's
    bins and RGB, flat pixels the record (0, 62)."""
    case = rc.BY_NAME[name]
    tx = None
    for kind in ("threshold", "half", "strip"):
        ref = bc.reference(case, kind, calib_dir, calib_tmp)
        tx = tx or _taxim(case, ref["folder"])
        inter, m = ref["interior"], ref["m"]
        hm, press, z_err, tol, im, idd = _deform_and_bins(tx, case, ref)
        cmp_ = m["compare"] & inter
        flat = m["flat"] & inter
        share = (~m["compare"][:, inter]).mean(axis=1)
        n_bad = _mismatches(f"{name} {kind}", cmp_, im, idd, m)
        rgbs = _render_endings(tx, case, hm, press)
        errs = {k: float(rgb_rel_err(v.cpu().numpy(), m["rgb"])[cmp_].max()) for k, v in rgbs.items()}
        errs_flat = {k: float(rgb_rel_err(v.cpu().numpy(), m["rgb"])[flat].max()) if flat.any() else 0.0 for k, v in rgbs.items()}
        print(f"{kind} {name}: {len(share)} frames, {int(cmp_.sum())} pixels compared ({int(flat.sum())} flat), margin rule left out {share.max():.3%} "
              f"of a frame's interior at the most; {n_bad} bin mismatches; max |Z - Zo| {z_err.max():.3e} mm; largest RGB error "
              + ", ".join(f"{k} {e:.2e} (flat {errs_flat[k]:.2e})" for k, e in errs.items()))
        assert (z_err <= tol).all()
        assert share.max() <= 0.06
        if kind == "threshold":
            assert share.max() == 0.0
            assert np.array_equal(im[:, inter], np.broadcast_to(ref["im"][:, None], im[:, inter].shape)), "bin 0 below the edge, bin 1 above"
        assert np.array_equal(im[cmp_], m["im"][cmp_]) and np.array_equal(idd[cmp_], m["idd"][cmp_])
        assert (im[flat] == bc.FLAT[0]).all() and (idd[flat] == bc.FLAT[1]).all(), "flat pixels carry the record (0, 62)"
        assert max(errs.values()) <= RGB_TOL and max(errs_flat.values()) <= RGB_TOL, (errs, errs_flat)
        if case.n_fused:
            assert torch.equal(rgbs["stream"], rgbs["tiled"]), "streaming and tiled RGB must be bit-equal"
