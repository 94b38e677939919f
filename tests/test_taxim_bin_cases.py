"""CPU: the inputs of tests/taxim_bin_cases.py are what they claim, from the two oracles alone (no GPU).

Lattice: every centre of every family lands on its intended record in the float64 ("direct") and in the float32 ("fft32") oracle,
none is left out by the margin rule, and the rule leaves out fewer than 2 % of the other pixels.  Facets: every interior pixel on the
intended record in both modes, the whole frame in contact.  Composites: at most 6 % of a frame's interior left out, the two modes
agree on every compared non-flat pixel, flat pixels are the record (0, 62).  Special points: the float32 restatement of the
reference's formula (the "fft32" oracle's shade, which blurs nothing) gives the bins the axis-aligned directions and t = 1 lie on."""
import math

import numpy as np
import pytest

import taxim_bin_cases as bc
import taxim_route_cases as rc
from oracle.taxim_oracle import TaximOracle


@pytest.fixture(scope="module")
def calib_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("bin_calib")


@pytest.fixture(scope="module")
def lattice_oracles(calib_dir):
    return TaximOracle(calib_dir, bc.LATTICE_SHAPE, "direct"), TaximOracle(calib_dir, bc.LATTICE_SHAPE, "fft32")


def test_lattice_sites_reach_all_four_borders():
    H, W = bc.LATTICE_SHAPE
    rows, cols = bc.lattice_sites(bc.LATTICE_SHAPE)
    assert rows[0] == 1 and rows[-1] == H - 2 and cols[0] == 1 and cols[-1] == W - 2
    assert np.diff(rows).min() >= 3 and np.diff(cols).min() >= 3, "a centre's four neighbours are its own"
    assert len(rows) * len(cols) * bc.LATTICE_FRAMES >= bc.NREC * bc.NREC


@pytest.mark.parametrize("name", bc.FAMILIES)
def test_lattice_family_lands_on_every_record(name, lattice_oracles):
    od, of = lattice_oracles
    fam = bc.family(name, bc.LATTICE_SHAPE, bc.grad_scales(od.p, bc.LATTICE_SHAPE))
    Z, s = fam["Z"], fam["sites"]
    assert Z.shape == (bc.LATTICE_FRAMES,) + bc.LATTICE_SHAPE and len(s) == bc.NREC * bc.NREC == 15376
    assert len(set(zip(fam["im"], fam["idd"]))) == len(s) and fam["im"].max() == fam["idd"].max() == 123
    c = (s[:, 0], s[:, 1], s[:, 2])
    m = bc.margins(od, Z)
    _, _, _, imf, idf = of.shade(Z, True)
    assert np.array_equal(m["im"][c], fam["im"]) and np.array_equal(m["idd"][c], fam["idd"]), "float64 oracle"
    assert np.array_equal(imf[c], fam["im"]) and np.array_equal(idf[c], fam["idd"]), "float32 oracle"
    assert m["compare"][c].all(), f"{int((~m['compare'][c]).sum())} centres left out by the margin rule"
    # the offsets: EDGE_OFFSET wherever tau allows it, otherwise 2 tau - a small part of a bin everywhere
    print(f"{name}: widest offset from the edge {fam['off_mag'].max():.2e} (magnitude) {fam['off_dir'].max():.2e} (direction) bin widths; "
          f"at EDGE_OFFSET: {np.mean(fam['off_mag'] == bc.EDGE_OFFSET):.1%} / {np.mean(fam['off_dir'] == bc.EDGE_OFFSET):.1%} of the centres")
    assert fam["off_mag"].max() < 1e-3 and fam["off_dir"].max() < 5e-3
    if name == "mag_hi":
        assert np.tan(fam["mag"]).max() <= bc.T_MAX * (1 + 1e-9)
    # the other pixels: the cap of the GPU test, measured here with both oracles
    other = ~bc.site_mask(Z.shape, s)
    left_out = [float((~m["compare"][f][other[f]]).mean()) for f in range(len(Z))]
    cmp_nonflat = other & m["compare"] & ~m["flat"]
    print(f"{name}: margin rule leaves out {max(left_out):.3%} of a frame's non-centre pixels at the most; {int(cmp_nonflat.sum())} compared non-flat ones")
    assert max(left_out) < 0.02
    assert not ((imf != m["im"]) | (idf != m["idd"]))[cmp_nonflat].any(), "the two oracles disagree on a pixel the rule compares"
    assert (m["im"][m["flat"]] == bc.FLAT[0]).all() and (m["idd"][m["flat"]] == bc.FLAT[1]).all()
    assert np.abs(Z[:-1]).max() <= 47.0 or name == "mag_hi", "|Z| <= 47 mm"


def test_special_points_float32_restatement(lattice_oracles):
    od, of = lattice_oracles
    H, W = bc.LATTICE_SHAPE
    names, Z, s = bc.special_frames(od.p, bc.LATTICE_SHAPE)
    _, mag, dr, im, idd = of.shade(Z, True)
    got = {n: (int(im[i, 1, 1]), int(idd[i, 1, 1])) for i, n in enumerate(names)}
    assert got["dir 0"][1] == 62 and got["dir +pi/2"][1] == 93 and got["dir -pi/2"][1] == 31
    assert got["dir +pi"][1] == 124 and got["dir -pi"][1] == 0
    assert got["t 1"] == (62, 93) and mag[names.index("t 1"), 1, 1] == np.float32(math.pi / 4)
    assert got["zero"] == bc.FLAT
    for q, d in (("++", 77), ("+-", 108), ("-+", 46), ("--", 15)):
        assert got["diag " + q][1] == d and got["1e-12 " + q] == (0, d) and got["1e3 " + q] == (123, d)
    # the reference computes a direction from a denormal t^2; the kernels document the flat record there (taxim_device.h, shade_dir_bin)
    assert got["tiny"] == (0, 77) and got["tiny -"] == (0, 46)
    g = (np.float32(1e-20)) ** 2 * 2
    assert 0 < g < np.finfo(np.float32).tiny
    # both sites of a point carry the same record, and so do the four borders around them (replicate padding)
    for i in range(len(names)):
        for a in (im, idd):
            assert a[i, 1, 1] == a[i, H - 2, W - 2] == a[i, 0, 0] == a[i, 0, 1] == a[i, 1, 0] == a[i, H - 1, W - 1] == a[i, H - 1, W - 2]


@pytest.mark.parametrize("name", bc.FACET_CASES)
def test_facets_carry_their_record(name, calib_dir, calib_tmp):
    case = rc.BY_NAME[name]
    ref = bc.reference(case, "facets", calib_dir, calib_tmp)
    inter, m = ref["interior"], ref["m"]
    assert len(ref["hm"]) == 372 and ref["M"].all(), "the whole frame in contact"
    span = ref["hm"].max(axis=(1, 2)) - ref["hm"].min(axis=(1, 2))
    assert (ref["press"] >= 1.05 * span / (1 - 0.4) + 1 - 1e-3).all()
    met = (m["im"] == ref["im"][:, None, None]) & (m["idd"] == ref["idd"][:, None, None])
    assert met[:, inter].all(), "float64 oracle"
    assert m["compare"][:, inter].all(), "zero exclusions"
    # the float32 oracle on 144 of the targets: the magnitude sweep (bins 121..123 among it), ten directions each of bins 0 and 1
    sel = np.r_[0:124, 124:248:13, 248:372:13]
    of = TaximOracle(ref["folder"], case.shape, "fft32")
    Zf, Mf = of.gel_pad_deformation(of.shifted_height_map(ref["hm"][sel], ref["press"][sel]))
    _, _, _, imf, idf = of.shade(Zf, True)
    assert Mf.all() and ((imf == ref["im"][sel, None, None]) & (idf == ref["idd"][sel, None, None]))[:, inter].all(), "float32 oracle"
    print(f"{name}: 372 facets, span up to {span.max() / 1e3:.2f} m, press up to {ref['press'].max() / 1e3:.2f} m")


def test_row_threshold_frames(calib_dir, calib_tmp):
    """One row per frame whose steepest pixel lies 4 tau_mag above (it alone carries bin 1) or below (the whole row is bin 0) the first
    magnitude-bin edge, within 1e-3 of the edge (relative, in t): a magnitude shortcut whose threshold is off by that much shows."""
    case = rc.BY_NAME[bc.ROW_CASE]
    ref = bc.reference(case, "rows", calib_dir, calib_tmp)
    m, Z = ref["m"], ref["Z"]
    assert (ref["oracle"].gel == 0).all(), "the deformed gel is linear in the dent's depth"
    assert rc.stream_strips(case.W)[0] == 1, "one strip: a wave holds a whole row"
    slots = set()
    for f, (y, side) in enumerate(ref["rows"]):
        mag = m["mag"][f, y]
        x = int(mag.argmax())
        slots.add(x % 3)
        assert m["compare"][f, y, x] and m["im"][f, y, x] == (1 if side > 0 else 0)
        assert 0 < side * (mag[x] - bc.X_BINR) < 1e-3 * bc.X_BINR, "within 1e-3 of the edge"
        others = np.delete(np.arange(case.W), x)
        assert (m["im"][f, y, others][m["compare"][f, y, others]] == 0).all() and (m["im"][f, :y] == 0).all(), "every other pixel: bin 0"
        # what the wave's outermost lanes hold (mirrored columns 10..12 and 75..77): a gel of z there is a spurious gradient of at most
        # z gsx when blurred against the zero shifted in from outside the wave - a fifth of the threshold t = 0.0127 at the most
        ends = np.abs(Z[f, y - 1:y + 2][:, [10, 11, 12, 75, 76, 77]]).max()
        assert ends * max(ref["gs"]) < 0.2 * np.tan(bc.X_BINR), ends
        assert ref["M"][f].any() and not ref["M"][f, :y + 2].any(), "a dent in contact, below the probed row"
        print(f"rows frame {f}: row {y} column {x} grad_mag - edge {mag[x] - bc.X_BINR:+.3e} rad, dent {np.abs(Z[f]).max():.3f} mm deep")
    assert slots == {0, 1, 2}, "the steepest pixel takes each of a lane's three pixel slots"


@pytest.mark.parametrize("name", bc.FACET_CASES)
def test_threshold_and_composite_frames(name, calib_dir, calib_tmp):
    case = rc.BY_NAME[name]
    th = bc.reference(case, "threshold", calib_dir, calib_tmp)
    inter = th["interior"]
    zmax = np.abs(th["Z"]).max()
    assert 1.0 <= zmax < 2.0, "threshold_points took ulp32 of these heights"
    assert th["M"].all() and th["m"]["compare"][:, inter].all()
    assert ((th["m"]["im"] == th["im"][:, None, None]) & (th["m"]["idd"] == th["idd"][:, None, None]))[:, inter].all()
    assert sorted(set(th["im"])) == [0, 1]
    for kind in ("half", "strip"):
        ref = bc.reference(case, kind, calib_dir, calib_tmp)
        m = ref["m"]
        assert ref["M"].all()
        share = (~m["compare"][:, inter]).mean(axis=1)
        flat = m["flat"] & inter
        nonflat = m["compare"] & ~m["flat"] & inter
        print(f"{name} {kind}: {len(share)} frames, left out {share.max():.3%} of a frame's interior at the most; {int(nonflat.sum())} compared non-flat "
              f"pixels, {int(flat.sum())} flat ones")
        assert share.max() <= 0.06
        assert (flat.reshape(len(flat), -1).any(1)).all() and (nonflat & ref["facet"]).reshape(len(flat), -1).any(1).all()
        assert (m["im"][flat] == bc.FLAT[0]).all() and (m["idd"][flat] == bc.FLAT[1]).all()
        of = TaximOracle(ref["folder"], case.shape, "fft32")
        Zf, Mf = of.gel_pad_deformation(of.shifted_height_map(ref["hm"], ref["press"]))
        _, _, _, imf, idf = of.shade(Zf, True)
        assert Mf.all() and not ((imf != m["im"]) | (idf != m["idd"]))[nonflat].any(), "the two oracles disagree on a compared pixel"
    s0, s1 = bc.strip_columns(case)
    assert s0 % 4 == 0 and s1 == rc.seams(*case.shape)[1] and s0 != s1
