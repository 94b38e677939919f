"""Time of the contact force field (`TactileContactModel`, one launch of tacex_contact_field) on 2048 frames of 320 x 240 - a C3 step's
height maps - for record + cells with and without the contact rectangles, and with the traction image, on sparse contact (one random
indenter per frame, a tenth of the frames flat) and on dense contact (a wavy plate over the whole sensor).  hipEvents around `--calls`
calls in a row, the variants alternating over `--reps` rounds after a warm-up.  Beside them, with the same events:
  - a copy of the height maps (`copy_`: 4 B / pixel read and 4 B / pixel written, 16-byte accesses) and the time ONE read of them takes
    at the 6.29 TB/s float4-copy rate of one MI355X (derived, not measured);
  - the same model written in torch ops (record sums and cells by index_add; not bit-equal, a cost comparison).

  --out FILE   also write the table as markdown."""
import numpy as np
import torch
from _bench_util import COPY_TBS, copy_ms, emit, parse_args, repeated, rounds, table

a = parse_args(calls=100, torch_calls=5, torch_help="calls per timing of the torch restatement (it is tens of times slower)")

from tacex_amd import ContactGel, TactileContactModel, _lib  # noqa: E402
from tacex_amd.utils.synthetic import PIXMM, dense_contact_depth_maps, synthetic_depth_maps  # noqa: E402

GRID = (9, 11)


def depth_pass(hm):
    lib = _lib.load_library()
    B, H, W = hm.shape
    fmin, ind = torch.zeros(B, device=hm.device), torch.zeros(B, device=hm.device)
    rows = torch.zeros((B, 4), dtype=torch.int32, device=hm.device)
    _lib.check(lib.tacex_indentation_depth(_lib.ptr(hm), 0.0045, 0.024, _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(rows), B, H, W,
                                           _lib.current_stream_handle(hm.device)), "tacex_indentation_depth")
    return fmin, ind, rows


def torch_restatement(hm, fmin, ind, gel, slip, pixmm, cell_of_pixel, ncells):
    """The model a user would write without the kernel: float32 per pixel, float64 sums, cells by index_add."""
    B, H, W = hm.shape
    kn, kt, mu = gel
    d = (-((hm - fmin[:, None, None]) - ind[:, None, None])).clamp_(min=0)
    p = kn * d
    jj = torch.arange(W, device=hm.device, dtype=torch.float32)[None, None, :]
    ii = torch.arange(H, device=hm.device, dtype=torch.float32)[None, :, None]
    rx, ry = (jj - slip[:, 3, None, None]) * pixmm, (ii - slip[:, 4, None, None]) * pixmm
    ux, uy = slip[:, 0, None, None] - slip[:, 2, None, None] * ry, slip[:, 1, None, None] + slip[:, 2, None, None] * rx
    n = torch.sqrt(ux * ux + uy * uy)
    on = d > 0
    s = torch.where(on & (n > 0), torch.minimum(kt * n, mu * p) / n, torch.zeros_like(n))
    area = pixmm * pixmm * 1e-6
    f = torch.stack((ux * s * area, uy * s * area, -p * area), dim=-1).double()  # (B,H,W,3)
    force = f.sum(dim=(1, 2))
    pd = p.double()
    sp = pd.sum(dim=(1, 2)).clamp_(min=1e-300)
    cop = torch.stack(((pd * jj).sum(dim=(1, 2)) / sp, (pd * ii).sum(dim=(1, 2)) / sp), dim=1)
    count = on.sum(dim=(1, 2))
    nslip = (on & (kt * n >= mu * p)).sum(dim=(1, 2))
    cells = torch.zeros((B, ncells, 3), dtype=torch.float64, device=hm.device).index_add_(1, cell_of_pixel, f.view(B, H * W, 3))
    return force, cop, count, nslip, cells.float()


def main():
    B, H, W = a.frames, a.height, a.width
    dev = "cuda:0"
    inputs = {"sparse contact": synthetic_depth_maps(B, H, W, seed=3, device=dev, flat_fraction=0.1)[0],
              "dense contact": dense_contact_depth_maps(B, H, W, seed=3, device=dev)[0]}
    gels = [ContactGel(3.0e4, 1.2e4, 0.6), ContactGel(8.0e4, 5.0e4, 0.35)]
    model = TactileContactModel(gels, B, dev, pixmm=PIXMM, grid=GRID)
    model.randomize(generator=torch.Generator(device=dev).manual_seed(2))
    g = torch.Generator().manual_seed(4)
    u = torch.rand((B, 5), generator=g)
    slip = torch.stack((0.06 * (u[:, 0] - 0.5), 0.06 * (u[:, 1] - 0.5), 0.2 * (u[:, 2] - 0.5), (0.3 + 0.4 * u[:, 3]) * W, (0.3 + 0.4 * u[:, 4]) * H), dim=1).to(dev)
    image = torch.empty((B, H, W, 3), device=dev)
    copy_dst = torch.empty((B, H, W), device=dev)
    variants, info = {}, {}
    for tag, hm in inputs.items():
        fmin, ind, rows = depth_pass(hm)
        r = rows.cpu().numpy().astype(np.int64)
        rect = np.clip(r[:, 1] - r[:, 0] + 1, 0, None) * np.clip(r[:, 3] - r[:, 2] + 1, 0, None)
        info[tag] = f"{tag}: the contact rectangles cover {rect.sum() / (B * H * W):.1%} of the pixels, {int((rect == 0).sum())} of {B} frames are empty"
        variants[f"{tag}: record + cells, contact rectangles"] = lambda hm=hm, f=fmin, i=ind, r=rows: model(hm, f, i, slip=slip, frame_rows=r)
        variants[f"{tag}: record + cells, whole frames"] = lambda hm=hm, f=fmin, i=ind: model(hm, f, i, slip=slip)
        variants[f"{tag}: record + cells + image, contact rectangles"] = lambda hm=hm, f=fmin, i=ind, r=rows: model(hm, f, i, slip=slip, frame_rows=r, image=image)
        variants[f"{tag}: record + cells + image, whole frames"] = lambda hm=hm, f=fmin, i=ind: model(hm, f, i, slip=slip, image=image)
    hm0 = inputs["dense contact"]
    variants["copy of the height maps (copy_, read + write)"] = lambda: copy_dst.copy_(hm0)
    read_ms = copy_ms(B * H * W * 4)
    rows_out = [(k, v, f"{read_ms / float(np.median(v)):.2f}") for k, v in rounds(variants, a.calls, a.reps, 5).items()]
    # the torch restatement (one gel for every env, allocates its temporaries like the code a user would write)
    ci = (torch.arange(H, device=dev) * GRID[0]) // H
    cj = (torch.arange(W, device=dev) * GRID[1]) // W
    cell_of_pixel = (ci[:, None] * GRID[1] + cj[None, :]).reshape(-1)
    for tag, hm in inputs.items():
        fmin, ind, _ = depth_pass(hm)
        fn = lambda hm=hm, f=fmin, i=ind: torch_restatement(hm, f, i, (3.0e4, 1.2e4, 0.6), slip, PIXMM, cell_of_pixel, GRID[0] * GRID[1])  # noqa: E731
        v = repeated(fn, a.torch_calls, a.reps, 1)
        rows_out.append((f"{tag}: torch restatement (force, centre of pressure, counts, cells)", v, f"{read_ms / float(np.median(v)):.2f}"))
    # where the time goes: the raw entry point (outputs allocated once) on the first 256 / 1024 / all frames, without and with cells
    lib = _lib.load_library()
    st = _lib.current_stream_handle(torch.device(dev))
    rec = torch.empty((B, 16), dtype=torch.float64, device=dev)
    cel = torch.empty((B, GRID[0], GRID[1], 3), device=dev)
    scale = []
    for tag, hm in inputs.items():
        fmin, ind, rows = depth_pass(hm)
        for nb in sorted({min(256, B), min(1024, B), B}):
            row = [f"{tag}, first {nb} frames"]
            for c, r in ((None, None), (None, rows), (cel, None), (cel, rows)):
                fn = lambda c=c, r=r, hm=hm, f=fmin, i=ind, nb=nb: lib.tacex_contact_field(  # noqa: E731
                    _lib.ptr(hm), _lib.ptr(f), _lib.ptr(i), _lib.ptr(model.gels), model.num_gels, _lib.ptr(model.gel_ids), _lib.ptr(slip), PIXMM,
                    _lib.ptr(r), GRID[0], GRID[1], _lib.ptr(rec), _lib.ptr(c), 0, nb, H, W, st)
                row.append(float(np.median(repeated(fn, a.calls, 3, 5))))
            scale.append(row)
    lines = table(["one read of the height maps / median"], rows_out)
    notes = [info[t] for t in inputs]
    lines += ["", "Raw entry point, outputs allocated once, median of 3 timings, ms:", "",
              "| frames | record only | record only, rectangles | record + cells | record + cells, rectangles |", "|---|---|---|---|---|"]
    lines += [f"| {r[0]} | {r[1]:.3f} | {r[2]:.3f} | {r[3]:.3f} | {r[4]:.3f} |" for r in scale]
    head = (f"# Contact force field: one call on {B} frames of {W} x {H}, grid {GRID[0]} x {GRID[1]}\n\n{a.calls} calls per timing between two hipEvents, "
            f"{a.reps} alternating rounds (median, min, max of the rounds), one MI355X; the torch restatement {a.torch_calls} calls per timing.  "
            f"The last column is derived: one read of the height maps ({B * H * W * 4 / 1e9:.3f} GB) at the {COPY_TBS} TB/s float4-copy rate takes "
            f"{read_ms:.3f} ms; the column is that time over the measured median (1 = the call costs one read of the height maps).\n\n")
    emit(lines, a.out, head, notes)


if __name__ == "__main__":
    main()
