"""Time of the contact point cloud (`TactileContactPoints`, one launch of tacex_contact_points) on 2048 frames of 320 x 240 - a C3 step's
height maps - on sparse contact (one random indenter per frame, a tenth of the frames flat) with and without the contact rectangles
and on dense contact (a wavy plate over the whole sensor: every pixel in contact), for K = 256, 1024 and 4096 points per env, with and
without normals, and with the repeat pad.  hipEvents around `--calls` calls in a row, the variants alternating over `--reps` rounds
after a warm-up.  Beside them, with the same events:
  - a copy of the height maps (`copy_`: 4 B / pixel read and 4 B / pixel written, 16-byte accesses) and the time ONE read of them takes
    at the 6.29 TB/s float4-copy rate of one MI355X (derived, not measured);
  - the same (B,K,3) points from torch ops without host synchronisation: a cumsum of the contact mask over every frame, a
    searchsorted of the K ranks in it and gathers (no normals, depths, pixels or labels; checked against the launch on every frame).

  --out FILE   also write the table as markdown."""
import numpy as np
import torch
from _bench_util import COPY_TBS, copy_ms, emit, parse_args, repeated, rounds, table

a = parse_args(calls=50, torch_calls=3, torch_help="calls per timing of the torch-ops baseline")

from tacex_amd import TactileContactPoints, _lib  # noqa: E402
from tacex_amd.utils.synthetic import PIXMM, dense_contact_depth_maps, synthetic_depth_maps  # noqa: E402


def depth_pass(hm):
    lib = _lib.load_library()
    B, H, W = hm.shape
    fmin, ind = torch.zeros(B, device=hm.device), torch.zeros(B, device=hm.device)
    rows = torch.zeros((B, 4), dtype=torch.int32, device=hm.device)
    _lib.check(lib.tacex_indentation_depth(_lib.ptr(hm), 0.0045, 0.024, _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(rows), B, H, W,
                                           _lib.current_stream_handle(hm.device)), "tacex_indentation_depth")
    return fmin, ind, rows


def torch_points(hm, fmin, ind, K, pixmm):
    """The (B,K,3) points a user would get without the kernel and without a host synchronisation: rank of every pixel by a cumsum
    over the frame, the pixel of every slot's rank by searchsorted, then gathers.  Zero pad, no jitter."""
    B, H, W = hm.shape
    S = ((hm - fmin[:, None, None]) - ind[:, None, None]).view(B, H * W)
    csum = (S < 0).to(torch.int32).cumsum(1, dtype=torch.int32)  # contact pixels up to and including each pixel
    N = csum[:, -1:].long()
    k = torch.arange(K, device=hm.device, dtype=torch.long)[None, :]
    rank = torch.where(N > K, (k * N) // K, k.expand(B, K))
    valid = rank < N
    idx = torch.searchsorted(csum, (rank + 1).to(torch.int32)).clamp_(max=H * W - 1)  # the first pixel whose count reaches rank + 1
    i, j = idx // W, idx % W
    pts = torch.stack(((j.float() - (W - 1) / 2) * pixmm, (i.float() - (H - 1) / 2) * pixmm, S.gather(1, idx)), dim=-1)
    return pts * valid[..., None]


def main():
    B, H, W = a.frames, a.height, a.width
    dev = "cuda:0"
    inputs = {"sparse contact": synthetic_depth_maps(B, H, W, seed=3, device=dev, flat_fraction=0.1)[0],
              "dense contact": dense_contact_depth_maps(B, H, W, seed=3, device=dev)[0]}
    models = {}

    def model(K, normals=True, pad="zero"):
        key = (K, normals, pad)
        if key not in models:
            models[key] = TactileContactPoints(B, dev, max_points=K, pixmm=PIXMM, normals=normals, pad=pad)
            models[key].pose = None
        return models[key]

    copy_dst = torch.empty((B, H, W), device=dev)
    variants, info, scalars = {}, {}, {}
    for tag, hm in inputs.items():
        fmin, ind, rows = depth_pass(hm)
        scalars[tag] = (fmin, ind, rows)
        r = rows.cpu().numpy().astype(np.int64)
        rect = np.clip(r[:, 1] - r[:, 0] + 1, 0, None) * np.clip(r[:, 3] - r[:, 2] + 1, 0, None)
        n = model(1024)(hm, fmin, ind, frame_rows=rows).num_contact.cpu().numpy()
        info[tag] = (f"{tag}: the contact rectangles cover {rect.sum() / (B * H * W):.1%} of the pixels, {int((rect == 0).sum())} of {B} frames are "
                     f"empty; contact pixels per frame: median {int(np.median(n))}, largest {int(n.max())}")
        for K in (256, 1024, 4096):
            variants[f"{tag}: K = {K}, contact rectangles"] = lambda hm=hm, f=fmin, i=ind, r=rows, K=K: model(K)(hm, f, i, frame_rows=r)
        variants[f"{tag}: K = 1024, whole frames"] = lambda hm=hm, f=fmin, i=ind: model(1024)(hm, f, i)
        variants[f"{tag}: K = 1024, contact rectangles, no normals"] = lambda hm=hm, f=fmin, i=ind, r=rows: model(1024, normals=False)(hm, f, i, frame_rows=r)
        variants[f"{tag}: K = 1024, contact rectangles, pad repeat"] = lambda hm=hm, f=fmin, i=ind, r=rows: model(1024, pad="repeat")(hm, f, i, frame_rows=r)
        variants[f"{tag}: K = 4096, contact rectangles, no normals"] = lambda hm=hm, f=fmin, i=ind, r=rows: model(4096, normals=False)(hm, f, i, frame_rows=r)
    hm0 = inputs["dense contact"]
    variants["copy of the height maps (copy_, read + write)"] = lambda: copy_dst.copy_(hm0)
    read_ms = copy_ms(B * H * W * 4)
    rows_out = [(k, v, f"{read_ms / float(np.median(v)):.2f}") for k, v in rounds(variants, a.calls, a.reps, 5).items()]
    notes = [info[t] for t in inputs]
    for tag, hm in inputs.items():
        fmin, ind, rows = scalars[tag]
        for K in (256, 1024, 4096):
            fn = lambda hm=hm, f=fmin, i=ind, K=K: torch_points(hm, f, i, K, PIXMM)  # noqa: E731
            v = repeated(fn, a.torch_calls, a.reps, 1)
            rows_out.append((f"{tag}: K = {K}, torch ops (cumsum + searchsorted + gather; points only)", v, f"{read_ms / float(np.median(v)):.2f}"))
            same = torch.equal(fn(), model(K)(hm, fmin, ind, frame_rows=rows).points)
            notes.append(f"{tag}, K = {K}: the torch-ops points {'equal' if same else 'DIFFER FROM'} the launch's on every frame")
    lines = table(["one read of the height maps / median"], rows_out)
    head = (f"# Contact point cloud: one call on {B} frames of {W} x {H}\n\n{a.calls} calls per timing between two hipEvents, "
            f"{a.reps} alternating rounds (median, min, max of the rounds), one MI355X; the torch-ops baseline {a.torch_calls} calls per timing.  "
            f"Normals on, zero pad and no pose unless the row says otherwise.  "
            f"The last column is derived: one read of the height maps ({B * H * W * 4 / 1e9:.3f} GB) at the {COPY_TBS} TB/s float4-copy rate takes "
            f"{read_ms:.3f} ms; the column is that time over the measured median (1 = the call costs one read of the height maps).\n\n")
    emit(lines, a.out, head, notes)


if __name__ == "__main__":
    main()
