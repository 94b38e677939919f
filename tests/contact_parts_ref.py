"""NumPy restatement of `tacex_contact_field_parts`, written from the function's comment in include/tacex_hip.h: TEST INFRASTRUCTURE
ONLY.  Record (b, l) holds the slots of `tacex_contact_field` over the pixels of label l alone, with the slip row (b, l): that is
`contact_field_ref.contact_frame` of the frame in which every other pixel is taken out of contact (a height of +inf: S = +inf, d = 0,
so the pixel adds to no sum, count or maximum).  A pixel whose label is >= L enters no record and has the image value (0, 0, -p)."""
import numpy as np
import contact_field_ref as C

f32 = np.float32


def parts_frame(hm, frame_min, indent, gel, labels, num_labels, slip, pixmm):
    """One frame -> (record (L,16) f64, image (H,W,3) f32, abs (L,16) f64).  labels (H,W) uint8, slip (L,5) or None."""
    hm, labels = np.asarray(hm, f32), np.asarray(labels)
    H, W = hm.shape
    L = int(num_labels)
    rec, ab, image = np.zeros((L, 16)), np.zeros((L, 16)), np.zeros((H, W, 3), f32)
    away = f32(np.inf)
    with np.errstate(all="ignore"):
        for l in range(L):
            mine = labels == l
            rec[l], _, img, ab[l] = C.contact_frame(np.where(mine, hm, away), frame_min, indent, gel, None if slip is None else slip[l], pixmm)
            image[mine] = img[mine]
        orphan = labels >= L
        img = C.contact_frame(np.where(orphan, hm, away), frame_min, indent, gel, None, pixmm)[2]
        image[orphan] = img[orphan]  # (no slip: tx = ty = 0)
    return rec, image, ab


def parts_batch(hm, frame_min, indent, gels, gel_ids, labels, num_labels, slip, pixmm):
    """(B,H,W) -> record (B,L,16), image (B,H,W,3) f32, abs (B,L,16).  An id outside the table: zeros."""
    B, H, W = hm.shape
    L = int(num_labels)
    rec, ab, image = np.zeros((B, L, 16)), np.zeros((B, L, 16)), np.zeros((B, H, W, 3), f32)
    for b in range(B):
        g = 0 if gel_ids is None else int(gel_ids[b])
        if 0 <= g < len(gels):
            rec[b], image[b], ab[b] = parts_frame(hm[b], frame_min[b], indent[b], gels[g], labels[b], L, None if slip is None else slip[b], pixmm)
    return rec, image, ab


# ---- label maps that split every contact patch (tests/test_contact_parts*.py) --------------------------------------------------------
LABEL_KINDS = ("halves", "checker", "some_255")


def case_labels(kind, hm, frame_min, indent, num_labels):
    """(B,H,W) uint8.  halves: the columns left of each frame's contact centroid are label 0, the others label 1 (mod L); checker:
    5-pixel squares cycling through the L labels; some_255: the checker with every third square's label 255 (no part)."""
    B, H, W = hm.shape
    L = int(num_labels)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        on = (hm[b] - f32(frame_min[b])) - f32(indent[b]) < 0
        if kind == "halves":
            mid = int(np.round(jj[on].mean())) if on.any() else W // 2
            out[b] = np.where(jj < mid, 0, 1 % L)
        else:
            sq = ii // 5 + jj // 5 + b
            out[b] = sq % L
            if kind == "some_255":
                out[b] = np.where(sq % 3 == 2, 255, out[b])
    return out


def case_part_slip(B, L, H, W, start=0):
    """(B,L,5) float32: `contact_field_ref.case_slip` rows, another one per label."""
    return np.stack([C.case_slip(B, H, W, start + l) for l in range(L)], axis=1).astype(f32)
