"""Plain numpy restatements of the per-pixel anomaly-map kernels (vv_error_maps, vv_error_zmaps, vv_paint_zmaps, vv_mask_kth): what
tests/test_gpu_pixel_maps.py compares the kernels with and tests/test_pixel_maps_host.py checks on the CPU.  Nothing here imports
the package: the formulas are written out again."""
import numpy as np

BIG = 100000
PATCH = 32


def patch_index(v, lo, hi):
    """nearest source pixel of the 32-pixel patch stretched over [lo, hi), in integers"""
    return ((2 * (np.asarray(v, np.int64) - lo) + 1) * PATCH) // (2 * (hi - lo))


def error_maps(out4, oc, tgt_src, tgt_coff, tgt0, tgt1, dtype, flow=True):
    """out4 [G,M,4], tgt0 [M,C0], tgt1 [M,C1] | None -> (e_raw [M], e_of [M] | None), every operation in ``dtype``: groups in
    ascending g, channels in ascending c."""
    out4 = np.asarray(out4, dtype)
    M = out4.shape[1]
    e = [np.zeros(M, dtype), np.zeros(M, dtype)]
    for g in range(out4.shape[0]):
        src = int(tgt_src[g])
        if src == 1 and not flow:
            continue
        tgt = np.asarray(tgt0 if src == 0 else tgt1, dtype)
        for c in range(int(oc[g])):
            d = out4[g, :, c] - tgt[:, int(tgt_coff[g]) + c]
            e[src] = (e[src] + d * d).astype(dtype)
    return e[0], (e[1] if flow else None)


def zmaps(e_raw, e_of, cube_stat, stats, w_raw, w_of):
    """float32 e [n,32,32] -> float64 z [n,32,32]: 1024 e in float32 (exact), then float64, every operation rounded on its own"""
    n = len(cube_stat)
    z = np.empty((n, PATCH, PATCH), np.float64)
    for m in range(n):
        if cube_stat[m] < 0:
            z[m] = BIG
            continue
        st = stats[cube_stat[m]]
        z[m] = w_raw * (((np.float32(1024) * e_raw[m]).astype(np.float64) - st[0]) / st[1])
        if e_of is not None:
            z[m] = z[m] + w_of * (((np.float32(1024) * e_of[m]).astype(np.float64) - st[2]) / st[3])
    return z


def paint_error_masks(z, frame_off, rects, h, w, out=None):
    """[F,h,w] float64: every cube's map stretched over its rectangle (y0, y1, x0, x1) and max-combined, background -BIG"""
    F = len(frame_off) - 1
    res = np.full((F, h, w), -float(BIG)) if out is None else out.copy()
    for f in range(F):
        for m in range(frame_off[f], frame_off[f + 1]):
            y0, y1, x0, x1 = (int(v) for v in rects[m])
            if y1 <= y0 or x1 <= x0:
                continue
            py, px = patch_index(np.arange(y0, y1), y0, y1), patch_index(np.arange(x0, x1), x0, x1)
            region = res[f, y0:y1, x0:x1]
            np.maximum(region, z[m][np.ix_(py, px)], out=region)
    return res


def kth_largest(mask, gt, pct):
    """the pixel score of one frame by sorting"""
    g = int((gt != 0).sum())
    if g == 0:
        return mask.max() if mask.size else -float(BIG)
    return np.sort(mask[gt != 0])[::-1][(g * pct + 99) // 100 - 1]


def kth_by_sweep(mask, gt, pct):
    """the same number from the criterion itself: the largest threshold (among the values the mask takes) at which at least pct
    percent of the ground-truth pixels lie at or above it"""
    sel = gt != 0
    if not sel.any():
        return mask.max()
    vals, n = mask[sel], int(sel.sum())
    return max(t for t in np.unique(vals) if 100 * int((vals >= t).sum()) >= pct * n)
