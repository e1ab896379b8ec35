"""Plain-numpy restatement of the pixel-level stages of a stream (include/vecvad_hip.h, vv_stream_paint / vv_stream_smooth): what
tests/test_gpu_stream_masks.py compares the kernels and the scorer with and tests/test_stream_masks_host.py checks on the CPU against
the centred filter of tests/smooth_restatement.py.  Nothing here imports the package."""
import numpy as np

from smooth_restatement import BIG, _shifted_sum


def resolve(boxes_int, h, w):
    """Integer boxes ``(x1, y1, x2, y2)`` -> int32 ``[n,4]`` rows ``(y0, y1, x0, x1)``: the rows ``range(y0, y1)`` and columns
    ``range(x0, x1)`` that ``mask[y1:y2, x1:x2]`` names in an ``h x w`` mask, by Python's own slice arithmetic."""
    out = np.zeros((len(boxes_int), 4), np.int32)
    for m, (x1, y1, x2, y2) in enumerate(np.asarray(boxes_int).reshape(-1, 4).tolist()):
        out[m, 0:2] = slice(y1, y2).indices(h)[:2]
        out[m, 2:4] = slice(x1, x2).indices(w)[:2]
    return out


def paint(rows, n, rects, h, w):
    """rows float64 ``[R,width]`` (one row of box scores per block), the first ``n`` boxes, rects ``[width,4]`` rows ``(y0, y1, x0,
    x1)`` -> ``(mask [h,w], box_max [n])``: every box fills its rectangle with the largest of its scores over the rows (``-BIG``
    without a row), maps are max-combined, untouched pixels are ``-BIG``.  Nothing at or above ``n`` is looked at."""
    box_max = np.full(n, -BIG)
    for r in np.asarray(rows, np.float64):
        box_max = np.maximum(box_max, r[:n])
    mask = np.full((h, w), -BIG)
    for b in range(n):
        y0, y1, x0, x1 = (int(v) for v in rects[b])
        if y1 > y0 and x1 > x0:
            mask[y0:y1, x0:x1] = np.maximum(mask[y0:y1, x0:x1], box_max[b])
    return mask, box_max


def trailing(masks, kt, ks):
    """masks float64 ``[F,h,w]``, the frames of ONE video so far (``-BIG`` = unpainted) -> S ``[F,h,w]``: frame ``t`` is the mean of the
    painted pixels of its ``ks x ks`` neighbourhood over the frames ``max(0, t - kt + 1) .. t``, where frame ``t`` is painted, else
    ``-BIG``.  The X and Y sums are the shifted adds of ``smooth_restatement`` (ascending offsets from +0.0); the T sum takes the
    frames in ascending order from +0.0; one division."""
    masks = np.asarray(masks, np.float64)
    F = masks.shape[0]
    assert kt >= 1 and ks % 2 == 1
    rs = ks // 2
    p = masks != -BIG
    B = _shifted_sum(_shifted_sum(np.where(p, masks, 0.0), 2, rs), 1, rs)
    b = _shifted_sum(_shifted_sum(p.astype(np.int64), 2, rs), 1, rs)
    S = np.full(masks.shape, -BIG)
    for t in range(F):
        C, c = np.zeros_like(B[0]), np.zeros_like(b[0])
        for g in range(max(0, t - kt + 1), t + 1):
            C += B[g]
            c += b[g]
        S[t][p[t]] = C[p[t]] / c[p[t]].astype(np.float64)
    return S
