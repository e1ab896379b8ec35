"""Plain-numpy restatement of the two render kernels ([mi355x] render; include/vecvad_hip.h, vv_flow_color and vv_render_overlay): what
the GPU tests compare against.  ``flow_color`` works in float64 from the float32 maximum radius on, as the reference's
``flow_to_image`` does on float32 input, and equals it element for element (tests/test_render_host.py); ``overlay`` follows the four
rules of the header literally, pixel by pixel, and is exact."""
import numpy as np

UNPAINTED = -100000.0
UNKNOWN = 1e7


def wheel():
    """The 55 x 3 Middlebury colour wheel from its published description: six segments (RY 15, YG 6, GC 4, CB 11, BM 13, MR 6), in each
    one channel ramps as floor(255 i / n), up or down, while the others rest at 0 or 255."""
    rows = []
    for n, fixed, ramp, up in ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True), (6, 0, 2, False)):
        for i in range(n):
            c = [0, 0, 0]
            c[fixed] = 255
            c[ramp] = (255 * i) // n if up else 255 - (255 * i) // n
            rows.append(c)
    return np.array(rows, np.float64)


def flow_parts(flow, maxrad=0.0):
    """(image uint8 [h,w,3], rad float64 [h,w], unknown bool [h,w]) of one float32 [h,w,2] field: ``rad`` is the normalised radius the
    ``rad <= 1`` branch looks at."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[2] == 2
    u, v = flow[..., 0].copy(), flow[..., 1].copy()
    with np.errstate(invalid='ignore'):
        unknown = ~((np.abs(u) <= UNKNOWN) & (np.abs(v) <= UNKNOWN))          # a NaN is unknown too
    u[unknown] = 0
    v[unknown] = 0
    if maxrad > 0:
        R = np.float32(maxrad)
    else:
        R = np.float32(max(-1.0, float(np.sqrt(u * u + v * v).max()))) if u.size else np.float32(-1)      # float32, product and sum rounded
    den = np.float64(R) + 2.0 ** -52
    u, v = u.astype(np.float64) / den, v.astype(np.float64) / den
    rad = np.sqrt(u ** 2 + v ** 2)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * 54 + 1
    k0 = np.floor(fk).astype(int)
    k1 = k0 + 1
    k1[k1 == 56] = 1
    f = fk - k0
    W = wheel()
    img = np.zeros(u.shape + (3,), np.uint8)
    for c in range(3):
        col = (1 - f) * (W[k0 - 1, c] / 255) + f * (W[k1 - 1, c] / 255)
        col = np.where(rad <= 1, 1 - rad * (1 - col), col * 0.75)
        img[..., c] = np.floor(255 * col)
    img[unknown] = 0
    return img, rad, unknown


def flow_color(flow, maxrad=0.0):
    """uint8 [n,h,w,3] of a float32 [n,h,w,2] batch, every image on its own."""
    flow = np.asarray(flow)
    return np.stack([flow_parts(f, maxrad)[0] for f in flow]) if len(flow) else np.zeros(flow.shape[:3] + (3,), np.uint8)


def level(v, lo, hi):
    v, lo, hi = np.float64(v), np.float64(lo), np.float64(hi)
    if v <= lo:
        return 0
    if v >= hi:
        return 255
    return int(np.floor((v - lo) / (hi - lo) * np.float64(255.0)))


def overlay(frames, mask, rects, scores, frame_off, lo, hi, alpha, gt=None, lut=None, bgr=True):
    """uint8 [n,h,w,3] RGB; arguments as for ``vec_vad_amd.render.overlay``, numpy arrays (frames [n,h,w,c], c in (1, 3))."""
    frames, mask = np.asarray(frames), np.asarray(mask)
    n, h, w, c = frames.shape
    out = np.zeros((n, h, w, 3), np.uint8)
    for f in range(n):
        base = np.repeat(frames[f], 3, axis=2) if c == 1 else (frames[f][..., ::-1] if bgr else frames[f])
        img = base.astype(np.int64)
        for y, x in zip(*np.nonzero(mask[f] != UNPAINTED)):  # rule 2
            col = lut[level(mask[f, y, x], lo, hi)].astype(np.int64)
            img[y, x] = (img[y, x] * (256 - alpha) + col * alpha + 128) >> 8
        edge = np.zeros((h, w), bool)                        # rule 3
        best = np.full((h, w), -np.inf)
        for m in range(int(frame_off[f]), int(frame_off[f + 1])):
            y0, y1, x0, x1 = (int(t) for t in rects[m])
            if y1 <= y0 or x1 <= x0:
                continue
            for y in range(max(y0, 0), min(y1, h)):
                for x in range(max(x0, 0), min(x1, w)):
                    if y in (y0, y1 - 1) or x in (x0, x1 - 1):
                        edge[y, x] = True
                        best[y, x] = max(best[y, x], scores[m])
        for y, x in zip(*np.nonzero(edge)):
            img[y, x] = lut[level(best[y, x], lo, hi)]
        if gt is not None:                                   # rule 4
            g = np.pad(np.asarray(gt[f]) != 0, 1)
            inner = g[:-2, 1:-1] & g[2:, 1:-1] & g[1:-1, :-2] & g[1:-1, 2:]
            img[g[1:-1, 1:-1] & ~inner] = 255
        out[f] = img
    return out
