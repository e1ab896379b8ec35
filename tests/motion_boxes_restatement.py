"""numpy-only restatement of the reference's motion foreground stage (fore_det/obj_det_with_motion.py get_mt_bboxes), split
into the two stages the HIP kernels implement.  Written from the stated semantics, not from cv2:

  motion_mask : cv2.GaussianBlur(ksize, sigma 0) = the fixed kernels [1,2,1]/4 and [1,4,6,4,1]/16, separable, BORDER_REFLECT_101,
                the integer weighted sum rounded half up once; absdiff of consecutive blurred frames; the two differences added
                as uint8 (numpy wraps modulo 256); threshold ``> binary_thr``; the appearance boxes' extended rectangles cleared
                (numpy slice: inclusive far edge, clipped to the frame); a pixel is set iff any channel is.
  mask_boxes  : cv2.findContours(RETR_EXTERNAL) + boundingRect + the reference's filter.  Foreground components are 8-connected;
                a component is external iff it is 4-adjacent to the 4-connected background region that contains the (virtual)
                one-pixel ring round the frame.  Boxes come in DESCENDING order of the component's first pixel in raster order
                (the contract of this build for the order of cv2's legacy contour list).

Labelling works on runs of equal pixels per row (a few python steps per run), so full-size frames stay affordable.
"""
import numpy as np

# get_mt_bboxes:157-173
CONSTANTS = {'UCSDped2': dict(area_thr=10 * 10, binary_thr=18, extend=2, ksize=3),
             'avenue': dict(area_thr=40 * 40, binary_thr=18, extend=2, ksize=5),
             'ShanghaiTech': dict(area_thr=8 * 8, binary_thr=15, extend=2, ksize=5)}
_WEIGHTS = {3: (np.array([1, 2, 1]), 4), 5: (np.array([1, 4, 6, 4, 1]), 8)}


def reflect101(i, n):
    """BORDER_REFLECT_101 index (dcb|abcd|cba), repeated until it lands inside -- n = 1 maps everything to 0."""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def blur(img, ksize):
    """img uint8 [H,W] or [H,W,C] -> same shape."""
    w, shift = _WEIGHTS[ksize]
    r = ksize // 2
    a = img.astype(np.int64)
    H, W = a.shape[:2]
    rows = [[reflect101(y + k, H) for y in range(H)] for k in range(-r, r + 1)]
    cols = [[reflect101(x + k, W) for x in range(W)] for k in range(-r, r + 1)]
    v = sum(int(w[k]) * a[rows[k]] for k in range(ksize))
    s = sum(int(w[k]) * v[:, cols[k]] for k in range(ksize))
    return ((s + (1 << (shift - 1))) >> shift).astype(np.uint8)


def motion_mask(frames3, ksize, binary_thr, ap_boxes=(), extend=2):
    """frames3 uint8 [3,H,W,C]; ap_boxes: rows x1, y1, x2, y2 (any dtype; truncated like astype(np.int32)) -> uint8 [H,W] 0/255."""
    b = [blur(f, ksize) for f in frames3]
    H, W = b[0].shape[:2]
    d = [np.abs(b[i].astype(np.int64) - b[i + 1].astype(np.int64)).astype(np.uint8) for i in range(2)]
    s = (d[0].astype(np.int64) + d[1].astype(np.int64)) % 256                 # uint8 + uint8 in numpy
    t = s > binary_thr
    for box in np.asarray(ap_boxes).reshape(-1, 4):
        x1, y1, x2, y2 = (int(v) for v in np.asarray(box).astype(np.int32))
        ey1, ey2 = max(0, y1 - extend), min(y2 + extend, H)
        ex1, ex2 = max(0, x1 - extend), min(x2 + extend, W)
        t[ey1:ey2 + 1, ex1:ex2 + 1] = False
    return (t.any(axis=2) * 255).astype(np.uint8)


def _runs(padded):
    """runs of equal values per row of a bool [H,W] image: arrays row, start, end (inclusive), value, and per-row offsets."""
    H, W = padded.shape
    change = np.ones((H, W), bool)
    change[:, 1:] = padded[:, 1:] != padded[:, :-1]
    row, start = np.nonzero(change)
    flat = row * W + start
    end = np.empty_like(start)
    end[:-1] = flat[1:] - 1 - row[:-1] * W
    end[-1] = W - 1
    last = np.r_[row[1:] != row[:-1], True]
    end[last] = W - 1
    off = np.searchsorted(row, np.arange(H + 1))
    return row, start, end, padded[row, start], off


def label_components(mask):
    """mask [H,W] (non-zero = foreground) -> list of (label, x, y, w, h, external) for every 8-connected foreground component,
    label = smallest linear pixel index y*W+x of the component, in ascending label order."""
    fg = np.zeros((mask.shape[0] + 2, mask.shape[1] + 2), bool)          # the virtual background ring
    fg[1:-1, 1:-1] = np.asarray(mask) != 0
    H, W = mask.shape
    row, start, end, val, off = _runs(fg)
    n = len(row)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    st, en, vl = start.tolist(), end.tolist(), val.tolist()
    touch = []                                                           # vertically 4-adjacent (fg run, bg run) pairs
    for r in range(1, fg.shape[0]):
        i, j, ie, je = off[r - 1], off[r], off[r], off[r + 1]
        while i < ie and j < je:
            if vl[i] == vl[j]:
                reach = 1 if vl[i] else 0                                # foreground also connects diagonally
                if st[i] <= en[j] + reach and st[j] <= en[i] + reach:
                    union(i, j)
            elif st[i] <= en[j] and st[j] <= en[i]:
                touch.append((i, j) if vl[i] else (j, i))
            if en[i] < en[j]:
                i += 1
            elif en[j] < en[i]:
                j += 1
            else:                                                        # both end here: their successors meet them diagonally
                if i + 1 < ie and vl[i + 1] and vl[j]:
                    union(i + 1, j)
                if j + 1 < je and vl[j + 1] and vl[i]:
                    union(i, j + 1)
                i += 1
                j += 1
    outer = find(0)                                                      # row 0 of the padded image is one background run
    comps = {}
    for k in range(n):
        if vl[k]:
            c = comps.setdefault(find(k), [k, st[k], en[k], int(row[k]), int(row[k]), False])
            c[1], c[2], c[4] = min(c[1], st[k]), max(c[2], en[k]), max(c[4], int(row[k]))
            # neighbours in the same row alternate in value: runs k-1 and k+1 are background (the ring guarantees they exist)
            if find(k - 1) == outer or find(k + 1) == outer:
                c[5] = True
    for f, b in touch:
        if find(b) == outer:
            comps[find(f)][5] = True
    out = []
    for c in comps.values():
        first, x0, x1, y0, y1, ext = c
        out.append(((y0 - 1) * W + st[first] - 1, x0 - 1, y0 - 1, x1 - x0 + 1, y1 - y0 + 1, ext))
    return sorted(out)


def mask_boxes(mask, area_thr, extend=2):
    """-> int64 [k,4]; shape (0,) when there is no box (np.array([]) in the reference)."""
    H, W = mask.shape
    boxes = []
    for _, x, y, w, h, ext in reversed(label_components(mask)):
        if ext and (w + 1) * (h + 1) > area_thr and w / h < 10 and h / w < 10:
            boxes.append([max(0, x - extend), max(0, y - extend), min(x + w + extend, W), min(y + h + extend, H)])
    return np.array(boxes, dtype=np.int64) if boxes else np.array([])


def get_mt_bboxes(img_batch, ap_bboxes, dataset_name):
    k = CONSTANTS[dataset_name]
    return mask_boxes(motion_mask(img_batch, k['ksize'], k['binary_thr'], ap_bboxes, k['extend']), k['area_thr'], k['extend'])
