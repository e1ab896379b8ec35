"""Plain-numpy restatement of the region- and track-based detection criteria (vec_vad_amd/scoring.py module docstring), written with
loops and an explicit threshold sweep, independently of the kernels and of ``scoring.link_tracks`` / ``scoring.region_curves``.
tests/test_gpu_regions.py compares the kernels with it and tests/test_region_host.py the host functions.  Nothing here imports the
package; not collected by pytest."""
import numpy as np

BIG = 100000
REGION_MAX = 64


def label(gt):
    """8-connected components of ``gt != 0`` (``[h,w]``) by flood fill, numbered 1.. in raster order of their first pixel."""
    h, w = gt.shape
    lab = np.zeros((h, w), np.int32)
    n = 0
    for y in range(h):
        for x in range(w):
            if gt[y, x] == 0 or lab[y, x]:
                continue
            n += 1
            lab[y, x] = n
            stack = [(y, x)]
            while stack:
                cy, cx = stack.pop()
                for ny in range(max(cy - 1, 0), min(cy + 2, h)):
                    for nx in range(max(cx - 1, 0), min(cx + 2, w)):
                        if gt[ny, nx] != 0 and not lab[ny, nx]:
                            lab[ny, nx] = n
                            stack.append((ny, nx))
    return lab, n


def label_frames(gt):
    labs, counts = zip(*[label(g) for g in gt]) if len(gt) else ((), ())
    return (np.stack(labs) if len(gt) else np.zeros(gt.shape, np.int32)), np.array(counts, np.int32)


def match(labels, scores, off, rects, pct, big=BIG):
    """(region_area [F,64], region_score [F,64], box_state [n]) by loops over boxes and regions."""
    F = len(labels)
    area = np.zeros((F, REGION_MAX), np.int32)
    best = np.full((F, REGION_MAX), -float(big))
    state = np.zeros(len(scores), np.uint8)
    for f in range(F):
        R = min(int(labels[f].max()) if labels[f].size else 0, REGION_MAX)
        for r in range(1, R + 1):
            area[f, r - 1] = int((labels[f] == r).sum())
        for m in range(off[f], off[f + 1]):
            y0, y1, x0, x1 = (int(v) for v in rects[m])
            if y1 <= y0 or x1 <= x0:
                continue
            box = labels[f, y0:y1, x0:x1]
            a_m = (y1 - y0) * (x1 - x0)
            hit = False
            for r in range(1, R + 1):
                inter = int((box == r).sum())
                if inter > 0 and 100 * inter >= pct * (a_m + int(area[f, r - 1]) - inter):
                    hit = True
                    best[f, r - 1] = max(best[f, r - 1], scores[m])
            state[m] = 1 if hit else 2
    return area, best, state


def links(labels, prev, same_video):
    """uint64 ``[F,64]`` link words by a loop over the pixel positions that are foreground in both frames."""
    F = len(labels)
    out = np.zeros((F, REGION_MAX), np.uint64)
    for f in range(F):
        before = labels[f - 1] if f > 0 else prev
        if before is None or not same_video[f]:
            continue
        both = (labels[f] > 0) & (before > 0)
        for r, q in set(zip(labels[f][both].tolist(), before[both].tolist())):
            if r <= REGION_MAX and q <= REGION_MAX:
                out[f, r - 1] |= np.uint64(1) << np.uint64(q - 1)
    return out


def tracks(n_regions, link_words, track_percent):
    """(track id per region in (frame, number) order, k per track): the connected components of the link graph by repeated label
    propagation (no union-find), numbered in order of their first region."""
    first = np.concatenate([[0], np.cumsum(n_regions)]).astype(np.int64)
    comp = np.arange(first[-1])
    edges = []
    for f in range(1, len(n_regions)):
        for r in range(int(n_regions[f])):
            for q in range(int(n_regions[f - 1])):
                if (int(link_words[f][r]) >> q) & 1:
                    edges.append((first[f] + r, first[f - 1] + q))
    changed = True
    while changed:
        changed = False
        for a, b in edges:
            lo = min(comp[a], comp[b])
            if comp[a] != lo or comp[b] != lo:
                comp[a] = comp[b] = lo
                changed = True
    ids = {}
    track = np.array([ids.setdefault(int(c), len(ids)) for c in comp], np.int64)
    length = np.array([int((track == t).sum()) for t in range(len(ids))], np.int64)
    return track, (length * track_percent + 99) // 100


def curve_area(x, y):
    """Area over x in [0, 1] of the polyline (0, 0) -> (x[i], y[i]): cut at x = 1 by interpolation, extended flat to x = 1."""
    px, py = [0.0] + list(x), [0.0] + list(y)
    area = 0.0
    for i in range(1, len(px)):
        if px[i] >= 1.0:
            if px[i] == px[i - 1]:
                return area
            yc = py[i - 1] + (py[i] - py[i - 1]) * (1.0 - px[i - 1]) / (px[i] - px[i - 1])
            return area + (1.0 - px[i - 1]) * (py[i - 1] + yc) / 2.0
        area += (px[i] - px[i - 1]) * (py[i] + py[i - 1]) / 2.0
    return area + (1.0 - px[-1]) * py[-1]


def sweep(region_scores, track, k, fp_scores, n_frames, big=BIG):
    """The criterion as defined: at every threshold (the distinct values above ``-big`` among region scores, the k-th largest region
    score of every track and the false-positive scores, descending) count the detected regions, the tracks with at least ``k`` detected
    regions and the false positives.  Returns (thresholds, fpr, rbdr, tbdr, rbdc, tbdc); no region: the two areas are nan."""
    region_scores, fp_scores = [float(v) for v in region_scores], [float(v) for v in fp_scores]
    n_tracks = len(k)
    members = [[region_scores[i] for i in range(len(region_scores)) if track[i] == t] for t in range(n_tracks)]
    track_vals = [sorted(m, reverse=True)[int(k[t]) - 1] for t, m in enumerate(members)]
    thresholds = sorted({v for v in region_scores + track_vals + fp_scores if v > -big}, reverse=True)
    fpr, rbdr, tbdr = [], [], []
    for t in thresholds:
        fpr.append(sum(1 for v in fp_scores if v >= t) / float(n_frames))
        rbdr.append(sum(1 for v in region_scores if v >= t) / float(len(region_scores)) if region_scores else 0.0)
        tbdr.append(sum(1 for tr in range(n_tracks) if sum(1 for v in members[tr] if v >= t) >= int(k[tr])) / float(n_tracks)
                    if n_tracks else 0.0)
    if not region_scores:
        return thresholds, fpr, rbdr, tbdr, float('nan'), float('nan')
    return thresholds, fpr, rbdr, tbdr, curve_area(fpr, rbdr), curve_area(fpr, tbdr)
