"""Plain-numpy restatement of the tracks of a stream (include/vecvad_hip.h, vv_stream_tracks): what tests/test_gpu_stream_tracks.py
compares the kernel and the scorer with and tests/test_stream_tracks_host.py checks on hand cases.  The matching is the sequential greedy
one over the sorted candidate pairs, with Python ints for the cross-multiplication.  Nothing here imports the package."""
from functools import cmp_to_key

import numpy as np

from stream_masks_restatement import BIG, resolve  # noqa: F401  (resolve: integer boxes -> the rectangles the kernel forms)


def _pair_order(a, b):
    """Candidate pairs ``(inter, union, slot, box)``: IoU descending, compared as cross products of integers, then the lower slot,
    then the lower box."""
    l, r = a[0] * b[1], b[0] * a[1]
    if l != r:
        return -1 if l > r else 1
    return -1 if a[2:] < b[2:] else (1 if a[2:] > b[2:] else 0)


class Tracker:
    """The state of one camera: ``meta`` int32 ``[max_tracks,8]`` rows ``(id, age, hits, y0, y1, x0, x1, 0)``, ``hist`` float64
    ``[max_tracks,window]`` and ``next_id``.  ``seen`` counts what the frames so far exercised: matches, deaths, births, births into a
    slot that held a track before (since the last reset), drops."""

    def __init__(self, max_tracks, window=8, iou_pct=30, max_age=5, min_hits=3):
        self.meta = np.zeros((max_tracks, 8), np.int32)
        self.hist = np.zeros((max_tracks, window), np.float64)
        self.next_id = 1
        self.window, self.iou_pct, self.max_age, self.min_hits = int(window), int(iou_pct), int(max_age), int(min_hits)
        self.seen = dict(match=0, death=0, birth=0, reuse=0, drop=0)
        self._used = set()

    def _free(self, t):
        self.meta[t] = 0
        self.hist[t] = 0.0

    def step(self, rows, n, rects, reset=False):
        """One issued frame.  rows float64 ``[R,width]`` (one row of box scores per block; R may be 0), the first ``n`` boxes, rects
        ``[>=n,4]`` rows ``(y0, y1, x0, x1)`` inside the mask.  Returns a dict: ``ids`` / ``hits`` int32 ``[n]``, ``scores`` float64
        ``[n]``, ``score`` (the frame's track score), ``live``, ``dropped``, ``next_id``.  Nothing at or above ``n`` is looked at."""
        meta, hist, W = self.meta, self.hist, self.window
        T = len(meta)
        if reset:                                                        # step 0
            for t in range(T):
                self._free(t)
            self._used = set()
        s = [-BIG] * n                                                   # step 1
        for r in np.asarray(rows, np.float64):
            for b in range(n):
                s[b] = max(s[b], float(r[b]))
        rect = [tuple(int(v) for v in rects[b]) for b in range(n)]
        dets = [b for b in range(n) if rect[b][1] > rect[b][0] and rect[b][3] > rect[b][2] and s[b] > -BIG]
        live = [t for t in range(T) if meta[t, 0] > 0]
        for t in live:                                                   # step 2
            meta[t, 1] += 1
        pairs = []                                                       # step 3
        for t in live:
            ty0, ty1, tx0, tx1 = (int(v) for v in meta[t, 3:7])
            for d in dets:
                y0, y1, x0, x1 = rect[d]
                iy, ix = min(ty1, y1) - max(ty0, y0), min(tx1, x1) - max(tx0, x0)
                inter = iy * ix if iy > 0 and ix > 0 else 0
                union = (ty1 - ty0) * (tx1 - tx0) + (y1 - y0) * (x1 - x0) - inter
                if inter > 0 and 100 * inter >= self.iou_pct * union:
                    pairs.append((inter, union, t, d))
        pairs.sort(key=cmp_to_key(_pair_order))
        of_track, of_det = {}, {}
        for inter, union, t, d in pairs:
            if t in of_track or d in of_det:
                continue
            of_track[t], of_det[d] = d, t
            meta[t, 1] = 0
            meta[t, 2] += 1
            meta[t, 3:7] = rect[d]
            hist[t, (int(meta[t, 2]) - 1) % W] = s[d]
            self.seen['match'] += 1
        for t in live:                                                   # step 4
            if t not in of_track and meta[t, 1] > self.max_age:
                self._free(t)
                self.seen['death'] += 1
        dropped = 0                                                      # step 5
        free = [t for t in range(T) if meta[t, 0] == 0]
        for d in dets:
            if d in of_det:
                continue
            if not free:
                dropped += 1
                self.seen['drop'] += 1
                continue
            t = free.pop(0)
            meta[t] = (self.next_id, 0, 1) + rect[d] + (0,)
            hist[t] = 0.0
            hist[t, 0] = s[d]
            self.next_id += 1
            of_det[d] = t
            self.seen['birth'] += 1
            self.seen['reuse'] += t in self._used
            self._used.add(t)
        ids, hits, scores = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -BIG)      # step 6
        frame = None
        for d, t in of_det.items():
            ids[d], hits[d] = meta[t, 0], meta[t, 2]
            k = int(hits[d])
            m = min(k, W)
            acc = 0.0
            for j in range(m):                                           # from the oldest to the newest
                acc += float(hist[t, (k - m + j) % W])
            scores[d] = acc / float(m)
            if k >= self.min_hits:
                frame = scores[d] if frame is None else max(frame, scores[d])
        return dict(ids=ids, hits=hits, scores=scores, score=-BIG if frame is None else float(frame),
                    live=int((meta[:, 0] > 0).sum()), dropped=dropped, next_id=self.next_id)

    def tracks(self):
        """The live slots in slot order, int32 ``[L,7]`` rows ``(id, age, hits, y0, y1, x0, x1)``."""
        return self.meta[self.meta[:, 0] > 0][:, :7].copy()
