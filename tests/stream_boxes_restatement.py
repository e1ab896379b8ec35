"""numpy restatement of ``vv_stream_boxes`` (include/vecvad_hip.h), shared by tests/test_stream_boxes_host.py and
tests/test_gpu_stream_boxes.py: what ``StreamScorer._prepare`` forms on the host for boxes it is given -- ``extract.boxes_to_crops``,
``scoring.box_paints`` and ``utils.calc_block_idx`` -- applied to the motion boxes ``vv_mask_boxes`` leaves for one window, behind
``n_ap`` appearance slots that stay as they are.  ``synthetic_frames`` are the test videos both files use."""
import numpy as np


def stream_boxes(count, boxes, n_ap, cap, H, W, grid_h, grid_w, hb, wb, block_mode, crops=None, masks=None, boxes_out=None):
    """count: int; boxes: int ``[mcap,4]`` rows (x1, y1, x2, y2), of which rows below ``min(count, mcap)`` are read.  ``crops`` int32
    ``[cap,4]``, ``masks`` uint8 ``[hb*wb,cap]`` and ``boxes_out`` int32 ``[cap,4]`` are what the buffers held before (None: zeros);
    copies are changed.  Returns ``(n, dropped, crops, masks, boxes_out)``."""
    from utils import calc_block_idx
    from vec_vad_amd.extract import boxes_to_crops
    from vec_vad_amd.scoring import box_paints
    boxes = np.asarray(boxes, np.int64).reshape(-1, 4)
    crops = np.zeros((cap, 4), np.int32) if crops is None else np.array(crops, np.int32)
    masks = np.zeros((hb * wb, cap), np.uint8) if masks is None else np.array(masks, np.uint8)
    boxes_out = np.zeros((cap, 4), np.int32) if boxes_out is None else np.array(boxes_out, np.int32)
    m = min(int(count), len(boxes), cap - n_ap)
    n, dropped = n_ap + m, int(count) - m
    h_step, w_step = grid_h / hb, grid_w / wb
    masks[:, n_ap:] = 0
    kept = boxes[:m].astype(np.float64)                   # the scorer's boxes are float64 rows
    crops[n_ap:n] = boxes_to_crops(kept, H, W)
    boxes_out[n_ap:n] = boxes[:m]
    for j, (bb, paints) in enumerate(zip(kept, box_paints(kept, grid_h, grid_w))):
        if not paints:
            continue
        for hi, wi in calc_block_idx(bb[0], bb[2], bb[1], bb[3], h_step, w_step, mode=block_mode):
            if 0 <= hi < hb and 0 <= wi < wb:
                masks[hi * wb + wi, n_ap + j] = 1
    return n, dropped, crops, masks, boxes_out


# ---- the synthetic test videos of the scorer tests ---------------------------------------------------------------------------------------
H, W = 48, 72
N_VIDEO = (4, 3)
# per video: rectangles (w, h, the (x, y) of every frame or None) drawn at value 200 on a static background of values 96..103 (low
# contrast: the differences of its blurred frames stay far below the threshold; 200 keeps the sum of two differences below 256, where
# the reference's uint8 sum wraps).  Video 1: A and B move throughout, C is 4x4 (its component fails UCSDped2's area filter), D
# appears in frame 2.  Video 2: E and F move from frame 0 to frame 1 and then stand still, so the window (1, 2, 2) of the last frame
# holds no motion at all.
RECTS = (((12, 10, [(6, 6), (9, 6), (12, 6), (15, 6)]), (14, 12, [(40, 28), (37, 29), (34, 30), (31, 31)]),
          (4, 4, [(60, 6), (62, 6), (64, 6), (66, 6)]), (10, 9, [None, None, (4, 30), (4, 32)])),
         ((14, 12, [(20, 16), (24, 18), (24, 18)]), (12, 10, [(50, 30), (47, 30), (47, 30)])))
SMALL = (4, 4)                                            # the rectangle the area filter rejects
COVERED = (1, 0)                                          # per video: the rectangle the appearance box of the second run covers
CAP = 6                                                   # stream_max_boxes of the scorer tests: holds every frame's boxes


def appearance_boxes():
    """One detector row (x1, y1, x2, y2, confidence) per frame: the covered rectangle of the frame, 3.5 px wider on every side.  What
    ``vv_motion_mask`` erases is that, truncated, plus its 2 px: every place the rectangle has in the frame's window and the blur's
    one pixel around it."""
    out = []
    for length, rects, k in zip(N_VIDEO, RECTS, COVERED):
        w, h, where = rects[k]
        for t in range(length):
            x, y = where[t]
            out.append(np.array([[x - 3.5, y - 3.5, x + w + 3.5, y + h + 3.5, 0.9]]))
    return out


def synthetic_frames():
    """-> (frames: list of uint8 ``[H,W]`` arrays in split order, fvi: the 1-based video of every frame)."""
    rng = np.random.default_rng(21)
    back = rng.integers(96, 104, (H, W), dtype=np.uint8)
    frames, fvi = [], []
    for v, (length, rects) in enumerate(zip(N_VIDEO, RECTS), start=1):
        for t in range(length):
            g = back.copy()
            for (w, h, where) in rects:
                if where[t] is not None:
                    x, y = where[t]
                    g[y:y + h, x:x + w] = 200
            frames.append(g)
            fvi.append(v)
    return frames, fvi


def motion_windows(fvi):
    """The 'hard' three-frame window of every frame of the split, as ``foreground._motion_bboxes`` forms it."""
    from vad_datasets import context_range
    return [context_range(i, 'hard', 1, len(fvi), fvi) for i in range(len(fvi))]
