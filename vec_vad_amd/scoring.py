"""Score aggregation on the GPU.

``frame_scores``: reference test.py:330-358 turns each cube's (raw, flow) reconstruction error into
``w_raw * (raw - mu_r) / sd_r + w_of * (of - mu_o) / sd_o``, paints it into a per-cube h x w float64 mask, max-combines the
masks, saves the frame mask with torch.save, re-loads it and takes ``.max()`` (test.py:387-392).  The maximum of a max-combined
mask is the maximum over the cubes whose painted rectangle is non-empty (``-1e5`` if there is none), which is what
``vv_frame_scores`` computes directly from the device-resident per-cube errors.

``roc_auc``: frame-level ROC-AUC (utils.py:29-41, sklearn roc_curve + auc) as the exact Mann-Whitney pair count.

Pixel-level evaluation (the criterion the reference saves its ``score_mask`` files for and never evaluates, test.py:362-365):
``box_rects`` resolves the painted rectangles on the host, ``cube_scores`` keeps the per-cube scores on the device, ``paint_masks``
paints the h x w masks there, ``merge_groups`` brings the cubes of several block groups into frame order and ``pixel_scores``
reduces a frame to the one number that carries its pixel-level ROC: with ``G`` the ground-truth pixels of an anomalous frame,
the frame is detected at threshold ``t`` iff ``100 * #{p in G: mask[p] >= t} >= percent * #G``, i.e. iff the ``k``-th largest
mask value over ``G``, ``k = ceil(#G * percent / 100)``, is ``>= t``; a normal frame is a false positive iff ``mask.max() >= t``.
The area under that ROC is ``roc_auc`` of those numbers against the frame labels.

Per-pixel anomaly maps (``[mi355x] pixel_maps``): a painted mask is constant inside every box.  ``error_zmaps`` turns the per-pixel
reconstruction errors of the bank (``FusedTrainer.score_cubes(maps=True)``) into one z-normalised 32 x 32 map per cube,
``paint_error_masks`` stretches every map over its cube's rectangle (nearest source pixel, ``patch_index``) and max-combines them
into fine masks with the support of the painted ones, and ``mask_pixel_scores`` is ``pixel_scores`` on such formed masks.

Region- and track-based detection criteria (``[mi355x] region_criterion``; RBDC / TBDC of Ramachandra and Jones, "Street Scene", WACV
2020), with regions and tracks derived from the per-pixel ground truth instead of hand-drawn annotations.  All percentages are
integers, so every comparison is exact in integer arithmetic.
  Detection: a scored cube ``m`` of a frame whose rectangle ``rects[m]`` (``box_rects`` row) is non-empty; area ``(y1-y0)*(x1-x0)``,
    score ``cube_scores[m]``.  A cube with an empty rectangle is no detection at all, as it paints nothing.
  Region: an 8-connected component of the non-zero ground-truth pixels of a frame, numbered ``1..R`` in raster order of each
    component's first pixel (``0`` = background); at most ``REGION_MAX`` = 64 per frame (``label_regions``).
  Match: detection ``m`` matches region ``r`` of its frame iff ``inter > 0 and 100 * inter >= region_iou_percent * (area_m + area_r -
    inter)`` in int64, ``inter`` = pixels of ``r`` inside the rectangle.  A detection that matches no region of its frame is a false
    positive (every detection of a normal frame is one); this does not depend on any threshold (``region_match``).
  Region score: the largest score among the detections that match the region, ``-BIG`` if none does; the region is detected at
    threshold ``t`` iff its score is ``>= t``.
  Track: regions of consecutive frames of one video are linked when they share a pixel position (``region_links``); tracks are the
    connected components of the link graph (``link_tracks``).  Track score: the ``k``-th largest region score of the track, ``k = (len
    * track_percent + 99) // 100`` -- the track is detected at ``t`` iff at least ``k`` of its regions are (``track_scores``).
  Curves (``region_curves``): thresholds are the distinct values among all region, track and false-positive scores, descending; a
    score of ``-BIG`` (a region no detection matches) is "never detected" and supplies no threshold.  At ``t``: ``fpr`` = false
    positives with score ``>= t`` / ``n_frames``, ``rbdr`` = regions with score ``>= t`` / regions, ``tbdr`` likewise for tracks.
    Each curve starts at (0, 0), is piecewise linear through its points, is cut at ``fpr = 1`` by linear interpolation on the segment
    that crosses it and extended flat to ``fpr = 1`` when its last point lies left of it; RBDC / TBDC are the trapezoid areas over
    ``fpr`` in [0, 1].  No region at all: ``nan``.  Region scores [3, 1], false positives [2], 2 frames: RBDC = 0.75.

Spatio-temporal smoothing (``[mi355x] smooth_masks``): ``smooth_masks`` filters a painted mask volume with the mean over the painted
pixels of a 3-D window that stays inside the frame's video -- three separable passes of fixed summation order, so the result is defined
to the bit -- and returns the maximum of every filtered mask, the smoothed frame score.

Macro AUROC and bootstrap intervals (``[mi355x] auc_statistics``): ``auc_bootstrap`` gives the micro AUROC (one group, or the mean over
the scenes) and the macro AUROC (the mean over the videos) of a score vector with percentile intervals from a moving-block bootstrap
inside every video or a cluster bootstrap over the videos; ``auc_counts`` computes the weighted, tie-aware pair counts of every replicate
and group on the GPU in integers (``vv_auc_boot_counts``), the statistic is formed on the host in float64.  ``auc_paired`` compares two
score vectors replicate by replicate: the draws depend on the seed alone.
"""
import math

import numpy as np
import torch

from . import _lib

BIG = 100000          # test.py:188 big_number
PIXEL_MAX_BOXES = 2048      # boxes of one frame ``pixel_scores`` takes (the LDS table of vv_pixel_scores)


def box_paints(bboxes, h, w):
    """1 where ``mask[ceil(y1):ceil(y2), ceil(x1):ceil(x2)] = score`` (test.py:352-355) touches at least one pixel."""
    out = np.zeros(len(bboxes), np.uint8)
    for m, b in enumerate(bboxes):
        x0, x1 = int(math.ceil(b[0])), int(math.ceil(b[2]))
        y0, y1 = int(math.ceil(b[1])), int(math.ceil(b[3]))
        out[m] = len(range(*slice(y0, y1).indices(h))) > 0 and len(range(*slice(x0, x1).indices(w))) > 0
    return out


def box_rects(bboxes, h, w):
    """The rectangle ``mask[ceil(y1):ceil(y2), ceil(x1):ceil(x2)]`` (test.py:352-355) of every box as int32 ``[n,4]`` rows
    ``(y0, y1, x0, x1)``: rows ``range(y0, y1)``, columns ``range(x0, x1)`` of an ``h x w`` mask.  Python slicing resolved here, on
    the host: a negative ceiling wraps, values past the edge clip; the kernels neither round nor wrap.  A row with ``y1 <= y0`` or
    ``x1 <= x0`` paints nothing: ``box_paints(b, h, w)[m] == (y1 > y0 and x1 > x0)``."""
    out = np.zeros((len(bboxes), 4), np.int32)
    for m, b in enumerate(bboxes):
        x0, x1 = int(math.ceil(b[0])), int(math.ceil(b[2]))
        y0, y1 = int(math.ceil(b[1])), int(math.ceil(b[3]))
        out[m, 0:2] = slice(y0, y1).indices(h)[:2]
        out[m, 2:4] = slice(x0, x1).indices(w)[:2]
    return out


def _dv(a, dt, dev):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dt).contiguous()


def _stats(stats, dev):
    stats = _dv(np.asarray(stats, np.float64).reshape(-1, 4) if not torch.is_tensor(stats) else stats, torch.float64, dev)
    return stats if stats.numel() else torch.zeros((1, 4), dtype=torch.float64, device=dev)


def cube_scores(raw, of, cube_stat, stats, w_raw, w_of):
    """The per-cube scores ``frame_scores`` max-reduces, kept: CUDA float64 ``[n]``, ``BIG`` where ``cube_stat`` is ``-1``, else
    ``w_raw * ((raw - mu_r) / sd_r) [+ w_of * ((of - mu_o) / sd_o)]`` in float64 with every product and sum rounded on its own (the
    kernel shares the device function with ``vv_frame_scores``).  Arguments as for ``frame_scores``.  A NaN score (zero training
    std, error equal to the mean) is outside the domain of everything downstream, as it is for ``frame_scores``."""
    if not raw.is_cuda:
        raise _lib.VecVadHipError('cube_scores needs device-resident scores; vec_vad_amd has no CPU path')
    dev = raw.device
    cube_stat, stats = _dv(cube_stat, torch.int32, dev), _stats(stats, dev)
    raw = raw.to(torch.float32).contiguous()
    of = of.to(torch.float32).contiguous() if of is not None else None
    n = raw.numel()
    if cube_stat.numel() != n or (of is not None and of.numel() != n):
        raise ValueError('cube_scores: raw, of and cube_stat must name the same %d cubes' % n)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().vv_cube_scores(raw.data_ptr(), of.data_ptr() if of is not None else None, cube_stat.data_ptr(),
                                        stats.data_ptr(), float(w_raw), float(w_of), float(BIG), n, out.data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream), 'vv_cube_scores')
    return out


def _csr(frame_off, n):
    """Host int64 copy of a CSR table, checked against ``n`` rows: the kernels trust it."""
    off = (frame_off.cpu().numpy() if torch.is_tensor(frame_off) else np.asarray(frame_off)).astype(np.int64).reshape(-1)
    if off.size < 1 or (np.diff(off) < 0).any() or off[0] < 0 or off[-1] > n:
        raise ValueError('frame_off must be non-decreasing offsets into the %d cubes given' % n)
    return off


def paint_masks(scores, frame_off, rects, h, w, out=None):
    """The painted masks of ``F`` frames on the device: ``out[f]`` is max-combined with ``scores[m]`` over the rectangle
    ``rects[m]`` (``box_rects`` rows) of every cube ``m`` in ``[frame_off[f], frame_off[f+1])`` -- what ``test.paint_frame`` paints
    per frame.  scores: CUDA float64 ``[n]`` (``cube_scores``); frame_off: int32 ``[F+1]``; rects: int32 ``[n,4]``.  ``out``: CUDA
    float64 ``[F,h,w]``, contiguous, max-accumulated into (a frame whose cubes come from several groups is painted once per
    group); None starts from the background ``-BIG``.  NaN scores are outside the domain (dropped, where numpy propagates)."""
    if not scores.is_cuda:
        raise _lib.VecVadHipError('paint_masks needs device-resident scores; vec_vad_amd has no CPU path')
    dev = scores.device
    scores = scores.to(torch.float64).contiguous().view(-1)
    off = _csr(frame_off, scores.numel())
    F = off.size - 1
    rects = _dv(rects, torch.int32, dev).view(-1, 4)
    if rects.shape[0] != scores.numel():
        raise ValueError('paint_masks: %d rectangles for %d scores' % (rects.shape[0], scores.numel()))
    if out is None:
        out = torch.full((F, h, w), -float(BIG), dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (F, h, w) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != dev:
        raise ValueError('paint_masks: out must be a contiguous float64 [%d,%d,%d] tensor on %s' % (F, h, w, dev))
    if scores.numel() == 0:           # nothing to paint: every frame keeps what it holds
        return out
    _lib.check(_lib.lib().vv_paint_masks(scores.data_ptr(), _dv(off, torch.int32, dev).data_ptr(), rects.data_ptr(), F, int(h),
                                        int(w), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), 'vv_paint_masks')
    return out


def merge_groups(groups, n_frames=None, device=None):
    """One cube list in frame order out of several.  ``groups``: list of ``(off, scores, rects)`` -- ``off`` a host int32 CSR over
    the same ``F`` frames (cubes of frame ``f`` = rows ``[off[f], off[f+1])`` of that group's tensors), ``scores`` ``[n_g]`` and
    ``rects`` ``[n_g,4]`` tensors on one device.  Returns ``(off, scores, rects)`` with the cubes ordered by frame, then by group
    in list order, then as they stand in the group.  The gather index is built on the host from the CSRs; the data moves with
    ``torch.cat`` + ``index_select`` and never visits the host.  ``n_frames`` and ``device`` tell ``F`` and where the (empty) tensors live for an empty list."""
    if not groups:
        if n_frames is None:
            raise ValueError('merge_groups: no group and no n_frames to tell the number of frames')
        return (np.zeros(n_frames + 1, np.int32), torch.zeros(0, dtype=torch.float64, device=device),
                torch.zeros((0, 4), dtype=torch.int32, device=device))
    offs = np.stack([_csr(off, len(sc)) for off, sc, _ in groups])                     # [G, F+1]
    if n_frames is not None and offs.shape[1] != n_frames + 1:
        raise ValueError('merge_groups: the groups cover %d frames, not %d' % (offs.shape[1] - 1, n_frames))
    base = np.concatenate([[0], np.cumsum([len(sc) for _, sc, _ in groups])[:-1]]).astype(np.int64)
    cnt = np.diff(offs, axis=1).T.reshape(-1)                                              # runs in (frame, group) order
    start = (offs[:, :-1] + base[:, None]).T.reshape(-1)                                   # first row of each run in the cat
    first = np.concatenate([[0], np.cumsum(cnt)])
    idx = np.repeat(start - first[:-1], cnt) + np.arange(first[-1])
    off = first[::offs.shape[0]].astype(np.int32)
    dev = groups[0][1].device
    idx = torch.from_numpy(idx).to(dev)
    scores = torch.cat([sc.reshape(-1) for _, sc, _ in groups]).index_select(0, idx)
    rects = torch.cat([rc.reshape(-1, 4) for _, _, rc in groups]).index_select(0, idx)
    return off, scores, rects


def pixel_scores(gt, scores, frame_off, rects, percent=40, out=None):
    """The pixel-level score of ``F`` frames (module docstring).  gt: uint8 ``[F,h,w]`` ground truth (non-zero = anomalous pixel;
    CUDA tensor, or a host array that is uploaded); scores / frame_off / rects as for ``paint_masks``, with ALL cubes of a frame in
    this one call (``merge_groups``): the quantile is not max-decomposable.  Returns ``(s_pix, gt_count)``, CUDA float64 ``[F]``
    and int32 ``[F]``: ``gt_count[f]`` = ground-truth pixels of frame ``f``; ``s_pix[f]`` = the ``k``-th largest value of the painted
    mask over them, ``k = (gt_count * percent + 99) // 100``, for an anomalous frame (``-BIG`` when fewer than ``k`` of them lie
    under a box) and ``mask.max()`` for a normal one, written into ``out`` when one is given.  The mask itself is never formed.  A frame with more than
    ``PIXEL_MAX_BOXES`` cubes is a ``ValueError`` before any launch.  NaN scores are outside the domain."""
    if not scores.is_cuda:
        raise _lib.VecVadHipError('pixel_scores needs device-resident scores; vec_vad_amd has no CPU path')
    if int(percent) != percent or not 1 <= int(percent) <= 100:
        raise ValueError('pixel_scores: percent must be an integer in 1..100, got %r' % (percent,))
    dev = scores.device
    scores = scores.to(torch.float64).contiguous().view(-1)
    off = _csr(frame_off, scores.numel())
    F = off.size - 1
    gt = _dv(gt, torch.uint8, dev)
    if gt.dim() != 3 or gt.shape[0] != F:
        raise ValueError('pixel_scores: gt must be [%d,h,w], got %s' % (F, tuple(gt.shape)))
    rects = _dv(rects, torch.int32, dev).view(-1, 4)
    if rects.shape[0] != scores.numel():
        raise ValueError('pixel_scores: %d rectangles for %d scores' % (rects.shape[0], scores.numel()))
    counts = np.diff(off)
    most = int(counts.max()) if F else 0
    if most > PIXEL_MAX_BOXES:
        raise ValueError('pixel_scores: frame %d has %d boxes, at most %d are supported' % (int(counts.argmax()), most, PIXEL_MAX_BOXES))
    if out is None:
        out = torch.empty(F, dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (F,) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != dev:
        raise ValueError('pixel_scores: out must be a contiguous float64 [%d] tensor on %s' % (F, dev))
    cnt = torch.empty(F, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().vv_pixel_scores(gt.data_ptr(), scores.data_ptr(), _dv(off, torch.int32, dev).data_ptr(), rects.data_ptr(),
                                         int(percent), float(BIG), F, int(gt.shape[1]), int(gt.shape[2]), most, out.data_ptr(),
                                         cnt.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), 'vv_pixel_scores')
    return out, cnt


PATCH = 32             # side of a cube's patch: the z-maps are [n, PATCH, PATCH]


def patch_index(v, lo, hi):
    """The patch row (column) painted at frame row (column) ``v`` of a rectangle ``[lo, hi)``: the nearest source pixel of the 32-pixel
    patch stretched over it, ``((2 * (v - lo) + 1) * 32) // (2 * (hi - lo))`` in integers -- ``0..31``, non-decreasing in ``v``, the
    identity when ``hi - lo == 32``.  What ``vv_paint_zmaps`` computes; numpy integer arrays or ints."""
    return ((2 * (v - lo) + 1) * PATCH) // (2 * (hi - lo))


def error_zmaps(e_raw, e_of, cube_stat, stats, w_raw, w_of):
    """The z-map of every cube: CUDA float64 ``[n,32,32]``, ``z[m][q] = w_raw * ((1024 * e_raw[m][q] - mu_r) / sd_r) [+ w_of * ((1024 *
    e_of[m][q] - mu_o) / sd_o)]`` -- the expression of ``cube_scores`` (the same device function, float64, every product, quotient and
    sum rounded on its own) with 1024 times the pixel's error in place of the cube's, ``BIG`` where ``cube_stat`` is ``-1``.  The cube's
    error is the sum of its 1024 pixel errors, so a cube whose error is spread evenly gets the constant map ``z = its cube score``, to
    the bit.  e_raw / e_of: CUDA float32 ``[n,32,32]`` (``of=None`` drops the flow term); cube_stat, stats as for ``cube_scores``.
    Costs 8 KB of device memory per cube: form the maps of a chunk of frames, not of a test set."""
    if not e_raw.is_cuda:
        raise _lib.VecVadHipError('error_zmaps needs device-resident error maps; vec_vad_amd has no CPU path')
    dev = e_raw.device
    cube_stat, stats = _dv(cube_stat, torch.int32, dev), _stats(stats, dev)
    e_raw = e_raw.to(torch.float32).contiguous()
    e_of = e_of.to(torch.float32).contiguous() if e_of is not None else None
    n = cube_stat.numel()
    if e_raw.numel() != n * PATCH * PATCH or (e_of is not None and e_of.numel() != n * PATCH * PATCH):
        raise ValueError('error_zmaps: e_raw, e_of must be [%d,%d,%d] maps of the %d cubes of cube_stat' % (n, PATCH, PATCH, n))
    out = torch.empty((n, PATCH, PATCH), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().vv_error_zmaps(e_raw.data_ptr(), e_of.data_ptr() if e_of is not None else None, cube_stat.data_ptr(),
                                        stats.data_ptr(), float(w_raw), float(w_of), float(BIG), n, out.data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream), 'vv_error_zmaps')
    return out


def paint_error_masks(z, frame_off, rects, h, w, out=None):
    """``paint_masks`` with a value that varies inside the box: pixel ``(y, x)`` of the rectangle ``(y0, y1, x0, x1)`` of cube ``m`` is
    max-combined with ``z[m][patch_index(y, y0, y1)][patch_index(x, x0, x1)]``.  z: CUDA float64 ``[n,32,32]`` (``error_zmaps``);
    frame_off, rects, h, w and ``out`` exactly as for ``paint_masks`` (CSR over ``F`` frames, ``box_rects`` rows, float64 ``[F,h,w]``
    max-accumulated into, background ``-BIG`` when None): a frame may be painted group by group, and the support of a fine mask is the
    support of the painted one.  For a box inside the frame the rectangle is the crop the cube was cut from.  NaNs are outside the
    domain."""
    if not z.is_cuda:
        raise _lib.VecVadHipError('paint_error_masks needs device-resident maps; vec_vad_amd has no CPU path')
    dev = z.device
    z = z.to(torch.float64).contiguous().view(-1, PATCH, PATCH)
    n = z.shape[0]
    off = _csr(frame_off, n)
    F = off.size - 1
    rects = _dv(rects, torch.int32, dev).view(-1, 4)
    if rects.shape[0] != n:
        raise ValueError('paint_error_masks: %d rectangles for %d maps' % (rects.shape[0], n))
    if out is None:
        out = torch.full((F, h, w), -float(BIG), dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (F, h, w) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != dev:
        raise ValueError('paint_error_masks: out must be a contiguous float64 [%d,%d,%d] tensor on %s' % (F, h, w, dev))
    if n == 0:                        # nothing to paint: every frame keeps what it holds
        return out
    _lib.check(_lib.lib().vv_paint_zmaps(z.data_ptr(), _dv(off, torch.int32, dev).data_ptr(), rects.data_ptr(), F, int(h), int(w),
                                        out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), 'vv_paint_zmaps')
    return out


def mask_pixel_scores(gt, masks, percent=40, out=None):
    """``pixel_scores`` on formed masks.  gt: uint8 ``[F,h,w]`` (CUDA tensor, or a host array that is uploaded); masks: CUDA float64
    ``[F,h,w]`` (``paint_error_masks``, ``paint_masks``).  Returns ``(s_pix, gt_count)``, CUDA float64 ``[F]`` and int32 ``[F]``:
    ``s_pix[f]`` = the ``k``-th largest value of ``masks[f]`` over the ground-truth pixels, ``k = (gt_count * percent + 99) // 100``, for
    an anomalous frame (a ``-BIG`` pixel counts as ``-BIG``) and ``masks[f].max()`` for a normal one, written into ``out`` when one is
    given.  Exact (a radix select on the integer image of the doubles), whatever the ties.  NaNs are outside the domain."""
    if not masks.is_cuda:
        raise _lib.VecVadHipError('mask_pixel_scores needs device-resident masks; vec_vad_amd has no CPU path')
    if int(percent) != percent or not 1 <= int(percent) <= 100:
        raise ValueError('mask_pixel_scores: percent must be an integer in 1..100, got %r' % (percent,))
    dev = masks.device
    if masks.dim() != 3:
        raise ValueError('mask_pixel_scores: masks must be [F,h,w], got %s' % (tuple(masks.shape),))
    masks = masks.to(torch.float64).contiguous()
    F, h, w = masks.shape
    gt = _dv(gt, torch.uint8, dev)
    if tuple(gt.shape) != (F, h, w):
        raise ValueError('mask_pixel_scores: gt must be [%d,%d,%d], got %s' % (F, h, w, tuple(gt.shape)))
    if out is None:
        out = torch.empty(F, dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (F,) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != dev:
        raise ValueError('mask_pixel_scores: out must be a contiguous float64 [%d] tensor on %s' % (F, dev))
    cnt = torch.empty(F, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().vv_mask_kth(gt.data_ptr(), masks.data_ptr(), int(percent), float(BIG), F, int(h), int(w), out.data_ptr(),
                                     cnt.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), 'vv_mask_kth')
    return out, cnt


SMOOTH_MAX = 33        # widest window of ``smooth_masks`` (VV_SMOOTH_MAX: a 32 x 32 tile with its halo of 16 fits a workgroup's LDS)


def smooth_window(name, v):
    """``v`` as a window of ``smooth_masks``: an odd integer in 1..``SMOOTH_MAX``, else a one-line ``ValueError`` that names it."""
    if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= SMOOTH_MAX or int(v) % 2 == 0:
        raise ValueError('%s must be an odd integer in 1..%d, got %r' % (name, SMOOTH_MAX, v))
    return int(v)


def smooth_masks(masks, video_idx, smooth_frames, smooth_pixels, lo=0, hi=None, out=None):
    """The spatio-temporal mean filter of a mask volume, restricted to the painted pixels (``[mi355x] smooth_masks``; the 3-D mean
    filter the object-centric VAD protocol runs over its map volume before it takes frame scores).  masks: CUDA float64 ``[F,h,w]``, a
    buffer of consecutive frames (``paint_masks``), ``-BIG`` = unpainted; video_idx: ``[F]`` integers, the video of every frame of the
    buffer; smooth_frames / smooth_pixels: odd windows in 1..33 along time / along both image axes.  A painted pixel becomes the mean of
    the painted pixels of its window -- frames of the buffer that belong to its video, rows and columns inside the image --, an
    unpainted pixel stays ``-BIG``: the support is preserved and windows (1, 1) return the masks.  The sums are separable (x, then y,
    then t), each taken in ascending offset order in float64, and the mean is one division: the result is defined to the bit
    (``include/vecvad_hip.h``, vv_smooth_masks).  A ``+BIG`` box (a block without a trained model) floods its neighbourhood: every
    painted pixel whose window reaches it gets a mean far above any trained score, on purpose.

    ``lo`` / ``hi`` (default: the whole buffer): only frames ``[lo, hi)`` are returned, the others serve as temporal halo -- a caller
    that filters a long volume chunk by chunk passes ``smooth_frames // 2`` extra frames on either side.  Returns ``(smoothed, frame_max)``,
    CUDA float64 ``[hi-lo,h,w]`` (``out`` when one is given) and ``[hi-lo]``: ``frame_max[f] = smoothed[f].max()`` (``-BIG`` for a frame
    without a painted pixel), the smoothed frame score.  NaNs are outside the domain."""
    if not torch.is_tensor(masks) or not masks.is_cuda:
        raise _lib.VecVadHipError('smooth_masks needs device-resident masks; vec_vad_amd has no CPU path')
    kt, ks = smooth_window('smooth_masks: smooth_frames', smooth_frames), smooth_window('smooth_masks: smooth_pixels', smooth_pixels)
    if masks.dim() != 3 or masks.dtype != torch.float64:
        raise ValueError('smooth_masks: masks must be a float64 [F,h,w] tensor, got %s %s' % (masks.dtype, tuple(masks.shape)))
    dev = masks.device
    masks = masks.contiguous()
    F, h, w = masks.shape
    if h * w >= 2 ** 31:
        raise ValueError('smooth_masks: frames of %d x %d pixels, fewer than 2^31 are supported' % (h, w))
    vid = np.asarray(video_idx.cpu() if torch.is_tensor(video_idx) else video_idx).reshape(-1)
    if vid.size != F or (vid.size and (vid.dtype.kind not in 'iu' or abs(vid.astype(np.int64)).max() >= 2 ** 31)):
        raise ValueError('smooth_masks: video_idx must name the video of each of the %d frames as an int32, got %s %s' % (
            F, vid.dtype, vid.shape))
    hi = F if hi is None else hi
    if int(lo) != lo or int(hi) != hi or not 0 <= lo <= hi <= F:
        raise ValueError('smooth_masks: frames [%r, %r) do not lie in the buffer of %d frames' % (lo, hi, F))
    lo, hi = int(lo), int(hi)
    if out is None:
        out = torch.empty((hi - lo, h, w), dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (hi - lo, h, w) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != dev:
        raise ValueError('smooth_masks: out must be a contiguous float64 [%d,%d,%d] tensor on %s' % (hi - lo, h, w, dev))
    fmax = torch.empty(hi - lo, dtype=torch.float64, device=dev)
    if hi == lo:
        return out, fmax
    work = torch.empty(max(1, int(_lib.lib().vv_smooth_masks_work(F, h, w, kt, ks))), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().vv_smooth_masks(masks.data_ptr(), _dv(vid.astype(np.int32), torch.int32, dev).data_ptr(), F, h, w, lo, hi, kt, ks,
                                         out.data_ptr(), fmax.data_ptr(), work.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               'vv_smooth_masks')
    return out, fmax


REGION_MAX = 64        # regions of one frame (the tables of vv_region_match / vv_region_links; one bit each in a link word)


def _percent(name, v):
    if int(v) != v or not 1 <= int(v) <= 100:
        raise ValueError('%s must be an integer in 1..100, got %r' % (name, v))
    return int(v)


def label_regions(gt, frame0=0):
    """The ground-truth regions of ``F`` frames (module docstring).  gt: uint8 ``[F,h,w]`` (non-zero = anomalous pixel; CUDA tensor, or
    a host array that is uploaded).  Returns ``(labels, n_regions)``, CUDA int32 ``[F,h,w]`` and ``[F]``: ``labels[f]`` holds ``0`` for
    background and ``1..R`` for the 8-connected components in raster order of their first pixel, ``n_regions[f] = R``.  A frame with
    more than ``REGION_MAX`` regions is a one-line ``ValueError`` that names it as frame ``frame0 + f``."""
    if not torch.is_tensor(gt):
        gt = torch.from_numpy(np.ascontiguousarray(gt))
    if not torch.cuda.is_available():
        raise _lib.VecVadHipError('label_regions needs a GPU; vec_vad_amd has no CPU path')
    dev = gt.device if gt.is_cuda else torch.device('cuda', torch.cuda.current_device())
    gt = _dv(gt, torch.uint8, dev)
    if gt.dim() != 3:
        raise ValueError('label_regions: gt must be [F,h,w], got %s' % (tuple(gt.shape),))
    F, h, w = gt.shape
    labels = torch.empty((F, h, w), dtype=torch.int32, device=dev)
    n_regions = torch.zeros(F, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().vv_label_regions(gt.data_ptr(), labels.data_ptr(), n_regions.data_ptr(), F, h, w,
                                          torch.cuda.current_stream(dev).cuda_stream), 'vv_label_regions')
    cnt = n_regions.cpu().numpy()
    if F and int(cnt.max()) > REGION_MAX:
        f = int(np.nonzero(cnt > REGION_MAX)[0][0])
        raise ValueError('label_regions: frame %d has %d ground-truth regions, at most %d are supported' % (frame0 + f, int(cnt[f]), REGION_MAX))
    return labels, n_regions


def _labels(name, labels):
    if not torch.is_tensor(labels) or not labels.is_cuda:
        raise _lib.VecVadHipError('%s needs device-resident labels; vec_vad_amd has no CPU path' % name)
    if labels.dim() != 3 or labels.dtype != torch.int32:
        raise ValueError('%s: labels must be an int32 [F,h,w] tensor (label_regions), got %s %s' % (name, labels.dtype, tuple(labels.shape)))
    return labels.contiguous()


def region_match(labels, scores, frame_off, rects, iou_percent=10):
    """Detections against regions (module docstring).  labels: CUDA int32 ``[F,h,w]`` (``label_regions``); scores / frame_off / rects
    as for ``pixel_scores``, with ALL cubes of a frame in this one call (``merge_groups``); any number of cubes per frame.  Returns
    ``(region_area, region_score, box_state)``: CUDA int32 ``[F,64]`` (pixels of region ``r`` of frame ``f`` at ``[f, r-1]``, 0 past the
    frame's last region), float64 ``[F,64]`` (the largest score among the detections that match the region, ``-BIG`` if none does) and
    uint8 ``[n]`` (0 = empty rectangle: no detection, 1 = matched a region, 2 = false positive).  NaN scores are outside the domain."""
    labels = _labels('region_match', labels)
    iou_percent = _percent('region_match: iou_percent', iou_percent)
    dev = labels.device
    F, h, w = labels.shape
    scores = _dv(scores, torch.float64, dev).view(-1)
    n = scores.numel()
    off = _csr(frame_off, n)
    if off.size - 1 != F:
        raise ValueError('region_match: frame_off covers %d frames, labels %d' % (off.size - 1, F))
    rects = _dv(rects, torch.int32, dev).view(-1, 4)
    if rects.shape[0] != n:
        raise ValueError('region_match: %d rectangles for %d scores' % (rects.shape[0], n))
    area = torch.empty((F, REGION_MAX), dtype=torch.int32, device=dev)
    best = torch.empty((F, REGION_MAX), dtype=torch.float64, device=dev)
    state = torch.zeros(n, dtype=torch.uint8, device=dev)      # a cube no frame of the CSR names stays 0
    _lib.check(_lib.lib().vv_region_match(labels.data_ptr(), scores.data_ptr(), _dv(off, torch.int32, dev).data_ptr(), rects.data_ptr(),
                                         iou_percent, float(BIG), F, h, w, n, area.data_ptr(), best.data_ptr(), state.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream), 'vv_region_match')
    return area, best, state


def region_links(labels, prev=None, same_video=None):
    """Links between the regions of consecutive frames (module docstring).  labels: CUDA int32 ``[F,h,w]``; prev: the label map of the
    frame before ``labels[0]`` (CUDA int32 ``[h,w]``) or None when there is none; same_video: ``[F]``, non-zero where frame ``f``
    continues the video of the frame before it (None: all ones).  Returns CUDA int64 ``[F,64]`` holding 64-bit words: bit ``q-1`` of
    ``links[f, r-1]`` is set iff region ``r`` of frame ``f`` shares a pixel position with region ``q`` of the frame before it; zeros
    for a frame with ``same_video[f] == 0`` and for frame 0 without ``prev``."""
    labels = _labels('region_links', labels)
    dev = labels.device
    F, h, w = labels.shape
    if prev is not None:
        if not torch.is_tensor(prev) or tuple(prev.shape) != (h, w) or prev.dtype != torch.int32 or prev.device != dev:
            raise ValueError('region_links: prev must be an int32 [%d,%d] tensor on %s' % (h, w, dev))
        prev = prev.contiguous()
    same = torch.ones(F, dtype=torch.uint8, device=dev) if same_video is None else \
        _dv(np.asarray(same_video).astype(bool).astype(np.uint8) if not torch.is_tensor(same_video) else (same_video != 0), torch.uint8, dev).view(-1)
    if same.numel() != F:
        raise ValueError('region_links: same_video names %d frames, labels %d' % (same.numel(), F))
    links = torch.zeros((F, REGION_MAX), dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().vv_region_links(prev.data_ptr() if prev is not None else None, labels.data_ptr(), same.data_ptr(), F, h, w,
                                         links.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), 'vv_region_links')
    return links


def link_tracks(n_regions, links, track_percent=10):
    """Tracks out of link words, on the host.  n_regions: ``[F]`` regions per frame (each ``<= REGION_MAX``); links: ``[F,64]`` 64-bit
    words (``region_links``, chunks concatenated in frame order; int64 or uint64).  The regions are listed in (frame, number) order;
    union-find over the link bits joins region ``r`` of frame ``f`` with every region ``q`` of frame ``f - 1`` whose bit is set.
    Returns ``(track, length, k)``: int64 ``[n_total]`` track id per region (tracks numbered ``0..T-1`` in order of their first
    region), int64 ``[T]`` regions per track and int64 ``[T]`` ``k = (length * track_percent + 99) // 100``."""
    track_percent = _percent('link_tracks: track_percent', track_percent)
    n_regions = np.asarray(n_regions.cpu() if torch.is_tensor(n_regions) else n_regions, np.int64).reshape(-1)
    F = n_regions.size
    links = links.cpu().numpy() if torch.is_tensor(links) else links
    words = np.ascontiguousarray(np.asarray(links)).reshape(F, REGION_MAX).view(np.uint64) if F else np.zeros((0, REGION_MAX), np.uint64)
    if F and (n_regions.min() < 0 or n_regions.max() > REGION_MAX):
        raise ValueError('link_tracks: n_regions must lie in 0..%d' % REGION_MAX)
    first = np.concatenate([[0], np.cumsum(n_regions)])
    parent = list(range(int(first[-1])))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for f in range(1, F):
        for r in range(int(n_regions[f])):
            word = int(words[f, r])
            q = 0
            while word:
                if word & 1:
                    if q >= n_regions[f - 1]:
                        raise ValueError('link_tracks: frame %d links to region %d of a frame with %d regions' % (f, q + 1, n_regions[f - 1]))
                    a, b = find(int(first[f]) + r), find(int(first[f - 1]) + q)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
                word >>= 1
                q += 1
    ids, track = {}, np.zeros(len(parent), np.int64)
    for i in range(len(parent)):
        track[i] = ids.setdefault(find(i), len(ids))      # roots are the first region of their track: ids grow in region order
    length = np.bincount(track, minlength=len(ids)).astype(np.int64)
    return track, length, (length * track_percent + 99) // 100


def track_scores(region_scores, track, k):
    """The ``k[t]``-th largest region score of every track ``t`` (float64 ``[T]``): the track is detected at ``t`` iff at least ``k`` of
    its regions are.  region_scores ``[n]``, track ``[n]`` (``link_tracks``), k ``[T]``."""
    region_scores, track = np.asarray(region_scores, np.float64).reshape(-1), np.asarray(track, np.int64).reshape(-1)
    k = np.asarray(k, np.int64).reshape(-1)
    out = np.empty(k.size, np.float64)
    for t in range(k.size):
        out[t] = np.sort(region_scores[track == t])[::-1][k[t] - 1]
    return out


def _area_to_one(x, y):
    """Trapezoid area over ``x`` in [0, 1] of the piecewise-linear curve through (x[i], y[i]) (x non-decreasing, x[0] == 0): cut at
    ``x = 1`` by interpolation on the segment that crosses it, extended flat when the last point lies left of it."""
    area = 0.0
    for i in range(1, len(x)):
        x0, x1, y0, y1 = x[i - 1], x[i], y[i - 1], y[i]
        if x1 > 1.0:
            if x0 < 1.0:
                yc = y0 + (y1 - y0) * (1.0 - x0) / (x1 - x0)
                area += (1.0 - x0) * (y0 + yc) / 2.0
            return area
        area += (x1 - x0) * (y0 + y1) / 2.0
    return area + (1.0 - x[-1]) * y[-1]


def region_curves(region_scores, track_scores, fp_scores, n_frames, log=print):
    """RBDC and TBDC from the three score lists (module docstring), on the host in float64.  Returns ``(fpr, rbdr, tbdr, rbdc, tbdc)``:
    the curve points, one per threshold in descending order behind the starting point (0, 0) (``fpr`` is not cut at 1; the areas
    are).  Without a region the two numbers are ``nan``, the arrays hold the false-positive curve against zeros and a line says so."""
    rs, ts, fp = (np.asarray(a, np.float64).reshape(-1) for a in (region_scores, track_scores, fp_scores))
    if int(n_frames) != n_frames or n_frames < 1:
        raise ValueError('region_curves: n_frames must be a positive integer, got %r' % (n_frames,))
    if (rs.size == 0) != (ts.size == 0):
        raise ValueError('region_curves: %d regions but %d tracks' % (rs.size, ts.size))
    if np.isnan(rs).any() or np.isnan(ts).any() or np.isnan(fp).any():
        raise ValueError('region_curves: NaN scores are outside the domain')
    every = np.concatenate([rs, ts, fp])
    thr = np.unique(every[every > -float(BIG)])[::-1]              # descending; -BIG = never detected
    rs_s, ts_s, fp_s = np.sort(rs), np.sort(ts), np.sort(fp)

    def at_least(sorted_scores):                                   # how many scores are >= each threshold
        return (sorted_scores.size - np.searchsorted(sorted_scores, thr, side='left')).astype(np.float64)

    fpr = np.concatenate([[0.0], at_least(fp_s) / float(n_frames)])
    rbdr = np.concatenate([[0.0], at_least(rs_s) / rs.size if rs.size else np.zeros(thr.size)])
    tbdr = np.concatenate([[0.0], at_least(ts_s) / ts.size if ts.size else np.zeros(thr.size)])
    if rs.size == 0:
        log('no ground-truth region in the test set: RBDC and TBDC are undefined (nan)')
        return fpr, rbdr, tbdr, float('nan'), float('nan')
    return fpr, rbdr, tbdr, float(_area_to_one(fpr, rbdr)), float(_area_to_one(fpr, tbdr))


def frame_scores(raw, of, frame_off, cube_stat, stats, paints, w_raw, w_of, out=None):
    """raw / of: CUDA float32 ``[n]`` per-cube errors (``of=None`` when useFlow is off); frame_off: int32 ``[F+1]`` CSR
    offsets of each frame's cubes; cube_stat: int32 ``[n]`` row of ``stats`` (``-1`` = block without a trained model ->
    score ``BIG``); stats: float64 ``[S,4]`` (mu_r, sd_r, mu_o, sd_o); paints: uint8 ``[n]``.
    Returns (and max-accumulates into ``out`` if given) the CUDA float64 ``[F]`` frame scores."""
    dev = raw.device
    if not raw.is_cuda:
        raise _lib.VecVadHipError('frame_scores needs device-resident scores; vec_vad_amd has no CPU path')

    def dv(a, dt):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=dev, dtype=dt).contiguous()

    frame_off, cube_stat, paints = dv(frame_off, torch.int32), dv(cube_stat, torch.int32), dv(paints, torch.uint8)
    stats = dv(np.asarray(stats, np.float64).reshape(-1, 4) if not torch.is_tensor(stats) else stats, torch.float64)
    if stats.numel() == 0:
        stats = torch.zeros((1, 4), dtype=torch.float64, device=dev)
    raw = raw.to(torch.float32).contiguous()
    of = of.to(torch.float32).contiguous() if of is not None else None
    F = frame_off.numel() - 1
    if out is None:
        out = torch.full((F,), -float(BIG), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().vv_frame_scores(raw.data_ptr(), of.data_ptr() if of is not None else None,
                                         frame_off.data_ptr(), cube_stat.data_ptr(), stats.data_ptr(), paints.data_ptr(),
                                         float(w_raw), float(w_of), float(BIG), F, out.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream), 'vv_frame_scores')
    return out


AUC_UNITS = {'none': 0, 'video': 1, 'block': 2}      # VV_AUC_UNIT_*
AUC_BOOT_MAX_VIDEOS = 65536                          # VV_AUC_BOOT_MAX_VIDEOS
AUC_WORK_BYTES = 256 << 20                           # device scratch of one vv_auc_boot_counts call; more replicates take more calls


def auc_settings(replicates=1000, unit='block', block=25, seed=0, confidence=95):
    """The settings of ``auc_bootstrap`` (the ``[mi355x] auc_*`` keys), checked: a dict, or a one-line ``ValueError`` that names the key."""
    def integer(name, v, lo, hi):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError('%s must be an integer in %d..%d, got %r' % (name, lo, hi, v))
        return int(v)
    unit = str(unit).strip().lower()
    if unit not in ('block', 'video'):
        raise ValueError("auc_bootstrap_unit must be 'block' or 'video', got %r" % (unit,))
    return dict(n_replicates=integer('auc_bootstrap', replicates, 0, 2 ** 31 - 1), unit=unit,
                block=integer('auc_bootstrap_block', block, 1, 2 ** 31 - 1), seed=integer('auc_bootstrap_seed', seed, 0, 2 ** 64 - 1),
                confidence=integer('auc_confidence', confidence, 50, 99))


def _runs(name, idx, n):
    """Per-frame ids that are constant over contiguous runs -> (run starts with ``n`` appended, id of every run); an id that comes back
    after another one is a ``ValueError``."""
    idx = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx).reshape(-1)
    if idx.size != n or (n and idx.dtype.kind not in 'iu'):
        raise ValueError('%s must name every one of the %d frames with an integer, got %s %s' % (name, n, idx.dtype, idx.shape))
    start = np.concatenate([[0], np.nonzero(idx[1:] != idx[:-1])[0] + 1]) if n else np.zeros(0, np.int64)
    ids = idx[start]
    if np.unique(ids).size != ids.size:
        raise ValueError('%s: the frames of one video must be contiguous' % name)
    return np.concatenate([start, [n]]).astype(np.int64), ids


def auc_tables(scores, labels, video_idx, groups=None, strata=None):
    """The host tables of ``vv_auc_boot_counts`` (``include/vecvad_hip.h``) for one score vector, as a dict of numpy arrays: ``order``,
    ``tie``, ``label``, ``group_off``, ``video_off``, ``stratum_off`` and the sizes ``n``, ``G``, ``V``, ``S``.  scores ``[n]`` floats
    (no NaN); labels ``[n]`` (non-zero = anomalous); video_idx ``[n]`` integers, the video of every frame (contiguous per video);
    groups ``[n]`` integers, the group of every frame (None: one group; groups are numbered in ascending order of their ids) and
    strata ``[n]`` integers likewise (None: one stratum; numbered in order of appearance).  Every group and every stratum must be
    made of whole videos and the videos of a stratum must follow one another; otherwise, and for more than ``AUC_BOOT_MAX_VIDEOS``
    videos or ``max(V_s) * n >= 2^31`` (U2 would not fit int64), a one-line ``ValueError``."""
    scores = np.asarray(scores.cpu() if torch.is_tensor(scores) else scores, np.float64).reshape(-1)
    n = scores.size
    if n >= 2 ** 31:
        raise ValueError('auc_tables: %d frames, fewer than 2^31 are supported' % n)
    if np.isnan(scores).any():
        raise ValueError('auc_tables: NaN scores are outside the domain')
    label = (np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).reshape(-1) != 0).astype(np.uint8)
    if label.size != n:
        raise ValueError('auc_tables: %d labels for %d scores' % (label.size, n))
    video_off, _ = _runs('auc_tables: video_idx', video_idx, n)
    V = video_off.size - 1
    if V > AUC_BOOT_MAX_VIDEOS:
        raise ValueError('auc_tables: %d videos, at most %d are supported' % (V, AUC_BOOT_MAX_VIDEOS))
    first = video_off[:-1]

    def per_video(name, ids):
        """ids ``[n]`` -> the id of every video, after checking that it is constant inside every video"""
        ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).reshape(-1)
        if ids.size != n or (n and ids.dtype.kind not in 'iu'):
            raise ValueError('auc_tables: %s must name every one of the %d frames with an integer, got %s %s' % (name, n, ids.dtype, ids.shape))
        if n and (ids != np.repeat(ids[first], np.diff(video_off))).any():
            raise ValueError('auc_tables: every one of the %s must be a union of whole videos' % name)
        return ids[first]

    if groups is None:
        grank, G = np.zeros(n, np.int64), 1
    else:
        gids = per_video('groups', groups)
        uniq = np.unique(gids)
        G = max(1, uniq.size)
        grank = np.searchsorted(uniq, np.asarray(groups.cpu() if torch.is_tensor(groups) else groups).reshape(-1)).astype(np.int64)
    if strata is None:
        stratum_off = np.array([0, V], np.int64)
    else:
        sids = per_video('strata', strata)
        s_start = np.concatenate([[0], np.nonzero(sids[1:] != sids[:-1])[0] + 1]) if V else np.zeros(0, np.int64)
        if np.unique(sids[s_start]).size != s_start.size:
            raise ValueError('auc_tables: the videos of one of the strata must follow one another')
        stratum_off = np.concatenate([s_start, [V]]).astype(np.int64)
    if V and int(np.diff(stratum_off).max()) * n >= 2 ** 31:
        raise ValueError('auc_tables: max(V_s) * n = %d * %d >= 2^31: U2 would not fit int64' % (int(np.diff(stratum_off).max()), n))
    order = np.lexsort((scores, grank))                                    # stable: by group, then ascending by score
    so, go = scores[order], grank[order]
    head = np.ones(n, bool)
    if n:
        head[1:] = (go[1:] != go[:-1]) | (so[1:] != so[:-1])
    group_off = np.searchsorted(go, np.arange(G + 1)).astype(np.int64)
    return dict(order=order.astype(np.int32), tie=(np.cumsum(head) - 1).astype(np.int32), label=label, group_off=group_off.astype(np.int32),
                video_off=video_off.astype(np.int32), stratum_off=stratum_off.astype(np.int32), n=n, G=G, V=V, S=stratum_off.size - 1)


def auc_tables_device(tables, device):
    """``auc_tables`` output with its six arrays as tensors on ``device`` (uploaded once per score vector)."""
    dev = dict(tables)
    for k in ('order', 'tie', 'label', 'group_off', 'video_off', 'stratum_off'):
        dev[k] = torch.from_numpy(np.ascontiguousarray(tables[k])).to(device)
    return dev


def auc_counts_device(t, unit, block, seed, r0, R, out=None, work=None):
    """``vv_auc_boot_counts`` on uploaded tables (``auc_tables_device``): the CUDA int64 ``[R, G, 3]`` rows ``(U2, P, N)`` of replicates
    ``r0 .. r0+R-1``, in as many calls as keep the scratch of one below ``AUC_WORK_BYTES`` (``work``: a uint8 scratch tensor to reuse)."""
    dev = t['order'].device
    if dev.type != 'cuda':
        raise _lib.VecVadHipError('auc_counts needs a GPU; vec_vad_amd has no CPU path')
    if unit not in AUC_UNITS:
        raise ValueError("auc_counts: unit must be 'none', 'video' or 'block', got %r" % (unit,))
    if isinstance(R, bool) or int(R) != R or R < 0 or int(r0) != r0 or r0 < 1 or int(block) != block or not 1 <= block < 2 ** 31:
        raise ValueError('auc_counts: r0 >= 1, R >= 0 and 1 <= block < 2^31 must be integers, got r0 = %r, R = %r, block = %r' % (r0, R, block))
    if int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise ValueError('auc_counts: seed must be an integer in 0..2^64-1, got %r' % (seed,))
    if unit == 'none' and R != 1:
        raise ValueError("auc_counts: unit 'none' is the full sample, R must be 1, got %r" % (R,))
    R, n, G, V = int(R), t['n'], t['G'], t['V']
    if out is None:
        out = torch.empty((R, G, 3), dtype=torch.int64, device=dev)
    l = _lib.lib()
    per = int(l.vv_auc_boot_work(n, V, 1, AUC_UNITS[unit]))
    if per < 0:
        raise _lib.VecVadHipError('vv_auc_boot_work refuses n = %d, V = %d' % (n, V))
    step = max(1, min(R, AUC_WORK_BYTES // max(1, per), (2 ** 31 - 1) // max(1, G, V)))
    for k in range(0, R, step):
        m = min(step, R - k)
        need = int(l.vv_auc_boot_work(n, V, m, AUC_UNITS[unit]))
        if work is None or work.numel() < need:
            work = torch.empty(max(8, need), dtype=torch.uint8, device=dev)
        _lib.check(l.vv_auc_boot_counts(t['order'].data_ptr(), t['tie'].data_ptr(), t['label'].data_ptr(), t['group_off'].data_ptr(),
                                        t['video_off'].data_ptr(), t['stratum_off'].data_ptr(), n, G, V, t['S'], int(seed), int(r0) + k,
                                        m, AUC_UNITS[unit], int(block), out[k:].data_ptr(), work.data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream), 'vv_auc_boot_counts')
    return out


def auc_counts(scores, labels, video_idx, groups, unit, block, seed, r0, R, strata=None):
    """Weighted Mann-Whitney counts of bootstrap replicates on the GPU: host int64 ``[R, G, 3]``, row ``(U2, P, N)`` of replicate ``r0 +
    k`` and group ``g`` -- ``P`` / ``N`` the weighted positive / negative frames of the group, ``U2`` = twice the weighted pairs
    (positive above negative) plus the tied ones; the group's AUROC is ``U2 / (2 P N)``.  scores / labels / video_idx / groups / strata:
    as for ``auc_tables``.  unit: ``'none'`` (the full sample, every weight 1, ``R = 1``), ``'video'`` (cluster bootstrap: in every
    stratum as many videos are drawn with replacement as it holds) or ``'block'`` (moving-block bootstrap inside every video: ``ceil(L /
    b)`` blocks of ``b = min(block, L)`` frames; the weighted length ``k * b`` is not trimmed to ``L``).  The draws are a counter-based
    function of ``(seed, replicate, stratum or video, draw)`` (``include/vecvad_hip.h``): they do not depend on the scores, and
    replicates ``1..R`` in one call equal ``1..k`` and ``k+1..R`` in two."""
    if not torch.cuda.is_available():
        raise _lib.VecVadHipError('auc_counts needs a GPU; vec_vad_amd has no CPU path')
    dev = scores.device if torch.is_tensor(scores) and scores.is_cuda else torch.device('cuda', torch.cuda.current_device())
    t = auc_tables_device(auc_tables(scores, labels, video_idx, groups, strata), dev)
    return auc_counts_device(t, unit, block, seed, r0, R).cpu().numpy()


def auc_statistic(counts):
    """The statistic of one replicate from its ``[G, 3]`` counts, in float64 on the host: the mean (``math.fsum``) over the valid groups
    -- ``P > 0 and N > 0`` -- of ``float(U2) / (2.0 * float(P) * float(N))``; a group with one class only is skipped, a replicate
    without a valid group is invalid: ``(nan, 0)``.  Returns ``(statistic, valid groups)``."""
    aucs = [float(int(u2)) / (2.0 * float(int(p)) * float(int(q))) for u2, p, q in np.asarray(counts).reshape(-1, 3) if p > 0 and q > 0]
    return (math.fsum(aucs) / len(aucs), len(aucs)) if aucs else (float('nan'), 0)


def auc_interval(replicates, confidence, what='auc_bootstrap'):
    """The percentile interval of ``[R]`` replicate statistics (NaN = invalid): with ``a`` the ascending valid ones and ``M`` their number,
    ``k = ((100 - confidence) * (M - 1)) // 200``, ``lo = a[k]``, ``hi = a[M - 1 - k]``.  When more than 5 % of the replicates are invalid
    (``n_invalid * 20 > R``) or none is valid the interval is NaN, and in the first case a warning names the count.  Returns ``(lo, hi,
    n_invalid)``."""
    reps = np.asarray(replicates, np.float64).reshape(-1)
    a = np.sort(reps[~np.isnan(reps)])
    n_invalid = int(reps.size - a.size)
    if n_invalid * 20 > reps.size:
        import warnings
        warnings.warn('%s: %d of %d replicates are invalid (more than 5 %%): no interval is given' % (what, n_invalid, reps.size))
        return float('nan'), float('nan'), n_invalid
    if a.size == 0:
        return float('nan'), float('nan'), n_invalid
    k = ((100 - int(confidence)) * (a.size - 1)) // 200
    return float(a[k]), float(a[a.size - 1 - k]), n_invalid


def auc_bootstrap(scores, labels, video_idx, scene_idx=None, replicates=1000, unit='block', block=25, seed=0, confidence=95):
    """Micro and macro AUROC of a score vector with bootstrap percentile intervals (``[mi355x] auc_statistics``).  Returns ``{'micro':
    entry, 'macro': entry}``.  micro: one group -- or, with ``scene_idx`` (``[n]`` integers), one group per scene, the reference's
    per-scene mean, with the scenes as the strata of the video bootstrap; macro: one group per video, the mean of the per-video AUROCs.
    An entry holds ``auc`` (the full-sample statistic, ``auc_statistic``), ``replicates`` (float64 ``[R]``, NaN where a replicate has no
    valid group), ``lo`` / ``hi`` / ``n_invalid`` (``auc_interval``), ``n_groups_valid`` (groups of the full sample with both classes)
    and the settings ``n_replicates``, ``unit``, ``block``, ``seed``, ``confidence``.  ``replicates = 0``: the statistics alone.  The
    pair counts of every replicate come from the GPU as integers (``auc_counts``); the statistic is formed here in float64.  A group
    with one class only -- a video without an anomalous frame, say -- is skipped in the mean, in the full sample and in every
    replicate on its own.  ``block = 25`` is an untuned pick and no claim of coverage is made for it."""
    st = auc_settings(replicates, unit, block, seed, confidence)
    if not torch.cuda.is_available():
        raise _lib.VecVadHipError('auc_bootstrap needs a GPU; vec_vad_amd has no CPU path')
    dev = scores.device if torch.is_tensor(scores) and scores.is_cuda else torch.device('cuda', torch.cuda.current_device())
    scores = np.asarray(scores.cpu() if torch.is_tensor(scores) else scores, np.float64).reshape(-1)
    starts, _ = _runs('auc_bootstrap: video_idx', video_idx, scores.size)
    video = np.repeat(np.arange(starts.size - 1), np.diff(starts))
    out, work = {}, None
    for name, groups in (('micro', scene_idx), ('macro', video)):
        t = auc_tables_device(auc_tables(scores, labels, video, groups, scene_idx), dev)
        full = auc_counts_device(t, 'none', 1, 0, 1, 1).cpu().numpy()[0]
        auc, n_valid = auc_statistic(full)
        reps = np.zeros(0, np.float64)
        if st['n_replicates']:
            work = torch.empty(min(AUC_WORK_BYTES, max(8, int(_lib.lib().vv_auc_boot_work(t['n'], t['V'], st['n_replicates'],
                                                                                         AUC_UNITS[st['unit']])))),
                               dtype=torch.uint8, device=dev) if work is None else work
            counts = auc_counts_device(t, st['unit'], st['block'], st['seed'], 1, st['n_replicates'], work=work).cpu().numpy()
            reps = np.array([auc_statistic(c)[0] for c in counts], np.float64)
        lo, hi, n_invalid = auc_interval(reps, st['confidence'], 'auc_bootstrap (%s)' % name) if reps.size else (float('nan'), float('nan'), 0)
        out[name] = dict(auc=auc, replicates=reps, lo=lo, hi=hi, n_invalid=n_invalid, n_groups_valid=n_valid, **st)
    return out


def auc_paired(boot_a, boot_b):
    """The paired comparison ``a - b`` of two ``auc_bootstrap`` results (or of two of their entries) made with the same seed and settings:
    the draws do not depend on the scores, so replicate ``r`` of both saw the same resample.  Per entry: ``diff`` (``a.auc - b.auc``),
    ``replicates`` (the per-replicate differences, NaN where either side is invalid), ``lo`` / ``hi`` / ``n_invalid`` by the rule of
    ``auc_interval`` on the differences, and ``frac_le0``: the share of the replicates valid on both sides whose difference is ``<= 0``
    (NaN without one).  That share is reported as it is; it is not a p-value."""
    if 'micro' in boot_a or 'micro' in boot_b:
        return {k: auc_paired(boot_a[k], boot_b[k]) for k in ('micro', 'macro')}
    keys = ('n_replicates', 'unit', 'block', 'seed', 'confidence')
    if any(boot_a[k] != boot_b[k] for k in keys) or len(boot_a['replicates']) != len(boot_b['replicates']):
        raise ValueError('auc_paired: the two results were made with different settings: %s against %s' % (
            {k: boot_a[k] for k in keys}, {k: boot_b[k] for k in keys}))
    d = np.asarray(boot_a['replicates'], np.float64) - np.asarray(boot_b['replicates'], np.float64)
    lo, hi, n_invalid = auc_interval(d, boot_a['confidence'], 'auc_paired') if d.size else (float('nan'), float('nan'), 0)
    ok = d[~np.isnan(d)]
    return dict(diff=float(boot_a['auc']) - float(boot_b['auc']), replicates=d, lo=lo, hi=hi, n_invalid=n_invalid,
                frac_le0=float((ok <= 0).sum()) / ok.size if ok.size else float('nan'))


def auc_flatten(result, prefix=''):
    """``{'micro': entry, 'macro': entry}`` -> one flat dict of arrays with ``micro_`` / ``macro_`` prefixed keys, for ``np.savez``."""
    return {'%s%s_%s' % (prefix, name, k): np.asarray(v) for name in ('micro', 'macro') for k, v in result[name].items()}


def roc_auc(scores, labels):
    """Frame-level ROC-AUC of CUDA float64 ``scores`` against boolean ``labels`` (tie-aware; nan when a class is empty)."""
    if not scores.is_cuda:
        raise _lib.VecVadHipError('roc_auc needs device-resident scores; vec_vad_amd has no CPU path')
    dev = scores.device
    scores = scores.to(torch.float64).contiguous().view(-1)
    labels = (labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels)))
    labels = (labels.to(dev) != 0).to(torch.uint8).contiguous().view(-1)
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().vv_roc_auc_counts(scores.data_ptr(), labels.data_ptr(), scores.numel(), out.data_ptr(),
                                           torch.cuda.current_stream(dev).cuda_stream), 'vv_roc_auc_counts')
    c2, p, n = (int(v) for v in out.cpu())
    return float('nan') if p == 0 or n == 0 else c2 / (2.0 * p * n)
