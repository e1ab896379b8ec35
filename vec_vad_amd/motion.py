"""Motion-based foreground boxes on the GPU (reference fore_det/obj_det_with_motion.py:144-223 ``get_mt_bboxes``): the
Gaussian blur / frame difference / threshold / box erase of N three-frame windows in ONE launch of ``vv_motion_mask``, and
cv2.findContours(RETR_EXTERNAL) + boundingRect + the reference's filter as connected-component labelling in ``vv_mask_boxes``.
All of it is integer arithmetic; results are bit-identical from run to run.

There is no CPU fallback: without libvecvad_hip.so / a gfx950 device these functions raise.
"""
import numpy as np
import torch

from . import _lib

# get_mt_bboxes:157-173
CONSTANTS = {'UCSDped2': dict(area_thr=10 * 10, binary_thr=18, extend=2, ksize=3),
             'avenue': dict(area_thr=40 * 40, binary_thr=18, extend=2, ksize=5),
             'ShanghaiTech': dict(area_thr=8 * 8, binary_thr=15, extend=2, ksize=5)}
DEFAULT_CAP = 1024


def _ap_table(ap_boxes_per_window, n):
    """per-window box lists -> int32 [M,5] rows (window, x1, y1, x2, y2), truncated like ``bbox.astype(np.int32)``."""
    if ap_boxes_per_window is None:
        return np.zeros((0, 5), np.int32)
    if len(ap_boxes_per_window) != n:
        raise ValueError('%d box lists for %d windows' % (len(ap_boxes_per_window), n))
    rows = []
    for i, b in enumerate(ap_boxes_per_window):
        b = np.asarray(b)
        if b.size == 0:
            continue
        b = b.reshape(-1, b.shape[-1])[:, :4].astype(np.int32)
        if (b[:, 2:] < 0).any():
            raise ValueError('appearance boxes with x2 < 0 or y2 < 0 are outside the documented domain (window %d)' % i)
        rows.append(np.concatenate([np.full((len(b), 1), i, np.int32), b], axis=1))
    return np.concatenate(rows, axis=0) if rows else np.zeros((0, 5), np.int32)


def motion_mask(frames, win, ksize, binary_thr, ap_boxes_per_window=None, extend=2):
    """frames: CUDA uint8 ``[F,H,W,C]`` (C = 1 or 3, contiguous); win: int ``[N,3]`` frame indices of each window;
    ap_boxes_per_window: N arrays ``[m,>=4]`` (x1, y1, x2, y2, ...) or None.  Returns the CUDA uint8 mask ``[N,H,W]`` (0 / 255)."""
    if not (torch.is_tensor(frames) and frames.is_cuda):
        raise _lib.VecVadHipError('motion_mask needs the frames in HBM (CUDA tensor); vec_vad_amd has no CPU path')
    if frames.dtype != torch.uint8 or frames.dim() != 4 or not frames.is_contiguous():
        raise ValueError('frames must be a contiguous uint8 [F,H,W,C] tensor')
    F, H, W, C = frames.shape
    win = np.ascontiguousarray(np.asarray(win, dtype=np.int64).reshape(-1, 3))
    if win.size and (win.min() < 0 or win.max() >= F):
        raise ValueError('window frame index outside [0, %d)' % F)
    n = win.shape[0]
    ap = _ap_table(ap_boxes_per_window, n)
    dev = frames.device
    mask = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    if n:
        win_d = torch.from_numpy(win.astype(np.int32)).to(dev)
        ap_d = torch.from_numpy(ap).to(dev) if len(ap) else None
        _lib.check(_lib.lib().vv_motion_mask(frames.data_ptr(), F, H, W, C, win_d.data_ptr(), n, int(ksize), int(binary_thr),
                                            ap_d.data_ptr() if ap_d is not None else None, len(ap), int(extend),
                                            mask.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), 'vv_motion_mask')
    return mask


def mask_boxes(mask, area_thr, extend=2, cap=DEFAULT_CAP):
    """mask: CUDA uint8 ``[N,H,W]`` (non-zero = foreground).  Returns (count int32 ``[N]``, boxes int32 ``[N,cap,4]``), both CUDA;
    rows ``boxes[n, :count[n]]`` are valid, in descending order of each component's first pixel.  Raises when a window has more
    than ``cap`` boxes."""
    if not (torch.is_tensor(mask) and mask.is_cuda):
        raise _lib.VecVadHipError('mask_boxes needs the mask in HBM (CUDA tensor); vec_vad_amd has no CPU path')
    if mask.dtype != torch.uint8 or mask.dim() != 3 or not mask.is_contiguous():
        raise ValueError('mask must be a contiguous uint8 [N,H,W] tensor')
    n, H, W = mask.shape
    dev = mask.device
    count = torch.zeros((n,), dtype=torch.int32, device=dev)
    boxes = torch.zeros((n, int(cap), 4), dtype=torch.int32, device=dev)
    if n:
        l = _lib.lib()
        ws = torch.empty((l.vv_mask_boxes_workspace_bytes(n, H, W),), dtype=torch.uint8, device=dev)
        _lib.check(l.vv_mask_boxes(mask.data_ptr(), n, H, W, int(area_thr), int(extend), int(cap), ws.data_ptr(), ws.numel(),
                                   count.data_ptr(), boxes.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), 'vv_mask_boxes')
        most = int(count.max())
        if most > cap:
            raise _lib.VecVadHipError('vv_mask_boxes: a window has %d boxes, capacity is %d (pass a larger cap)' % (most, cap))
    return count, boxes


def motion_boxes(frames, win, ap_boxes_per_window, dataset_name, cap=DEFAULT_CAP):
    """``get_mt_bboxes`` of every window with the per-dataset constants of the reference: a list of int64 ``[k,4]`` arrays
    (x1, y1, x2, y2), shape ``(0,)`` where a window has no box (``np.array([])`` in the reference)."""
    if dataset_name not in CONSTANTS:
        raise NotImplementedError
    k = CONSTANTS[dataset_name]
    mask = motion_mask(frames, win, k['ksize'], k['binary_thr'], ap_boxes_per_window, k['extend'])
    count, boxes = mask_boxes(mask, k['area_thr'], k['extend'], cap)
    count, boxes = count.cpu().numpy(), boxes.cpu().numpy()
    return [boxes[i, :count[i]].astype(np.int64) if count[i] else np.array([]) for i in range(len(count))]
