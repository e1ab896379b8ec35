"""Cube extraction on the GPU: crop + cv2-style bilinear resize of every box of a frame stack
in ONE launch of ``vv_crop_resize`` (reference vad_datasets.py:70-93 ``get_foreground`` does one ``cv2.resize`` call per
box per frame on the host), and the whole-frame resizes of calc_optical_flow.py:46-59,82.
``cube_cut`` / ``cube_energy`` (``vv_cube_cut`` / ``vv_cube_energy``) do the boxes of many consecutive frames per launch, every box
with its own frame window, for test.py's direct path (foreground.extract_device); ``flow_pairs_prep`` / ``flow_resize_back``
(``vv_flow_pairs_prep`` / ``vv_flow_resize_back``) are the two whole-frame resizes around FlowNet2 for many frame pairs per launch
(calc_optical_flow.chunk_flows).

There is no CPU fallback: without libvecvad_hip.so / a gfx950 device these functions raise.
"""
import math

import numpy as np
import torch

from . import _lib


def boxes_to_crops(bboxes, H, W):
    """``img[..., ceil(y1):ceil(y2), ceil(x1):ceil(x2)]`` of vad_datasets.py:74-76 as int32 ``[n,4]`` (x_min, y_min, x_max,
    y_max) after numpy's clipping of slice ends to the array.  An empty crop raises, as ``cv2.resize`` does on it."""
    crops = np.zeros((len(bboxes), 4), np.int32)
    for i, b in enumerate(bboxes):
        x0, x1 = int(math.ceil(b[0])), int(math.ceil(b[2]))
        y0, y1 = int(math.ceil(b[1])), int(math.ceil(b[3]))
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
        if x1 <= x0 or y1 <= y0:
            raise ValueError('box %d (%s) selects an empty crop of the %dx%d frame (cv2.resize asserts !ssize.empty())'
                             % (i, list(map(float, b[:4])), H, W))
        crops[i] = (x0, y0, x1, y1)
    return crops


def crop_resize(frames, crops, out_h, out_w):
    """frames: CUDA tensor ``[T,H,W,C]`` uint8 or float32 (contiguous); crops: int32 ``[n,4]`` (numpy or CUDA tensor).
    Returns a CUDA tensor ``[n,T,out_h,out_w,C]`` of the same dtype."""
    if not frames.is_cuda:
        raise _lib.VecVadHipError('crop_resize needs the frames in HBM (CUDA tensor); vec_vad_amd has no CPU path')
    if frames.dtype not in (torch.uint8, torch.float32):
        raise TypeError('crop_resize handles uint8 and float32 frames (the two dtypes the reference resizes), got %s'
                        % frames.dtype)
    if frames.dim() != 4 or not frames.is_contiguous():
        raise ValueError('frames must be a contiguous [T,H,W,C] tensor')
    T, H, W, C = frames.shape
    if not torch.is_tensor(crops):
        crops = torch.from_numpy(np.ascontiguousarray(crops, dtype=np.int32))
    crops = crops.to(device=frames.device, dtype=torch.int32).contiguous()
    n = crops.shape[0]
    out = torch.empty((n, T, out_h, out_w, C), dtype=frames.dtype, device=frames.device)
    if n:
        _lib.check(_lib.lib().vv_crop_resize(frames.data_ptr(), int(frames.dtype == torch.float32), T, H, W, C,
                                            crops.data_ptr(), n, out_h, out_w, out.data_ptr(),
                                            torch.cuda.current_stream(frames.device).cuda_stream), 'vv_crop_resize')
    return out


def resize(img, dsize, device='cuda'):
    """``cv2.resize(img, dsize)`` (default INTER_LINEAR) for an HxW or HxWxC uint8 / float32 numpy image; ``dsize=(w,h)``."""
    img = np.asarray(img)
    squeeze = img.ndim == 2
    a = img[:, :, None] if squeeze else img
    H, W, _ = a.shape
    fr = torch.from_numpy(np.ascontiguousarray(a)).to(device)[None]
    out = crop_resize(fr, np.array([[0, 0, W, H]], np.int32), int(dsize[1]), int(dsize[0]))[0, 0].cpu().numpy()
    return out[:, :, 0] if squeeze else out


def get_foreground(img, bboxes, patch_size, device='cuda'):
    """Drop-in for reference vad_datasets.py:70-93: ``img`` ``[C,H,W]`` or ``[T,C,H,W]`` (numpy) -> ``[n,C,P,P]`` or
    ``[n,T,C,P,P]`` numpy patches.  One upload, one launch, one download for all boxes and frames."""
    img = np.asarray(img)
    single = img.ndim == 3
    fr = img[None] if single else img
    fr = torch.from_numpy(np.ascontiguousarray(np.transpose(fr, [0, 2, 3, 1]))).to(device)
    if len(bboxes) == 0:
        return np.array([])                           # np.array(list()) in the reference
    out = foreground_cubes(fr, bboxes, patch_size)    # [n,T,P,P,C]
    out = out.permute(0, 1, 4, 2, 3).contiguous().cpu().numpy()
    return out[:, 0] if single else out


def foreground_cubes(frames, bboxes, patch_size):
    """Device-resident variant: frames CUDA ``[T,H,W,C]`` -> cubes CUDA ``[n,T,P,P,C]`` (the layout of the saved
    ``*_foreground_*.npy`` cube files and of ``CubeStore``), no host round trip."""
    crops = boxes_to_crops(bboxes, frames.shape[1], frames.shape[2])
    return crop_resize(frames, crops, patch_size, patch_size)


def chunk_windows(ranges):
    """Bookkeeping of one chunk of consecutive frames (pure, no GPU): ``ranges`` = the ``context_range`` of each frame of the
    chunk (global frame indices; a border mode repeats a frame inside a window).  Returns (``used``: every frame some window
    names, once, ascending -- what the chunk decodes and uploads; ``win``: int32 ``[len(ranges), T]``, the windows as indices
    into ``used``)."""
    used = sorted({f for r in ranges for f in r})
    local = {f: k for k, f in enumerate(used)}
    win = np.array([[local[f] for f in r] for r in ranges], np.int32).reshape(len(ranges), -1)
    return used, win


def check_tables(crops, win, F, H, W, slot=None, slots=None):
    """The tables of a ``cube_cut`` / ``cube_energy`` launch against the chunk they index (pure, no GPU; numpy int32 arrays): every
    crop non-empty and inside the ``H x W`` frame, every window index in ``[0, F)``, one window row per crop, and with ``slot`` one
    entry per crop, each below ``slots``, no slot >= 0 named twice.  Raises ValueError on the first rule a table breaks: the
    kernels would skip such a box or clamp such an index without a word, and a skipped box leaves its cube of the store unwritten."""
    crops, win = np.asarray(crops).reshape(-1, 4), np.asarray(win)
    n = crops.shape[0]
    if win.ndim != 2 or win.shape[0] != n or win.shape[1] < 1:
        raise ValueError('win must be [n,T] with one row per crop and T >= 1, got %s for %d crops' % (tuple(win.shape), n))
    x0, y0, x1, y1 = crops[:, 0], crops[:, 1], crops[:, 2], crops[:, 3]
    bad = np.nonzero(~((0 <= x0) & (x0 < x1) & (x1 <= W) & (0 <= y0) & (y0 < y1) & (y1 <= H)))[0]
    if len(bad):
        raise ValueError('crop %d (%s) is empty or does not lie inside the %dx%d frame' % (bad[0], crops[bad[0]].tolist(), H, W))
    bad = np.nonzero(((win < 0) | (win >= F)).any(1))[0]
    if len(bad):
        raise ValueError('window %d (%s) names a frame outside the chunk of %d frames' % (bad[0], win[bad[0]].tolist(), F))
    if slot is not None:
        slot = np.asarray(slot).reshape(-1)
        if slot.shape[0] != n:
            raise ValueError('slot must have one entry per crop, got %d for %d crops' % (slot.shape[0], n))
        bad = np.nonzero(slot >= slots)[0]
        if len(bad):
            raise ValueError('box %d names slot %d of a store of %d cubes' % (bad[0], slot[bad[0]], slots))
        named = slot[slot >= 0]
        if len(np.unique(named)) != len(named):
            raise ValueError('two boxes name the same slot')


def _chunk_args(frames, crops, win, slot=None, slots=None):
    """Checks the tables on the host and returns them as int32 device tensors next to the frames.  A table that is already a
    device tensor is read back for the check (a sync), so hand numpy arrays over where that matters."""
    if not frames.is_cuda:
        raise _lib.VecVadHipError('the frames of a chunk must be in HBM (CUDA tensor); vec_vad_amd has no CPU path')
    if frames.dim() != 4 or not frames.is_contiguous():
        raise ValueError('frames must be a contiguous [F,H,W,C] tensor')

    def host(a):
        return a.cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a, dtype=np.int32)

    def dv(a):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
        return t.to(device=frames.device, dtype=torch.int32).contiguous()

    check_tables(host(crops), host(win), frames.shape[0], frames.shape[1], frames.shape[2],
                 None if slot is None else host(slot), slots)
    return dv(crops).reshape(-1, 4), dv(win), None if slot is None else dv(slot).reshape(-1)


def cube_cut(frames, crops, win, slot, patch_size, out):
    """``vv_cube_cut``: the boxes of many frames in one launch.  frames: CUDA ``[F,H,W,C]`` uint8 | float32, the decoded frames
    of a chunk, each once; crops int32 ``[n,4]``; win int32 ``[n,T]`` = each box's context frames as indices into the chunk;
    slot int32 ``[n]`` = the cube of ``out`` (CUDA ``[slots,T,P,P,C]``, same dtype, contiguous) that the box fills, ``< 0`` =
    skip.  Every written value equals ``crop_resize(frames[win[i]], crops[i:i+1], P, P)`` bit for bit.  A table that breaks
    ``check_tables`` raises before anything is launched."""
    if out.dim() != 5:
        raise ValueError('out must be a [slots,T,P,P,C] tensor')
    crops, win, slot = _chunk_args(frames, crops, win, slot, out.shape[0])
    n, T = win.shape
    F, H, W, C = frames.shape
    P = int(patch_size)
    if frames.dtype not in (torch.uint8, torch.float32) or out.dtype != frames.dtype:
        raise TypeError('cube_cut handles uint8 and float32 frames and writes the same dtype, got %s -> %s' % (frames.dtype, out.dtype))
    if not out.is_contiguous() or out.device != frames.device or tuple(out.shape[1:]) != (T, P, P, C):
        raise ValueError('out must be a contiguous [slots,%d,%d,%d,%d] tensor next to the frames' % (T, P, P, C))
    if n:
        _lib.check(_lib.lib().vv_cube_cut(frames.data_ptr(), int(frames.dtype == torch.float32), F, H, W, C, crops.data_ptr(),
                                         win.data_ptr(), slot.data_ptr(), n, T, P, out.data_ptr(), out.shape[0],
                                         torch.cuda.current_stream(frames.device).cuda_stream), 'vv_cube_cut')
    return out


def cube_energy(frames, crops, win, patch_size, thr):
    """``vv_cube_energy``: the motion test of train.py:159-170 without writing a patch.  frames: CUDA float32 ``[F,H,W,C]`` flow
    fields of a chunk (C = 2); crops / win as for ``cube_cut``, checked in the same way.  Returns CUDA (energy float64 ``[n]`` =
    sum of squares of the resized patch, mean over the context frames; keep uint8 ``[n]`` = energy > thr)."""
    crops, win, _ = _chunk_args(frames, crops, win)
    if frames.dtype != torch.float32:
        raise TypeError('cube_energy works on float32 flow fields, got %s' % frames.dtype)
    n, T = win.shape
    F, H, W, C = frames.shape
    P = int(patch_size)
    if not 0 < P <= 1024 or T * P * P > 0x7fffffff:
        raise ValueError('cube_energy needs 0 < patch_size <= 1024 and T * patch_size^2 below 2^31, got T = %d, patch_size = %d' % (T, P))
    energy = torch.empty(n, dtype=torch.float64, device=frames.device)
    keep = torch.empty(n, dtype=torch.uint8, device=frames.device)
    if n:
        _lib.check(_lib.lib().vv_cube_energy(frames.data_ptr(), F, H, W, C, crops.data_ptr(), win.data_ptr(), n, T, P,
                                            float(thr), energy.data_ptr(), keep.data_ptr(),
                                            torch.cuda.current_stream(frames.device).cuda_stream), 'vv_cube_energy')
    return energy, keep


def _host_i32(a):
    return a.cpu().numpy().astype(np.int32) if torch.is_tensor(a) else np.ascontiguousarray(a, dtype=np.int32)


def flow_pairs_prep(frames, pairs, out_h, out_w, out=None):
    """``vv_flow_pairs_prep``: FlowNet2's input for many frame pairs in one launch.  frames: CUDA uint8 ``[F,H,W,C]`` (C = 1 | 3), the
    decoded frames of a chunk; pairs int32 ``[N,2]`` = (first, second) frame of each pair as indices into the chunk.  Returns (or
    fills ``out``, CUDA float32 ``[N,3,2,out_h,out_w]`` contiguous) ``out[n,c,k] = float(resize(frames[pairs[n,k]])[..., c])``, the
    values of ``crop_resize`` on the whole frame; a grey frame's plane is written three times.  A pair that names a frame outside
    the chunk raises before anything is launched (the kernel alone would clamp the index without a word)."""
    pairs_h = _host_i32(pairs)
    if pairs_h.ndim != 2 or pairs_h.shape[1] != 2:
        raise ValueError('pairs must be [N,2], got %s' % (tuple(pairs_h.shape),))
    if frames.dim() != 4:
        raise ValueError('frames must be a contiguous [F,H,W,C] tensor')
    F, H, W, C = frames.shape
    bad = np.nonzero(((pairs_h < 0) | (pairs_h >= F)).any(1))[0]
    if len(bad):
        raise ValueError('pair %d (%s) names a frame outside the chunk of %d frames' % (bad[0], pairs_h[bad[0]].tolist(), F))
    if not frames.is_cuda:
        raise _lib.VecVadHipError('the frames of a chunk must be in HBM (CUDA tensor); vec_vad_amd has no CPU path')
    if frames.dtype != torch.uint8 or not frames.is_contiguous() or C not in (1, 3):
        raise TypeError('flow_pairs_prep handles contiguous uint8 frames of 1 or 3 channels, got %s %s' % (frames.dtype, tuple(frames.shape)))
    N, oh, ow = pairs_h.shape[0], int(out_h), int(out_w)
    if out is None:
        out = torch.empty((N, 3, 2, oh, ow), dtype=torch.float32, device=frames.device)
    elif (out.dtype != torch.float32 or not out.is_contiguous() or out.device != frames.device
          or tuple(out.shape) != (N, 3, 2, oh, ow)):
        raise ValueError('out must be a contiguous float32 [%d,3,2,%d,%d] tensor next to the frames' % (N, oh, ow))
    if N:
        pairs_d = torch.from_numpy(pairs_h).to(frames.device)
        _lib.check(_lib.lib().vv_flow_pairs_prep(frames.data_ptr(), F, H, W, C, pairs_d.data_ptr(), N, oh, ow, out.data_ptr(),
                                                torch.cuda.current_stream(frames.device).cuda_stream), 'vv_flow_pairs_prep')
    return out


def flow_resize_back(flow, rows, H, W, out):
    """``vv_flow_resize_back``: FlowNet2's planar output back at frame size, vectors not rescaled.  flow: CUDA float32 ``[N,2,fh,fw]``
    contiguous; rows int32 ``[N]`` = the field of ``out`` (CUDA float32 ``[R,H,W,2]`` contiguous) that pair n fills, ``< 0`` = skip.
    Every written field equals ``crop_resize(flow[n].permute(1,2,0).contiguous()[None], whole, H, W)[0,0]`` bit for bit.  A row
    ``>= R``, or one named twice, raises before anything is launched."""
    rows_h = _host_i32(rows).reshape(-1)
    if flow.dim() != 4 or flow.shape[1] != 2 or rows_h.shape[0] != flow.shape[0]:
        raise ValueError('flow must be [N,2,fh,fw] with one row per pair, got %s for %d rows' % (tuple(flow.shape), rows_h.shape[0]))
    if out.dim() != 4 or tuple(out.shape[1:]) != (int(H), int(W), 2):
        raise ValueError('out must be a [R,%d,%d,2] tensor, got %s' % (H, W, tuple(out.shape)))
    bad = np.nonzero(rows_h >= out.shape[0])[0]
    if len(bad):
        raise ValueError('pair %d names row %d of an output of %d fields' % (bad[0], rows_h[bad[0]], out.shape[0]))
    named = rows_h[rows_h >= 0]
    if len(np.unique(named)) != len(named):
        raise ValueError('two pairs name the same row')
    if not flow.is_cuda:
        raise _lib.VecVadHipError('the flow must be in HBM (CUDA tensor); vec_vad_amd has no CPU path')
    if flow.dtype != torch.float32 or out.dtype != torch.float32:
        raise TypeError('flow_resize_back works on float32 fields, got %s -> %s' % (flow.dtype, out.dtype))
    if not flow.is_contiguous() or not out.is_contiguous() or out.device != flow.device:
        raise ValueError('flow and out must be contiguous tensors on one device')
    N, _, fh, fw = flow.shape
    if N:
        rows_d = torch.from_numpy(rows_h).to(flow.device)
        _lib.check(_lib.lib().vv_flow_resize_back(flow.data_ptr(), N, fh, fw, rows_d.data_ptr(), int(H), int(W), out.data_ptr(),
                                                 out.shape[0], torch.cuda.current_stream(flow.device).cuda_stream),
                   'vv_flow_resize_back')
    return out
