"""Pictures of what the test stage computes (``[mi355x] render``): optical flow in the Middlebury colour coding and frames with the
score mask, the scored boxes and the ground-truth contour drawn over them.  Both run on the GPU (vv_flow_color, vv_render_overlay;
include/vecvad_hip.h states the arithmetic) and return CUDA uint8 ``[n,h,w,3]`` tensors in RGB order; there is no CPU path.
``tests/render_restatement.py`` restates both in plain numpy."""
import numpy as np
import torch

from . import _lib

UNPAINTED = -100000.0      # VV_RENDER_UNPAINTED: the background of a painted mask


def colormap():
    """The default colour table of ``overlay``: uint8 ``[256,3]`` RGB, dark blue -> cyan -> yellow -> red, by an integer formula
    (no matplotlib).  For level ``i`` in 0..255 with ``s, t = divmod(i, 64)``::

        s = 0   (0, 4 t, 128 + 2 t)        dark blue (0, 0, 128) -> just short of cyan
        s = 1   (4 t, 255, 255 - 4 t)      cyan (0, 255, 255) -> just short of yellow
        s = 2   (255, 255 - 2 t, 0)        yellow (255, 255, 0) -> orange
        s = 3   (255, 127 - 2 t, 0)        orange -> red (255, 1, 0)

    Every level has its own colour, so a picture can be read back into levels."""
    lut = np.zeros((256, 3), np.uint8)
    for i in range(256):
        s, t = divmod(i, 64)
        lut[i] = ((0, 4 * t, 128 + 2 * t), (4 * t, 255, 255 - 4 * t), (255, 255 - 2 * t, 0), (255, 127 - 2 * t, 0))[s]
    return lut


def _need(name, t, dtype, what):
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise ValueError('%s must be a %s tensor, got %s' % (name, what, '%s %s' % (t.dtype, tuple(t.shape)) if torch.is_tensor(t)
                                                              else type(t).__name__))


def flow_color(flow, maxrad=0.0):
    """Flow fields as Middlebury colour images: flow CUDA float32 ``[n,h,w,2]`` (or one field ``[h,w,2]``) -> CUDA uint8 ``[n,h,w,3]``
    (``[h,w,3]``), RGB, with the semantics of the reference's ``flow_to_image``: direction picks the hue off the 55-entry wheel, the
    radius the saturation.  ``maxrad <= 0``: every image is normalised by its own largest radius, as the reference does; ``maxrad >
    0``: that radius for every image, so that the frames of a video share one scale.  A pixel with ``|u|`` or ``|v|`` above 1e7 is
    unknown: black, and left out of the maximum; a NaN pixel is treated alike (the reference turns the whole image black).  float32
    arithmetic: a byte differs from the float64 reference by at most 1, except where the normalised radius is within rounding of 1."""
    _need('flow_color: flow', flow, torch.float32, 'float32 [n,h,w,2]')
    if not flow.is_cuda:
        raise _lib.VecVadHipError('flow_color needs a device-resident flow; vec_vad_amd has no CPU path')
    single = flow.dim() == 3
    if flow.dim() not in (3, 4) or flow.shape[-1] != 2:
        raise ValueError('flow_color: flow must be a float32 [n,h,w,2] tensor, got %s' % (tuple(flow.shape),))
    maxrad = float(maxrad)
    if maxrad != maxrad:
        raise ValueError('flow_color: maxrad must be a number, got nan')
    fl = (flow[None] if single else flow).contiguous()
    n, h, w, _ = fl.shape
    nb = int(_lib.lib().vv_flow_color_work(n, h, w))
    if nb < 0:
        raise ValueError('flow_color: images of %d x %d pixels, fewer than 2^31 - 4096 are supported' % (h, w))
    dev = fl.device
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    work = torch.empty(max(4, nb), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().vv_flow_color(fl.data_ptr(), n, h, w, maxrad, out.data_ptr(), work.data_ptr(),
                                       torch.cuda.current_stream(dev).cuda_stream), 'vv_flow_color')
    return out[0] if single else out


def overlay(frames, mask, rects, scores, frame_off, lo, hi, alpha, gt=None, lut=None, bgr=True):
    """Frames with their score masks drawn over them: CUDA uint8 ``[n,h,w,3]``, RGB.

    frames: CUDA uint8 ``[n,h,w]`` / ``[n,h,w,1]`` (grey) or ``[n,h,w,3]`` (``bgr``: stored B, G, R as the decoders of this project
    return them; False: R, G, B).  mask: CUDA float64 ``[n,h,w]`` (``scoring.paint_masks`` / ``smooth_masks``), ``-100000.0`` =
    unpainted.  rects int32 ``[m,4]`` (``scoring.box_rects`` rows), scores float64 ``[m]``, frame_off ``[n+1]`` CSR offsets of every
    frame's boxes -- ``m`` may be 0.  A value ``v`` has the level 0 for ``v <= lo``, 255 for ``v >= hi`` and ``floor((v - lo) / (hi -
    lo) * 255)`` between; ``lut`` (uint8 ``[256,3]`` RGB; None: ``colormap()``) turns a level into a colour.  Per pixel, later rules win:
    the frame; a painted pixel is blended with the colour of its mask value, ``(base * (256 - alpha) + colour * alpha + 128) >> 8``
    (``alpha`` 0..256); a pixel on the one-pixel outline of a box gets the colour of the largest score among those boxes, opaque;
    with ``gt`` (uint8 ``[n,h,w]``) a ground-truth pixel with a 4-neighbour that is zero or outside the frame is white.  Exact."""
    _need('overlay: frames', frames, torch.uint8, 'uint8 [n,h,w] or [n,h,w,c]')
    _need('overlay: mask', mask, torch.float64, 'float64 [n,h,w]')
    if not frames.is_cuda:
        raise _lib.VecVadHipError('overlay needs device-resident frames; vec_vad_amd has no CPU path')
    dev = frames.device
    if frames.dim() == 3:
        frames = frames[..., None]
    if frames.dim() != 4 or frames.shape[-1] not in (1, 3):
        raise ValueError('overlay: frames must be a uint8 [n,h,w] or [n,h,w,c] tensor with c in (1, 3), got %s' % (tuple(frames.shape),))
    n, h, w, c = frames.shape
    if tuple(mask.shape) != (n, h, w) or mask.device != dev:
        raise ValueError('overlay: mask must be a float64 [%d,%d,%d] tensor on %s, got %s on %s' % (n, h, w, dev, tuple(mask.shape),
                                                                                                   mask.device))
    if gt is not None:
        _need('overlay: gt', gt, torch.uint8, 'uint8 [n,h,w]')
        if tuple(gt.shape) != (n, h, w) or gt.device != dev:
            raise ValueError('overlay: gt must be a uint8 [%d,%d,%d] tensor on %s, got %s on %s' % (n, h, w, dev, tuple(gt.shape),
                                                                                                   gt.device))
        gt = gt.contiguous()
    if h * w > 2 ** 31 - 1025:
        raise ValueError('overlay: frames of %d x %d pixels, fewer than 2^31 - 1024 are supported' % (h, w))
    lo, hi = float(lo), float(hi)
    if not hi > lo:
        raise ValueError('overlay: the range must have lo < hi, got %r, %r' % (lo, hi))
    if int(alpha) != alpha or not 0 <= alpha <= 256:
        raise ValueError('overlay: alpha must be an integer in 0..256, got %r' % (alpha,))
    lut = colormap() if lut is None else (lut.cpu().numpy() if torch.is_tensor(lut) else np.asarray(lut))
    if lut.dtype != np.uint8 or lut.shape != (256, 3):
        raise ValueError('overlay: lut must be a uint8 [256,3] table, got %s %s' % (lut.dtype, lut.shape))
    scores = (scores if torch.is_tensor(scores) else torch.from_numpy(np.asarray(scores, np.float64))).to(device=dev, dtype=torch.float64)
    scores = scores.contiguous().view(-1)
    m = scores.numel()
    rects = (rects if torch.is_tensor(rects) else torch.from_numpy(np.asarray(rects, np.int32).reshape(-1, 4))).to(device=dev, dtype=torch.int32)
    if rects.numel() != 4 * m:
        raise ValueError('overlay: %d rectangle entries for %d scores' % (rects.numel(), m))
    rects = rects.contiguous().view(-1, 4)
    off = (frame_off.cpu().numpy() if torch.is_tensor(frame_off) else np.asarray(frame_off)).astype(np.int64).reshape(-1)
    if off.size != n + 1 or (np.diff(off) < 0).any() or off[0] < 0 or off[-1] > m:
        raise ValueError('overlay: frame_off must be %d non-decreasing offsets into the %d boxes given' % (n + 1, m))
    frames, mask = frames.contiguous(), mask.contiguous()
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    off_d = torch.from_numpy(off.astype(np.int32)).to(dev)
    lut_d = torch.tensor(lut).to(dev)        # a copy: the caller's table may be read-only
    _lib.check(_lib.lib().vv_render_overlay(
        frames.data_ptr(), c, 1 if bgr else 0, mask.data_ptr(), gt.data_ptr() if gt is not None else None,
        rects.data_ptr() if m else None, scores.data_ptr() if m else None, off_d.data_ptr(), m, lut_d.data_ptr(), lo, hi, int(alpha), n, h, w,
        out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), 'vv_render_overlay')
    return out
