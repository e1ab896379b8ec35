"""Fixed grid of patches (reference fore_det/simple_patch.py): the 'simple_patch' foreground mode needs no detector."""
import numpy as np


def get_patch_loc(h, w, h_num, w_num):
    """``h_num * w_num`` boxes (x_min, y_min, x_max, y_max), float64 ``[h_num*w_num, 4]``, x-major: patch origins are spaced over
    ``[0, h-1)`` x ``[0, w-1)``, every patch is ``h/h_num`` x ``w/w_num`` and is clipped to ``h-1`` / ``w-1``."""
    ys = np.linspace(0, h - 1, h_num, endpoint=False)
    xs = np.linspace(0, w - 1, w_num, endpoint=False)
    x_min, y_min = (g.ravel() for g in np.meshgrid(xs, ys, indexing='ij'))
    return np.stack([x_min, y_min, np.minimum(x_min + w / w_num, w - 1), np.minimum(y_min + h / h_num, h - 1)], axis=1)
