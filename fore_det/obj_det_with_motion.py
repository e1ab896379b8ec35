"""Drop-in surface of the reference's fore_det/obj_det_with_motion.py without the detector: ``get_mt_bboxes`` runs on the GPU
(vec_vad_amd/motion.py: ``vv_motion_mask`` + ``vv_mask_boxes``), ``del_cover_bboxes`` is host numpy for users who bring their
own detector output.  ``get_ap_bboxes`` (mmdet cascade R-CNN) is not part of this build."""
import numpy as np

COVER_THR = {'UCSDped2': 0.6, 'avenue': 0.6, 'ShanghaiTech': 0.65}


def del_cover_bboxes(bboxes, dataset_name):
    """Drop every box that a LARGER box covers by more than the dataset's ratio of the smaller box's own area
    (obj_det_with_motion.py:94-141).  Areas and overlaps count pixels inclusively (``+ 1``); the kept boxes come out in ascending
    order of area, as the reference returns them."""
    if dataset_name not in COVER_THR:
        raise NotImplementedError
    bboxes = np.asarray(bboxes)
    assert bboxes.ndim == 2 and bboxes.shape[1] == 4
    x1, y1, x2, y2 = bboxes[:, 0], bboxes[:, 1], bboxes[:, 2], bboxes[:, 3]
    areas = (y2 - y1 + 1) * (x2 - x1 + 1)
    order = areas.argsort()
    keep = []
    for k, i in enumerate(order):
        rest = order[k + 1:]
        w = np.maximum(0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1)
        h = np.maximum(0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1)
        if not (w * h / areas[i] > COVER_THR[dataset_name]).any():
            keep.append(i)
    return bboxes[keep]


def get_mt_bboxes(cur_img, img_batch, ap_bboxes, dataset_name, verbose=False):
    """Motion based bounding boxes of one frame (obj_det_with_motion.py:144-223).  ``img_batch``: uint8 ``(3, h, w, c)``, the frame
    and its two neighbours; ``ap_bboxes``: ``(n, 4)`` appearance boxes whose extended rectangles are excluded.  Returns an int64
    ``(k, 4)`` array, ``np.array([])`` when there is none.  ``cur_img`` is only drawn on by the reference and is left alone here;
    there are no windows to show, so ``verbose=True`` raises."""
    if verbose:
        raise NotImplementedError('verbose=True opens cv2 windows in the reference; this build has none')
    import torch
    from vec_vad_amd.motion import motion_boxes
    img_batch = np.asarray(img_batch)
    if img_batch.ndim != 4 or img_batch.shape[0] != 3 or img_batch.dtype != np.uint8:
        raise ValueError('img_batch must be uint8 (3, h, w, c): the frame with one neighbour on each side')
    frames = torch.from_numpy(np.ascontiguousarray(img_batch)).to('cuda')
    return motion_boxes(frames, [[0, 1, 2]], [np.asarray(ap_bboxes).reshape(-1, 4)], dataset_name)[0]
