"""Detector-free part of the reference's ``fore_det`` package: the motion stage (``get_mt_bboxes``, on the GPU), the overlap
filter for detector output brought from elsewhere (``del_cover_bboxes``) and the fixed patch grid (``get_patch_loc``).  The mmdet
detector itself (``get_ap_bboxes``, ``inference.py``) is not part of this build."""
