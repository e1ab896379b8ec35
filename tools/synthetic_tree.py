"""What the ``time_direct_*.py`` tools share: the synthetic UCSDped2-shaped tree, the size of a directory, a wall-clock meter."""
import os
import time

import numpy as np

SUBS = {'train': 'Train', 'test': 'Test'}


def make_tree(videos, boxes_per_frame, seed=11, flow=True):
    """raw_datasets/ (+ optical_flow/ with ``flow``) + bbox files like UCSDped2 in the working directory: 240x360 grey .tif frames,
    [h,w,2] flow .npy, random boxes of which the first of every frame lies in a still corner and fails the motion test.  ``videos``:
    ``{'train' | 'test': frames per video}``, built in that order; a test video gets its ``_gt`` masks."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    H, W = 240, 360
    for mode, counts in videos.items():
        sub = SUBS[mode]
        all_boxes = []
        for v, n in enumerate(counts, start=1):
            name = '%s%03d' % (sub, v)
            os.makedirs(os.path.join('raw_datasets', 'UCSDped2', sub, name))
            if flow:
                os.makedirs(os.path.join('optical_flow', 'UCSDped2', sub, name))
            if mode == 'test':
                os.makedirs(os.path.join('raw_datasets', 'UCSDped2', sub, name + '_gt'))
            for k in range(n):
                g = rng.integers(0, 256, (H, W), dtype=np.uint8)
                Image.fromarray(g).save(os.path.join('raw_datasets', 'UCSDped2', sub, name, '%04d.tif' % (k + 1)))
                if flow:
                    fl = (rng.standard_normal((H, W, 2)) * 2).astype(np.float32)
                    fl[:60, :90] = 0                                   # a still corner: boxes there fail the motion test
                    np.save(os.path.join('optical_flow', 'UCSDped2', sub, name, '%04d.npy' % (k + 1)), fl)
                if mode == 'test':
                    gt = np.zeros((H, W), np.uint8)
                    if k % 2:
                        gt[100:120, 100:130] = 255
                    Image.fromarray(gt).save(os.path.join('raw_datasets', 'UCSDped2', sub, name + '_gt', '%04d.bmp' % (k + 1)))
                bb = []
                for m in range(boxes_per_frame):
                    x0, y0 = rng.uniform(95, W - 70), rng.uniform(65, H - 70)
                    bb.append([x0, y0, x0 + rng.uniform(8, 64), y0 + rng.uniform(8, 64), rng.random()])
                bb[0] = [5.0, 4.0, 40.0, 50.0, 0.9]                # inside the still corner -> dropped
                all_boxes.append(np.array(bb).reshape(-1, 5))
        arr = np.empty(len(all_boxes), dtype=object)
        for i, b in enumerate(all_boxes):
            arr[i] = b
        np.save(os.path.join('raw_datasets', 'UCSDped2', 'bboxes_%s_obj_det_with_motion.npy' % mode), arr, allow_pickle=True)


def tree_bytes(path):
    return sum(os.path.getsize(os.path.join(d, f)) for d, _, files in os.walk(path) for f in files) if os.path.isdir(path) else 0


def metered(meter, fn, key, sync=None):
    """``fn`` with the wall time of every call added to ``meter[key]``; ``sync`` (e.g. ``torch.cuda.synchronize``) runs before the
    clock is read."""
    def run(*a, **k):
        t0 = time.perf_counter()
        try:
            return fn(*a, **k)
        finally:
            if sync:
                sync()
            meter[key] += time.perf_counter() - t0
    return run
