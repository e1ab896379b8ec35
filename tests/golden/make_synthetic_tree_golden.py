"""Golden values for the synthetic UCSDped2 tree of the timing tools (``tools/time_direct_*.py``): ``synthetic_tree.npz``.

Run ONCE, at the commit before ``tools/synthetic_tree.py`` existed, where the builders were ``time_direct_test.make_tree`` and
``time_direct_train.make_train_tree``; ``tests/test_synthetic_tree.py`` holds the shared builder to these values.  ``summarise`` is
what both sides apply to a tree: every file DECODED (the bytes of a .tif depend on the PIL build), one ``_util.digest`` row per frame,
flow field and ground-truth mask in path order, and the box arrays in full.

    python tests/golden/make_synthetic_tree_golden.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TREE_ARGS = dict(test_frames=6, train_videos=(3, 2), boxes=3)       # small counts in the shape of the tools' calls


def summarise(root='.'):
    """{name: array} of the tree under ``root``: digests of the decoded files per kind, the relative paths, the boxes."""
    from PIL import Image
    sys.path.insert(0, os.path.dirname(HERE))
    from _util import digest
    kinds = {'.tif': 'frames', '.bmp': 'gt', '.npy': 'flow'}
    rows, paths, out = {}, {}, {}
    for d, dirs, files in os.walk(root):
        dirs.sort()
        for f in sorted(files):
            p, ext = os.path.join(d, f), os.path.splitext(f)[1]
            if f.startswith('bboxes_'):
                boxes = np.load(p, allow_pickle=True)
                out[f[:-4] + '_counts'] = np.array([len(b) for b in boxes], np.int64)
                out[f[:-4]] = np.concatenate([np.asarray(b, np.float64).reshape(-1, 5) for b in boxes])
                continue
            a = np.load(p) if ext == '.npy' else np.asarray(Image.open(p))
            rows.setdefault(kinds[ext], []).append(np.concatenate([digest(a.astype(np.float64)), a.shape, [a.dtype.itemsize]]))
            paths.setdefault(kinds[ext], []).append(os.path.relpath(p, root))
    for k in rows:
        out[k] = np.array(rows[k])
        out[k + '_paths'] = np.array(paths[k])
    return out


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), 'tools'))
    from time_direct_test import make_tree
    from time_direct_train import make_train_tree
    res = {}
    for tag, build in (('test_tool', lambda: make_tree(TREE_ARGS['test_frames'], TREE_ARGS['boxes'])),
                       ('train_tool', lambda: make_train_tree(TREE_ARGS['train_videos'], TREE_ARGS['boxes']))):
        with tempfile.TemporaryDirectory() as work:
            os.chdir(work)
            build()
            res.update({'%s/%s' % (tag, k): v for k, v in summarise('.').items()})
            os.chdir(HERE)
    np.savez_compressed(os.path.join(HERE, 'synthetic_tree.npz'), **res)
    print({k: v.shape for k, v in res.items()})
