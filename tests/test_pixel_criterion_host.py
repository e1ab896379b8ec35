"""Host side of the pixel-level criterion ([mi355x] pixel_criterion): the rectangles the kernels are handed, the equivalence of
the threshold sweep that defines the criterion with the one number per frame the GPU computes, the config keys, the ShanghaiTech
refusal before any GPU work and the order ``merge_groups`` leaves the cubes in.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 37, 53


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


def test_box_rects_are_python_slices_and_agree_with_box_paints():
    from vec_vad_amd import scoring
    import test as S
    boxes = np.array([
        [-3.5, -2.5, 10.2, 8.0],          # hangs over the top-left corner: ceil gives -3 / -2, which WRAP as slice starts
        [40.1, 30.3, 70.0, 50.0],         # hangs over the bottom-right corner: clipped
        [-60.0, -50.0, 5.0, 6.0],         # starts further out than the frame is large: clipped to 0
        [-10.2, -8.7, -2.1, -1.0],        # wholly negative ceilings: a rectangle counted from the far edges
        [3.2, 3.2, 3.9, 9.0],             # ceil(x1) == ceil(x2): no column
        [5.0, 7.2, 9.0, 7.9],             # ceil(y1) == ceil(y2): no row
        [60.0, 40.0, 80.0, 60.0],         # past the frame on both axes
        [20.0, 10.0, 10.0, 30.0],         # x2 < x1
        [0.0, 0.0, 53.0, 37.0],           # the whole frame
        [0.0, 35.5, 0.5, 37.5],           # the last row, first column
        [-0.5, -0.5, 1.0, 1.0],           # ceil(-0.5) = 0: no wrap
    ])
    rects = scoring.box_rects(boxes, H, W)
    assert rects.dtype == np.int32 and rects.shape == (len(boxes), 4)
    paints = scoring.box_paints(boxes, H, W)
    for m, b in enumerate(boxes):
        ys = slice(int(math.ceil(b[1])), int(math.ceil(b[3]))).indices(H)
        xs = slice(int(math.ceil(b[0])), int(math.ceil(b[2]))).indices(W)
        assert rects[m].tolist() == [ys[0], ys[1], xs[0], xs[1]], m
        assert bool(paints[m]) == (rects[m, 1] > rects[m, 0] and rects[m, 3] > rects[m, 2]), m
        # and that IS the region test.paint_frame writes
        want = S.paint_frame([1.0], [b], H, W) == 1.0
        got = np.zeros((H, W), bool)
        got[rects[m, 0]:max(rects[m, 0], rects[m, 1]), rects[m, 2]:max(rects[m, 2], rects[m, 3])] = True
        assert np.array_equal(want, got), m
    assert rects[0].tolist() == [35, 8, 50, 11] and not paints[0]       # wrapped start behind the stop: empty
    assert rects[3].tolist() == [29, 36, 43, 51] and paints[3]
    assert paints.tolist() == [0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1]
    assert scoring.box_rects(np.zeros((0, 4)), H, W).shape == (0, 4)


def _pixel_score(mask, gt, pct):
    g = int((gt > 0).sum())
    if g == 0:
        return mask.max()
    k = (g * pct + 99) // 100
    return np.sort(mask[gt > 0])[::-1][k - 1]


def test_threshold_sweep_equals_the_kth_largest_value():
    """The criterion as defined (a sweep over thresholds) against the one number per frame: for every frame and every threshold,
    'detected' / 'false positive' is exactly ``s_pix >= t``."""
    import test as S
    rng = np.random.default_rng(17)
    frames = []
    for i in range(24):
        n = (0, 1, 5, 9)[(i + i // 8) % 4]               # every kind of ground truth meets three box counts
        x0, y0 = rng.uniform(-6, W - 4, n), rng.uniform(-6, H - 4, n)
        boxes = np.stack([x0, y0, x0 + rng.uniform(0.5, 30, n), y0 + rng.uniform(0.5, 25, n)], 1).reshape(n, 4)
        scores = np.round(rng.standard_normal(n), 1)                       # tied scores
        if n == 9:
            scores[3] = scores[7] = scores.max()                           # tied top scores
            scores[1] = S.BIG
        gt = np.zeros((H, W), np.uint8)
        kind = i % 8
        if kind == 1:
            gt[5, 7] = 255                                                 # |G| = 1 -> k = 1
        elif kind == 2:
            gt[10, 10:15] = 1                                              # |G| = 5 -> k = 2 at 40 %
        elif kind == 3:
            gt[20, 30:36] = 255                                            # |G| = 6 -> k = 3 at 40 %
        elif kind == 5:
            gt[8:30, 12:44] = 1                                            # a rectangle partly under boxes
        elif kind == 6:
            gt[:] = 255                                                    # the whole frame
        elif kind == 7:
            gt[rng.random((H, W)) < 0.1] = 7
        frames.append((S.paint_frame(scores, boxes, H, W), gt))
    sizes = sorted({int((g > 0).sum()) for _, g in frames})
    assert sizes[:4] == [0, 1, 5, 6] and sizes[-1] == H * W
    assert (5 * 40 + 99) // 100 == 2 and (6 * 40 + 99) // 100 == 3 and (1 * 40 + 99) // 100 == 1
    thresholds = np.unique(np.concatenate([m.ravel() for m, _ in frames]))
    thresholds = np.concatenate([thresholds, thresholds + 0.05, [-S.BIG - 1.0, S.BIG + 1.0]])
    assert len(thresholds) > 20
    some_detected = some_missed = 0
    for pct in (40, 100, 1):
        for f, (mask, gt) in enumerate(frames):
            sp = _pixel_score(mask, gt, pct)
            g = gt > 0
            for t in thresholds:
                if g.any():
                    flagged = 100 * int((mask[g] >= t).sum()) >= pct * int(g.sum())
                    some_detected += flagged and t > -S.BIG
                    some_missed += not flagged
                else:
                    flagged = bool((mask >= t).any())
                assert flagged == bool(sp >= t), (pct, f, t, sp)
    assert some_detected and some_missed


def test_the_three_keys_parse_with_defaults_and_a_bad_percent_is_rejected(tmp_path):
    import train as T
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    for key in ('pixel_criterion', 'pixel_overlap_percent', 'device_score_masks'):
        assert c['cp'].has_option('mi355x', key), key
    assert c['pixel_criterion'] is False and c['device_score_masks'] is False and c['pixel_overlap_percent'] == 40
    p = tmp_path / 'config.cfg'
    p.write_text(_config_text().replace('pixel_criterion = False', 'pixel_criterion = True')
                 .replace('device_score_masks = False', 'device_score_masks = True')
                 .replace('pixel_overlap_percent = 40', 'pixel_overlap_percent = 100'))
    c = T.read_config(str(p))
    assert c['pixel_criterion'] is True and c['device_score_masks'] is True and c['pixel_overlap_percent'] == 100
    # a file from before the keys
    keys = ('pixel_criterion', 'pixel_overlap_percent', 'device_score_masks')
    p.write_text('\n'.join(l for l in _config_text().splitlines() if not l.startswith(keys)) + '\n')
    c = T.read_config(str(p))
    assert not any(c['cp'].has_option('mi355x', k) for k in keys)
    assert c['pixel_criterion'] is False and c['device_score_masks'] is False and c['pixel_overlap_percent'] == 40
    for bad in ('0', '101', '-5', '40.5'):
        p.write_text(_config_text().replace('pixel_overlap_percent = 40', 'pixel_overlap_percent = ' + bad))
        with pytest.raises(ValueError):
            T.read_config(str(p))


def test_shanghaitech_is_refused_before_the_gpu_is_touched(tmp_path, monkeypatch):
    import foreground as FG
    import test as S
    import train as T

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')

    monkeypatch.setattr(torch.cuda, 'set_device', touched)
    monkeypatch.setattr(torch.cuda, 'current_device', touched)
    monkeypatch.setattr(FG, 'load_bboxes', touched)
    monkeypatch.chdir(tmp_path)
    cfg = _config_text().replace('dataset_name = UCSDped2', 'dataset_name = ShanghaiTech')
    for saved in ('False', 'True'):
        open('config.cfg', 'w').write(cfg.replace('pixel_criterion = False', 'pixel_criterion = True')
                                      .replace('scores_saved = False', 'scores_saved = ' + saved))
        c = T.read_config('config.cfg')
        assert c['dataset_name'] == 'ShanghaiTech' and c['pixel_criterion']
        with pytest.raises(ValueError, match='ShanghaiTech') as e:
            S.main('config.cfg')
        assert '\n' not in str(e.value)                      # a one-line reason
        with pytest.raises(ValueError, match='ShanghaiTech'):
            FG.gt_source(c)
    assert os.listdir('.') == ['config.cfg']                 # nothing written either


def test_a_tree_without_pixel_ground_truth_is_refused(tmp_path, monkeypatch):
    import foreground as FG
    import train as T
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    os.makedirs('raw_datasets/UCSDped2/Test/Test001')
    for k in range(2):
        Image.fromarray(np.zeros((240, 360), np.uint8)).save('raw_datasets/UCSDped2/Test/Test001/%03d.tif' % (k + 1))
    open('config.cfg', 'w').write(_config_text())
    c = T.read_config('config.cfg')
    with pytest.raises(ValueError, match='ground truth') as e:
        FG.gt_source(c)
    assert '\n' not in str(e.value)
    os.makedirs('raw_datasets/UCSDped2/Test/Test001_gt')
    for k in range(2):
        g = np.zeros((240, 360) if k == 0 else (120, 360), np.uint8)
        g[3, 4] = 255
        Image.fromarray(g).save('raw_datasets/UCSDped2/Test/Test001_gt/%03d.bmp' % (k + 1))
    gt = FG.gt_source(c)
    assert len(gt) == 2
    g0 = gt(0)
    assert g0.dtype == np.uint8 and g0.shape == (240, 360) and g0.flags['C_CONTIGUOUS'] and g0[3, 4] != 0 and (g0 != 0).sum() == 1
    with pytest.raises(ValueError, match='240x360') as e:
        gt(1)                                                # a mask of the wrong size
    assert '\n' not in str(e.value)


def test_merge_groups_orders_by_frame_then_group_then_list():
    from vec_vad_amd import scoring
    # 4 frames.  Group A: frames 0 (2 cubes), 2 (1), 3 (2); group B: empty; group C: frames 1 (1), 2 (3) -- frame 1 in C only
    off_a = np.array([0, 2, 2, 3, 5], np.int32)
    off_b = np.zeros(5, np.int32)
    off_c = np.array([0, 0, 1, 4, 4], np.int32)

    def group(off, tag):
        n = int(off[-1])
        return off, torch.arange(n, dtype=torch.float64) + tag, (torch.arange(n * 4, dtype=torch.int32).reshape(n, 4) + int(tag))

    groups = [group(off_a, 100.0), group(off_b, 200.0), group(off_c, 300.0)]
    off, sc, rc = scoring.merge_groups(groups)
    assert off.dtype == np.int32 and off.tolist() == [0, 2, 3, 7, 9]
    assert sc.dtype == torch.float64 and sc.tolist() == [100, 101, 300, 102, 301, 302, 303, 103, 104]
    assert rc.dtype == torch.int32 and rc.shape == (9, 4)
    assert rc[:, 0].tolist() == [100, 104, 300, 108, 304, 308, 312, 112, 116]
    # a window of frames: offsets keep pointing into the whole group
    off2, sc2, _ = scoring.merge_groups([(o[1:4], s, r) for o, s, r in groups], n_frames=2)
    assert off2.tolist() == [0, 1, 5] and sc2.tolist() == [300, 102, 301, 302, 303]
    # one group alone is returned in its own order; no group at all needs the number of frames
    off3, sc3, _ = scoring.merge_groups(groups[2:])
    assert off3.tolist() == off_c.tolist() and sc3.tolist() == [300, 301, 302, 303]
    off4, sc4, rc4 = scoring.merge_groups([], n_frames=3)
    assert off4.tolist() == [0, 0, 0, 0] and sc4.numel() == 0 and tuple(rc4.shape) == (0, 4)
    with pytest.raises(ValueError):
        scoring.merge_groups([])
    with pytest.raises(ValueError):
        scoring.merge_groups([(off_a, groups[0][1], groups[0][2]), (off_c[:-1], groups[2][1], groups[2][2])])
    assert scoring.PIXEL_MAX_BOXES == 2048
