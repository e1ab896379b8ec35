"""GPU tests of the motion foreground stage: ``vv_motion_mask`` and ``vv_mask_boxes`` (vec_vad_amd/motion.py), the
``fore_det.get_mt_bboxes`` drop-in and the chunked ``foreground.load_bboxes('obj_det_with_motion')`` against the numpy
restatement (tests/motion_boxes_restatement.py).  Every comparison is exact -- masks, boxes, their order and their counts:
each step is integer arithmetic."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_boxes_restatement as MR  # noqa: E402

pytestmark = pytest.mark.gpu
TILE_H, TILE_W = 16, 64          # LDS tile of the kernels (vv_motion.hip)


def _scene(rng, F, H, W, C, noise):
    """F frames: a static texture, rectangles that move a few pixels per frame, and sensor noise of the given amplitude"""
    base = rng.integers(40, 120, (H, W, 1), dtype=np.uint8).repeat(C, axis=2) // 2
    fr = np.empty((F, H, W, C), np.uint8)
    rects = [(rng.integers(0, H - 40), rng.integers(0, W - 60), rng.integers(8, 40), rng.integers(8, 60),
              rng.integers(-7, 8), rng.integers(-7, 8), rng.integers(100, 256, C)) for _ in range(6)]
    for t in range(F):
        img = base.astype(np.int64) + rng.integers(0, noise + 1, (H, W, C))
        for (y, x, h, w, vy, vx, col) in rects:
            yy, xx = int(np.clip(y + vy * t, 0, H - 1)), int(np.clip(x + vx * t, 0, W - 1))
            img[yy:yy + h, xx:xx + w] = col
        fr[t] = np.clip(img, 0, 255)
    return fr


def _windows(F, N):
    """three-frame windows of consecutive frames, repeated frames at both borders as border_mode='hard' produces them"""
    win = [[max(i - 1, 0), i, min(i + 1, F - 1)] for i in range(F)]
    win += [[F - 1, F - 1, F - 1], [2, 0, 5]]                                  # a still window and an unordered one
    return [win[i % len(win)] for i in range(N)]


def _ap_lists(rng, N, H, W, many_in=None):
    out = []
    for i in range(N):
        k = (0, 1, 4)[i % 3]
        b = []
        for _ in range(k):
            x1, y1 = rng.uniform(0, W - 10), rng.uniform(0, H - 10)
            b.append([x1, y1, x1 + rng.uniform(5, 120), y1 + rng.uniform(5, 90)])
        if i % 3 == 2:
            b[0] = [W - 30.5, H - 20.5, W + 25.0, H + 40.0]                     # hangs over the right and bottom edges
            b[1] = [0.0, 0.0, 0.9, 0.9]
        if i == many_in:                                                        # more boxes on one tile than the kernel keeps in LDS
            b += [[3.0 * j, 2.0 + j % 5, 3.0 * j + 1.5, 4.0 + j % 5] for j in range(70)]
        out.append(np.array(b, np.float32).reshape(-1, 4))
    return out


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('hw', [(240, 360), (360, 640), (480, 856)])
def test_motion_mask_equals_restatement(hw, C):
    import torch
    from vec_vad_amd.motion import motion_mask
    H, W = hw
    rng = np.random.default_rng(H + C)
    F = 8
    scene = _scene(rng, F, H, W, C, noise=14)
    noise = rng.integers(0, 256, (F, H, W, C), dtype=np.uint8)
    for frames, ksize, thr, N in ((scene, 3, 18, 16), (scene, 5, 15, 5), (scene, 5, 18, 1), (noise, 5, 15, 3), (noise, 3, 18, 1)):
        win = _windows(F, N)
        ap = _ap_lists(rng, N, H, W, many_in=1 if N > 1 else None)
        got = motion_mask(torch.from_numpy(frames).cuda(), win, ksize, thr, ap, extend=2).cpu().numpy()
        assert got.shape == (N, H, W) and got.dtype == np.uint8
        for n in range(N):
            want = MR.motion_mask(frames[win[n]], ksize, thr, ap[n], extend=2)
            assert np.array_equal(got[n], want), (hw, C, ksize, thr, n, int((got[n] != want).sum()))
        if frames is scene:
            assert 0 < (got == 255).mean() < 0.5                                # a real mask, neither empty nor saturated
    # no appearance boxes at all, and a frame size that is not a multiple of 4 (byte-wise loads and stores)
    odd = _scene(rng, 4, 50, 77, C, noise=30)
    got = motion_mask(torch.from_numpy(odd).cuda(), _windows(4, 4), 5, 15, None).cpu().numpy()
    for n, w in enumerate(_windows(4, 4)):
        assert np.array_equal(got[n], MR.motion_mask(odd[w], 5, 15))


def _ring(H, W, cy, cx, r0, r1):
    y, x = np.mgrid[:H, :W]
    d = np.maximum(abs(y - cy), abs(x - cx))
    return (d >= r0) & (d <= r1)


def _spiral(H, W):
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    while True:
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
                break
            dy, dx = dx, -dy
        else:
            return m
        y, x = ny, nx
        m[y, x] = True


def _mask_set(H, W, seed):
    rng = np.random.default_rng(seed)
    m = {d: rng.random((H, W)) < d for d in (0.05, 0.3, 0.5)}
    m['spiral'] = _spiral(H, W)
    comb = np.zeros((H, W), bool)
    comb[3:H - 3, 1::2] = True                                                  # teeth one pixel apart ...
    comb[H - 3, :] = True                                                       # ... joined by a spine
    m['comb'] = comb
    m['checker'] = np.indices((H, W)).sum(axis=0) % 2 == 1                       # one huge 8-connected component
    rings = np.zeros((H, W), bool)
    for r in range(4, min(H, W) // 2, 9):
        rings |= _ring(H, W, H // 2, W // 2, r, r + 3)
    m['rings'] = rings
    nested = np.zeros((H, W), bool)                                             # a grid of rings, each with a blob inside
    for cy in range(20, H - 20, 40):
        for cx in range(20, W - 20, 40):
            nested |= _ring(H, W, cy, cx, 12, 15) | _ring(H, W, cy, cx, 0, 6)
    m['nested'] = nested
    m['empty'] = np.zeros((H, W), bool)
    m['full'] = np.ones((H, W), bool)
    return m


def _check_boxes(masks, area_thr, extend, cap):
    import torch
    from vec_vad_amd.motion import mask_boxes
    names = list(masks)
    stack = np.stack([masks[k] for k in names]).astype(np.uint8) * np.uint8(255)
    stack[0][stack[0] != 0] = 1                                                 # any non-zero value is foreground
    dev = torch.from_numpy(stack).cuda()
    count, boxes = mask_boxes(dev, area_thr, extend, cap)
    count2, boxes2 = mask_boxes(dev, area_thr, extend, cap)
    assert torch.equal(count, count2) and torch.equal(boxes, boxes2)            # bit-identical from run to run
    count, boxes = count.cpu().numpy(), boxes.cpu().numpy()
    comps = {}
    for i, k in enumerate(names):
        want = MR.mask_boxes(stack[i], area_thr, extend)
        assert count[i] == len(want), (k, int(count[i]), len(want))
        assert np.array_equal(boxes[i, :count[i]], want.reshape(-1, 4)), k
        comps[k] = MR.label_components(stack[i])
    return dict(zip(names, count)), comps


def test_mask_boxes_equals_restatement_on_given_masks():
    H, W = 240, 360
    masks = _mask_set(H, W, 3)
    counts, comps = _check_boxes(masks, 0, 0, 8192)                             # every external component is a box
    # what this input set has to contain (checked with the restatement)
    assert max(sum(1 for c in v if not c[5]) for v in comps.values()) >= 10      # enclosed components
    assert any(c[3] > TILE_W and c[4] > TILE_H for v in comps.values() for c in v)       # a component over several LDS tiles
    assert max(counts.values()) > 200
    assert counts['checker'] == 1 and counts['full'] == 1 and counts['empty'] == 0 and counts['spiral'] == 1
    assert counts['nested'] == sum(1 for c in comps['nested'] if c[5]) == len(comps['nested']) // 2
    _check_boxes(masks, 8 * 8, 2, 8192)                                         # the reference's filter and extension
    _check_boxes({k: masks[k] for k in (0.3, 'rings', 'nested')}, 10 * 10, 2, 1024)


def test_mask_boxes_full_size_and_odd_size():
    big = _mask_set(480, 856, 5)
    _check_boxes({k: big[k] for k in (0.3, 'rings', 'spiral')}, 8 * 8, 2, 4096)
    odd = _mask_set(101, 131, 9)                                                # W % 4 != 0, partial tiles
    _check_boxes(odd, 0, 0, 4096)
    _check_boxes({'one': np.ones((1, 1), bool), 'dot': np.zeros((1, 1), bool)}, 0, 0, 4)


def test_mask_boxes_capacity_is_reported_not_truncated():
    import torch
    from vec_vad_amd import _lib
    from vec_vad_amd.motion import mask_boxes
    m = np.zeros((64, 96), np.uint8)
    m[::4, ::4] = 255                                                           # 16 x 24 = 384 isolated pixels
    dev = torch.from_numpy(m[None]).cuda()
    count, boxes = mask_boxes(dev, 0, 0, cap=384)
    assert int(count[0]) == 384
    with pytest.raises(_lib.VecVadHipError, match='384'):
        mask_boxes(dev, 0, 0, cap=383)


# ---- drop-in and the chunked dataset pass ---------------------------------------------------------------------------------------
def _moving_ped2_tree(rng, n_train=(5, 4)):
    """raw_datasets/ + optical_flow/ laid out like UCSDped2 (240x360 grey .tif, [h,w,2] flow .npy) with objects that move"""
    from PIL import Image
    H, W = 240, 360
    videos = []
    for v, n in enumerate(n_train, start=1):
        name = 'Train%03d' % v
        os.makedirs(os.path.join('raw_datasets', 'UCSDped2', 'Train', name))
        os.makedirs(os.path.join('optical_flow', 'UCSDped2', 'Train', name))
        frames = _scene(rng, n, H, W, 1, noise=10)[:, :, :, 0]
        for k in range(n):
            Image.fromarray(frames[k]).save(os.path.join('raw_datasets', 'UCSDped2', 'Train', name, '%03d.tif' % (k + 1)))
            np.save(os.path.join('optical_flow', 'UCSDped2', 'Train', name, '%03d.npy' % (k + 1)),
                    (rng.standard_normal((H, W, 2)) * 2).astype(np.float32))
        videos.append(frames)
    return videos


def test_get_mt_bboxes_and_chunked_load_bboxes(tmp_path, monkeypatch):
    import foreground as FG
    import train as T
    import vad_datasets as V
    from fore_det.obj_det_with_motion import get_mt_bboxes
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(11)
    videos = _moving_ped2_tree(rng)
    cfg = open(os.path.join(ROOT, 'config.cfg')).read()
    cfg = cfg.replace('train_bbox_saved = True', 'train_bbox_saved = False').replace('epochs = 10', 'epochs = 1')
    cfg = cfg.replace('motion_frames_per_launch = 16', 'motion_frames_per_launch = 4')  # chunks end inside videos and at their borders
    open('config.cfg', 'w').write(cfg)
    c = T.read_config('config.cfg')
    assert c['mode_fg'] == 'obj_det_with_motion' and c['cp'].getint('mi355x', 'motion_frames_per_launch') == 4

    flat = [np.repeat(f[:, :, None], 3, axis=2) for vid in videos for f in vid]      # decoded frames are 3-channel BGR
    fvi = [v for v, vid in enumerate(videos, start=1) for _ in vid]
    batches = [np.stack([flat[i] for i in V.context_range(k, 'hard', 1, len(flat), fvi)]) for k in range(len(flat))]
    assert np.array_equal(batches[0][0], batches[0][1]) and np.array_equal(batches[4][1], batches[4][2])     # video borders repeat

    def expected(ap_all):
        out = []
        for k, b in enumerate(batches):
            mt = MR.get_mt_bboxes(b, ap_all[k], 'UCSDped2')
            out.append(np.concatenate((ap_all[k], mt), axis=0) if mt.shape[0] > 0 else ap_all[k])
        return out

    path = os.path.join('raw_datasets', 'UCSDped2', 'bboxes_train_obj_det_with_motion.npy')
    # ---- no detector output at all: motion boxes only
    none = [np.zeros((0, 4), np.float32) for _ in flat]
    logs = []
    got = FG.load_bboxes(c, 'train', log=logs.append)
    assert any('motion boxes only' in s for s in logs) and os.path.exists(path)
    want = expected(none)
    assert len(got) == len(want) == 9 and sum(len(w) for w in want) >= 9
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), k
    # the drop-in, frame by frame
    for k in (0, 3, 4, 8):
        one = get_mt_bboxes(flat[k].copy(), batches[k], none[k], 'UCSDped2')
        mt = MR.get_mt_bboxes(batches[k], none[k], 'UCSDped2')
        assert one.dtype == mt.dtype == np.int64 and np.array_equal(one, mt)
    # ---- with the file the reference's 'obj_det' mode saves: those boxes first, and no motion box on top of them
    os.remove(path)
    ap_all = []
    for k in range(len(flat)):
        b = want[k][:k % 3].astype(np.float32) + np.float32(0.25)                # cover some of the moving objects
        ap_all.append(np.concatenate([b, [[300.5, 200.5, 380.0, 260.0]]]).astype(np.float32))
    arr = np.empty(len(ap_all), dtype=object)
    for k, b in enumerate(ap_all):
        arr[k] = b
    np.save(os.path.join('raw_datasets', 'UCSDped2', 'bboxes_train_obj_det.npy'), arr, allow_pickle=True)
    got = FG.load_bboxes(c, 'train', log=lambda *a: None)
    want2 = expected(ap_all)
    assert any(len(w2) != len(a) for w2, a in zip(want2, ap_all))               # motion boxes were added somewhere
    for k, (g, w) in enumerate(zip(got, want2)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), k
        assert np.array_equal(g[:len(ap_all[k])], ap_all[k])
    # ---- cube extraction runs on the written file
    FG.extract_train(c, 'cuda', log=lambda *a: None)
    raw = np.load('data/raw2flow/UCSDped2_foreground_train_obj_det_with_motion-raw.npy', allow_pickle=True)
    assert raw.shape == (1, 1) and raw[0][0].shape[1:] == (5, 32, 32, 3) and len(raw[0][0]) > 0
