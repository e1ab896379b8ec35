"""CPU tests of the motion foreground stage: the numpy restatement (tests/motion_boxes_restatement.py) against independent
scipy formulations and hand-computed answers, the host-side drop-ins (``get_patch_loc``, ``del_cover_bboxes``) and the
not-saved branch of ``foreground.load_bboxes`` that needs no GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_boxes_restatement as MR  # noqa: E402


# ---- blur ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ksize', [3, 5])
@pytest.mark.parametrize('shape', [(17, 23, 3), (40, 31, 1), (2, 9, 3), (9, 2, 1), (1, 7, 3), (3, 3, 3), (64, 5, 3)])
def test_blur_equals_float64_mirror_correlation_rounded_half_up(ksize, shape):
    """scipy's 'mirror' is BORDER_REFLECT_101 (also when the image is narrower than the kernel radius + 1)."""
    from scipy.ndimage import correlate1d
    rng = np.random.default_rng(ksize * 100 + shape[0])
    w = {3: np.array([1, 2, 1]) / 4.0, 5: np.array([1, 4, 6, 4, 1]) / 16.0}[ksize]
    for trial in range(4):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        if trial == 3:
            img[...] = rng.choice([0, 255], shape)                          # extreme values, exact .5 ties
        f = correlate1d(correlate1d(img.astype(np.float64), w, axis=0, mode='mirror'), w, axis=1, mode='mirror')
        want = np.floor(f + 0.5).astype(np.uint8)
        assert np.array_equal(MR.blur(img, ksize), want)


def test_blur_border_by_hand():
    img = np.zeros((5, 5, 1), np.uint8)
    img[0, 0] = 160
    # corner: reflect-101 mirrors about the edge pixel, which keeps weight 2 per axis and gains nothing from the zero neighbours
    assert MR.blur(img, 3)[0, 0, 0] == (2 * 2 * 160 + 8) >> 4
    assert MR.blur(img, 3)[0, 1, 0] == (2 * 1 * 160 + 8) >> 4 and MR.blur(img, 3)[1, 1, 0] == (160 + 8) >> 4
    assert MR.blur(img, 5)[0, 0, 0] == (6 * 6 * 160 + 128) >> 8 and MR.blur(img, 5)[2, 2, 0] == (160 + 128) >> 8


# ---- motion mask ----------------------------------------------------------------------------------------------------------
def _flat(v, shape=(12, 16, 3)):
    return np.full(shape, v, np.uint8)


def test_uint8_wrap_of_the_two_differences():
    """|0-200| + |200-0| = 400 -> 144 as uint8: still above the threshold; 128 + 128 wraps to 0 and vanishes."""
    m = MR.motion_mask(np.stack([_flat(0), _flat(200), _flat(0)]), 3, 18)
    assert (m == 255).all()
    m = MR.motion_mask(np.stack([_flat(0), _flat(128), _flat(0)]), 3, 18)
    assert (m == 0).all()
    m = MR.motion_mask(np.stack([_flat(0), _flat(9), _flat(0)]), 5, 18)          # 18 is not > 18
    assert (m == 0).all()
    f = _flat(0)
    f[:, :, 1] = 10                                                              # one channel above the threshold is enough
    assert (MR.motion_mask(np.stack([_flat(0), f, _flat(0)]), 5, 18) == 255).all()


def test_erase_rectangle_inclusive_far_edge_and_clipping():
    fr = np.stack([_flat(0, (20, 30, 1)), _flat(100, (20, 30, 1)), _flat(0, (20, 30, 1))])
    m = MR.motion_mask(fr, 3, 18, [[5.9, 4.2, 9.9, 8.7]], extend=2)              # truncated to 5, 4, 9, 8
    want = np.full((20, 30), 255, np.uint8)
    want[2:11, 3:12] = 0                                                         # rows 4-2 .. 8+2 and columns 5-2 .. 9+2, inclusive
    assert np.array_equal(m, want)
    m = MR.motion_mask(fr, 3, 18, [[25, 15, 40, 60], [0, 0, 0, 0]], extend=2)    # hangs over the right and bottom edges
    want = np.full((20, 30), 255, np.uint8)
    want[13:, 23:] = 0
    want[0:3, 0:3] = 0
    assert np.array_equal(m, want)


# ---- components -------------------------------------------------------------------------------------------------------------
def _scipy_components(mask):
    """(label = first pixel in raster order, x, y, w, h, external) by scipy: 8-connected foreground, externality by a flood
    fill of the padded background with 4-connectivity."""
    from scipy import ndimage
    fg = np.asarray(mask) != 0
    H, W = fg.shape
    lab, n = ndimage.label(fg, structure=np.ones((3, 3)))
    pad = np.zeros((H + 2, W + 2), bool)
    pad[1:-1, 1:-1] = fg
    blab, _ = ndimage.label(~pad)                                               # default structure: 4-connectivity
    outer = blab == blab[0, 0]
    near = np.zeros_like(outer)                                                 # pixels 4-adjacent to the outer background
    near[1:] |= outer[:-1]
    near[:-1] |= outer[1:]
    near[:, 1:] |= outer[:, :-1]
    near[:, :-1] |= outer[:, 1:]
    near = near[1:-1, 1:-1]
    out = []
    for k, sl in enumerate(ndimage.find_objects(lab), start=1):
        ys, xs = np.nonzero(lab == k)
        first = int((ys * W + xs).min())
        out.append((first, sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start,
                    bool(near[lab == k].any())))
    return sorted(out)


def _ring(n, r0, r1):
    y, x = np.mgrid[:n, :n]
    d = np.maximum(abs(y - n // 2), abs(x - n // 2))
    return ((d >= r0) & (d <= r1)).astype(np.uint8) * 255


def _spiral(n):
    """one-pixel wide square spiral walked inwards from the top-left corner, one background pixel between its laps"""
    m = np.zeros((n, n), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 255
    while True:
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
                break
            dy, dx = dx, -dy
        else:
            return m
        y, x = ny, nx
        m[y, x] = 255


@pytest.mark.parametrize('name', ['r05', 'r30', 'r50', 'rings', 'spiral', 'checker', 'comb', 'empty', 'full'])
def test_components_equal_scipy_label_and_flood_fill(name):
    rng = np.random.default_rng(7)
    if name[0] == 'r' and name[1:].isdigit():
        m = (rng.random((60, 90)) < int(name[1:]) / 100).astype(np.uint8)
    elif name == 'rings':
        m = _ring(61, 3, 5) | _ring(61, 9, 12) | _ring(61, 16, 16) | _ring(61, 22, 30) | _ring(61, 0, 0)
    elif name == 'spiral':
        m = _spiral(41)
    elif name == 'checker':
        m = (np.indices((33, 47)).sum(axis=0) % 2).astype(np.uint8)
    elif name == 'comb':
        m = np.zeros((30, 41), np.uint8)
        m[2:28, ::2] = 1
        m[28, :] = 1
    else:
        m = np.full((9, 13), 0 if name == 'empty' else 1, np.uint8)
    got = MR.label_components(m)
    want = _scipy_components(m)
    assert got == want
    if name == 'rings':
        assert sum(1 for c in got if not c[5]) >= 3                             # the nested rings and the centre dot
    if name == 'checker':
        assert len(got) == 1


# ---- known answers ----------------------------------------------------------------------------------------------------------
def test_ring_with_a_blob_inside_gives_one_box():
    m = np.zeros((60, 80), np.uint8)
    m[10:40, 20:60] = 1
    m[13:37, 23:57] = 0
    m[20:30, 30:45] = 1                                                          # enclosed: no external contour
    assert MR.mask_boxes(m, 100, 2).tolist() == [[18, 8, 62, 42]]


def test_two_blobs_touching_diagonally_are_one_component():
    m = np.zeros((60, 80), np.uint8)
    m[10:20, 10:20] = 1
    m[20:30, 20:30] = 1
    assert MR.mask_boxes(m, 100, 2).tolist() == [[8, 8, 32, 32]]
    m[20:30, 20:30] = 0
    m[21:31, 20:30] = 1                                                          # one row further: two components, descending order
    assert MR.mask_boxes(m, 100, 2).tolist() == [[18, 19, 32, 33], [8, 8, 22, 22]]


def test_line_dropped_by_aspect_and_small_blob_by_area():
    m = np.zeros((100, 120), np.uint8)
    m[10:13, 20:100] = 1                                                         # 3 x 80: w / h = 26.7
    m[50:54, 50:54] = 1                                                          # 4 x 4: (4+1)*(4+1) = 25 <= 100
    assert MR.mask_boxes(m, 100, 2).shape == (0,)
    assert MR.mask_boxes(m, 24, 2).tolist() == [[48, 48, 56, 56]]
    m[60:63, 20:50] = 1                                                          # 3 x 30: w / h = 10 is not < 10
    m[70:73, 20:49] = 1                                                          # 3 x 29 passes
    assert MR.mask_boxes(m, 100, 2).tolist() == [[18, 68, 51, 75]]


def test_blob_on_the_frame_edge_is_clipped():
    m = np.zeros((50, 70), np.uint8)
    m[0:12, 0:15] = 1
    m[40:50, 55:70] = 1
    assert MR.mask_boxes(m, 100, 2).tolist() == [[53, 38, 70, 50], [0, 0, 17, 14]]


def test_get_mt_bboxes_restatement_on_a_moving_square():
    fr = np.zeros((3, 60, 80, 3), np.uint8)
    for t in range(3):
        fr[t, 20:40, 10 + 12 * t:30 + 12 * t] = 200
    out = MR.get_mt_bboxes(fr, np.zeros((0, 4)), 'UCSDped2')
    assert out.dtype == np.int64 and out.shape[1] == 4 and len(out) >= 1
    assert out[:, 0].min() <= 10 and out[:, 2].max() >= 54
    assert MR.get_mt_bboxes(fr, np.array([[0., 0., 80., 60.]]), 'UCSDped2').shape == (0,)


# ---- host-side drop-ins -----------------------------------------------------------------------------------------------------
def test_get_patch_loc_equals_the_reference_golden():
    from fore_det.simple_patch import get_patch_loc
    from vad_datasets import frame_size
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'simple_patch_boxes.npz'))
    assert len(g.files) == 6
    for key in g.files:
        name, grid = key.split('_')
        h_num, w_num = (int(v) for v in grid.split('x'))
        got = get_patch_loc(frame_size[name][0], frame_size[name][1], h_num, w_num)
        assert got.dtype == g[key].dtype and np.array_equal(got, g[key]), key


def test_del_cover_bboxes_by_hand():
    from fore_det.obj_det_with_motion import del_cover_bboxes
    big = [0., 0., 99., 99.]                     # area 10000
    inside = [10., 10., 29., 29.]                # area 400, fully covered by big -> dropped
    half = [90., 0., 109., 9.]                   # area 200, 100 of it inside big: ratio 0.5 -> kept
    edge = [95., 50., 104., 59.]                 # area 100, columns 95..99 inside big: ratio 0.5 -> kept
    most = [93., 70., 102., 80.]                 # area 110, columns 93..99 inside: ratio 0.7 -> dropped at 0.6 and at 0.65
    sixty = [94., 80., 103., 84.]                # area 50, columns 94..99 inside: ratio 0.6 is not > 0.6 -> kept
    b = np.array([big, inside, half, edge, most, sixty])
    out = del_cover_bboxes(b, 'UCSDped2')
    assert out.tolist() == [sixty, edge, half, big]          # ascending area; the largest box is never dropped
    assert del_cover_bboxes(b, 'ShanghaiTech').tolist() == [sixty, edge, half, big]
    assert del_cover_bboxes(np.zeros((0, 4)), 'avenue').shape == (0, 4)
    with pytest.raises(NotImplementedError):
        del_cover_bboxes(b, 'UCSDped1')


def test_get_mt_bboxes_verbose_raises():
    from fore_det.obj_det_with_motion import get_mt_bboxes
    with pytest.raises(NotImplementedError):
        get_mt_bboxes(None, np.zeros((3, 8, 8, 3), np.uint8), np.zeros((0, 4)), 'UCSDped2', verbose=True)


# ---- load_bboxes ------------------------------------------------------------------------------------------------------------
def _ped2_frames(n_per_video):
    from PIL import Image
    for v, n in enumerate(n_per_video, start=1):
        d = os.path.join('raw_datasets', 'UCSDped2', 'Train', 'Train%03d' % v)
        os.makedirs(d)
        for k in range(n):
            Image.fromarray(np.zeros((240, 360), np.uint8)).save(os.path.join(d, '%03d.tif' % (k + 1)))


def _config(mode_fg):
    import train as T
    cfg = open(os.path.join(ROOT, 'config.cfg')).read()
    cfg = cfg.replace('train_bbox_saved = True', 'train_bbox_saved = False')
    cfg = cfg.replace('foreground_extraction_mode = obj_det_with_motion', 'foreground_extraction_mode = ' + mode_fg)
    open('config.cfg', 'w').write(cfg)
    return T.read_config('config.cfg')


def test_load_bboxes_simple_patch_without_a_saved_file(tmp_path, monkeypatch):
    import foreground as FG
    monkeypatch.chdir(tmp_path)
    _ped2_frames((3, 2))
    c = _config('simple_patch')
    assert c['mode_fg'] == 'simple_patch' and not c['cp'].getboolean('UCSDped2', 'train_bbox_saved')
    boxes = FG.load_bboxes(c, 'train', log=lambda *a: None)
    path = os.path.join('raw_datasets', 'UCSDped2', 'bboxes_train_simple_patch.npy')
    assert os.path.exists(path) and not [f for f in os.listdir(os.path.dirname(path)) if '.tmp' in f]
    saved = np.load(path, allow_pickle=True)
    assert saved.dtype == object and saved.shape == (5,) and len(boxes) == 5
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'simple_patch_boxes.npz'))
    want = np.concatenate([g['UCSDped2_3x4'], g['UCSDped2_6x8']], axis=0)
    for b, s in zip(boxes, saved):
        assert b.shape == (60, 4) and np.array_equal(b, want) and np.array_equal(s, want)
    assert np.array_equal(FG.load_bboxes(c, 'train')[4], want)                  # second call: the file is there


def test_load_bboxes_obj_det_without_a_file_still_raises(tmp_path, monkeypatch):
    import foreground as FG
    monkeypatch.chdir(tmp_path)
    _ped2_frames((2,))
    c = _config('obj_det')
    with pytest.raises(NotImplementedError):
        FG.load_bboxes(c, 'train')
    assert not os.path.exists(os.path.join('raw_datasets', 'UCSDped2', 'bboxes_train_obj_det.npy'))
