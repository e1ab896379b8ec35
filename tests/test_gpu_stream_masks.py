"""GPU: the pixel-level stages of a stream (vec_vad_amd/stream.py: masks / smooth / render) -- ``vv_stream_paint`` and ``vv_stream_smooth``
against the numpy restatement of tests/stream_masks_restatement.py and against the batch route's ``scoring.paint_masks`` /
``scoring.smooth_masks``; ``StreamScorer`` with the switches on against the restatement fed with what ``wait()`` returns and against a
scorer with the switches off; the picture against ``render.overlay`` and tests/render_restatement.py; ``stream.main`` with the keys on.
Every comparison is bit for bit: maxima do not round, and the sums are taken in one stated order on both sides."""
import os

import numpy as np
import pytest
import torch

import render_restatement as RR
import stream_masks_restatement as R
from test_gpu_stream import COUNTS, N_VIDEO, _stream, net, tree  # noqa: F401  (the fixtures of the synthetic tree)

pytestmark = pytest.mark.gpu

BIG = R.BIG
H, W = 45, 70              # 2 x 3 tiles of 32, ragged in both directions; a halo of 16 is wider than the last tile (6 columns)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. vv_stream_paint ---------------------------------------------------------------------------------------------------------------
# x1, y1, x2, y2
HAND = np.array([[0, 0, W, H],             # 0: the whole frame, with the lowest score
                 [10, 10, 10, 30],         # 1: an empty rectangle
                 [60, 5, W, 20],           # 2: on the right edge
                 [20, 35, 50, H],          # 3: on the bottom edge
                 [15, 10, 40, 30],         # 4, 5: overlapping; the larger score of 4 sits in row 0, that of 5 in row 1
                 [30, 20, 55, 40],
                 [2, 2, 6, 6],             # 6: +BIG in one row
                 [16, 11, 30, 25],         # 7: -BIG in both rows, over box 4
                 [-20, 30, 90, 50],        # 8: a negative x1 counts from the right edge, y2 clips
                 [65, 40, 90, 60]], np.int32)      # 9: past both edges
HAND_ROWS = np.array([[-3.0, 7.0, 1.25, 0.5, 2.0, 0.5, BIG, -BIG, 1.5, -BIG],
                      [-BIG, 9.0, -BIG, 0.75, 1.0, 3.0, -BIG, -BIG, -2.0, 4.5]])


def _paint_case(name):
    """(rows [2,width], n, boxes [width,4]): the first n slots are the case, the others poison."""
    rng = np.random.default_rng(7)
    if name == 'hand':
        n, width, boxes, rows = len(HAND), len(HAND) + 4, HAND, HAND_ROWS
    elif name == 'empty':
        n, width, boxes, rows = 0, 6, HAND[:0], HAND_ROWS[:, :0]
    else:
        from vec_vad_amd.stream import PAINT_STAGE
        n = PAINT_STAGE + int(name)
        width = n + 3
        x0, y0 = rng.integers(-5, W - 2, n), rng.integers(-5, H - 2, n)
        boxes = np.stack([x0, y0, x0 + rng.integers(1, 9, n), y0 + rng.integers(1, 9, n)], axis=1).astype(np.int32)
        rows = rng.standard_normal((2, n)) * 4
        rows[rng.random((2, n)) < 0.3] = -BIG
    all_rows = np.tile(np.array([[np.nan, np.inf, 1e30]]), (2, width))[:, :width].copy()      # what must never be read
    all_rows[:, :n] = rows
    all_boxes = np.tile(np.array([[0, 0, W, H]], np.int32), (width, 1))                        # garbage that would flood the mask
    all_boxes[:n] = boxes
    return all_rows, n, all_boxes


@pytest.mark.parametrize('host', ['none', 'some', 'all', 'all-no-table'])
@pytest.mark.parametrize('case', ['hand', 'empty', '-1', '0', '1'])
def test_stream_paint_equals_the_restatement_and_paint_masks(case, host):
    """n_host of the rectangles come from the host, the others the kernel resolves from the boxes and writes back.  Slots at or above n
    hold NaN, Inf, 1e30 scores and whole-frame boxes and rectangles: they are neither read (the mask would show) nor written."""
    from vec_vad_amd import scoring
    from vec_vad_amd.stream import stream_paint
    rows, n, boxes = _paint_case(case)
    width = rows.shape[1]
    n_host = {'none': 0, 'some': n // 3, 'all': n, 'all-no-table': n}[host]
    want_rects = R.resolve(boxes[:n], H, W)
    want_mask, want_max = R.paint(rows, n, want_rects, H, W)
    rects = np.tile(np.array([[0, H, 0, W]], np.int32), (width, 1))      # rows >= n_host: garbage the kernel must not read
    rects[:n_host] = want_rects[:n_host]
    d_rects, d_max = cu(rects), cu(np.full(width, 55.5))
    mask = torch.full((H, W), 7.0, dtype=torch.float64, device='cuda')
    off = cu(np.array([-4, -4], np.int32))
    stream_paint(cu(rows), cu(np.array([n], np.int32)), n_host, d_rects, None if host == 'all-no-table' else cu(boxes), mask, d_max, off)
    got_mask, got_max, got_rects = mask.cpu().numpy(), d_max.cpu().numpy(), d_rects.cpu().numpy()
    assert np.array_equal(_bits(got_mask), _bits(want_mask))
    assert np.array_equal(_bits(got_max[:n]), _bits(want_max)) and (got_max[n:] == 55.5).all()
    assert np.array_equal(got_rects[:n], want_rects) and np.array_equal(got_rects[n:], rects[n:])
    assert off.tolist() == [0, n]
    assert got_mask.max() == (want_max[(want_rects[:, 1] > want_rects[:, 0]) & (want_rects[:, 3] > want_rects[:, 2])].max(initial=-BIG))
    # the batch route's painter fed with the maxima and the rectangles the kernel left
    batch = scoring.paint_masks(d_max[:n], np.array([0, n], np.int32), d_rects[:n], H, W)[0]
    assert torch.equal(batch, mask)
    if case == 'hand':
        assert got_mask[0, 69] == -3.0 and got_mask[3, 3] == BIG and got_mask[12, 17] == 2.0 and got_mask[25, 35] == 3.0
        assert got_mask[44, 69] == 4.5 and got_mask[30, 60] == 1.5 and got_mask[30, 40] == 3.0
        assert want_rects[8].tolist() == [30, H, 50, W] and want_rects[1].tolist() == [10, 30, 10, 10]
    if case == 'empty':
        assert (got_mask == -BIG).all()


def test_stream_paint_without_rows_or_slots_fills_the_background():
    from vec_vad_amd.stream import stream_paint
    mask = torch.full((H, W), 7.0, dtype=torch.float64, device='cuda')
    off, n3 = cu(np.array([-4, -4], np.int32)), cu(np.array([3], np.int32))
    # boxes that belong to no block: no score row at all; their maxima read -BIG
    d_max = cu(np.full(4, 55.5))
    stream_paint(torch.zeros((0, 4), dtype=torch.float64, device='cuda'), n3, 3, cu(R.resolve(HAND[:4], H, W)), None, mask, d_max, off)
    assert bool((mask == -BIG).all()) and d_max.tolist() == [-BIG, -BIG, -BIG, 55.5] and off.tolist() == [0, 3]
    # a frame without a box: no slot (n is clamped to the width)
    mask.fill_(7.0)
    stream_paint(torch.zeros((0, 0), dtype=torch.float64, device='cuda'), n3, 0, torch.zeros((1, 4), dtype=torch.int32, device='cuda'), None,
                 mask, d_max, off)
    assert bool((mask == -BIG).all()) and off.tolist() == [0, 0]


# ---- 2. vv_stream_smooth --------------------------------------------------------------------------------------------------------------
def _video_masks(F=7):
    """A video of 45x70 masks: random boxes, frame 3 with nothing painted, frame 4 with a +BIG box."""
    rng = np.random.default_rng(21)
    m = np.full((F, H, W), -BIG)
    for f in range(F):
        if f == 3:
            continue
        for _ in range(5):
            y0, x0 = rng.integers(0, H - 3), rng.integers(0, W - 3)
            y1, x1 = rng.integers(y0 + 1, min(H, y0 + 30) + 1), rng.integers(x0 + 1, min(W, x0 + 40) + 1)
            m[f, y0:y1, x0:x1] = np.maximum(m[f, y0:y1, x0:x1], rng.standard_normal() * 3)
        if f == 4:
            m[f, 20:26, 30:41] = BIG
    return m


@pytest.mark.parametrize('ks', [1, 3, 9, 33])
@pytest.mark.parametrize('kt', [1, 2, 5])
def test_stream_smooth_equals_the_restatement_and_the_centred_filter(kt, ks):
    """Seven frames through a ring of kt slots that starts out full of poison -- what the video before left there: NaN sums, 1e30
    masks.  Until the video has kt frames the window is shorter than the ring and the poisoned slots must not be read; later the
    slot order wraps.  Entries of the table behind the count are garbage."""
    from vec_vad_amd import scoring
    from vec_vad_amd.stream import stream_smooth
    m = _video_masks()
    F = len(m)
    want = R.trailing(m, kt, ks)
    ring = torch.full((kt, H, W), 1e30, dtype=torch.float64, device='cuda')
    Bsum = torch.full((kt, H, W), float('nan'), dtype=torch.float64, device='cuda')
    bcnt = torch.full((kt, H, W), 12345, dtype=torch.int16, device='cuda')
    out = torch.empty((H, W), dtype=torch.float64, device='cuda')
    partial = torch.empty(((H * W + 255) // 256,), dtype=torch.float64, device='cuda')
    dm = cu(m)
    wrapped = False
    for t in range(F):
        frames = list(range(max(0, t - kt + 1), t + 1))
        slots = [f % kt for f in frames]
        wrapped |= slots != sorted(slots)
        ring[t % kt].copy_(dm[t])
        win = np.full(1 + kt, 77, np.int32)
        win[0], win[1:1 + len(slots)] = len(slots), slots
        out.fill_(5.0), partial.fill_(5.0)
        stream_smooth(ring, cu(win), kt, ks, Bsum, bcnt, out, partial)
        got = out.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want[t])), (t, kt, ks)
        assert float(partial.max()) == want[t].max() and bool((partial >= -BIG).all())
        centred, fmax = scoring.smooth_masks(dm[:t + 1], np.zeros(t + 1, np.int32), 2 * kt - 1, ks, lo=t, hi=t + 1)
        assert torch.equal(centred[0], out) and float(fmax[0]) == float(partial.max())
    assert wrapped == (kt in (2, 5))
    assert (want[3] == -BIG).all() and want[4].max() > 1000                       # nothing painted | the +BIG box floods
    if kt > 1 and ks > 1:
        assert (want[5][m[5] != -BIG] > 1000).any()                               # ... into the next frame's window


def test_stream_smooth_bad_arguments_return_without_a_launch():
    from vec_vad_amd import _lib
    l = _lib.lib()
    t = torch.zeros(64, dtype=torch.float64, device='cuda')
    p, st = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    good = [p, 1, 4, 4, p, 1, 3, p, p, p, p, st]
    for i, v in ((0, None), (4, None), (7, None), (8, None), (9, None), (10, None), (1, 0), (2, -1), (5, 0), (5, 34), (6, 0), (6, 4), (6, 35)):
        args = list(good)
        args[i] = v
        assert l.vv_stream_smooth(*args) == 1, i                                  # VV_ERR_BAD_ARG
    good = [p, 2, 4, p, 0, p, None, 4, 4, p, p, p, st]
    for i, v in ((3, None), (11, None), (9, None), (5, None), (1, -1), (4, -1)):
        args = list(good)
        args[i] = v
        assert l.vv_stream_paint(*args) == 1, i
    torch.cuda.synchronize()
    assert not t.any()


# ---- 3. the scorer --------------------------------------------------------------------------------------------------------------------
KT, KS = 2, 9              # a ring of two slots: it wraps inside a video of three frames, and the window is short at a video's start


def _keep_all(tree, name):
    """The tree's configuration with ``motionThr = 0``, written next to it: frames set into a corner of noise have other flows than the
    ones the tree's threshold was picked for, and a picture of boxes that were all dropped shows nothing."""
    import re
    cfg, subs = re.subn(r'\[UCSDped2\]\nmotionThr = [^\n]*\n', '[UCSDped2]\nmotionThr = 0\n', open('config.cfg').read())
    assert subs == 1
    open(name, 'w').write(cfg)
    return cfg


def _run(tree, net, frame_shape=(48, 72, 3), frames=None, sync_error_after=None, c=None, **kw):
    """The tree's frames (or ``frames``) through one ``StreamScorer(**kw)``; returns the waited ``StreamResult``s."""
    from vec_vad_amd.stream import StreamScorer
    frames = tree['frames'] if frames is None else frames
    boxes, fvi = tree['boxes'], tree['fvi'][:len(frames)]
    sc = StreamScorer(dict(tree['c'], smooth_frames=KT, smooth_pixels=KS) if c is None else c, *tree['arts'], frame_shape, flownet2=net, **kw)
    res = []
    try:
        for i, f in enumerate(frames):
            if i and fvi[i] != fvi[i - 1]:
                res += sc.end_video()
            if sync_error_after is not None and i == sync_error_after:
                torch.cuda.set_sync_debug_mode('error')
            res += sc.push(f, ap_boxes=boxes[i]) if kw.get('boxes') == 'motion' else sc.push(f, boxes[i])
        res += sc.end_video()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert [r.frame for r in res] == list(range(len(frames)))
    return [(r, r.wait()) for r in res]


@pytest.mark.parametrize('mode', ['one-round', 'rounds', 'motion'])
def test_scorer_masks_equal_the_restatement_of_what_wait_returns(tree, net, monkeypatch, mode):
    from vad_datasets import frame_size
    from vec_vad_amd.scoring import box_rects
    monkeypatch.chdir(tree['root'])
    gh, gw = frame_size['UCSDped2'][:2]
    kw = dict(max_boxes=2 if mode == 'rounds' else 8, boxes='motion' if mode == 'motion' else 'given')
    got = _run(tree, net, masks=True, smooth=True, **kw)
    if mode == 'motion':
        off = [w for _, w in _run(tree, net, **kw)]
    else:
        off = _stream(tree, net, kw['max_boxes'])
    video, painted, found = [], 0, 0
    for f, ((r, (score, box, kept)), (oscore, obox, okept)) in enumerate(zip(got, off)):
        assert _bits(score) == _bits(oscore) and np.array_equal(_bits(box), _bits(obox)) and kept.tolist() == okept.tolist(), f
        assert r.picture is None and r.mask.dtype == np.float64 and r.mask.shape == (gh, gw) == r.smooth_mask.shape
        want, _ = R.paint(box[None, :], len(box), box_rects(r.boxes, gh, gw), gh, gw)
        assert np.array_equal(_bits(r.mask), _bits(want)), f
        assert r.mask.max() == score, f
        if f and tree['fvi'][f] != tree['fvi'][f - 1]:
            video = []
        video.append(r.mask)
        smooth = R.trailing(np.stack(video[-KT:]), KT, KS)[-1]      # the window never reaches further back than KT frames
        assert np.array_equal(_bits(r.smooth_mask), _bits(smooth)), f
        assert isinstance(r.smooth_score, float) and r.smooth_score == smooth.max(), f
        painted += bool((r.mask > -BIG).any())
        found += len(r.boxes) - len(tree['boxes'][f])
    assert painted >= 3
    if mode == 'motion':
        assert found >= 3                                            # rectangles the kernel resolved, behind those of the host
    else:
        assert (got[2][0].mask == -BIG).all() and got[2][0].smooth_score == -BIG      # the frame without boxes


def test_switches_off_leave_the_result_bare(tree, net, monkeypatch):
    monkeypatch.chdir(tree['root'])
    for r, _ in _run(tree, net, max_boxes=8):
        assert r.mask is None and r.smooth_mask is None and r.smooth_score is None and r.picture is None


# ---- 4. the picture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('render_boxes', [True, False], ids=['outlines', 'no-outlines'])
@pytest.mark.parametrize('source', ['score', 'smooth'])
def test_picture_equals_overlay_and_its_restatement(tree, net, monkeypatch, source, render_boxes):
    """The first video's four frames set into the corner of 240x360 noise frames, all three switches on, every push behind the first
    under torch's sync debug mode: a synchronising call would raise."""
    from vad_datasets import frame_size
    from vec_vad_amd import render
    from vec_vad_amd.scoring import box_rects
    monkeypatch.chdir(tree['root'])
    gh, gw = frame_size['UCSDped2'][:2]
    rng = np.random.default_rng(9)
    frames = []
    for f in tree['frames'][:N_VIDEO[0]]:
        big = rng.integers(0, 256, (gh, gw, 3), dtype=np.uint8)
        big[:48, :72] = f
        frames.append(big)
    lo, hi, alpha = -5.0, 20.0, (256 * 50 + 50) // 100
    import train as T
    _keep_all(tree, 'config_picture.cfg')
    c = dict(T.read_config('config_picture.cfg'), smooth_frames=KT, smooth_pixels=KS, render_range=(lo, hi), render_source=source, render_boxes=render_boxes)
    assert c['render_alpha'] == 50
    got = _run(tree, net, (gh, gw, 3), frames=frames, sync_error_after=1, c=c, max_boxes=8, masks=True, smooth=True, render=True)
    lut = render.colormap()
    drawn = 0
    for f, (r, (score, box, kept)) in enumerate(got):
        assert r.picture.dtype == np.uint8 and r.picture.shape == (gh, gw, 3)
        shown = r.smooth_mask if source == 'smooth' else r.mask
        n = len(box) if render_boxes else 0
        rects = box_rects(r.boxes, gh, gw)[:n]
        want = render.overlay(cu(frames[f][None]), cu(shown[None]), rects, box[:n], [0, n], lo, hi, alpha, bgr=True)[0].cpu().numpy()
        assert np.array_equal(r.picture, want), f
        restated = RR.overlay(frames[f][None], shown[None], rects, box[:n], [0, n], lo, hi, alpha, lut=lut, bgr=True)[0]
        assert np.array_equal(r.picture, restated), f
        assert np.array_equal(r.picture[100:, 100:], frames[f][100:, 100:, ::-1])      # outside every box: the frame, as RGB
        drawn += bool((r.picture[:48, :72] != frames[f][:48, :72, ::-1]).any())
    assert drawn >= 2


# ---- 5. the script --------------------------------------------------------------------------------------------------------------------
def test_stream_main_with_the_keys_on_writes_the_new_files_and_the_same_scores(tree, net, monkeypatch, capsys):
    """The tree's test frames are rewritten as 240x360 frames (a picture needs the nominal size), then ``stream.main`` runs with the keys
    off and with them on."""
    import glob
    from PIL import Image
    import stream as STREAM
    monkeypatch.chdir(tree['root'])
    rng = np.random.default_rng(3)
    for path in sorted(glob.glob('raw_datasets/UCSDped2/Test/Test*/*')):
        small = np.asarray(Image.open(path))
        big = rng.integers(0, 256, (240, 360), dtype=np.uint8) if path.endswith('.tif') else np.zeros((240, 360), np.uint8)
        big[:48, :72] = small
        Image.fromarray(big).save(path)
    saved = open('config.cfg').read()
    cfg = _keep_all(tree, 'config.cfg')
    n = sum(N_VIDEO)
    try:
        A = STREAM.main('config.cfg', flownet2=net)
        a_file = open('results/UCSDped2/stream_scores_obj_det_with_motion_SelfComplete.npy', 'rb').read()
        assert not glob.glob('results/UCSDped2/stream_scores_smooth_*') and not os.path.exists('results/UCSDped2/stream_render')
        on = cfg.replace('stream_smooth = off', 'stream_smooth = on').replace('stream_render = off', 'stream_render = on')
        on = on.replace('render_range = auto', 'render_range = -5,20')
        assert on.count(' = on\n') == 2 and cfg.count(' = on\n') == 0
        open('config.cfg', 'w').write(on)
        capsys.readouterr()
        B = STREAM.main('config.cfg', flownet2=net)
        out = capsys.readouterr().out
    finally:
        open('config.cfg', 'w').write(saved)
    assert np.array_equal(_bits(A), _bits(B)) and (A > -BIG).sum() >= 3
    assert open('results/UCSDped2/stream_scores_obj_det_with_motion_SelfComplete.npy', 'rb').read() == a_file
    S = np.load('results/UCSDped2/stream_scores_smooth_obj_det_with_motion_SelfComplete.npy')
    assert S.dtype == np.float64 and S.shape == (n,) and ((S > -BIG) == (A > -BIG)).all() and not np.array_equal(S, A)
    auc = float(np.load('results/UCSDped2/raw2flow_obj_det_with_motion_SelfComplete_stream_smooth_results.npz')['roc_auc'])
    assert 'Frame-level AUC of the smoothed stream is {}'.format(auc) in out.splitlines()
    assert sorted(os.listdir('results/UCSDped2/stream_render')) == sorted('%d.png' % i for i in range(n))
    img = np.asarray(Image.open('results/UCSDped2/stream_render/0.png'))
    assert img.shape == (240, 360, 3) and img.dtype == np.uint8
