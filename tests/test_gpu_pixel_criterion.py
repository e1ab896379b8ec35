"""Pixel-level evaluation on the GPU: vv_cube_scores, vv_paint_masks and vv_pixel_scores against the host arithmetic the repository
pins to the reference (``test.paint_frame``) followed by plain numpy, then the scoring level (``score_frames`` / ``score_store``
with the ``pixel`` keyword) and the script level (``test.main`` with ``[mi355x] pixel_criterion``).  The kernels select and copy
doubles, so every comparison is ``==``; only the AUROC is compared at 1e-12."""
import glob
import os

import numpy as np
import pytest
import torch

from _util import small_config

pytestmark = pytest.mark.gpu

BIG = 100000
SIZES = [(37, 53), (1, 1), (240, 360)]          # odd h*w with a ragged tail; one pixel; the UCSDped2 frame


def _kth(mask, gt, pct):
    g = int((gt != 0).sum())
    if g == 0:
        return mask.max()
    return np.sort(mask[gt != 0])[::-1][(g * pct + 99) // 100 - 1]


# ---- cube scores ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 1, 257])
def test_cube_scores_are_the_numpy_expression(n):
    from vec_vad_amd import scoring
    import test as S
    rng = np.random.default_rng(5 + n)
    raw = (rng.random(n) * 50).astype(np.float32)
    of = (rng.random(n) * 9).astype(np.float32)
    stats = np.array([[20.0, 7.5, 4.0, 1.25], [25.0, 3.0, 5.0, 2.0]])
    cs = rng.integers(-1, 2, n).astype(np.int32)
    if n > 2:
        cs[:3] = [0, -1, 1]
    h, w = 60, 90
    counts = np.zeros(12, np.int64)
    for m in range(n):
        counts[rng.integers(0, 11)] += 1                    # the last frame stays without cubes
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    x0, y0 = rng.uniform(-4, w - 5, n), rng.uniform(-4, h - 5, n)
    boxes = np.stack([x0, y0, x0 + rng.uniform(0.2, 20, n), y0 + rng.uniform(0.2, 20, n)], 1).reshape(n, 4)
    for use_flow in (True, False):
        got = scoring.cube_scores(torch.from_numpy(raw).cuda(), torch.from_numpy(of).cuda() if use_flow else None, cs, stats, 0.3, 1.0)
        assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (n,)
        want = np.empty(n)
        for m in range(n):
            if cs[m] < 0:
                want[m] = S.BIG
            else:
                st = stats[cs[m]]
                want[m] = 0.3 * ((raw[m] - st[0]) / st[1])
                if use_flow:
                    want[m] = want[m] + 1.0 * ((of[m] - st[2]) / st[3])
        assert np.array_equal(got.cpu().numpy(), want)
        if n > 1:
            assert (want == S.BIG).any() and (want != S.BIG).any()
        if n == 0:
            continue
        fs = scoring.frame_scores(torch.from_numpy(raw).cuda(), torch.from_numpy(of).cuda() if use_flow else None, off, cs, stats,
                                  scoring.box_paints(boxes, h, w), 0.3, 1.0).cpu().numpy()
        for f in range(12):
            sl = slice(off[f], off[f + 1])
            assert fs[f] == S.paint_frame(want[sl], boxes[sl], h, w).max(), f
        assert fs[11] == -S.BIG


# ---- painted masks and pixel scores: one scene per frame size -------------------------------------------------------------------
COUNTS7 = [257, 0, 1, 63, 64, 65, 9]           # boxes per frame: wave (64) and LDS-pass (256) borders, none, one


def _scene(h, w, counts, seed):
    """Boxes, scores, rectangles and the host-painted masks of ``len(counts)`` frames.  Every frame with at least 5 boxes holds an
    empty rectangle, a wrapped and a clipped one and a ``BIG`` score; the first and the last frame a whole-frame box (lowest score);
    scores are rounded to 0.1 (ties) and the last frame's two best scores are equal."""
    from vec_vad_amd import scoring
    import test as S
    rng = np.random.default_rng(seed)
    boxes, scores = [], []
    for f, n in enumerate(counts):
        x0, y0 = rng.uniform(-6, w + 3, n), rng.uniform(-6, h + 3, n)
        b = np.stack([x0, y0, x0 + rng.uniform(0.3, 0.4 * w + 2, n), y0 + rng.uniform(0.3, 0.4 * h + 2, n)], 1).reshape(n, 4)
        s = np.round(rng.standard_normal(n) * 3, 1)
        if n >= 5:
            b[0] = [3.2, 3.2, 3.9, 9.0]                                  # ceil(x1) == ceil(x2): paints nothing
            b[1] = [-w * 0.5, -h * 0.5, w * 0.3, h * 0.3]                # negative ceilings wrap: usually empty
            b[2] = [w * 0.6, h * 0.6, w + 40.0, h + 40.0]                # clipped at the far edges
            s[2] = S.BIG
            s[0] = 2 * S.BIG                                             # would win everywhere if an empty rectangle painted
        if n >= 9:
            b[6] = [-w * 0.3, -h * 0.3, -1.0, -1.0]                      # negative ceilings on both ends: counted from the far edges
        if n >= 5 and f in (0, len(counts) - 1):
            b[3] = [0.0, 0.0, float(w), float(h)]                        # the whole frame, under everything else
            s[3] = -50.0
        if n >= 5 and f == len(counts) - 1:
            s[4] = s[5] = 40.0                                           # tied top scores below BIG
            b[4] = [w * 0.1, h * 0.1, w * 0.5, h * 0.5]
            b[5] = [w * 0.3, h * 0.3, w * 0.7, h * 0.7]
        boxes.append(b)
        scores.append(s)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    boxes, scores = np.concatenate(boxes), np.concatenate(scores)
    rects = scoring.box_rects(boxes, h, w)
    masks = np.stack([S.paint_frame(scores[off[f]:off[f + 1]], boxes[off[f]:off[f + 1]], h, w) for f in range(len(counts))])
    return dict(h=h, w=w, off=off, boxes=boxes, scores=scores, rects=rects, masks=masks)


@pytest.fixture(scope='module')
def scenes():
    return {(h, w, F): _scene(h, w, COUNTS7[:F], 100 + h) for (h, w) in SIZES for F in (1, 7)}


@pytest.mark.parametrize('F', [1, 7])
@pytest.mark.parametrize('h,w', SIZES, ids=['37x53', '1x1', '240x360'])
def test_paint_masks_equal_paint_frame(scenes, h, w, F):
    from vec_vad_amd import scoring
    sc = scenes[(h, w, F)]
    off, rects = sc['off'], sc['rects']
    scores = torch.from_numpy(sc['scores']).cuda()
    if h > 1:
        empty = (rects[:, 1] <= rects[:, 0]) | (rects[:, 3] <= rects[:, 2])
        assert empty.any() and (~empty).any() and (sc['scores'] == BIG).any()
        assert ((rects[:, 0] == 0) & (rects[:, 1] == h) & (rects[:, 2] == 0) & (rects[:, 3] == w)).any()      # a whole-frame box
        assert (sc['masks'] == BIG).any() and (sc['masks'] < BIG).any()
    got = scoring.paint_masks(scores, off, rects, h, w)
    assert got.dtype == torch.float64 and tuple(got.shape) == (F, h, w) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), sc['masks'])
    if F == 7:
        assert (sc['masks'][1] == -BIG).all()                            # the frame without boxes is the background
    # two groups painted into one `out`: even and odd boxes of every frame, each group with its own CSR
    out = torch.full((F, h, w), -float(BIG), dtype=torch.float64, device='cuda')
    for par in (0, 1):
        pick = np.concatenate([np.arange(off[f], off[f + 1])[par::2] for f in range(F)]).astype(np.int64)
        cnt = [len(np.arange(off[f], off[f + 1])[par::2]) for f in range(F)]
        goff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        ret = scoring.paint_masks(scores[torch.from_numpy(pick).cuda()], goff, rects[pick], h, w, out=out)
        assert ret is out
    assert np.array_equal(out.cpu().numpy(), sc['masks'])
    # max-accumulation: painting over a mask that is already higher somewhere keeps the higher value
    high = torch.full((F, h, w), 1.5, dtype=torch.float64, device='cuda')
    scoring.paint_masks(scores, off, rects, h, w, out=high)
    assert np.array_equal(high.cpu().numpy(), np.maximum(sc['masks'], 1.5))


def test_paint_masks_without_frames_touch_nothing():
    from vec_vad_amd import scoring
    buf = torch.full((2, 37, 53), 7.0, dtype=torch.float64, device='cuda')
    out = scoring.paint_masks(torch.zeros(0, dtype=torch.float64, device='cuda'), np.zeros(1, np.int32), np.zeros((0, 4), np.int32),
                              37, 53, out=buf[:0])
    assert tuple(out.shape) == (0, 37, 53) and bool((buf == 7.0).all())
    # frames, but no box at all: the caller's background stays
    out = scoring.paint_masks(torch.zeros(0, dtype=torch.float64, device='cuda'), np.zeros(3, np.int32), np.zeros((0, 4), np.int32),
                              37, 53, out=buf)
    assert out is buf and bool((buf == 7.0).all())


def _ground_truths(sc, variant):
    """uint8 ``[F,h,w]``: frame ``f`` gets ground truth of kind ``(f + variant) % 7`` -- none, one pixel, 5 pixels, 6 pixels, a
    rectangle partly under boxes, pixels outside every box, the whole frame -- with values 1 and 255."""
    h, w, masks = sc['h'], sc['w'], sc['masks']
    F = len(masks)
    rng = np.random.default_rng(7 + variant)
    gt = np.zeros((F, h, w), np.uint8)
    for f in range(F):
        kind, val = (f + variant) % 7, (1, 255)[(f + variant) % 2]
        flat = gt[f].reshape(-1)
        if kind in (1, 2, 3):
            flat[rng.choice(h * w, min((1, 5, 6)[kind - 1], h * w), replace=False)] = val
        elif kind == 4:
            gt[f, h // 5:max(h // 5 + 1, 3 * h // 4), w // 4:max(w // 4 + 1, 4 * w // 5)] = val
        elif kind == 5:
            free = np.nonzero(masks[f].reshape(-1) == -BIG)[0]
            flat[free[:7] if len(free) else [0]] = val
        elif kind == 6:
            gt[f] = val
    return gt


@pytest.mark.parametrize('F', [1, 7])
@pytest.mark.parametrize('h,w', SIZES, ids=['37x53', '1x1', '240x360'])
def test_pixel_scores_equal_the_kth_largest_of_the_painted_mask(scenes, h, w, F):
    from vec_vad_amd import scoring
    sc = scenes[(h, w, F)]
    scores = torch.from_numpy(sc['scores']).cuda()
    above = at_bg = 0
    for variant in range(7 if F == 7 else 14):
        gt = _ground_truths(sc, variant)
        gt_dev = torch.from_numpy(gt).cuda()
        for pct in ((40, 1, 100) if variant < 3 or F == 1 else (40,)):
            got, cnt = scoring.pixel_scores(gt_dev, scores, sc['off'], sc['rects'], pct)
            assert got.dtype == torch.float64 and cnt.dtype == torch.int32 and tuple(got.shape) == tuple(cnt.shape) == (F,)
            want = np.array([_kth(sc['masks'][f], gt[f], pct) for f in range(F)])
            assert np.array_equal(cnt.cpu().numpy(), (gt != 0).reshape(F, -1).sum(1))
            assert np.array_equal(got.cpu().numpy(), want), (variant, pct, got.cpu().numpy(), want)
            again, cnt2 = scoring.pixel_scores(gt_dev, scores, sc['off'], sc['rects'], pct)
            assert torch.equal(again, got) and torch.equal(cnt2, cnt)                  # bit-identical run to run
            anomalous = (gt != 0).reshape(F, -1).any(1)
            above += int((want[anomalous] > -BIG).sum())
            at_bg += int((want[anomalous] == -BIG).sum())
    if h > 1 and F == 7:
        # a run in which every answer is the background proves nothing
        assert above >= 2 and at_bg >= 1, (above, at_bg)
    if h > 1 and F == 7:
        last = np.sort(sc['scores'][sc['off'][6]:sc['off'][7]])
        assert last[-4] == last[-3] == 40.0 and last[-2] == BIG                        # tied top scores below the BIG box
    # host ground truth is uploaded; percent is checked
    got, _ = scoring.pixel_scores(_ground_truths(sc, 0), scores, sc['off'], sc['rects'])
    assert np.array_equal(got.cpu().numpy(), [_kth(sc['masks'][f], _ground_truths(sc, 0)[f], 40) for f in range(F)])
    for bad in (0, 101, 40.5):
        with pytest.raises(ValueError):
            scoring.pixel_scores(gt_dev, scores, sc['off'], sc['rects'], bad)


def test_pixel_scores_take_2048_boxes_and_refuse_2049():
    from vec_vad_amd import scoring
    import test as S
    h, w = 37, 53
    rng = np.random.default_rng(23)
    n = 2049
    x0, y0 = rng.uniform(-3, 0.6 * w, n), rng.uniform(-3, h - 2, n)            # the right third of the frame stays uncovered
    boxes = np.stack([x0, y0, x0 + rng.uniform(0.5, 6, n), y0 + rng.uniform(0.5, 6, n)], 1)
    scores = np.round(rng.standard_normal(n) * 3, 1)
    rects = scoring.box_rects(boxes, h, w)
    gt = (rng.random((1, h, w)) < 0.3).astype(np.uint8) * 255
    sd = torch.from_numpy(scores).cuda()
    mask = S.paint_frame(scores[:2048], boxes[:2048], h, w)
    assert (mask[gt[0] != 0] == -BIG).any() and (mask[gt[0] != 0] > -BIG).any()
    for pct in (40, 100):
        got, cnt = scoring.pixel_scores(gt, sd[:2048], np.array([0, 2048], np.int32), rects[:2048], pct)
        assert got.item() == _kth(mask, gt[0], pct) and cnt.item() == int((gt != 0).sum())
    assert got.item() == -BIG and _kth(mask, gt[0], 40) > -BIG
    sentinel = torch.full((1,), 7.0, dtype=torch.float64, device='cuda')
    with pytest.raises(ValueError, match='frame 0 has 2049 boxes') as e:
        scoring.pixel_scores(gt, sd, np.array([0, 2049], np.int32), rects, 40, out=sentinel)
    assert '\n' not in str(e.value)
    torch.cuda.synchronize()
    assert sentinel.item() == 7.0
    # the entry point itself: VV_ERR_UNSUPPORTED (3), nothing launched
    from vec_vad_amd import _lib
    off = torch.tensor([0, 2049], dtype=torch.int32, device='cuda')
    cnt = torch.full((1,), -1, dtype=torch.int32, device='cuda')
    st = _lib.lib().vv_pixel_scores(torch.from_numpy(gt).cuda().data_ptr(), sd.data_ptr(), off.data_ptr(),
                                    torch.from_numpy(rects).cuda().data_ptr(), 40, float(BIG), 1, h, w, 2049, sentinel.data_ptr(),
                                    cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 3 and sentinel.item() == 7.0 and cnt.item() == -1


# ---- scoring level: the cube_set / models construction of tests/test_gpu_direct.py --------------------------------------------
COUNTS = [3, 0, 9, 1, 0, 4, 7]
HB = WB = 2
FH, FW = 240, 360
LABELS = np.array([False, False, True, False, False, True, True])


def _net(seed):
    from oracle import unet_oracle as O
    from model.unet import SelfCompleteNet4
    net = SelfCompleteNet4(features_root=32, tot_raw_num=5, tot_of_num=1, border_mode='predict', rawRange=None, useFlow=True,
                           padding=False)
    net.load_state_dict(O.seeded_state_dict('net4', nf=32, padding=False, seed=seed))
    return net.cuda().eval()


@pytest.fixture(scope='module')
def cube_set():
    """24 cubes in 7 frames on a 2x2 block grid: cube k lies in block (k % 2, (k // 2) % 2) -- (1, 1) is the block without a
    model --, cube 5 lies in (1, 0) and (0, 1).  Ground truth on frames 2, 5 and 6: inside the first box of frame 2, the whole
    first box of frame 5, and 50 pixels of frame 6 that no box covers."""
    from oracle import unet_oracle as O
    from vec_vad_amd import scoring
    rng = np.random.default_rng(3)
    raws, flows, cube_frame, cube_blocks, boxes = [], [], [], [], []
    for f, cnt in enumerate(COUNTS):
        if cnt:
            rw, fl = O.seeded_cubes(cnt, 1, 50 + f)
            raws.append(rw)
            flows.append(fl)
        for _ in range(cnt):
            k = len(cube_frame)
            cube_frame.append(f)
            cube_blocks.append([(1, 0), (0, 1)] if k == 5 else [(k % 2, (k // 2) % 2)])
            x0, y0 = rng.uniform(-5, FW - 30), rng.uniform(-5, FH - 30)
            boxes.append([x0, y0, x0 + rng.uniform(8, 64), y0 + rng.uniform(8, 64)])
    raw, flow, boxes = np.concatenate(raws), np.concatenate(flows), np.array(boxes)
    fset = [[[[] for _ in range(WB)] for _ in range(HB)] for _ in COUNTS]
    for k, (f, blocks) in enumerate(zip(cube_frame, cube_blocks)):
        for (hi, wi) in blocks:
            fset[f][hi][wi].append(k)

    def lists(pick, empty):
        return [[[pick(np.array(cell, np.int64)) if cell else empty for cell in row] for row in fr] for fr in fset]

    host = (lists(lambda i: raw[i], np.zeros((0, 5, 32, 32, 3), np.uint8)),
            lists(lambda i: flow[i, 0], np.zeros((0, 32, 32, 2), np.float32)), lists(lambda i: boxes[i], np.zeros((0, 4))))
    rects = scoring.box_rects(boxes, FH, FW)
    first = np.concatenate([[0], np.cumsum(COUNTS)])
    gt = np.zeros((7, FH, FW), np.uint8)
    y0, y1, x0, x1 = rects[first[2]]
    assert y1 - y0 >= 4 and x1 - x0 >= 4
    gt[2, y0 + 1:y1 - 1, x0 + 1:x1 - 1] = 255
    y0, y1, x0, x1 = rects[first[5]]
    gt[5, y0:y1, x0:x1] = 1
    covered = np.zeros((FH, FW), bool)
    for y0, y1, x0, x1 in rects[first[6]:first[7]]:
        covered[y0:y1, x0:x1] = True
    gt[6].reshape(-1)[np.nonzero(~covered.reshape(-1))[0][1000:1050]] = 255
    assert [bool(g.any()) for g in gt] == LABELS.tolist()
    return dict(raw=raw, flow=flow, boxes=boxes, cube_frame=cube_frame, cube_blocks=cube_blocks, host=host, gt=gt)


@pytest.fixture(scope='module')
def models():
    n0 = _net(0)
    return dict(net_set=[[[n0], [n0]], [[n0], []]],
                st_r=[[(900.0, 35.0), (880.0, 40.0)], [(910.0, 30.0), (0.0, 1.0)]],
                st_o=[[(50.0, 4.0), (52.0, 5.0)], [(49.0, 3.0), (0.0, 1.0)]])


def _load_masks(d, n):
    assert sorted(os.listdir(d)) == sorted(str(f) for f in range(n))
    return [torch.load(os.path.join(d, str(f)), weights_only=False) for f in range(n)]


@pytest.mark.parametrize('use_flow', [True, False], ids=['flow', 'no-flow'])
def test_pixel_scores_and_device_masks_on_both_routes(tmp_path, cube_set, models, use_flow):
    """``score_frames`` (host-painted masks), ``score_store`` whole and ``score_store`` in two parts through one reused store (both
    with device-painted masks): the same pixel scores, equal to the k-th largest value of the host-painted mask FILES over the
    ground truth; the same mask files; the frame scores of a call without the keyword."""
    import test as S
    from foreground import block_groups
    m, gt = models, cube_set['gt']
    fset, fset2, bset = cube_set['host']
    da, db, dc = (str(tmp_path / d) for d in ('staged', 'direct', 'parts'))

    def pixel(device_masks, chunk):
        out = torch.full((7,), -float(S.BIG), dtype=torch.float64, device='cuda')
        return S.PixelEval(lambda i: gt[i], 40, out, LABELS, device_masks, chunk)

    common = (FH, FW, 1.0, 0.5, use_flow, 'cuda')
    pa = pixel(False, 3)
    fs_a = S.score_frames(m['net_set'], m['st_r'], m['st_o'], fset, fset2, bset, *common, score_batch=4, result_dir=da, pixel=pa)
    store = (torch.from_numpy(cube_set['raw']).cuda(), torch.from_numpy(cube_set['flow']).cuda())
    groups = block_groups(cube_set['cube_frame'], cube_set['cube_blocks'], 7)
    trainers = {}
    fs_0 = S.score_store(m['net_set'], m['st_r'], m['st_o'], store, groups, cube_set['boxes'], *common, 4, trainers=trainers)
    pb = pixel(True, 2)
    fs_b = S.score_store(m['net_set'], m['st_r'], m['st_o'], store, groups, cube_set['boxes'], *common, 4, None, db, trainers=trainers,
                         pixel=pb)
    pc = pixel(True, 64)
    part = (torch.zeros((12, 5, 32, 32, 3), dtype=torch.uint8, device='cuda'), torch.zeros((12, 1, 32, 32, 2), device='cuda'))
    out = torch.full((7,), -float(S.BIG), dtype=torch.float64, device='cuda')
    for (lo, hi), frames_ in (((0, 12), (0, 3)), ((12, 24), (3, 7))):
        part[0].copy_(torch.from_numpy(cube_set['raw'][lo:hi]))
        part[1].copy_(torch.from_numpy(cube_set['flow'][lo:hi]))
        g2 = block_groups(cube_set['cube_frame'][lo:hi], cube_set['cube_blocks'][lo:hi], 7)
        S.score_store(m['net_set'], m['st_r'], m['st_o'], part, g2, cube_set['boxes'][lo:hi], *common, 4, None, dc, out=out,
                      frame_range=frames_, trainers=trainers, pixel=pc)
    # frame scores: unchanged by the keyword, equal on every route
    assert np.array_equal(fs_0, fs_a) and np.array_equal(fs_0, fs_b) and np.array_equal(fs_0, out.cpu().numpy())
    assert fs_0[1] == -S.BIG and (fs_0 == S.BIG).any()
    # masks: device-painted files = host-painted files
    ma, mb, mc = _load_masks(da, 7), _load_masks(db, 7), _load_masks(dc, 7)
    for f in range(7):
        for other in (mb[f], mc[f]):
            assert type(other) is type(ma[f]) and other.dtype == ma[f].dtype == np.float64 and other.shape == ma[f].shape == (FH, FW)
            assert other.flags['C_CONTIGUOUS'] and np.array_equal(other, ma[f]), f
        assert ma[f].max() == fs_0[f]
    # pixel scores: equal on the three routes, and the k-th largest of the host-painted mask files
    sa, sb, sc = pa.out.cpu().numpy(), pb.out.cpu().numpy(), pc.out.cpu().numpy()
    want = np.array([_kth(ma[f], gt[f], 40) for f in range(7)])
    assert np.array_equal(sa, want) and np.array_equal(sb, want) and np.array_equal(sc, want), (sa, sb, sc, want)
    assert np.array_equal(want[~LABELS], fs_0[~LABELS])                    # a normal frame: the frame score
    assert (want[LABELS] > -S.BIG).sum() >= 2 and (want[LABELS] == -S.BIG).sum() >= 1
    # a label that contradicts the ground truth is an error
    bad = S.PixelEval(lambda i: gt[i], 40, torch.empty(7, dtype=torch.float64, device='cuda'), ~LABELS, False, 64)
    with pytest.raises(ValueError, match='disagree'):
        S.score_store(m['net_set'], m['st_r'], m['st_o'], store, groups, cube_set['boxes'], *common, 4, trainers=trainers, pixel=bad)


# ---- script level ---------------------------------------------------------------------------------------------------------------
def _ped2_tree(rng):
    """A UCSDped2-shaped tree (240x360 grey .tif frames, [h,w,2] flow .npy, box files): 4 + 3 training frames, 4 test frames with
    ground truth on frames 1 and 3.  Frame 1's ground truth lies inside one of its boxes (detected at some threshold), frame 3's far
    from all of its boxes (never detected: pixel score -BIG)."""
    from PIL import Image
    H, W = 240, 360
    test_boxes = [[[200.0, 130.0, 264.0, 194.0], [30.0, 150.0, 70.0, 200.0], [150.2, 30.7, 215.0, 90.0]],
                  [[100.5, 80.5, 160.0, 140.0], [250.0, 20.0, 300.0, 70.0]],
                  [],
                  [[20.0, 20.0, 60.0, 70.0], [220.0, 150.0, 280.0, 210.0]]]
    gts = {1: (slice(100, 120), slice(110, 140)), 3: (slice(100, 120), slice(100, 130))}
    for mode, sub, counts in (('train', 'Train', (4, 3)), ('test', 'Test', (4,))):
        all_boxes = []
        for v, n in enumerate(counts, start=1):
            name = '%s%03d' % (sub, v)
            os.makedirs(os.path.join('raw_datasets', 'UCSDped2', sub, name))
            os.makedirs(os.path.join('optical_flow', 'UCSDped2', sub, name))
            if mode == 'test':
                os.makedirs(os.path.join('raw_datasets', 'UCSDped2', sub, name + '_gt'))
            for k in range(n):
                Image.fromarray(rng.integers(0, 256, (H, W), dtype=np.uint8)).save(
                    os.path.join('raw_datasets', 'UCSDped2', sub, name, '%03d.tif' % (k + 1)))
                np.save(os.path.join('optical_flow', 'UCSDped2', sub, name, '%03d.npy' % (k + 1)),
                        (rng.standard_normal((H, W, 2)) * 2).astype(np.float32))
                if mode == 'test':
                    gt = np.zeros((H, W), np.uint8)
                    if k in gts:
                        gt[gts[k]] = 255
                    Image.fromarray(gt).save(os.path.join('raw_datasets', 'UCSDped2', sub, name + '_gt', '%03d.bmp' % (k + 1)))
                    bb = [b + [0.9] for b in test_boxes[k]]
                else:
                    bb = []
                    for _ in range(3):
                        x0, y0 = rng.uniform(5, W - 70), rng.uniform(5, H - 70)
                        bb.append([x0, y0, x0 + rng.uniform(8, 64), y0 + rng.uniform(8, 64), rng.random()])
                all_boxes.append(np.array(bb).reshape(-1, 5))
        arr = np.empty(len(all_boxes), dtype=object)
        for i, b in enumerate(all_boxes):
            arr[i] = b
        np.save(os.path.join('raw_datasets', 'UCSDped2', 'bboxes_%s_obj_det_with_motion.npy' % mode), arr, allow_pickle=True)


def test_main_pixel_criterion_staged_and_direct(tmp_path, monkeypatch, capsys):
    import train as T
    import test as S
    from utils import frame_roc_auc
    monkeypatch.chdir(tmp_path)
    _ped2_tree(np.random.default_rng(29))
    cfg = small_config()
    res = 'results/UCSDped2/'
    f_scores, p_scores = res + 'frame_scores_obj_det_with_motion_SelfComplete.npy', res + 'pixel_scores_obj_det_with_motion_SelfComplete.npy'
    p_npz = res + 'raw2flow_obj_det_with_motion_SelfComplete_pixel_results.npz'

    def masks():
        return [torch.load(res + 'score_mask/%d' % f, weights_only=False) for f in range(4)]

    T.main('config.cfg')
    auc_off = S.main('config.cfg')                                           # the stock keys: no pixel file
    fs_off, masks_off = np.load(f_scores), masks()
    assert auc_off is not None and not os.path.exists(p_scores) and not os.path.exists(p_npz)
    assert 'Pixel-level' not in capsys.readouterr().out
    on = cfg.replace('pixel_criterion = False', 'pixel_criterion = True')
    got = {}
    for route, text in (('staged', on.replace('test_foreground_saved = False', 'test_foreground_saved = True')),
                        ('direct', on.replace('direct_test = False', 'direct_test = True')
                         .replace('device_score_masks = False', 'device_score_masks = True')
                         .replace('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = 2'))):
        for p in (f_scores, p_scores, p_npz):
            if os.path.exists(p):
                os.remove(p)
        open('config.cfg', 'w').write(text)
        c = T.read_config('config.cfg')
        assert c['pixel_criterion'] and c['direct_test'] == (route == 'direct')
        auc = S.main('config.cfg')
        printed = capsys.readouterr().out
        assert 'Pixel-level AUC (overlap 40%) is ' in printed and 'Pixel-level AUC@ROC (device pair count) is ' in printed
        assert auc == auc_off and np.array_equal(np.load(f_scores), fs_off), route
        for ma, mb in zip(masks_off, masks()):
            assert mb.dtype == ma.dtype and np.array_equal(ma, mb), route
        got[route] = (np.load(p_scores), dict(np.load(p_npz)))
    for p in glob.glob('data/raw2flow/*foreground_test*'):
        os.remove(p)
    ps, npz = got['staged']
    assert ps.shape == (4,) and ps.dtype == np.float64 and np.array_equal(ps, got['direct'][0])
    assert sorted(npz) == sorted(got['direct'][1]) and all(np.array_equal(npz[k], got['direct'][1][k]) for k in npz)
    labels = np.load('data/raw2flow/UCSDped2_frame_labels_test.npy')
    assert labels.tolist() == [False, True, False, True]
    want = np.array([_kth(m, g, 40) for m, g in zip(masks_off, _gt_files())])
    assert np.array_equal(ps, want)
    assert ps[1] > -S.BIG and ps[3] == -S.BIG and fs_off[3] > -S.BIG         # one anomalous frame detected, one never
    assert ps[0] == fs_off[0] and ps[2] == fs_off[2] == -S.BIG               # normal frames: the frame score
    assert abs(float(npz['roc_auc']) - frame_roc_auc(ps, labels)) < 1e-12
    # scores_saved = True: the pixel result comes from the saved file, nothing is scored
    os.remove(p_npz)
    open('config.cfg', 'w').write(on.replace('scores_saved = False', 'scores_saved = True'))

    def scored(*a, **k):
        raise AssertionError('scores_saved = True must not score')

    monkeypatch.setattr(S, 'score_frames', scored)
    monkeypatch.setattr(S, 'score_direct', scored)
    assert S.main('config.cfg') == auc_off
    again = dict(np.load(p_npz))
    assert sorted(again) == sorted(npz) and all(np.array_equal(again[k], npz[k]) for k in npz)


def _gt_files():
    from PIL import Image
    return [np.array(Image.open(p).convert('L')) for p in sorted(glob.glob('raw_datasets/UCSDped2/Test/Test001_gt/*.bmp'))]
