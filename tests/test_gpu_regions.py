"""Region- and track-based detection criteria on the GPU ([mi355x] region_criterion): vv_label_regions, vv_region_match and
vv_region_links against the plain-numpy restatement (tests/region_restatement.py: flood fill, loops over boxes and regions, a threshold
sweep), then the script level (``test.main`` staged and direct).  The outputs are integers and selected doubles, so every comparison
is ``==``; only the two areas under the curves are compared at 1e-12."""
import glob
import os

import numpy as np
import pytest
import torch

from _util import small_config
import region_restatement as R

pytestmark = pytest.mark.gpu

BIG = 100000
SIZES = [(1, 1), (37, 53), (240, 360)]
IDS = ['1x1', '37x53', '240x360']


# ---- labelling ----------------------------------------------------------------------------------------------------------------------
def _spiral(h, w):
    """A one-pixel wide rectangular spiral from the top-left corner inwards, one blank pixel between its arms."""
    g = np.zeros((h, w), np.uint8)
    y = x = 0
    g[0, 0] = 1
    lens = [w - 1, h - 1, w - 1]
    a, b = h - 3, w - 3
    while a > 0 and b > 0:
        lens += [a, b]
        a, b = a - 2, b - 2
    for i, n in enumerate(lens):
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[i % 4]
        for _ in range(n):
            y, x = y + dy, x + dx
            g[y, x] = 1
    return g


def _label_frames(h, w):
    """uint8 ``[7,h,w]``: a spiral; empty; full; a "U" with a diagonal and an anti-diagonal chain inside it; regions on all four borders
    and corners; exactly 64 isolated pixels; overlapping and touching rectangles with values 1 and 255."""
    gt = np.zeros((7, h, w), np.uint8)
    if h * w == 1:
        gt[[0, 2, 5]] = 255
        return gt
    rng = np.random.default_rng(h)
    gt[0] = _spiral(h, w) * 255
    gt[2] = 1
    gt[3, 2:h - 2, 3] = gt[3, 2:h - 2, w - 4] = gt[3, h - 3, 3:w - 3] = 7          # the "U": its arms meet only in the last rows
    for i in range(10):
        gt[3, 4 + i, 6 + i] = 1                                                   # joined only diagonally (NW-SE) ...
        gt[3, 4 + i, 32 - i] = 1                                                  # ... and NE-SW
    gt[4, 0, 5:8] = gt[4, h - 1, 10:12] = gt[4, 6:9, 0] = gt[4, 12:14, w - 1] = 255
    gt[4, 0, 0] = gt[4, 0, w - 1] = gt[4, h - 1, 0] = gt[4, h - 1, w - 1] = 1
    gt[5, 1:32:4, 2:34:4] = 255                                                   # 8 x 8 isolated pixels
    for _ in range(10):
        y0, x0 = int(rng.integers(0, h - 3)), int(rng.integers(0, w - 3))
        gt[6, y0:y0 + int(rng.integers(1, h // 3)), x0:x0 + int(rng.integers(1, w // 3))] = (1, 255)[int(rng.integers(0, 2))]
    return gt


def _raw_label(gt):
    """vv_label_regions itself (no cap check): (labels, n_regions) as numpy."""
    from vec_vad_amd import _lib
    g = torch.from_numpy(np.ascontiguousarray(gt)).cuda()
    F, h, w = g.shape
    labels = torch.full((F, h, w), -7, dtype=torch.int32, device='cuda')
    cnt = torch.full((F,), -7, dtype=torch.int32, device='cuda')
    st = _lib.lib().vv_label_regions(g.data_ptr(), labels.data_ptr(), cnt.data_ptr(), F, h, w, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0
    return labels.cpu().numpy(), cnt.cpu().numpy()


@pytest.fixture(scope='module')
def label_scenes():
    out = {}
    for h, w in SIZES:
        gt = _label_frames(h, w)
        out[(h, w)] = (gt,) + R.label_frames(gt)
    return out


@pytest.mark.parametrize('h,w', SIZES, ids=IDS)
def test_labels_are_the_flood_fill_in_raster_order(label_scenes, h, w):
    from vec_vad_amd import scoring
    gt, want, want_n = label_scenes[(h, w)]
    if h > 1:
        assert want_n.tolist()[:6] == [1, 0, 1, 3, 8, 64]                          # one spiral; nothing; everything; U + 2 chains; ...
    labels, n = scoring.label_regions(gt)                                          # F = 7, host ground truth uploaded
    assert labels.dtype == torch.int32 and n.dtype == torch.int32 and tuple(labels.shape) == (7, h, w) and tuple(n.shape) == (7,)
    assert np.array_equal(n.cpu().numpy(), want_n) and np.array_equal(labels.cpu().numpy(), want)
    again, n2 = scoring.label_regions(torch.from_numpy(gt).cuda())                 # bit-identical run to run
    assert torch.equal(again, labels) and torch.equal(n2, n)
    for f in range(7):                                                             # F = 1: every frame on its own
        one, n1 = scoring.label_regions(gt[f:f + 1])
        assert np.array_equal(one.cpu().numpy(), want[f:f + 1]) and n1.tolist() == [int(want_n[f])], f
    empty, n0 = scoring.label_regions(np.zeros((0, h, w), np.uint8))
    assert tuple(empty.shape) == (0, h, w) and tuple(n0.shape) == (0,)


def test_labels_of_noise_with_more_regions_than_the_cap():
    """Dense noise makes the union-find join labels from everywhere; the count is the true one far above the cap and the labels are
    still the raster ranks.  The wrapper refuses the frame by name."""
    from vec_vad_amd import scoring
    rng = np.random.default_rng(2)
    gt = np.stack([(rng.random((37, 53)) < p).astype(np.uint8) for p in (0.45, 0.2, 0.6, 0.3)])      # round the percolation threshold
    want, want_n = R.label_frames(gt)
    assert want_n[1] > 64 and want_n[3] > 64
    labels, n = _raw_label(gt)
    assert np.array_equal(n, want_n) and np.array_equal(labels, want)
    first = int(np.nonzero(want_n > 64)[0][0])
    with pytest.raises(ValueError, match='frame %d has %d ground-truth regions' % (10 + first, want_n[first])) as e:
        scoring.label_regions(gt, frame0=10)
    assert '\n' not in str(e.value)


def test_64_isolated_pixels_are_accepted_and_65_refused():
    from vec_vad_amd import scoring
    gt = np.zeros((3, 37, 53), np.uint8)
    gt[:, 1:32:4, 2:34:4] = 1
    gt[1, 36, 52] = 1                                                              # the 65th, last in raster order
    labels, n = _raw_label(gt)
    assert n.tolist() == [64, 65, 64] and labels[1, 36, 52] == 65 and labels[1, 1, 2] == 1
    ok, n_ok = scoring.label_regions(gt[[0, 2]])
    assert n_ok.tolist() == [64, 64] and int(ok.max()) == 64
    with pytest.raises(ValueError, match='frame 1 has 65 ground-truth regions') as e:
        scoring.label_regions(gt)
    assert '\n' not in str(e.value)


# ---- match --------------------------------------------------------------------------------------------------------------------------
NAMED = dict(bbox=0, inside=1, contains_far=2, contains=3, touch=4, on_bound=5, short=6, empty_a=7, empty_b=8)


def _match_scene(h, w):
    """Ground truth, rectangles ((y0, y1, x0, x1) rows), scores and the CSR of 7 frames: the named boxes above on frame 0; one box over
    two regions on frame 1; ground truth without boxes; boxes without ground truth; 3000 boxes on frame 4; nothing; random."""
    rng = np.random.default_rng(100 + h)
    gt = np.zeros((7, h, w), np.uint8)
    gt[0, 5:10, 5:15] = 255                       # region 1 of frame 0: 50 pixels
    gt[0, 20, 5:15] = 1                           # region 2: 10 pixels
    rects0 = [(5, 10, 5, 15),                     # the region's bounding box: IoU 1
              (6, 8, 6, 9),                       # wholly inside: 6 / 50
              (0, 20, 0, 30),                     # wholly contains, 600 pixels: 50 / 600 < 10 %
              (3, 12, 3, 17),                     # wholly contains, 126 pixels: 50 / 126
              (9, 14, 14, 20),                    # touches region 1 in the one pixel (9, 14): 1 / 79
              (16, 26, 5, 15),                    # 100 pixels round the 10 of region 2: 100 * 10 == 10 * 100, on the bound
              (16, 26, 6, 16),                    # one pixel short: 9 of them, 900 < 10 * 101
              (5, 5, 3, 9), (7, 3, 2, 8)]         # empty rectangles
    scores0 = [1.0, 5.0, 9.0, 3.0, 8.0, -2.5, 7.0, 2.0 * BIG, 2.0 * BIG]
    gt[1, 5:8, 5:8] = gt[1, 5:8, 10:13] = 255
    rects1, scores1 = [(5, 8, 5, 13)], [0.25]     # one box over two regions: 9 / 24 each
    gt[2, 11:14, 20:29] = 1
    rects3, scores3 = [(1, 9, 1, 9), (12, 30, 20, 50), (4, 4, 4, 4)], [0.5, -0.5, 1.0]
    side = max(8, h // 4)
    for k in range(8):
        y0, x0 = int(rng.integers(0, h - side)), int(rng.integers(0, w - side))
        gt[4, y0:y0 + int(rng.integers(2, side)), x0:x0 + int(rng.integers(2, side))] = 255

    def random_rects(n):
        y0, x0 = rng.integers(0, h, n), rng.integers(0, w, n)
        y1 = np.minimum(h, y0 + rng.integers(0, max(2, h // 3), n))
        x1 = np.minimum(w, x0 + rng.integers(0, max(2, w // 3), n))
        return np.stack([y0, y1, x0, x1], 1).tolist(), np.round(rng.standard_normal(n) * 3, 1).tolist()

    rects4, scores4 = random_rects(3000)
    gt[6] = gt[4][::-1, ::-1]
    gt[6, h // 2:h // 2 + 9, w // 3:w // 3 + 14] = 1
    rects6, scores6 = random_rects(70)
    per = [(rects0, scores0), (rects1, scores1), ([], []), (rects3, scores3), (rects4, scores4), ([], []), (rects6, scores6)]
    off = np.concatenate([[0], np.cumsum([len(r) for r, _ in per])]).astype(np.int32)
    rects = np.array([r for rs, _ in per for r in rs], np.int32).reshape(-1, 4)
    scores = np.array([s for _, ss in per for s in ss], np.float64)
    labels, n = R.label_frames(gt)
    assert n.max() <= 64
    return dict(gt=gt, labels=labels, n=n, off=off, rects=rects, scores=scores)


@pytest.fixture(scope='module')
def match_scenes():
    return {(h, w): _match_scene(h, w) for (h, w) in SIZES[1:]}


@pytest.mark.parametrize('F', [1, 7])
@pytest.mark.parametrize('h,w', SIZES[1:], ids=IDS[1:])
def test_region_match_equals_the_loops(match_scenes, h, w, F):
    from vec_vad_amd import scoring
    sc = match_scenes[(h, w)]
    off = sc['off'][:F + 1]
    n = int(off[-1])
    labels = torch.from_numpy(sc['labels'][:F]).cuda()
    scores, rects = torch.from_numpy(sc['scores'][:n]).cuda(), sc['rects'][:n]
    for pct in (10, 1, 100, 39):
        area, best, state = scoring.region_match(labels, scores, off, rects, pct)
        assert area.dtype == torch.int32 and best.dtype == torch.float64 and state.dtype == torch.uint8
        assert tuple(area.shape) == tuple(best.shape) == (F, 64) and tuple(state.shape) == (n,)
        w_area, w_best, w_state = R.match(sc['labels'][:F], sc['scores'][:n], off, rects, pct)
        assert np.array_equal(area.cpu().numpy(), w_area), pct
        assert np.array_equal(state.cpu().numpy(), w_state), (pct, np.nonzero(state.cpu().numpy() != w_state)[0][:10])
        assert np.array_equal(best.cpu().numpy(), w_best), pct
        again = scoring.region_match(labels, scores, off, rects, pct)
        assert all(torch.equal(x, y) for x, y in zip(again, (area, best, state)))      # bit-identical run to run
        if pct == 10:                                                                  # the named cases do what their names say
            st = w_state[:9].tolist()
            assert st == [1, 1, 2, 1, 2, 1, 2, 0, 0], st
            assert w_area[0, :3].tolist() == [50, 10, 0]
            assert w_best[0, 0] == 5.0 and w_best[0, 1] == -2.5                        # the larger score wins; on the bound counts
            assert w_best[0, 2] == -BIG
            if F == 7:
                assert w_state[9] == 1 and w_best[1, 0] == w_best[1, 1] == 0.25        # one box over two regions
                assert w_best[2, 0] == -BIG and sc['n'][2] == 1                        # ground truth, no box
                assert w_state[10:13].tolist() == [2, 2, 0] and sc['n'][3] == 0        # boxes, no ground truth: false positives
                big = w_state[13:3013]
                assert (big == 0).any() and (big == 1).any() and (big == 2).any()      # 3000 boxes of every kind
        if pct == 1:
            assert w_state[NAMED['touch']] == 1 and w_state[NAMED['contains_far']] == 1
        if pct == 100:
            assert w_state[:9].tolist() == [1, 2, 2, 2, 2, 2, 2, 0, 0]
    for bad in (0, 101, 10.5):
        with pytest.raises(ValueError):
            scoring.region_match(labels, scores, off, rects, bad)


def test_region_match_on_one_pixel_and_on_nothing():
    from vec_vad_amd import scoring
    labels = torch.tensor([[[1]], [[0]]], dtype=torch.int32, device='cuda')
    scores = torch.tensor([2.0, 3.0, 4.0], dtype=torch.float64, device='cuda')
    rects = np.array([[0, 1, 0, 1], [0, 0, 0, 1], [0, 1, 0, 1]], np.int32)
    area, best, state = scoring.region_match(labels, scores, np.array([0, 2, 3], np.int32), rects, 100)
    assert state.tolist() == [1, 0, 2] and area[:, 0].tolist() == [1, 0] and best[:, 0].tolist() == [2.0, -BIG]
    # no frame; frames without any box
    area, best, state = scoring.region_match(labels[:0], scores[:0], np.zeros(1, np.int32), rects[:0], 10)
    assert tuple(area.shape) == (0, 64) and tuple(state.shape) == (0,)
    area, best, state = scoring.region_match(labels, scores[:0], np.zeros(3, np.int32), rects[:0], 10)
    assert area[:, 0].tolist() == [1, 0] and bool((best == -BIG).all()) and tuple(state.shape) == (0,)


# ---- links --------------------------------------------------------------------------------------------------------------------------
def _moving_labels(h, w):
    """Labels of 7 frames: a blob that moves 3 pixels per frame (a chain), a bar that splits in two at frame 3 and a pixel that never
    moves; at 37 x 53 they also cross the 2048-position tiles of the link kernel's grid at 240 x 360."""
    gt = np.zeros((7, h, w), np.uint8)
    for f in range(7):
        gt[f, 4:9, 2 + 3 * f:8 + 3 * f] = 255
        if f < 3:
            gt[f, 20:23, 10:30] = 1
        else:
            gt[f, 20:23, 10:18] = gt[f, 20:23, 22:30] = 1
        gt[f, h - 1, w - 1] = 1
    gt[5, 4:9, :] = 0                                          # the blob is missing in frame 5: its track breaks
    return R.label_frames(gt)[0]


@pytest.mark.parametrize('h,w', SIZES[1:], ids=IDS[1:])
def test_region_links_whole_and_in_chunks(h, w):
    from vec_vad_amd import scoring
    lab = _moving_labels(h, w)
    dev = torch.from_numpy(lab).cuda()
    same = np.array([1, 1, 1, 1, 0, 1, 1], np.uint8)           # frame 4 starts another video
    for sv in (None, same):
        want = R.links(lab, None, np.ones(7) if sv is None else sv)
        whole = scoring.region_links(dev, None, sv)
        assert whole.dtype == torch.int64 and tuple(whole.shape) == (7, 64)
        assert np.array_equal(whole.cpu().numpy().view(np.uint64), want)
        a = scoring.region_links(dev[:3], None, None if sv is None else sv[:3])
        b = scoring.region_links(dev[3:], dev[2].clone(), None if sv is None else sv[3:])
        assert torch.equal(torch.cat([a, b]), whole)           # [0,3) + [3,7) with the label map carried
    assert want[3, 1] == want[3, 2] == 2 and want[1, 0] == 1   # both halves of the split bar link to the bar
    assert (want[4] == 0).all() and (want[0] == 0).all() and want[5].tolist().count(0) == 64 - 3      # cut; no frame before; blob missing
    # frame 0 with a frame before it, in F = 1 calls; same_video = 0 on frame 0 cuts that link too
    one = scoring.region_links(dev[1:2], dev[0].clone(), None)
    assert np.array_equal(one.cpu().numpy().view(np.uint64), R.links(lab[1:2], lab[0], [1]))
    assert int(scoring.region_links(dev[1:2], dev[0].clone(), [0]).abs().sum()) == 0
    none = scoring.region_links(dev[:0], None, None)           # F == 0
    assert tuple(none.shape) == (0, 64)
    # bit 63: 64 regions in both frames
    g = np.zeros((2, 37, 53), np.uint8)
    g[:, 1:32:4, 2:34:4] = 1
    l64 = R.label_frames(g)[0]
    got = scoring.region_links(torch.from_numpy(l64).cuda(), None, None).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, R.links(l64, None, [1, 1])) and got[1, 63] == np.uint64(1) << np.uint64(63)


def test_bad_arguments_are_statuses_and_empty_shapes_are_ok():
    from vec_vad_amd import _lib
    l = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    gt = torch.zeros((2, 4, 5), dtype=torch.uint8, device='cuda')
    lab = torch.full((2, 4, 5), 9, dtype=torch.int32, device='cuda')
    cnt = torch.full((2,), 9, dtype=torch.int32, device='cuda')
    sc = torch.zeros(3, dtype=torch.float64, device='cuda')
    off = torch.tensor([0, 1, 3], dtype=torch.int32, device='cuda')
    rc = torch.zeros((3, 4), dtype=torch.int32, device='cuda')
    area = torch.full((2, 64), 9, dtype=torch.int32, device='cuda')
    best = torch.full((2, 64), 9.0, dtype=torch.float64, device='cuda')
    state = torch.full((3,), 9, dtype=torch.uint8, device='cuda')
    same = torch.ones(2, dtype=torch.uint8, device='cuda')
    links = torch.full((2, 64), 9, dtype=torch.int64, device='cuda')
    g, L, c, s, o, r, A, B, S, V, K = (t.data_ptr() for t in (gt, lab, cnt, sc, off, rc, area, best, state, same, links))
    BAD, OK = 1, 0
    assert l.vv_label_regions(None, L, c, 2, 4, 5, st) == BAD and l.vv_label_regions(g, None, c, 2, 4, 5, st) == BAD
    assert l.vv_label_regions(g, L, None, 2, 4, 5, st) == BAD
    assert l.vv_label_regions(g, L, c, -1, 4, 5, st) == BAD and l.vv_label_regions(g, L, c, 2, -4, 5, st) == BAD
    assert l.vv_label_regions(g, L, c, 2, 65536, 32768, st) == BAD                 # h * w = 2^31
    assert l.vv_label_regions(None, None, None, 0, 4, 5, st) == OK                 # F == 0
    for pct in (0, 101, -3):
        assert l.vv_region_match(L, s, o, r, pct, float(BIG), 2, 4, 5, 3, A, B, S, st) == BAD
    assert l.vv_region_match(None, s, o, r, 10, float(BIG), 2, 4, 5, 3, A, B, S, st) == BAD
    assert l.vv_region_match(L, None, o, r, 10, float(BIG), 2, 4, 5, 3, A, B, S, st) == BAD
    assert l.vv_region_match(L, s, None, r, 10, float(BIG), 2, 4, 5, 3, A, B, S, st) == BAD
    assert l.vv_region_match(L, s, o, None, 10, float(BIG), 2, 4, 5, 3, A, B, S, st) == BAD
    assert l.vv_region_match(L, s, o, r, 10, float(BIG), 2, 4, 5, 3, None, B, S, st) == BAD
    assert l.vv_region_match(L, s, o, r, 10, float(BIG), 2, 4, 5, 3, A, None, S, st) == BAD
    assert l.vv_region_match(L, s, o, r, 10, float(BIG), 2, 4, 5, 3, A, B, None, st) == BAD
    assert l.vv_region_match(L, s, o, r, 10, float(BIG), 2, 4, 5, -1, A, B, S, st) == BAD
    assert l.vv_region_match(L, s, o, r, 10, float(BIG), -2, 4, 5, 3, A, B, S, st) == BAD
    assert l.vv_region_match(L, s, o, r, 10, float(BIG), 2, 65536, 32768, 3, A, B, S, st) == BAD
    assert l.vv_region_match(None, None, None, None, 10, float(BIG), 0, 4, 5, 0, None, None, None, st) == OK
    assert l.vv_region_links(None, None, V, 2, 4, 5, K, st) == BAD and l.vv_region_links(None, L, None, 2, 4, 5, K, st) == BAD
    assert l.vv_region_links(None, L, V, 2, 4, 5, None, st) == BAD and l.vv_region_links(None, L, V, -1, 4, 5, K, st) == BAD
    assert l.vv_region_links(None, L, V, 2, 4, -5, K, st) == BAD and l.vv_region_links(None, L, V, 2, 65536, 32768, K, st) == BAD
    assert l.vv_region_links(None, None, None, 0, 4, 5, None, st) == OK
    torch.cuda.synchronize()
    for t in (lab, cnt, area, state, links):                                       # nothing was launched, nothing written
        assert bool((t == 9).all())
    assert bool((best == 9.0).all())
    # empty shapes with frames: h * w == 0 (no pixel to read, NULL maps allowed) and n == 0 (NULL box arrays allowed)
    assert l.vv_label_regions(None, None, c, 2, 0, 5, st) == OK
    assert l.vv_region_match(None, None, torch.zeros(3, dtype=torch.int32, device='cuda').data_ptr(), None, 10, float(BIG), 2, 0, 5, 0,
                             A, B, None, st) == OK
    assert l.vv_region_links(None, None, V, 2, 4, 0, K, st) == OK
    torch.cuda.synchronize()
    assert cnt.tolist() == [0, 0] and bool((area == 0).all()) and bool((best == -BIG).all()) and bool((links == 0).all())


# ---- script level -------------------------------------------------------------------------------------------------------------------
TEST_VIDEOS = (4, 3)                  # frames of Test001, Test002


def _blob(k):
    """The ground-truth blob of test frame ``k`` (0..6), or None: it moves 10 columns per frame through frames 1-3 of the first video
    (one track of three regions) and stands where it stopped in frames 4-5, the first two of the second video (a track of its own)."""
    if k in (1, 2, 3):
        return slice(100, 120), slice(100 + 10 * k, 130 + 10 * k)
    if k in (4, 5):
        return slice(100, 120), slice(130, 160)
    return None


def _ped2_tree(rng):
    """A UCSDped2-shaped tree in the manner of tests/test_gpu_pixel_criterion.py (240x360 grey .tif frames, [h,w,2] flow .npy, box
    files): 4 + 3 training frames, two test videos of 4 + 3 frames with the moving blob above and at most 3 boxes per frame."""
    from PIL import Image
    H, W = 240, 360
    found = [100.5, 80.5, 160.0, 140.0]               # rows 81..139, columns 101..159: holds the blob of frames 1 and 2, IoU 600 / 3481
    test_boxes = [[[200.0, 130.0, 264.0, 194.0], [30.0, 150.0, 70.0, 200.0]],
                  [found, [250.0, 20.0, 300.0, 70.0]],
                  [found],
                  [[20.0, 20.0, 60.0, 70.0], [220.0, 150.0, 280.0, 210.0], [10.0, 170.0, 50.0, 230.0]],
                  [[118.2, 90.7, 172.0, 131.0]],      # rows 91..130, columns 119..171: holds the standing blob
                  [],
                  [[20.0, 20.0, 60.0, 70.0]]]
    k_test = 0
    for mode, sub, counts in (('train', 'Train', (4, 3)), ('test', 'Test', TEST_VIDEOS)):
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
                    if _blob(k_test) is not None:
                        gt[_blob(k_test)] = 255
                    Image.fromarray(gt).save(os.path.join('raw_datasets', 'UCSDped2', sub, name + '_gt', '%03d.bmp' % (k + 1)))
                    bb = [b + [0.9] for b in test_boxes[k_test]]
                    k_test += 1
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


def _gt_files():
    from PIL import Image
    return np.stack([np.array(Image.open(p).convert('L')) for p in sorted(glob.glob('raw_datasets/UCSDped2/Test/Test*_gt/*.bmp'))])


def _same_npz(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_main_region_criterion_staged_and_direct(tmp_path, monkeypatch, capsys):
    import train as T
    import test as S
    from vec_vad_amd import scoring
    monkeypatch.chdir(tmp_path)
    _ped2_tree(np.random.default_rng(31))
    # one cube per launch on every route: a part of 3 cubes then launches the shapes the whole set does, which is what makes cube
    # scores equal bit for bit between the routes (launches of other sizes may re-associate fp32 sums)
    cfg = small_config().replace('score_batch = 2048', 'score_batch = 1')
    assert T.read_config('config.cfg')['score_batch'] == 2048
    open('config.cfg', 'w').write(cfg)
    res = 'results/UCSDped2/'
    tag = 'obj_det_with_motion_SelfComplete'
    f_scores, p_scores, r_scores = res + 'frame_scores_%s.npy' % tag, res + 'pixel_scores_%s.npy' % tag, res + 'region_scores_%s.npz' % tag
    r_npz = res + 'raw2flow_%s_region_results.npz' % tag
    n = sum(TEST_VIDEOS)

    def masks():
        return [torch.load(res + 'score_mask/%d' % f, weights_only=False) for f in range(n)]

    def same_masks(a, b):
        return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))

    def direct(text):
        return (text.replace('direct_test = False', 'direct_test = True').replace('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = 2')
                .replace('direct_max_cubes = 524288', 'direct_max_cubes = 3'))

    T.main('config.cfg')
    pix = cfg.replace('pixel_criterion = False', 'pixel_criterion = True')
    base = {}
    for route, text in (('direct', direct(cfg)), ('staged', pix)):         # region_criterion = False: no region file appears
        open('config.cfg', 'w').write(text)
        auc_off = S.main('config.cfg')
        base[route] = (auc_off, open(f_scores, 'rb').read(), masks())
        assert auc_off is not None and not os.path.exists(r_scores) and not os.path.exists(r_npz)
        out = capsys.readouterr().out
        assert 'RBDC' not in out and 'TBDC' not in out
    ps_off = open(p_scores, 'rb').read()
    print('frame scores, staged minus direct in parts:', np.load(f_scores) - np.frombuffer(base['direct'][1][-8 * n:], np.float64))

    # what the region stage is handed, chunk by chunk, kept for the restatement
    seen = []
    stage = S.PixelEval.region_stage

    def recording(self, gt, off, scores, rects, a, b):
        seen[-1].append((a, b, np.array(off), scores.cpu().numpy(), rects.cpu().numpy()))
        return stage(self, gt, off, scores, rects, a, b)

    monkeypatch.setattr(S.PixelEval, 'region_stage', recording)
    on = pix.replace('region_criterion = False', 'region_criterion = True')
    got = {}
    for route, text in (('staged', on.replace('test_foreground_saved = False', 'test_foreground_saved = True')),
                        ('direct', direct(on.replace('pixel_criterion = True', 'pixel_criterion = False')))):
        for p in (f_scores, p_scores, r_scores, r_npz):
            if os.path.exists(p):
                os.remove(p)
        open('config.cfg', 'w').write(text)
        c = T.read_config('config.cfg')
        assert c['region_criterion'] and c['direct_test'] == (route == 'direct') and c['pixel_criterion'] == (route == 'staged')
        assert c['direct_max_cubes'] == (3 if route == 'direct' else 524288)
        seen.append([])
        auc = S.main('config.cfg')
        printed = capsys.readouterr().out
        assert 'RBDC (IoU 10%) is ' in printed and 'TBDC (IoU 10%, 10% of a track) is ' in printed
        assert 'derived from the per-pixel ground truth' in printed
        # frame scores, score_mask files and pixel scores: byte for byte those of the same run without the key
        auc_off, fs_off, masks_off = base[route]
        assert auc == auc_off and open(f_scores, 'rb').read() == fs_off and same_masks(masks(), masks_off), route
        if route == 'staged':
            assert open(p_scores, 'rb').read() == ps_off
        else:
            assert not os.path.exists(p_scores)                            # the region key alone writes no pixel file
        got[route] = (dict(np.load(r_scores)), dict(np.load(r_npz)))
    for p in glob.glob('data/raw2flow/*foreground_test*'):
        os.remove(p)
    assert len(seen[0]) == 1 and len(seen[1]) >= 4                         # one chunk staged; chunks of 2 frames in parts of 3 cubes direct
    state, curves = got['staged']
    assert _same_npz(state, got['direct'][0]) and _same_npz(curves, got['direct'][1])    # chunks and parts change nothing
    assert sorted(state) == ['fp_score', 'n_frames', 'region_area', 'region_frame', 'region_score', 'region_track', 'track_score']
    assert sorted(curves) == ['fpr', 'rbdc', 'rbdr', 'tbdc', 'tbdr']

    # the restatement, fed with the staged run's cube scores and rectangles and with the ground-truth FILES
    (a, b, off, scores, rects), = seen[0]
    assert (a, b) == (0, n)
    gt = _gt_files()
    labels, n_reg = R.label_frames(gt)
    assert n_reg.tolist() == [0, 1, 1, 1, 1, 1, 0]
    w_area, w_best, w_state = R.match(labels, scores, off, rects, 10)
    video = np.repeat(np.arange(len(TEST_VIDEOS)), TEST_VIDEOS)
    same = np.concatenate([[0], video[1:] == video[:-1]])
    track, k = R.tracks(n_reg, R.links(labels, None, same), 10)
    pick = np.arange(64)[None, :] < n_reg[:, None]
    assert np.array_equal(state['region_score'], w_best[pick]) and np.array_equal(state['region_area'], w_area[pick])
    assert state['region_area'].tolist() == [600] * 5
    assert state['region_frame'].tolist() == [1, 2, 3, 4, 5] and int(state['n_frames']) == n
    assert state['region_track'].tolist() == track.tolist() == [0, 0, 0, 1, 1]          # the video boundary cuts the track
    assert np.array_equal(state['fp_score'], np.sort(scores[w_state == 2])[::-1])
    det = state['region_score'] > -BIG
    assert det.tolist() == [True, True, False, True, False]                # found on frames 1, 2 and 4; missed on 3 and 5
    assert len(state['fp_score']) == int((w_state == 2).sum()) >= 5 and (w_state == 0).sum() == 0
    thr, w_fpr, w_rbdr, w_tbdr, w_rbdc, w_tbdc = R.sweep(w_best[pick], track, k, scores[w_state == 2], n)
    assert np.array_equal(state['track_score'], [sorted(w_best[pick][track == t], reverse=True)[k[t] - 1] for t in range(2)])
    assert curves['fpr'][1:].tolist() == w_fpr and curves['rbdr'][1:].tolist() == w_rbdr and curves['tbdr'][1:].tolist() == w_tbdr
    assert abs(float(curves['rbdc']) - w_rbdc) < 1e-12 and abs(float(curves['tbdc']) - w_tbdc) < 1e-12
    assert 0.0 <= float(curves['rbdc']) <= 0.6 + 1e-12 and 0.0 <= float(curves['tbdc']) <= 1.0      # 3 of the 5 regions are ever found

    # scores_saved = True: the curves are recomputed from the saved region file, nothing is scored
    os.remove(r_npz)
    open('config.cfg', 'w').write(on.replace('pixel_criterion = True', 'pixel_criterion = False')
                                  .replace('scores_saved = False', 'scores_saved = True'))

    def scored(*a, **k):
        raise AssertionError('scores_saved = True must not score')

    monkeypatch.setattr(S, 'score_frames', scored)
    monkeypatch.setattr(S, 'score_direct', scored)
    monkeypatch.setattr(scoring, 'label_regions', scored)
    assert S.main('config.cfg') == base['direct'][0]
    assert _same_npz(dict(np.load(r_npz)), curves)
