"""Per-pixel anomaly maps on the GPU ([mi355x] pixel_maps): vv_error_maps against a float64 restatement (the float-summation bar of
tests/_util.py), the bank / trainer level (``FusedTrainer.score_cubes(maps=True)``), then vv_error_zmaps, vv_paint_zmaps and
vv_mask_kth, which form, select and copy doubles and are compared with ``==`` against tests/pixel_maps_restatement.py, their tie to
the kernels of the painted masks, and ``test.main`` on a synthetic UCSDped2 tree, staged and direct."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

import pixel_maps_restatement as R
from _util import SENT, bar, gen, small_config

pytestmark = pytest.mark.gpu

BIG = R.BIG
SIZES = [(37, 53), (1, 1), (240, 360)]          # odd h*w with a ragged tail; one pixel; the UCSDped2 frame
IDS = ['37x53', '1x1', '240x360']
STATS = np.array([[20.0, 7.5, 4.0, 1.25], [25.0, 3.0, 5.0, 2.0]])


# ---- 1. vv_error_maps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('G', [6, 2])
def test_error_maps_against_float64(G, B):
    from vec_vad_amd import _lib
    HW, C0, C1 = 1024, 15, 2
    M = B * HW
    if G == 6:
        oc, tsrc, tcoff = [3, 3, 3, 3, 3, 2], [0, 0, 0, 0, 0, 1], [0, 3, 6, 9, 12, 0]
    else:                                        # raw UNets only, no flow map asked for
        oc, tsrc, tcoff = [3, 3], [0, 0], [3, 12]
    flow = G == 6
    g = gen(41, G, B)
    out4 = torch.randn(G, M, 4, generator=g) * 0.3 + 0.5
    tgt0 = torch.rand(M, C0, generator=g)
    tgt1 = torch.randn(M, C1, generator=g) * 2
    for k in range(G):
        out4[k, :, oc[k]:] = 0.0                 # as vv_outconv_fwd stores it
    e64 = R.error_maps(out4.numpy(), oc, tsrc, tcoff, tgt0.numpy(), tgt1.numpy(), np.float64, flow)
    e32 = R.error_maps(out4.numpy(), oc, tsrc, tcoff, tgt0.numpy(), tgt1.numpy(), np.float32, flow)
    dev = lambda a: torch.tensor(a, dtype=torch.int32, device='cuda')
    oc_d, ts_d, tc_d = dev(oc), dev(tsrc), dev(tcoff)
    o4, t0, t1 = out4.cuda(), tgt0.cuda(), tgt1.cuda()
    e_raw = torch.full((M + 64,), SENT, device='cuda')
    e_of = torch.full((M + 64,), SENT, device='cuda')
    _lib.check(_lib.lib().vv_error_maps(G, B, HW, o4.data_ptr(), oc_d.data_ptr(), ts_d.data_ptr(), tc_d.data_ptr(), t0.data_ptr(), C0,
                                        t1.data_ptr() if flow else None, C1, e_raw.data_ptr(), e_of.data_ptr() if flow else None,
                                        torch.cuda.current_stream().cuda_stream), 'vv_error_maps')
    torch.cuda.synchronize()
    assert bool((e_raw[M:] == SENT).all()) and bool((e_of[M if flow else 0:] == SENT).all())      # nothing behind the outputs
    bar('error_maps', 'e_raw G%d B%d' % (G, B), e_raw[:M], torch.from_numpy(e64[0]), torch.from_numpy(e32[0]), family='pixel_maps')
    if flow:
        bar('error_maps', 'e_of G%d B%d' % (G, B), e_of[:M], torch.from_numpy(e64[1]), torch.from_numpy(e32[1]), family='pixel_maps')
        assert e64[1].max() > 0
    assert e64[0].max() > 0


# ---- 2. bank level ------------------------------------------------------------------------------------------------------------
def _net(kind, seed=0):
    from oracle import unet_oracle as O
    from model.unet import SelfCompleteNet4, SelfCompleteNetFull
    cls, tot_of = {'net4': (SelfCompleteNet4, 1), 'full': (SelfCompleteNetFull, 5)}[kind]
    net = cls(features_root=32, tot_raw_num=5, tot_of_num=tot_of, border_mode='predict', rawRange=None, useFlow=True, padding=False)
    net.load_state_dict(O.seeded_state_dict(kind, nf=32, padding=False, seed=seed))
    return net.cuda().eval(), tot_of


def _seq32(a):
    """sum over the channel axis (1), one channel after the other, in the dtype of ``a``"""
    acc = torch.zeros_like(a[:, 0])
    for c in range(a.shape[1]):
        acc = acc + a[:, c]
    return acc


@pytest.mark.parametrize('kind,n,precision', [('net4', 5, 'fp32'), ('full', 3, 'fp32'), ('net4', 5, 'bf16')],
                         ids=['net4', 'full', 'net4-bf16'])
def test_score_cubes_with_maps(kind, n, precision, monkeypatch):
    from oracle import unet_oracle as O
    from vec_vad_amd.trainer import FusedTrainer
    monkeypatch.setenv('VV_PRECISION', precision)
    net, tot_of = _net(kind)
    assert net.bank().precision == precision
    raw, flow = O.seeded_cubes(2 * n, tot_of, 7)
    raw_d, flow_d = torch.from_numpy(raw).cuda(), torch.from_numpy(flow).cuda()
    tr = FusedTrainer(net)
    halves = [torch.arange(0, n, device='cuda'), torch.arange(n, 2 * n, device='cuda')]
    plain = [tuple(t.clone() for t in tr.score_cubes(raw_d, flow_d, i)) for i in halves]
    with pytest.raises(RuntimeError, match='did not store the reconstructions'):
        net.bank().error_maps(net.bank().workspace(n))
    # four calls: the eager one, the one that captures, two replays -- every one on other cubes than the one before
    got, kept = [], []
    for call in range(4):
        out = tr.score_cubes(raw_d, flow_d, halves[call % 2], maps=True)
        assert len(out) == 4 and tuple(out[2].shape) == tuple(out[3].shape) == (n, 32, 32) and out[2].dtype == torch.float32
        got.append(out)
        kept.append(tuple(t.clone() for t in out))
    if tr._graph_ok():                                                               # a capture of its own next to the plain one
        assert all(type(tr._graphs[(k, n, raw_d.data_ptr(), flow_d.data_ptr())]) is not str for k in ('eval', 'eval_maps'))
    for call in range(4):
        for a, b in zip(got[call], kept[call]):
            assert torch.equal(a, b), call                                           # no later call wrote into what this one returned
        for a, b in zip(got[call][:2], plain[call % 2]):
            assert torch.equal(a, b), call                                           # r, o: the bits of the plain call
        for a, b in zip(got[call], got[call % 2]):
            assert torch.equal(a, b), call                                           # eager, captured and replayed: the same bits
    again = tr.score_cubes(raw_d, flow_d, halves[1])                                 # the plain capture still replays its own plan
    assert torch.equal(again[0], plain[1][0]) and torch.equal(again[1], plain[1][1])
    # the maps against the module's own eval-mode reconstructions and targets
    x, x_of = O.cubes_to_inputs(raw, flow)
    for h, idx in enumerate(halves):
        sl = slice(h * n, (h + 1) * n)
        with torch.no_grad():
            of_o, raw_o, of_t, raw_t = net(x[sl].cuda(), x_of[sl].cuda())
        r, o, e_raw, e_of = got[h]
        for what, e, rec, tgt, s in (('raw', e_raw, raw_o, raw_t, r), ('of', e_of, of_o, of_t, o)):
            d64, d32 = (rec.double() - tgt.double()).cpu(), (rec - tgt).cpu()
            bar('score_cubes_maps', '%s %s %s' % (kind, precision, what), e, _seq32(d64 * d64), _seq32(d32 * d32), family='pixel_maps')
            # the sum of a map is the cube's score: the score kernel's own fp32 sum against the exact sum of the map
            flat = e.cpu().reshape(n, -1)
            seq = torch.from_numpy(np.cumsum(flat.numpy(), axis=1, dtype=np.float32)[:, -1].copy())
            bar('score_cubes_maps', '%s %s sum %s' % (kind, precision, what), s, flat.double().sum(1), seq, family='pixel_maps')
            bar('score_cubes_maps', '%s %s map sum %s' % (kind, precision, what), e.sum((1, 2)), s.cpu(), seq, family='pixel_maps')
            assert float(e.min()) >= 0.0 and float(e.max()) > 0.0


def test_launch_loops_with_maps_drop_the_tail_padding():
    """``score_index_list`` and ``score_cubes_device`` with ``maps``: launches of 4 cubes over 10, the tail launch padded by repeating
    the last cube -- what comes back is, cube for cube, what the same launches return, and nothing of the padding."""
    import test as S
    from oracle import unet_oracle as O
    from vec_vad_amd.trainer import FusedTrainer
    net, tot_of = _net('net4', seed=1)
    raw, flow = O.seeded_cubes(12, tot_of, 9)
    raw_d, flow_d = torch.from_numpy(raw).cuda(), torch.from_numpy(flow).cuda()
    tr = FusedTrainer(net)
    idx = np.array([3, 0, 7, 7, 11, 2, 5, 9, 1, 6], np.int64)

    def launches(lists):
        outs = [tr.score_cubes(raw_d, flow_d, torch.tensor(l, device='cuda'), maps=True) for l, _ in lists]
        return [torch.cat([o[k][:m] for o, (_, m) in zip(outs, lists)]) for k in range(4)]

    want = launches([(idx[0:4], 4), (idx[4:8], 4), (np.concatenate([idx[8:10], idx[9:10], idx[9:10]]), 2)])
    got = S.score_index_list(tr, raw_d, flow_d, idx, 4, maps=True)
    plain = S.score_index_list(tr, raw_d, flow_d, idx, 4)
    assert len(got) == 4 and len(plain) == 2 and tuple(got[2].shape) == (10, 32, 32)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    # the staged loop: per-frame lists through a staging buffer of 6 cubes -> launches (0..3), (4, 5, 5, 5), (6..9)
    cubes = [raw[idx[0:3]], raw[idx[3:3]], raw[idx[3:10]]]
    flows = [flow[idx[0:3], 0], flow[idx[3:3], 0], flow[idx[3:10], 0]]
    want = launches([(idx[0:4], 4), (np.concatenate([idx[4:6], idx[5:6], idx[5:6]]), 2), (idx[6:10], 4)])
    got = S.score_cubes_device(tr, cubes, flows, 4, chunk_cubes=6, maps=True)
    plain = S.score_cubes_device(tr, cubes, flows, 4, chunk_cubes=6)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert len(plain) == 2 and torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    none = S.score_cubes_device(tr, [raw[:0]], [flow[:0, 0]], 4, maps=True)
    assert len(none) == 4 and tuple(none[2].shape) == (0, 32, 32) and none[3] is None


# ---- 3. z-maps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 1, 257])
def test_error_zmaps_are_the_numpy_expression(n):
    from vec_vad_amd import scoring
    rng = np.random.default_rng(11 + n)
    e_raw = (rng.random((n, 32, 32)) * 50 / 1024).astype(np.float32)
    e_of = (rng.random((n, 32, 32)) * 9 / 1024).astype(np.float32)
    cs = rng.integers(-1, 2, n).astype(np.int32)
    if n > 2:
        cs[:3] = [0, -1, 1]
    for use_flow in (True, False):
        got = scoring.error_zmaps(torch.from_numpy(e_raw).cuda(), torch.from_numpy(e_of).cuda() if use_flow else None, cs, STATS, 0.3, 1.0)
        assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (n, 32, 32)
        want = R.zmaps(e_raw, e_of if use_flow else None, cs, STATS, 0.3, 1.0)
        assert np.array_equal(got.cpu().numpy(), want)
        if n > 1:
            assert (want == BIG).any() and (want != BIG).any()
    with pytest.raises(ValueError):
        scoring.error_zmaps(torch.zeros((n + 1, 32, 32), device='cuda'), None, cs, STATS, 1.0, 1.0)


# ---- 4. / 5. fine masks and the criterion on them: one scene per frame size ------------------------------------------------------
COUNTS7 = [257, 0, 1, 63, 64, 65, 9]           # boxes per frame: more than one LDS pass (256), none, one, the wave border


def _scene(h, w, counts, seed):
    """Boxes, z-maps (values rounded to 0.5: ties), rectangles and the numpy-painted fine masks of ``len(counts)`` frames.  Every
    frame with at least 9 boxes holds an empty rectangle, one of a single pixel, one narrower than 32, one of exactly 32, one wider,
    one clipped at the far edges, a ``BIG`` map and a whole-frame box under everything else."""
    from vec_vad_amd import scoring
    rng = np.random.default_rng(seed)
    boxes = []
    for f, n in enumerate(counts):
        x0, y0 = rng.uniform(-6, w + 3, n), rng.uniform(-6, h + 3, n)
        b = np.stack([x0, y0, x0 + rng.uniform(0.3, 0.4 * w + 2, n), y0 + rng.uniform(0.3, 0.4 * h + 2, n)], 1).reshape(n, 4)
        if n >= 9:
            b[0] = [3.2, 3.2, 3.9, 9.0]                                  # ceil(x1) == ceil(x2): paints nothing
            b[1] = [4.5, 6.5, 5.5, 7.5]                                  # one pixel
            b[2] = [2.0, 1.0, 19.0, 12.0]                                # narrower than the patch
            b[3] = [1.0, 2.0, 33.0, 34.0]                                # exactly 32 x 32
            b[4] = [0.0, 0.0, float(w), float(h)]                        # the whole frame
            b[5] = [w * 0.6, h * 0.6, w + 40.0, h + 40.0]                # clipped at the far edges
            b[6] = [5.0, 3.0, 50.0, 36.0]                                # wider than the patch, overlapping the others
        boxes.append(b)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    boxes = np.concatenate(boxes)
    n = len(boxes)
    z = np.round(rng.standard_normal((n, 32, 32)) * 3 * 2) / 2
    for f, c in enumerate(counts):
        if c >= 9:
            z[off[f] + 0] = 2 * BIG                                      # would win everywhere if an empty rectangle painted
            z[off[f] + 4] = -50.0 + np.round(rng.standard_normal((32, 32)))      # under everything else
            z[off[f] + 5] = BIG
    rects = scoring.box_rects(boxes, h, w)
    masks = R.paint_error_masks(z, off, rects, h, w)
    return dict(h=h, w=w, off=off, boxes=boxes, z=z, rects=rects, masks=masks)


@pytest.fixture(scope='module')
def scenes():
    return {(h, w, F): _scene(h, w, COUNTS7[:F], 200 + h) for (h, w) in SIZES for F in (1, 7)}


@pytest.mark.parametrize('F', [1, 7])
@pytest.mark.parametrize('h,w', SIZES, ids=IDS)
def test_paint_error_masks_equal_the_restatement(scenes, h, w, F):
    from vec_vad_amd import scoring
    sc = scenes[(h, w, F)]
    off, rects = sc['off'], sc['rects']
    z = torch.from_numpy(sc['z']).cuda()
    if h > 1:
        hh, ww = rects[:, 1] - rects[:, 0], rects[:, 3] - rects[:, 2]
        empty = (hh <= 0) | (ww <= 0)
        assert empty.any() and ((hh == 1) & (ww == 1)).any() and ((hh == 32) & (ww == 32)).any()
        assert ((hh > 0) & (hh < 32) & (ww > 0) & (ww < 32)).any() and ((hh > 32) | (ww > 32)).any()
        assert ((rects[:, 1] == h) & (rects[:, 3] == w) & (rects[:, 0] > 0)).any()                    # clipped at the far edges
        assert ((rects[:, 0] == 0) & (rects[:, 1] == h) & (rects[:, 2] == 0) & (rects[:, 3] == w)).any()
        assert (np.diff(off) > 256).any()                                                          # more boxes than one LDS pass
        assert (sc['masks'] == BIG).any() and (sc['masks'] < BIG).any() and not (sc['masks'] > BIG).any()
        inner = sc['masks'][0][1:12, 2:19]
        assert len(np.unique(inner)) > 4                                                           # not constant inside a box
    got = scoring.paint_error_masks(z, off, rects, h, w)
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
        ret = scoring.paint_error_masks(z[torch.from_numpy(pick).cuda()], goff, rects[pick], h, w, out=out)
        assert ret is out
    assert np.array_equal(out.cpu().numpy(), sc['masks'])
    # max-accumulation: painting over a mask that is already higher somewhere keeps the higher value
    high = torch.full((F, h, w), 1.5, dtype=torch.float64, device='cuda')
    scoring.paint_error_masks(z, off, rects, h, w, out=high)
    assert np.array_equal(high.cpu().numpy(), np.maximum(sc['masks'], 1.5))
    # the support is that of the painted mask
    flat = scoring.paint_masks(torch.zeros(len(rects), dtype=torch.float64, device='cuda'), off, rects, h, w)
    assert torch.equal(flat > -BIG, got > -BIG)


def test_paint_error_masks_without_boxes_touch_nothing():
    from vec_vad_amd import scoring
    buf = torch.full((2, 37, 53), 7.0, dtype=torch.float64, device='cuda')
    none = torch.zeros((0, 32, 32), dtype=torch.float64, device='cuda')
    out = scoring.paint_error_masks(none, np.zeros(1, np.int32), np.zeros((0, 4), np.int32), 37, 53, out=buf[:0])
    assert tuple(out.shape) == (0, 37, 53) and bool((buf == 7.0).all())
    out = scoring.paint_error_masks(none, np.zeros(3, np.int32), np.zeros((0, 4), np.int32), 37, 53, out=buf)
    assert out is buf and bool((buf == 7.0).all())
    # boxes, every one of them empty
    z = torch.full((2, 32, 32), 9.0, dtype=torch.float64, device='cuda')
    out = scoring.paint_error_masks(z, np.array([0, 1, 2], np.int32), np.array([[5, 5, 1, 9], [3, 8, 4, 4]], np.int32), 37, 53, out=buf)
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
@pytest.mark.parametrize('h,w', SIZES, ids=IDS)
def test_mask_pixel_scores_equal_the_sorted_selection(scenes, h, w, F):
    from vec_vad_amd import scoring
    sc = scenes[(h, w, F)]
    masks = sc['masks'].copy()
    if F == 7:
        masks[1] = -BIG                                                  # (it is: the frame without boxes)
        masks[3, :, : w // 2] = -BIG                                     # a frame that is half background
    md = torch.from_numpy(masks).cuda()
    above = at_bg = tied = 0
    for variant in range(7):
        gt = _ground_truths(sc, variant)
        gt_dev = torch.from_numpy(gt).cuda()
        for pct in (1, 40, 100):
            got, cnt = scoring.mask_pixel_scores(gt_dev, md, pct)
            assert got.dtype == torch.float64 and cnt.dtype == torch.int32 and tuple(got.shape) == tuple(cnt.shape) == (F,)
            want = np.array([R.kth_largest(masks[f], gt[f], pct) for f in range(F)])
            assert np.array_equal(cnt.cpu().numpy(), (gt != 0).reshape(F, -1).sum(1))
            assert np.array_equal(got.cpu().numpy(), want), (variant, pct, got.cpu().numpy(), want)
            anomalous = (gt != 0).reshape(F, -1).any(1)
            above += int((want[anomalous] > -BIG).sum())
            at_bg += int((want[anomalous] == -BIG).sum())
            for f in np.nonzero(anomalous)[0]:
                tied += int((masks[f][gt[f] != 0] == want[f]).sum() > 1)
            assert np.array_equal(want[~anomalous], masks.reshape(F, -1).max(1)[~anomalous])      # a normal frame: the maximum
    if h > 1 and F == 7:
        assert above >= 2 and at_bg >= 1 and tied >= 2, (above, at_bg, tied)
    # host ground truth is uploaded, `out` is filled, percent is checked
    out = torch.zeros(F, dtype=torch.float64, device='cuda')
    got, _ = scoring.mask_pixel_scores(_ground_truths(sc, 0), md, out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), [R.kth_largest(masks[f], _ground_truths(sc, 0)[f], 40) for f in range(F)])
    for bad in (0, 101, 40.5):
        with pytest.raises(ValueError):
            scoring.mask_pixel_scores(gt_dev, md, bad)


def test_mask_pixel_scores_select_among_close_and_signed_values():
    """keys that differ only in their low digits, both signs, both zeros, the extremes: the radix select walks every digit"""
    from vec_vad_amd import scoring
    rng = np.random.default_rng(3)
    h, w = 24, 31
    base = 1.0 + np.arange(h * w) * 2.0 ** -52                           # consecutive doubles
    vals = np.concatenate([base[:300], -base[:300], [0.0, -0.0, BIG, -BIG, 5e-324, -5e-324, 1.7e308, -1.7e308]])
    masks = rng.choice(vals, (3, h, w))
    gt = (rng.random((3, h, w)) < 0.6).astype(np.uint8)
    gt[2] = 0
    for pct in (1, 40, 73, 100):
        got, _ = scoring.mask_pixel_scores(gt, torch.from_numpy(masks).cuda(), pct)
        assert np.array_equal(got.cpu().numpy(), [R.kth_largest(masks[f], gt[f], pct) for f in range(3)]), pct


# ---- 6. tie to the kernels of the painted masks -------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', SIZES, ids=IDS)
def test_even_maps_give_the_painted_masks_and_their_pixel_scores(scenes, h, w):
    from vec_vad_amd import scoring
    sc = scenes[(h, w, 7)]
    off, rects = sc['off'], sc['rects']
    n = len(rects)
    rng = np.random.default_rng(5)
    s_raw = rng.integers(0, 1 << 14, n).astype(np.float32) / 8            # multiples of 2^-3 below 2^11: s / 1024 is exact
    s_of = rng.integers(0, 1 << 12, n).astype(np.float32) / 8
    cs = rng.integers(-1, 2, n).astype(np.int32)
    e_raw = np.broadcast_to((s_raw / np.float32(1024))[:, None, None], (n, 32, 32)).copy()
    e_of = np.broadcast_to((s_of / np.float32(1024))[:, None, None], (n, 32, 32)).copy()
    assert np.array_equal(e_raw[:, 0, 0] * np.float32(1024), s_raw) and np.array_equal(e_of[:, 0, 0] * np.float32(1024), s_of)
    for use_flow in (True, False):
        cube = scoring.cube_scores(torch.from_numpy(s_raw).cuda(), torch.from_numpy(s_of).cuda() if use_flow else None, cs, STATS, 0.3, 1.0)
        z = scoring.error_zmaps(torch.from_numpy(e_raw).cuda(), torch.from_numpy(e_of).cuda() if use_flow else None, cs, STATS, 0.3, 1.0)
        assert torch.equal(z, cube[:, None, None].expand(n, 32, 32))
        fine, painted = scoring.paint_error_masks(z, off, rects, h, w), scoring.paint_masks(cube, off, rects, h, w)
        assert torch.equal(fine, painted)
        for variant in (0, 3):
            gt = torch.from_numpy(_ground_truths(dict(sc, masks=painted.cpu().numpy()), variant)).cuda()
            for pct in (1, 40, 100):
                a, ca = scoring.mask_pixel_scores(gt, fine, pct)
                b, cb = scoring.pixel_scores(gt, cube, off, rects, pct)
                assert torch.equal(a, b) and torch.equal(ca, cb), (variant, pct)


# ---- 7. script level ----------------------------------------------------------------------------------------------------------
N_TEST = 24


def _load(d, n):
    assert sorted(os.listdir(d)) == sorted(str(f) for f in range(n))
    return [torch.load(os.path.join(d, str(f)), weights_only=False) for f in range(n)]


def test_main_pixel_maps_staged_and_direct(tmp_path, monkeypatch, capsys):
    import train as T
    import test as S
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from synthetic_tree import make_tree
    monkeypatch.chdir(tmp_path)
    make_tree({'train': (4, 3), 'test': (N_TEST,)}, 3)                     # the first box of a frame fails the motion test: two are cut
    cfg = small_config().replace('pixel_criterion = False', 'pixel_criterion = True')
    assert 'save_score_masks = True' in cfg and 'pixel_maps = False' in cfg
    res = 'results/UCSDped2/'
    tail = 'obj_det_with_motion_SelfComplete'
    files = [res + 'frame_scores_%s.npy' % tail, res + 'pixel_scores_%s.npy' % tail]
    npzs = [res + 'raw2flow_%s_frame_results.npz' % tail, res + 'raw2flow_%s_pixel_results.npz' % tail]
    fine_npy, fine_npz = res + 'pixel_scores_fine_%s.npy' % tail, res + 'raw2flow_%s_pixel_fine_results.npz' % tail

    def written():
        return ([np.load(p) for p in files], [dict(np.load(p)) for p in npzs], _load(res + 'score_mask', N_TEST))

    open('config.cfg', 'w').write(cfg)
    T.main('config.cfg')
    S.main('config.cfg')                                                   # pixel_maps = False: what everything else must stay
    off_out = capsys.readouterr().out
    base = written()
    assert 'Fine pixel-level' not in off_out and not os.path.exists(fine_npy) and not os.path.exists(fine_npz)
    assert not os.path.exists(res + 'error_mask')
    on = cfg.replace('pixel_maps = False', 'pixel_maps = True')
    got = {}
    for route, text in (('staged', on.replace('test_foreground_saved = False', 'test_foreground_saved = True')),
                        ('direct', on.replace('direct_test = False', 'direct_test = True')
                         .replace('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = 5'))):
        for p in files + npzs + [fine_npy, fine_npz] + glob.glob(res + 'score_mask/*') + glob.glob(res + 'error_mask/*'):
            if os.path.exists(p):
                os.remove(p)
        open('config.cfg', 'w').write(text)
        c = T.read_config('config.cfg')
        assert c['pixel_maps'] and c['pixel_criterion'] and c['direct_test'] == (route == 'direct')
        S.main('config.cfg')
        printed = capsys.readouterr().out
        assert 'Fine pixel-level AUC (overlap 40%) is ' in printed and 'Fine pixel-level AUC@ROC (device pair count) is ' in printed
        assert printed.index('Pixel-level AUC@ROC (device pair count)') < printed.index('Fine pixel-level AUC (overlap')
        now = written()
        for a, b in zip(base[0], now[0]):
            assert a.dtype == b.dtype and np.array_equal(a, b), route
        for a, b in zip(base[1], now[1]):
            assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a), route
        for a, b in zip(base[2], now[2]):
            assert a.dtype == b.dtype and np.array_equal(a, b), route
        got[route] = (_load(res + 'error_mask', N_TEST), np.load(fine_npy), dict(np.load(fine_npz)))
    for p in glob.glob('data/raw2flow/*foreground_test*'):
        os.remove(p)
    fine, ps_fine, npz = got['staged']
    for f in range(N_TEST):
        a, b = fine[f], got['direct'][0][f]
        assert type(a) is np.ndarray and a.dtype == b.dtype == np.float64 and a.shape == b.shape == (240, 360) and a.flags['C_CONTIGUOUS']
        assert np.array_equal(a, b), f
        assert np.array_equal(a > -BIG, base[2][f] > -BIG), f                # the support of the score mask
    assert ps_fine.shape == (N_TEST,) and ps_fine.dtype == np.float64 and np.array_equal(ps_fine, got['direct'][1])
    assert sorted(npz) == sorted(got['direct'][2]) and all(np.array_equal(npz[k], got['direct'][2][k]) for k in npz)
    from PIL import Image
    gts = [np.array(Image.open(p).convert('L')) for p in sorted(glob.glob('raw_datasets/UCSDped2/Test/Test001_gt/*.bmp'))]
    assert len(gts) == N_TEST and [bool(g.any()) for g in gts] == [bool(k % 2) for k in range(N_TEST)]
    want = np.array([R.kth_largest(m, g, 40) for m, g in zip(fine, gts)])
    assert np.array_equal(ps_fine, want)
    # the maps say something the boxes do not: some mask varies inside its support, and a normal frame's fine score is its maximum
    assert any(len(np.unique(m[m > -BIG])) > 2 for m in fine)
    assert all(ps_fine[f] == fine[f].max() for f in range(0, N_TEST, 2))
    # scores_saved = True: the fine result comes from the saved file, nothing is scored
    os.remove(fine_npz)
    open('config.cfg', 'w').write(on.replace('scores_saved = False', 'scores_saved = True'))

    def scored(*a, **k):
        raise AssertionError('scores_saved = True must not score')

    monkeypatch.setattr(S, 'score_frames', scored)
    monkeypatch.setattr(S, 'score_direct', scored)
    S.main('config.cfg')
    again = dict(np.load(fine_npz))
    assert sorted(again) == sorted(npz) and all(np.array_equal(again[k], npz[k]) for k in npz)
