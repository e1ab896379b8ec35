"""GPU: the per-pixel error mask of a stream ([mi355x] stream_maps; vec_vad_amd/stream.py) -- ``vv_stream_zpaint`` against the numpy
restatement of tests/stream_maps_restatement.py, against the batch route's ``vv_error_zmaps`` + ``vv_paint_zmaps`` and, on constant
maps, against ``vv_stream_paint``; ``StreamScorer(maps=True)`` against the batch API at the same launch size, in motion mode against the
restatement of its own launches, under torch's sync debug mode, and through ``stream.main``.  Every comparison is bit for bit."""
import glob
import os

import numpy as np
import pytest
import torch

import stream_maps_restatement as R
import stream_masks_restatement as SM
from test_gpu_stream import COUNTS, H, N_VIDEO, W, _bits, _stream, net, tree  # noqa: F401  (fixtures of the synthetic tree)

pytestmark = pytest.mark.gpu

BIG = R.BIG
CAP, N = 8, 5
W_RAW, W_OF = 0.7, 1.3
STATS = ((0.9, 0.4, 0.3, 0.2), (1.4, 0.7, 0.1, 0.5))


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tables(h, w):
    """The frame's rectangle table (two rounds of CAP rows) and the device's box table.  Round 0: exactly 32 x 32 | shrunk, overlapping
    it | stretched over most of the frame | (device) clipped at the frame's corner, from a box with a negative x1 that wraps | (device)
    empty.  Round 1: other rectangles of the same kinds.  Rows 5..7 of a round cover the whole frame: only n keeps them out."""
    rects = np.zeros((2 * CAP, 4), np.int32)
    boxes = np.full((2 * CAP, 4), 7, np.int32)
    rects[0], rects[1], rects[2] = (2, 34, 3, 35), (10, 26, 20, 36), (0, h, 5, 53)
    boxes[3], boxes[4] = (-12, h - 12, w + 20, h + 9), (-5, 3, 2, 20)          # -> (h-12, h, w-12, w) and an empty column range
    rects[3], rects[4] = (1, 2, 3, 4), (0, h, 0, w)                            # host rows the kernel must NOT use at n_host = 3
    rects[8], rects[9], rects[10] = (4, 36, 20, 52), (0, 20, 0, 16), (3, 35, 1, 49)
    boxes[11], boxes[12] = (w - 20, -20, w + 3, h + 4), (30, 30, 30, 35)
    rects[5:8], rects[13:16] = (0, h, 0, w), (0, h, 0, w)
    boxes[5:8], boxes[13:16] = (0, 0, w, h), (0, 0, w, h)
    resolved = rects.copy()
    for g in (3, 4, 11, 12):
        resolved[g] = R.resolve([boxes[g]], h, w)[0]
    assert resolved[3].tolist() == [h - 12, h, w - 12, w] and resolved[4, 2] >= resolved[4, 3] and resolved[12, 2] == resolved[12, 3]
    return rects, boxes, resolved


def _maps(seed, counted):
    """float32 [CAP,32,32] errors; every slot that does not count is NaN."""
    rng = np.random.default_rng(seed)
    e_raw, e_of = (rng.random((CAP, 32, 32)) * 2e-3).astype(np.float32), (rng.random((CAP, 32, 32)) * 5e-4).astype(np.float32)
    for b in range(CAP):
        if b not in counted:
            e_raw[b], e_of[b] = np.nan, np.nan
    return e_raw, e_of


LAUNCHES = (dict(keep=[1, 1, 1, 1, 1, 1, 1, 1], mask=[1, 1, 0, 1, 1, 1, 1, 1], slot0=0, n_host=3, counted=(0, 1, 3, 4)),
            dict(keep=[1, 0, 1, 1, 1, 1, 1, 1], mask=[0, 1, 1, 1, 0, 1, 1, 1], slot0=CAP, n_host=CAP + 3, counted=(2, 3)))


def _zpaint(kw, e_raw, e_of, stats, rects, boxes, out, first, n=N):
    from vec_vad_amd.stream import stream_zpaint
    stream_zpaint(cu(e_raw), cu(e_of) if e_of is not None else None, cu(np.array(stats, np.float64)) if stats is not None else None,
                  W_RAW, W_OF, cu(np.array(kw['keep'], np.uint8)), cu(np.array(kw['mask'], np.uint8)), cu(np.array([n], np.int32)),
                  kw['slot0'], cu(rects), kw['n_host'], cu(boxes) if boxes is not None else None, out, first)


def _out(h, w, shift):
    """A mask full of garbage (NaN, Inf, large values), 16-byte aligned (``shift`` 0) or 8 bytes past that (``shift`` 1: no pair of
    pixels can go out as one 16-byte store)."""
    buf = torch.full((h * w + 2,), float('nan'), dtype=torch.float64, device='cuda')
    buf[::3], buf[1::3] = float('inf'), 3e5
    assert buf.data_ptr() % 16 == 0
    out = buf[shift:shift + h * w].view(h, w)
    assert out.data_ptr() % 16 == 8 * shift and out.is_contiguous()
    return buf, out


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'misaligned'])
@pytest.mark.parametrize('model', [True, False], ids=['stats', 'no-model'])
@pytest.mark.parametrize('flow', [True, False], ids=['flow', 'no-flow'])
@pytest.mark.parametrize('h,w', [(37, 53), (48, 72)])
def test_zpaint_equals_the_restatement_and_the_batch_kernels(h, w, flow, model, shift):
    from vec_vad_amd import scoring
    rects, boxes, resolved = _tables(h, w)
    a, b = LAUNCHES
    ea, eb = _maps(1, a['counted']), _maps(2, b['counted'])
    stats_a = STATS[0] if model else None
    buf, out = _out(h, w, shift)
    edge = buf.clone()
    args = lambda kw, e, st: dict(e_raw=e[0], e_of=e[1] if flow else None, stats=st, w_raw=W_RAW, w_of=W_OF, keep=kw['keep'], mask=kw['mask'],
                                  n=N, slot0=kw['slot0'], rects=rects, n_host=kw['n_host'], boxes=boxes)
    # the first launch of a frame: written whole over the garbage
    _zpaint(a, ea[0], ea[1] if flow else None, stats_a, rects, boxes, out, True)
    got = out.cpu().numpy()
    want = R.launch(h=h, w=w, **args(a, ea, stats_a))
    assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(want))
    assert (want == -BIG).any() and (want > -BIG).sum() > 32 * 32                       # background, and more than one rectangle
    assert ((want == BIG).any() and (np.abs(want) == BIG).all()) if not model else (np.abs(want[want > -BIG]) < BIG).all()
    assert (got[h - 12:, w - 12:] > -BIG).all()                                         # the device's rectangle, clipped at the corner
    # the batch route on the counted slots: error_zmaps, then paint_error_masks over the resolved rectangles
    cnt = [s for s in a['counted']]
    z = scoring.error_zmaps(cu(ea[0][cnt]), cu(ea[1][cnt]) if flow else None, np.full(len(cnt), 0 if model else -1, np.int32),
                            np.array([STATS[0]], np.float64), W_RAW, W_OF)
    batch = scoring.paint_error_masks(z, [0, len(cnt)], resolved[cnt], h, w)[0].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(batch))
    # another block of another round accumulates
    _zpaint(b, eb[0], eb[1] if flow else None, STATS[1], rects, boxes, out, False)
    got2 = out.cpu().numpy()
    want2 = R.frame([args(a, ea, stats_a), args(b, eb, STATS[1])], h, w)
    assert np.isfinite(got2).all() and np.array_equal(_bits(got2), _bits(want2)) and not np.array_equal(got2, got)
    cnt = [s for s in b['counted']]
    z = scoring.error_zmaps(cu(eb[0][cnt]), cu(eb[1][cnt]) if flow else None, np.zeros(len(cnt), np.int32), np.array([STATS[1]], np.float64),
                            W_RAW, W_OF)
    batch2 = scoring.paint_error_masks(z, [0, len(cnt)], resolved[[CAP + s for s in cnt]], h, w, out=cu(batch[None]))[0].cpu().numpy()
    assert np.array_equal(_bits(got2), _bits(batch2))
    # nothing outside the mask was written
    keep_out = torch.ones_like(buf, dtype=torch.bool)
    keep_out[shift:shift + h * w] = False
    assert torch.equal(buf[keep_out].view(torch.int64), edge[keep_out].view(torch.int64))


@pytest.mark.parametrize('n,cap', [(0, CAP), (-3, CAP), (N, 0)])
def test_zpaint_without_boxes_leaves_the_background(n, cap):
    from vec_vad_amd.stream import stream_zpaint
    h, w = 37, 53
    rects, boxes, _ = _tables(h, w)
    e = np.full((CAP, 32, 32), np.nan, np.float32)
    _, out = _out(h, w, 0)
    ones = cu(np.ones(cap, np.uint8))
    stream_zpaint(cu(e), cu(e), cu(np.array(STATS[0])), W_RAW, W_OF, ones, ones, cu(np.array([n], np.int32)), 0, cu(rects), 3, cu(boxes), out, True)
    assert bool((out == -BIG).all())
    before = out.clone()
    stream_zpaint(cu(e), cu(e), cu(np.array(STATS[0])), W_RAW, W_OF, ones, ones, cu(np.array([n], np.int32)), 0, cu(rects), 3, cu(boxes), out, False)
    assert torch.equal(out, before)


@pytest.mark.parametrize('flow', [True, False], ids=['flow', 'no-flow'])
def test_constant_maps_reproduce_the_mask_of_stream_paint(flow):
    """e = c over the patch, the cube's error sum 1024 c (exact: c has at most 14 significant bits): the fine mask is the score mask."""
    from vec_vad_amd.stream import stream_paint, stream_scores
    h, w = 48, 72
    rects, boxes, _ = _tables(h, w)
    kw = LAUNCHES[0]
    rng = np.random.default_rng(7)
    c_raw = (rng.integers(1, 2 ** 14, CAP) / 2.0 ** 22).astype(np.float32)
    c_of = (rng.integers(1, 2 ** 14, CAP) / 2.0 ** 24).astype(np.float32)
    e_raw, e_of = (np.broadcast_to(c[:, None, None], (CAP, 32, 32)).copy() for c in (c_raw, c_of))
    _, out = _out(h, w, 0)
    _zpaint(kw, e_raw, e_of if flow else None, STATS[0], rects, boxes, out, True)
    row = torch.full((1, CAP), 55.5, dtype=torch.float64, device='cuda')
    cell = torch.full((1,), -BIG, dtype=torch.float64, device='cuda')
    n_dev = cu(np.array([N], np.int32))
    stream_scores(cu(np.float32(1024) * c_raw), cu(np.float32(1024) * c_of) if flow else None, cu(np.array(STATS[0])), W_RAW, W_OF,
                  cu(np.array(kw['keep'], np.uint8)), n_dev, cu(np.array(kw['mask'], np.uint8)), row[0], cell)
    mask = torch.empty((h, w), dtype=torch.float64, device='cuda')
    stream_paint(row, n_dev, kw['n_host'], cu(rects[:CAP]), cu(boxes[:CAP]), mask, torch.zeros(CAP, dtype=torch.float64, device='cuda'),
                 torch.zeros(2, dtype=torch.int32, device='cuda'))
    assert torch.equal(out.view(torch.int64), mask.view(torch.int64))
    assert len(np.unique(out.cpu().numpy())) >= 4                                   # the background and three boxes' scores


def test_zpaint_bad_arguments_return_without_a_launch():
    from vec_vad_amd import _lib
    l = _lib.lib()
    e = torch.zeros(CAP * 1024, dtype=torch.float32, device='cuda')
    st = torch.ones(4, dtype=torch.float64, device='cuda')
    flags, n = torch.ones(CAP, dtype=torch.uint8, device='cuda'), torch.full((1,), CAP, dtype=torch.int32, device='cuda')
    rects = torch.tensor([[0, 4, 0, 4]] * CAP, dtype=torch.int32, device='cuda')
    guard = torch.zeros(16, dtype=torch.float64, device='cuda')
    good = [e.data_ptr(), e.data_ptr(), st.data_ptr(), 1.0, 1.0, BIG, flags.data_ptr(), flags.data_ptr(), n.data_ptr(), CAP, 0,
            rects.data_ptr(), CAP, None, 4, 4, guard.data_ptr(), 1, torch.cuda.current_stream().cuda_stream]
    for i, v in ((16, None), (8, None), (11, None), (9, -1), (14, 0), (15, 0), (14, -4), (15, -1), (0, None), (6, None), (7, None), (10, -1)):
        args = list(good)
        args[i] = v
        assert l.vv_stream_zpaint(*args) == 1, i                                    # VV_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert not guard.any()
    assert l.vv_stream_zpaint(*good) == 0                                           # and the good call does launch
    torch.cuda.synchronize()
    assert bool((guard > -BIG).all())


# ---- the scorer --------------------------------------------------------------------------------------------------------------------------
def _run(tree, net, sync_error_after=None, **kw):
    """The tree's frames through one ``StreamScorer(**kw)``; returns the ``StreamResult``s and what ``wait()`` returned."""
    from vec_vad_amd.stream import StreamScorer
    sc = StreamScorer(tree['c'], *tree['arts'], (H, W, 3), flownet2=net, **kw)
    res = []
    try:
        for i, f in enumerate(tree['frames']):
            if i and tree['fvi'][i] != tree['fvi'][i - 1]:
                res += sc.end_video()
            if sync_error_after is not None and i == sync_error_after:
                torch.cuda.set_sync_debug_mode('error')
            res += sc.push(f, ap_boxes=tree['boxes'][i]) if kw.get('boxes') == 'motion' else sc.push(f, tree['boxes'][i])
        res += sc.end_video()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert [r.frame for r in res] == list(range(len(tree['frames'])))
    return sc, [(r, r.wait()) for r in res]


def _batch_masks(tree, net, B):
    """Per frame the fine mask of the batch API at launches of exactly ``B`` cubes: ``score_index_list(..., batch=B, maps=True)``,
    ``scoring.error_zmaps``, ``scoring.paint_error_masks`` over ``box_rects`` of the kept cubes, group by group."""
    import foreground as FG
    import test as S
    from vad_datasets import frame_size
    from vec_vad_amd import scoring
    from vec_vad_amd.trainer import FusedTrainer
    c, (net_set, st_r, st_o) = tree['c'], tree['arts']
    h, w = frame_size['UCSDped2'][:2]
    info, parts = FG.extract_device(c, 'test', 'cuda', log=lambda *a: None, flownet2=net)
    part = next(parts)
    n = info['n_frames']
    assert part['frames'] == (0, n) and n == len(tree['frames'])
    masks = torch.full((n, h, w), -BIG, dtype=torch.float64, device='cuda')
    trainers = {}
    for (key, hh, ww), (idx, off) in part['groups'].items():
        models = net_set[hh][ww]
        for f in range(n):
            ids = idx[off[f]:off[f + 1]]
            if not len(ids):
                continue
            if models:
                tr = trainers.setdefault(id(models[0]), FusedTrainer(models[0]))
                _, _, e_raw, e_of = S.score_index_list(tr, part['raw'], part['flow'], ids, c['score_batch'], batch=B, maps=True)
                so = st_o[hh][ww] if c['useFlow'] else (0.0, 1.0)
                stats, cube_stat = np.array([[st_r[hh][ww][0], st_r[hh][ww][1], so[0], so[1]]], np.float64), np.zeros(len(ids), np.int32)
            else:
                e_raw, e_of = torch.zeros((len(ids), 32, 32), device='cuda'), None
                stats, cube_stat = np.array([[0.0, 1.0, 0.0, 1.0]]), np.full(len(ids), -1, np.int32)
            z = scoring.error_zmaps(e_raw, e_of if c['useFlow'] else None, cube_stat, stats, c['w_raw'], c['w_of'])
            scoring.paint_error_masks(z, [0, len(ids)], scoring.box_rects(part['boxes'][ids], h, w), h, w, out=masks[f:f + 1])
    return masks.cpu().numpy()


@pytest.mark.parametrize('max_boxes', [8, 2], ids=['one-round', 'rounds'])
def test_scorer_error_masks_equal_the_batch_api_at_the_same_launch_size(tree, net, monkeypatch, max_boxes):
    from vad_datasets import frame_size
    monkeypatch.chdir(tree['root'])
    gh, gw = frame_size['UCSDped2'][:2]
    assert max(COUNTS) > 2 and max(COUNTS) <= 8
    _, got = _run(tree, net, max_boxes=max_boxes, maps=True, masks=True)
    off = _stream(tree, net, max_boxes)
    want = _batch_masks(tree, net, max_boxes)
    between = 0
    for f, ((r, (score, box, kept)), (oscore, obox, okept)) in enumerate(zip(got, off)):
        assert _bits(score) == _bits(oscore) and np.array_equal(_bits(box), _bits(obox)) and kept.tolist() == okept.tolist(), f
        assert r.error_mask.dtype == np.float64 and r.error_mask.shape == (gh, gw), f
        assert np.array_equal(_bits(r.error_mask), _bits(want[f])), f
        assert np.array_equal(r.error_mask > -BIG, r.mask > -BIG), f                 # the support of the painted score mask
        assert isinstance(r.fine_score, float) and r.fine_score == r.error_mask.max(), f
        vals = r.error_mask[r.error_mask > -BIG]
        between += bool(len(vals)) and bool((vals < BIG).all())
        if len(vals):
            assert len(np.unique(vals)) > len(box), f                                # finer than one value per box
    assert (got[2][0].error_mask == -BIG).all() and got[2][0].fine_score == -BIG      # the frame without boxes
    assert between >= 3                                                               # frames with values of a trained model


def test_scorer_in_motion_mode_equals_the_restatement_of_its_launches(tree, net, monkeypatch):
    """Motion mode: one round, every block, rectangles behind the host's resolved on the device.  Every ``vv_stream_zpaint`` launch is
    recorded (device clones); a frame's mask must be the restatement of its launches, its support that of the score mask painted
    from ``result.boxes`` and the box scores ``wait()`` returns, and a motion box that found no slot (``dropped``) is in neither."""
    import vec_vad_amd.stream as VS
    from vad_datasets import frame_size
    from vec_vad_amd.scoring import box_rects
    monkeypatch.chdir(tree['root'])
    gh, gw = frame_size['UCSDped2'][:2]
    calls, real = [], VS.stream_zpaint

    def recorded(e_raw, e_of, stats, w_raw, w_of, keep, mask, n, slot0, rects, n_host, boxes, out, first):
        cl = lambda t: t.clone() if t is not None else None
        calls.append(dict(e_raw=cl(e_raw), e_of=cl(e_of), stats=cl(stats), w_raw=w_raw, w_of=w_of, keep=cl(keep), mask=cl(mask), n=cl(n),
                          slot0=slot0, rects=cl(rects), n_host=n_host, boxes=cl(boxes), first=bool(first)))
        return real(e_raw, e_of, stats, w_raw, w_of, keep, mask, n, slot0, rects, n_host, boxes, out, first)

    monkeypatch.setattr(VS, 'stream_zpaint', recorded)
    cap = max(COUNTS)                                                                 # the fullest frame leaves no slot to a motion box
    sc, got = _run(tree, net, max_boxes=cap, boxes='motion', maps=True)
    monkeypatch.setattr(VS, 'stream_zpaint', real)
    frames = []
    for kw in calls:
        first = kw.pop('first')
        assert first or frames
        if first:
            frames.append([])
        host = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in kw.items()}
        host['n'] = int(host['n'][0])
        host['rects'], host['boxes'] = host['rects'].reshape(-1, 4), host['boxes'].reshape(-1, 4) if host['boxes'] is not None else None
        if host['e_raw'] is not None:
            host['e_raw'] = host['e_raw'].reshape(-1, 32, 32)
            host['e_of'] = host['e_of'].reshape(-1, 32, 32) if host['e_of'] is not None else None
        frames[-1].append(host)
    assert len(frames) == len(got) and all(len(fr) == sc.hb * sc.wb for fr in frames)
    found = dropped = 0
    for f, ((r, (score, box, kept)), launches) in enumerate(zip(got, frames)):
        want = R.frame(launches, gh, gw)
        assert np.array_equal(_bits(r.error_mask), _bits(want)), f
        assert r.fine_score == r.error_mask.max(), f
        painted, _ = SM.paint(box[None, :], len(box), box_rects(r.boxes, gh, gw), gh, gw)
        assert np.array_equal(r.error_mask > -BIG, painted > -BIG), f
        assert launches[0]['n'] == len(r.boxes) <= cap and launches[0]['n_host'] == len(tree['boxes'][f])
        found += len(r.boxes) - len(tree['boxes'][f])
        dropped += r.dropped
    assert found >= 3 and dropped >= 1


def test_push_does_not_synchronise_with_maps(tree, net, monkeypatch):
    """From the second video on every ``push`` and ``end_video`` runs under ``torch.cuda.set_sync_debug_mode('error')``."""
    monkeypatch.chdir(tree['root'])
    _, plain = _run(tree, net, max_boxes=8, maps=True)
    _, strict = _run(tree, net, max_boxes=8, maps=True, sync_error_after=N_VIDEO[0])
    for (a, wa), (b, wb) in zip(plain, strict):
        assert _bits(wa[0]) == _bits(wb[0]) and np.array_equal(_bits(a.error_mask), _bits(b.error_mask)) and a.fine_score == b.fine_score
    assert sum(-BIG < r.fine_score < BIG for r, _ in strict) >= 3


def test_maps_off_leaves_the_result_bare_and_captures_no_maps_graph(tree, net, monkeypatch):
    monkeypatch.chdir(tree['root'])
    sc, got = _run(tree, net, max_boxes=8)
    assert sc.maps is False and not hasattr(sc, 'zmask')
    assert all(r.error_mask is None and r.fine_score is None for r, _ in got)
    trainers = {id(ent[0]): ent[0] for ent in sc.blocks.values() if ent is not None}
    assert trainers and all(k[0] != 'eval_maps' for tr in trainers.values() for k in tr._graphs)
    on, _ = _run(tree, net, max_boxes=8, maps=True)
    trainers = {id(ent[0]): ent[0] for ent in on.blocks.values() if ent is not None}
    assert any(k[0] == 'eval_maps' and v != 'warm' for tr in trainers.values() for k, v in tr._graphs.items())      # captured at construction


def test_stream_main_with_the_key_on_writes_the_fine_scores(tree, net, monkeypatch, capsys):
    import stream as STREAM
    from utils import save_roc_pr_curve_data
    monkeypatch.chdir(tree['root'])
    saved = open('config.cfg').read()
    n = sum(N_VIDEO)
    try:
        A = STREAM.main('config.cfg', flownet2=net)
        a_file = open('results/UCSDped2/stream_scores_obj_det_with_motion_SelfComplete.npy', 'rb').read()
        assert not glob.glob('results/UCSDped2/*fine*')
        assert saved.count('\nstream_maps = off\n') == 1
        open('config.cfg', 'w').write(saved.replace('\nstream_maps = off\n', '\nstream_maps = on\n'))
        capsys.readouterr()
        B = STREAM.main('config.cfg', flownet2=net)
        out = capsys.readouterr().out
    finally:
        open('config.cfg', 'w').write(saved)
    assert np.array_equal(_bits(A), _bits(B)) and (A > -BIG).sum() >= 3
    assert open('results/UCSDped2/stream_scores_obj_det_with_motion_SelfComplete.npy', 'rb').read() == a_file
    fine = np.load('results/UCSDped2/stream_scores_fine_obj_det_with_motion_SelfComplete.npy')
    assert fine.dtype == np.float64 and fine.shape == (n,) and ((fine > -BIG) == (A > -BIG)).all() and not np.array_equal(fine, A)
    labels = np.load('data/raw2flow/UCSDped2_frame_labels_test.npy')
    auc = save_roc_pr_curve_data(fine, labels, 'own_fine.npz', verbose=False)
    assert float(np.load('results/UCSDped2/raw2flow_obj_det_with_motion_SelfComplete_stream_fine_results.npz')['roc_auc']) == auc
    assert "Frame-level AUC of the stream's error maps is {}".format(auc) in out.splitlines()
    assert sorted(os.path.basename(p) for p in glob.glob('results/UCSDped2/*fine*')) == [
        'raw2flow_obj_det_with_motion_SelfComplete_stream_fine_results.npz', 'stream_scores_fine_obj_det_with_motion_SelfComplete.npy']
