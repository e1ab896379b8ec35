"""GPU: several cameras in one scorer (vec_vad_amd/multistream.py, stream.py with ``[mi355x] stream_cameras``) -- ``vv_stream_cut_multi``
and ``vv_stream_scores_multi`` against their single-camera counterparts called per camera, ``MultiStreamScorer`` with one camera against
``StreamScorer``, and three cameras out of phase against a restatement built from the existing API at the same launch sizes
(``chunk_flows`` at 3 pairs per launch, scoring launches of ``3 * max_boxes`` cubes).  All comparisons are bit for bit: both sides run
the same arithmetic in the same order on the same inputs.  The synthetic tree and its helpers are those of tests/test_gpu_stream.py."""
import numpy as np
import pytest
import torch

from stream_restatement import BIG
from test_gpu_stream import COUNTS, CROPS, H, N_VIDEO, P, W, WINDOWS, _bits, _stream, net, tree  # noqa: F401  (fixtures of the synthetic tree)

pytestmark = pytest.mark.gpu

CAP = 4
R, RF = 6, 5                                                  # ring slots per camera of the kernel tests (context 4 / 4)
LOCAL_WINDOWS = [WINDOWS['wrapped'], WINDOWS['repeated'], ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0])]      # a different pair per camera


def _dv(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


# ---- 1. vv_stream_cut_multi ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('counts', [(0, 1, 4), (4,), (0,)], ids=['three-cameras', 'one-full', 'one-empty'])
@pytest.mark.parametrize('C', [1, 3])
def test_stream_cut_multi_equals_stream_cut_per_camera(C, counts):
    from vec_vad_amd.extract import cube_energy
    from vec_vad_amd.multistream import stream_cut_multi
    from vec_vad_amd.stream import stream_cut
    cams = len(counts)
    rng = np.random.default_rng(20 + C + cams)
    raw = torch.from_numpy(rng.integers(0, 256, (cams * R, H, W, C), dtype=np.uint8)).cuda()
    flow = rng.standard_normal((cams * RF, H, W, 2)).astype(np.float32) * np.linspace(0.2, 3.0, W, dtype=np.float32)[None, None, :, None]
    flow = torch.from_numpy(flow).cuda()
    crops = np.stack([np.roll(CROPS, k, axis=0) for k in range(cams)])                     # [cams,CAP,4], another order per camera
    wr = np.array([LOCAL_WINDOWS[k][0] for k in range(cams)], np.int32)                    # local slots; the kernel gets absolute ones
    wf = np.array([LOCAL_WINDOWS[k][1] for k in range(cams)], np.int32)
    # a threshold between the sorted energies of the boxes that count, so that both keep values occur
    e = np.sort(np.concatenate([cube_energy(flow[k * RF:(k + 1) * RF], crops[k, :n], np.tile(wf[k], (n, 1)), P, 0.0)[0].cpu().numpy()
                                for k, n in enumerate(counts) if n] + [np.zeros(0)]))
    thr = 1.0
    if len(e) >= 2:
        assert e[len(e) // 2 - 1] < e[len(e) // 2]
        thr = float((e[len(e) // 2 - 1] + e[len(e) // 2]) / 2)

    def poisoned():
        return (torch.full((cams * CAP, 5, P, P, C), 201, dtype=torch.uint8, device='cuda'), torch.full((cams * CAP, 5, P, P, 2), -7.5, device='cuda'),
                torch.full((cams * CAP,), 9, dtype=torch.uint8, device='cuda'), torch.full((cams * CAP,), -3.0, dtype=torch.float64, device='cuda'))

    ref_raw, ref_flow, ref_keep, ref_e = poisoned()
    for k, n in enumerate(counts):
        s = slice(k * CAP, (k + 1) * CAP)
        stream_cut(raw[k * R:(k + 1) * R], flow[k * RF:(k + 1) * RF], _dv([n]), _dv(crops[k]), _dv(wr[k]), _dv(wf[k]), thr, ref_raw[s],
                   ref_flow[s], ref_keep[s], ref_e[s])
    got_raw, got_flow, got_keep, got_e = poisoned()
    offs = np.arange(cams, dtype=np.int32)[:, None]
    stream_cut_multi(raw, flow, cams, _dv(counts), _dv(crops), _dv(wr + offs * R), _dv(wf + offs * RF), thr, got_raw, got_flow, got_keep, got_e)
    assert torch.equal(got_raw, ref_raw) and torch.equal(got_flow, ref_flow)               # the cubes, and the poison in untouched slots
    assert torch.equal(got_keep, ref_keep) and torch.equal(got_e, ref_e)
    counted = np.concatenate([np.arange(k * CAP, k * CAP + n) for k, n in enumerate(counts)] + [np.zeros(0, np.int64)]).astype(np.int64)
    untouched = np.setdiff1d(np.arange(cams * CAP), counted)
    assert bool((got_keep[untouched] == 9).all()) and bool((got_e[untouched] == -3.0).all())
    assert bool((got_raw[untouched] == 201).all()) and bool((got_flow[untouched] == -7.5).all())
    if len(counted) >= 2:
        assert sorted(set(got_keep[counted].tolist())) == [0, 1]                          # both classes occur
        assert bool((got_raw[counted] != 201).any()) and bool((got_flow[counted] != -7.5).any())
    # without the energy table nothing else changes
    got2_raw, got2_flow, got2_keep, _ = poisoned()
    stream_cut_multi(raw, flow, cams, _dv(counts), _dv(crops), _dv(wr + offs * R), _dv(wf + offs * RF), thr, got2_raw, got2_flow, got2_keep)
    assert torch.equal(got2_raw, ref_raw) and torch.equal(got2_flow, ref_flow) and torch.equal(got2_keep, ref_keep)


# ---- 2. vv_stream_scores_multi -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['flow', 'no-flow', 'no-model'])
def test_stream_scores_multi_equals_stream_scores_per_camera(variant):
    """Three cameras of 8 slots with n = (5, 0, 8); box rows 11 apart and cells 3 apart, poison between them.  NaN and Inf sit in every
    slot that does not count (at or above n, dropped by the motion test, outside the block's mask); camera 1 (n = 0) keeps its cell."""
    from vec_vad_amd.multistream import stream_scores_multi
    from vec_vad_amd.stream import stream_scores
    rng = np.random.default_rng(9)
    cams, cap, ns, bs, fs = 3, 8, (5, 0, 8), 11, 3
    keep = (rng.random(cams * cap) < 0.7).astype(np.uint8)
    mask = (rng.random(cams * cap) < 0.7).astype(np.uint8)
    keep[[0, 16]], mask[[0, 16]] = 1, 1                                   # a box that counts in each camera that has boxes
    keep[1], mask[2] = 0, 0                                                # and boxes below n that do not
    counts = np.array([b < ns[k] and keep[k * cap + b] and mask[k * cap + b] for k in range(cams) for b in range(cap)], bool)
    raw = (rng.random(cams * cap) * 40).astype(np.float32)
    of = (rng.random(cams * cap) * 9).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30], np.float32)
    raw[~counts] = bad[np.arange((~counts).sum()) % 4]
    of[~counts] = bad[(np.arange((~counts).sum()) + 1) % 4]
    assert counts[:cap].any() and counts[2 * cap:].any() and not counts[cap:2 * cap].any() and (~counts[:5]).any()
    stats = _dv((17.3, 4.1, 3.9, 1.7), np.float64) if variant != 'no-model' else None
    d_of = _dv(of, np.float32) if variant == 'flow' else None
    cells0 = np.array([-float(BIG), 7.25, 1.5])
    w_raw, w_of = 0.7, 1.3
    ref_rows = torch.full((cams, cap), 55.5, dtype=torch.float64, device='cuda')
    ref_cell = _dv(cells0, np.float64)
    for k in range(cams):
        s = slice(k * cap, (k + 1) * cap)
        stream_scores(_dv(raw[s], np.float32), d_of[s].contiguous() if d_of is not None else None, stats, w_raw, w_of, _dv(keep[s], np.uint8),
                      _dv([ns[k]]), _dv(mask[s], np.uint8), ref_rows[k], ref_cell[k:k + 1])
    got_rows = torch.full((cams * bs,), 55.5, dtype=torch.float64, device='cuda')
    got_cell = torch.full((cams * fs,), 66.5, dtype=torch.float64, device='cuda')
    got_cell[::fs] = ref_cell.new_tensor(cells0)
    stream_scores_multi(_dv(raw, np.float32), d_of, stats, w_raw, w_of, _dv(keep, np.uint8), _dv(ns), _dv(mask, np.uint8), cams, cap, got_rows,
                        bs, got_cell, fs)
    rows, cell = got_rows.cpu().numpy().reshape(cams, bs), got_cell.cpu().numpy().reshape(cams, fs)
    assert np.array_equal(_bits(rows[:, :cap]), _bits(ref_rows.cpu().numpy()))
    assert np.array_equal(_bits(cell[:, 0]), _bits(ref_cell.cpu().numpy()))
    assert (rows[:, cap:] == 55.5).all() and (cell[:, 1:] == 66.5).all()                 # nothing between the rows and the cells
    assert np.isfinite(rows).all() and np.isfinite(cell).all()                           # NaN and Inf reached nothing
    assert (rows[1] == 55.5).all() and cell[1, 0] == 7.25                                # the camera with n = 0
    assert (rows[0, 5:cap] == 55.5).all() and rows[0, 1] == -BIG and rows[0, 2] == -BIG
    if variant == 'no-model':
        assert cell[0, 0] == BIG and cell[2, 0] == BIG and set(rows[2, :cap].tolist()) <= {BIG, -BIG}
    else:
        assert -BIG < cell[0, 0] < BIG and cell[0, 0] == rows[0, :5].max() and cell[2, 0] == max(rows[2, :cap].max(), 1.5)


def test_multi_entry_points_refuse_bad_arguments_without_a_launch():
    from vec_vad_amd import _lib
    from vec_vad_amd.multistream import stream_cut_multi, stream_scores_multi
    l = _lib.lib()
    t = torch.zeros(64, dtype=torch.uint8, device='cuda')
    p = t.data_ptr()
    for cams in (0, -1):                                                  # VV_ERR_BAD_ARG = 1
        assert l.vv_stream_cut_multi(p, 1, p, 1, 4, 4, 1, cams, p, p, p, p, 1, 1, 1, 2, 0.0, p, p, p, None, None) == 1
        assert l.vv_stream_scores_multi(None, None, None, 1.0, 1.0, 1e5, p, p, p, cams, 1, p, 1, p, 1, None) == 1
    assert l.vv_stream_cut_multi(p, 1, p, 1, 4, 4, 1, 1, p, p, p, p, 1, 1, 1, 2000, 0.0, p, p, p, None, None) == 1          # P > 1024
    assert l.vv_stream_cut_multi(None, 1, p, 1, 4, 4, 1, 1, p, p, p, p, 1, 1, 1, 2, 0.0, p, p, p, None, None) == 1          # no ring
    assert l.vv_stream_scores_multi(None, None, None, 1.0, 1.0, 1e5, p, p, p, 2, 4, p, 3, p, 1, None) == 1                 # rows overlap
    assert l.vv_stream_scores_multi(None, None, None, 1.0, 1.0, 1e5, p, None, p, 2, 4, p, 4, p, 1, None) == 1              # no n table
    f64 = torch.zeros(8, dtype=torch.float64, device='cuda')
    i32 = torch.zeros(8, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='box_stride'):
        stream_scores_multi(None, None, None, 1.0, 1.0, t, i32, t, 2, 4, f64, 3, f64, 1)
    with pytest.raises(ValueError, match='contiguous CUDA'):
        stream_scores_multi(None, None, None, 1.0, 1.0, t, i32, t, 2, 4, f64[:7], 4, f64, 1)       # the second camera's row does not fit
    ring, fring = torch.zeros((4, 8, 8, 1), dtype=torch.uint8, device='cuda'), torch.zeros((2, 8, 8, 2), device='cuda')
    with pytest.raises(ValueError, match='cams must be at least 1 and divide'):
        stream_cut_multi(ring, fring, 3, i32, i32, i32, i32, 0.0, t, t, t)


# ---- the scorer ----------------------------------------------------------------------------------------------------------------------------
# Video A = frames 0..3 of the fixture, video B = frames 4..6.  Camera 0 plays A then B; camera 1 starts a tick later with B then A;
# camera 2 is idle for three ticks, then plays A.  ('push', one frame or None per camera) | ('end', cameras | None)
SCRIPT = [('push', (0, None, None)), ('push', (1, 4, None)), ('push', (2, 5, None)), ('push', (3, 6, 0)), ('end', [0]), ('end', [1]),
          ('push', (4, 0, 1)), ('push', (5, 1, 2)), ('push', (6, 2, 3)), ('end', [0, 2]), ('push', (None, 3, None)), ('end', None)]
SECOND = 6                                                    # the first call of every camera's second video (camera 2: mid-video)


def _fixture_source(tree):
    return lambda k, fi: (tree['frames'][fi], np.asarray(tree['boxes'][fi], np.float64).reshape(-1, 5)[:, :4])


def _noise_source(tree, keep_camera):
    """The fixture for ``keep_camera``; for the others fresh noise frames and other boxes, in number and place."""
    plain = _fixture_source(tree)

    def source(k, fi):
        if k == keep_camera:
            return plain(k, fi)
        rng = np.random.default_rng(1000 + 10 * k + fi)
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        bb = []
        for _ in range((COUNTS[fi] + 1 + k) % 6):
            x0, y0 = rng.uniform(0, W - 40), rng.uniform(0, H - 30)
            bb.append([x0, y0, x0 + rng.uniform(8, 38), y0 + rng.uniform(8, 28)])
        return frame, np.array(bb, np.float64).reshape(-1, 4)
    return source


def _scorer(tree, net, max_boxes, cameras):
    from vec_vad_amd.multistream import MultiStreamScorer
    return MultiStreamScorer(tree['c'], *tree['arts'], (H, W, 3), cameras, flownet2=net, max_boxes=max_boxes)


def _play(sc, script, source, sync_error_from=None, refuse_before=None):
    """The calls of ``script`` through ``sc``.  Returns per call the list of ``(camera, frame, (score, box_scores, kept))``, waited for
    after the last call.  ``sync_error_from``: calls from that index on run under torch's sync debug mode 'error'.  ``refuse_before``:
    ahead of that call a push whose last camera hands over a float32 frame is tried; it must raise and change nothing."""
    cams = sc.cameras
    calls = []
    try:
        for i, (kind, arg) in enumerate(script):
            if refuse_before == i:
                assert kind == 'push' and arg[cams - 1] is not None
                items = [source(k, fi) if fi is not None else (None, None) for k, fi in enumerate(arg)]
                frames = [it[0] for it in items]
                frames[cams - 1] = frames[cams - 1].astype(np.float32)
                before = ([s.count for s in sc.sched.cams], list(sc.frames), [id(h) for h in sc.held], sc.raw_ring.clone())
                with pytest.raises(ValueError, match='uint8 frames') as e:
                    sc.push(frames, [it[1] for it in items])
                assert '\n' not in str(e.value)
                assert before[:3] == ([s.count for s in sc.sched.cams], list(sc.frames), [id(h) for h in sc.held])
                assert torch.equal(before[3], sc.raw_ring)
            if sync_error_from is not None and i >= sync_error_from:
                torch.cuda.set_sync_debug_mode('error')
            if kind == 'push':
                items = [source(k, fi) if fi is not None else (None, None) for k, fi in enumerate(arg)]
                res = sc.push([it[0] for it in items], [it[1] for it in items])
            else:
                res = sc.end_video(arg)
            torch.cuda.set_sync_debug_mode('default')
            assert [r.camera for r in res] == sorted(r.camera for r in res) and all(r.dropped == 0 for r in res)
            assert len({id(r._event) for r in res}) <= 1                                  # one event for the tick
            calls.append(res)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return [[(r.camera, r.frame, r.wait()) for r in res] for res in calls]


def _restate(tree, net, m, script, source, cams=3):
    """The results of ``script`` from the existing API only, at the launch sizes of a ``cams``-camera scorer of ``m`` boxes: flows from
    ``chunk_flows`` on the tick's stacked pair frames in camera order at ``cams`` pairs per launch; cubes and energies from
    ``cube_cut`` / ``cube_energy`` into a store of ``cams * m`` slots; ``score_index_list`` at launches of ``cams * m`` cubes;
    ``scoring.cube_scores`` and the maximum over the boxes that paint a pixel.  Returns ``(calls, info)``: per call what ``_play``
    returns; per call ``dict(issuing, idle, mid_video, rounds)``."""
    import test as S
    from calc_optical_flow import chunk_flows
    from utils import calc_block_idx
    from vad_datasets import frame_size
    from vec_vad_amd import scoring
    from vec_vad_amd.extract import boxes_to_crops, cube_cut, cube_energy
    from vec_vad_amd.trainer import FusedTrainer
    c, (net_set, st_r, st_o) = tree['c'], tree['arts']
    cp, method = c['cp'], c['method']
    gh, gw = frame_size['UCSDped2'][:2]
    h_step, w_step = gh / c['h_block'], gw / c['w_block']
    mode, thr = cp.getint('UCSDped2', 'test_block_mode'), cp.getfloat('UCSDped2', 'motionThr')
    T, Tf = cp.getint(method, 'context_frame_num') + 1, cp.getint(method, 'context_of_num') + 1
    store_raw = torch.zeros((cams * m, T, P, P, 3), dtype=torch.uint8, device='cuda')
    store_flow = torch.zeros((cams * m, Tf, P, P, 2), dtype=torch.float32, device='cuda')
    trainers = {}
    video = [[] for _ in range(cams)]                         # per camera: the (frame, boxes) of its current video
    flows = [{} for _ in range(cams)]                         # per camera: frame of the current video -> its flow field
    pushes = [0] * cams
    calls, info = [], []
    for kind, arg in script:
        if kind == 'push':
            idle = [k for k, fi in enumerate(arg) if fi is None and not video[k]]
            for k, fi in enumerate(arg):
                if fi is not None:
                    video[k].append(source(k, fi))
            issues = [(k, len(video[k]) - 2, False) for k, fi in enumerate(arg) if fi is not None and len(video[k]) >= 2]
            ended = []
        else:
            ended = [k for k in (range(cams) if arg is None else arg) if video[k]]
            idle = [k for k in range(cams) if not video[k]]
            issues = [(k, len(video[k]) - 1, True) for k in ended]
        mid_video = [k for k in range(cams) if video[k] and k not in ended]
        out, rounds = [], 0
        if issues:
            # the flows of the tick: one launch of `cams` pairs, the pairs in camera order
            stack, pairs = [], []
            for k, t, last in issues:
                a, b = (t - 1, t) if last else ((t, t) if t == 0 else (t, t + 1))
                pairs.append((len(stack), len(stack) + 1))
                stack += [video[k][a][0], video[k][b][0]]
            fl = torch.empty((len(issues), H, W, 2), device='cuda')
            chunk_flows(net, torch.from_numpy(np.stack(stack)).cuda(), pairs, np.arange(len(issues)), fl, cams)
            per = []
            for j, (k, t, last) in enumerate(issues):
                flows[k][t] = fl[j].clone()
                boxes = video[k][t][1]
                n = len(boxes)
                crops, paints = boxes_to_crops(boxes, H, W), scoring.box_paints(boxes, gh, gw)
                cells = [sorted(calc_block_idx(bb[0], bb[2], bb[1], bb[3], h_step, w_step, mode=mode)) if paints[b] else []
                         for b, bb in enumerate(boxes)]
                rstack = torch.from_numpy(np.stack([video[k][max(t - T + 1 + i, 0)][0] for i in range(T)])).cuda()
                fstack = torch.stack([flows[k][max(t - Tf + 1 + i, 0)] for i in range(Tf)])
                keep = cube_energy(fstack, crops, np.tile(np.arange(Tf, dtype=np.int32), (n, 1)), P, thr)[1].cpu().numpy().astype(bool) \
                    if n else np.zeros(0, bool)
                per.append(dict(k=k, n=n, crops=crops, cells=cells, rstack=rstack, fstack=fstack, keep=keep, score=np.full(n, -float(BIG))))
            rounds = max((p['n'] + m - 1) // m for p in per)
            for r in range(rounds):
                ids, owner = [], []
                for p in per:
                    lo, hi = r * m, min(p['n'], (r + 1) * m)
                    if hi <= lo:
                        continue
                    slots = (p['k'] * m + np.arange(hi - lo)).astype(np.int32)
                    cube_cut(p['rstack'], p['crops'][lo:hi], np.tile(np.arange(T, dtype=np.int32), (hi - lo, 1)), slots, P, store_raw)
                    cube_cut(p['fstack'], p['crops'][lo:hi], np.tile(np.arange(Tf, dtype=np.int32), (hi - lo, 1)), slots, P, store_flow)
                    ids += slots.tolist()
                    owner += [(p, b) for b in range(lo, hi)]
                for (hh, ww) in sorted({cell for p, b in owner for cell in p['cells'][b]}):
                    models = net_set[hh][ww]
                    if models:
                        if id(models[0]) not in trainers:
                            trainers[id(models[0])] = FusedTrainer(models[0])
                        e_r, e_o = S.score_index_list(trainers[id(models[0])], store_raw, store_flow, np.array(ids, np.int64), c['score_batch'],
                                                      batch=cams * m)
                        so = st_o[hh][ww] if c['useFlow'] else (0.0, 1.0)
                        stats, cube_stat = np.array([[st_r[hh][ww][0], st_r[hh][ww][1], so[0], so[1]]], np.float64), np.zeros(len(ids), np.int32)
                    else:
                        e_r, e_o, stats, cube_stat = torch.zeros(len(ids), device='cuda'), None, np.array([[0.0, 1.0, 0.0, 1.0]]), np.full(len(ids), -1, np.int32)
                    sc = scoring.cube_scores(e_r, e_o if c['useFlow'] else None, cube_stat, stats, c['w_raw'], c['w_of']).cpu().numpy()
                    for (p, b), v in zip(owner, sc):
                        if p['keep'][b] and (hh, ww) in p['cells'][b]:
                            p['score'][b] = max(p['score'][b], float(v))
            for p in per:
                out.append((p['k'], pushes[p['k']] - 1, (float(p['score'].max()) if p['n'] else -float(BIG), p['score'], p['keep'])))
        calls.append(out)
        info.append(dict(issuing=[k for k, _, _ in issues], idle=idle, mid_video=mid_video, rounds=rounds, ended=ended))
        if kind == 'push':
            for k, fi in enumerate(arg):
                pushes[k] += fi is not None
        for k in ended:
            video[k], flows[k] = [], {}
    return calls, info


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert [(k, f) for k, f, _ in g] == [(k, f) for k, f, _ in w], i
        for (k, f, (gs, gb, gk)), (_, _, (ws, wb, wk)) in zip(g, w):
            assert gk.tolist() == wk.tolist(), (i, k, f)
            assert np.array_equal(_bits(gb), _bits(wb)), (i, k, f, gb, wb)
            assert _bits(gs) == _bits(ws), (i, k, f, gs, ws)


_plain = {}


def _plain_run(tree, net, m):
    """The run of ``SCRIPT`` on the fixture at ``m`` boxes, made once and shared by the tests that compare with it (never changed)."""
    if m not in _plain:
        _plain[m] = _play(_scorer(tree, net, m, 3), SCRIPT, _fixture_source(tree))
    return _plain[m]


@pytest.mark.parametrize('max_boxes', [8, 2], ids=['one-round', 'rounds'])
def test_one_camera_equals_the_stream_scorer(tree, net, monkeypatch, max_boxes):
    monkeypatch.chdir(tree['root'])
    want = _stream(tree, net, max_boxes)
    sc = _scorer(tree, net, max_boxes, 1)
    got = []
    for i, (f, b) in enumerate(zip(tree['frames'], tree['boxes'])):
        if i and tree['fvi'][i] != tree['fvi'][i - 1]:
            got += sc.end_video()
        got += sc.push([f], [b])
    got += sc.end_video([0])
    assert [(r.camera, r.frame) for r in got] == [(0, i) for i in range(len(tree['frames']))]
    for f, (r, (ws, wb, wk)) in enumerate(zip(got, want)):
        gs, gb, gk = r.wait()
        assert gk.tolist() == wk.tolist() and gk.dtype == wk.dtype, f
        assert np.array_equal(_bits(gb), _bits(wb)) and _bits(gs) == _bits(ws), (f, gs, ws)
        assert np.array_equal(r.boxes, np.asarray(tree['boxes'][f], np.float64).reshape(-1, 5)[:, :4])
    assert sum(-BIG < r.wait()[0] < BIG for r in got) >= 3


@pytest.mark.parametrize('max_boxes', [8, 2], ids=['one-round', 'rounds'])
def test_three_cameras_out_of_phase_equal_the_restatement_at_the_same_launch_sizes(tree, net, monkeypatch, max_boxes):
    monkeypatch.chdir(tree['root'])
    got = _plain_run(tree, net, max_boxes)
    want, info = _restate(tree, net, max_boxes, SCRIPT, _fixture_source(tree))
    assert any(i['issuing'] and i['idle'] for i in info)                                  # a tick with an idle camera
    assert any(len(i['ended']) == 1 and len(i['mid_video']) == 2 for i in info)           # one camera ends while the others are mid-video
    assert any(len(i['issuing']) == 3 for i in info) and any(len(i['issuing']) == 1 for i in info)
    assert (max(i['rounds'] for i in info) > 1) == (max_boxes < max(COUNTS))              # a tick of more than one round
    if max_boxes == 2:
        assert max(i['rounds'] for i in info) == 3 and any(i['rounds'] > 1 and len(i['issuing']) > 1 for i in info)
    _same(got, want)
    results = [r for call in got for r in call]
    assert sorted((k, f) for k, f, _ in results) == [(0, f) for f in range(7)] + [(1, f) for f in range(7)] + [(2, f) for f in range(4)]
    kept_all = np.concatenate([k for _, _, (_, _, k) in results])
    assert kept_all.any() and not kept_all.all()                                           # the motion test keeps some boxes and drops others
    assert sum(-BIG < s < BIG for _, _, (s, _, _) in results) >= 3                         # frames scored by a trained model


@pytest.mark.parametrize('max_boxes', [8, 2], ids=['one-round', 'rounds'])
def test_a_camera_does_not_see_the_other_cameras(tree, net, monkeypatch, max_boxes):
    """The run again with the frames of cameras 0 and 2 replaced by noise and their boxes moved and recounted (so the rounds of the
    ticks change too): every result of camera 1 is bit-identical."""
    monkeypatch.chdir(tree['root'])
    plain = _plain_run(tree, net, max_boxes)
    noisy = _play(_scorer(tree, net, max_boxes, 3), SCRIPT, _noise_source(tree, 1))
    mine = lambda calls: [[r for r in call if r[0] == 1] for call in calls]
    _same(mine(noisy), mine(plain))
    others = lambda calls: [s for call in calls for k, _, (s, _, _) in call if k != 1]
    assert others(noisy) != others(plain)                                                  # the other cameras did score something else


def test_push_and_end_video_do_not_synchronise(tree, net, monkeypatch):
    """From the second videos on every ``push`` and ``end_video`` runs under ``torch.cuda.set_sync_debug_mode('error')``: a synchronising
    call would raise.  ``wait()`` is called after the mode is back to its default.  The scores are those of the plain run."""
    monkeypatch.chdir(tree['root'])
    strict = _play(_scorer(tree, net, 8, 3), SCRIPT, _fixture_source(tree), sync_error_from=SECOND)
    _same(strict, _plain_run(tree, net, 8))


def test_a_tick_of_three_cameras_launches_what_a_tick_of_one_camera_does(tree, net, monkeypatch):
    """A one-round tick whose boxes all lie in block (0, 0): one replay of the flow graph and one scoring launch, for three cameras as
    for one."""
    from vec_vad_amd.trainer import FusedTrainer
    monkeypatch.chdir(tree['root'])
    count = dict(replay=0, score_cubes=0)
    plain = FusedTrainer.score_cubes

    def score_cubes(self, *a, **k):
        count['score_cubes'] += 1
        return plain(self, *a, **k)

    class Counting:
        def __init__(self, graph):
            self.graph = graph

        def replay(self):
            count['replay'] += 1
            return self.graph.replay()

    src = _fixture_source(tree)
    for cams in (3, 1):
        sc = _scorer(tree, net, 8, cams)
        monkeypatch.setattr(sc, 'flow_graph', Counting(sc.flow_graph))
        monkeypatch.setattr(FusedTrainer, 'score_cubes', score_cubes)
        first, second = [src(k, 0) for k in range(cams)], [src(k, 1) for k in range(cams)]
        assert sc.push([f for f, _ in first], [b for _, b in first]) == [] and count == dict(replay=0, score_cubes=0)
        res = sc.push([f for f, _ in second], [b for _, b in second])
        assert len(res) == cams and all(len(r.boxes) == COUNTS[0] > 0 for r in res)
        assert count == dict(replay=1, score_cubes=1), (cams, count)
        assert all(len(r.wait()[1]) == COUNTS[0] for r in res)
        monkeypatch.setattr(FusedTrainer, 'score_cubes', plain)
        count.update(replay=0, score_cubes=0)


def test_a_refused_push_leaves_every_camera_as_it_was(tree, net, monkeypatch):
    monkeypatch.chdir(tree['root'])
    got = _play(_scorer(tree, net, 8, 3), SCRIPT, _fixture_source(tree), refuse_before=SECOND)
    _same(got, _plain_run(tree, net, 8))


def test_stream_main_with_two_cameras(tree, net, monkeypatch, capsys):
    """``stream.main`` with ``stream_cameras = 2``: video A goes to camera 0, video B to camera 1; the written scores are those of a
    ``MultiStreamScorer`` driven by hand in the documented schedule, bit for bit, and lie where ``stream_cameras = 1`` puts its own."""
    import stream as STREAM
    import train as T
    from utils import save_roc_pr_curve_data
    monkeypatch.chdir(tree['root'])
    saved = open('config.cfg').read()
    assert saved.count('\nstream_cameras = 1\n') == 1
    one = STREAM.main('config.cfg', flownet2=net)
    try:
        open('config.cfg', 'w').write(saved.replace('\nstream_cameras = 1\n', '\nstream_cameras = 2\n'))
        c = T.read_config('config.cfg')
        assert c['stream_cameras'] == 2
        capsys.readouterr()
        two = STREAM.main('config.cfg', flownet2=net)
        out = capsys.readouterr().out
        written = np.load('results/UCSDped2/stream_scores_obj_det_with_motion_SelfComplete.npy')
        auc_file = float(np.load('results/UCSDped2/raw2flow_obj_det_with_motion_SelfComplete_stream_results.npz')['roc_auc'])
    finally:
        open('config.cfg', 'w').write(saved)
    assert written.dtype == np.float64 and np.array_equal(written, two) and two.shape == one.shape == (sum(N_VIDEO),)
    labels = np.load('data/raw2flow/UCSDped2_frame_labels_test.npy')
    auc = save_roc_pr_curve_data(written, labels, 'own.npz', verbose=False)
    assert 'Frame-level AUC of the stream is {}'.format(auc) in out.splitlines() and auc_file == auc
    # by hand: frames 0..3 on camera 0 and 4..6 on camera 1 in lockstep; B ends with its third frame, A one tick later
    from vec_vad_amd.multistream import MultiStreamScorer
    sc = MultiStreamScorer(c, *tree['arts'], (H, W, 3), 2, flownet2=net)
    assert sc.cap == c['stream_max_boxes']
    script = [('push', (0, 4)), ('push', (1, 5)), ('push', (2, 6)), ('end', [1]), ('push', (3, None)), ('end', [0])]
    hand = np.full(sum(N_VIDEO), -float(BIG))
    first = (0, N_VIDEO[0])                                                                # a camera's first test frame
    for call in _play(sc, script, _fixture_source(tree)):
        for k, f, (s, _, _) in call:
            hand[first[k] + f] = s
    assert np.array_equal(_bits(hand), _bits(two)), (hand, two)
    assert ((one > -BIG) == (two > -BIG)).all() and (two > -BIG).sum() >= 3
    print('stream.main at stream_cameras = 2 against 1: largest |difference| of a frame score = %.3e' % np.abs(one - two).max())
