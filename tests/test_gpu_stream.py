"""GPU: frame-by-frame scoring (vec_vad_amd/stream.py, stream.py) -- ``vv_stream_cut`` against ``extract.cube_cut`` / ``cube_energy``,
``vv_stream_scores`` against the numpy restatement of tests/stream_restatement.py, ``StreamScorer`` against the existing API at the same
launch size, ``stream.main`` against ``test.main``, and ``push`` under torch's sync debug mode.  The kernel and scorer comparisons are bit
for bit: both sides run the same arithmetic in the same order on the same inputs."""
import os
import shutil

import numpy as np
import pytest
import torch

from _util import small_config
from stream_restatement import BIG, stream_scores as restated

pytestmark = pytest.mark.gpu

H, W, P, CAP = 48, 72, 32, 4
# x0, y0, x1, y1: narrower than 32 px (upscaled) | non-integer downscale | exactly 32 x 32 | touching the right and bottom frame edges
CROPS = np.array([[5, 3, 25, 40], [10, 2, 60, 45], [20, 8, 52, 40], [30, 10, 72, 48]], np.int32)
WINDOWS = {'wrapped': ([3, 4, 5, 0, 1], [3, 4, 0, 1, 2]), 'repeated': ([2, 2, 2, 2, 3], [2, 2, 2, 2, 3])}      # raw ring of 6, flow ring of 5


def _rings(C):
    rng = np.random.default_rng(5 + C)
    raw = torch.from_numpy(rng.integers(0, 256, (6, H, W, C), dtype=np.uint8)).cuda()
    flow = rng.standard_normal((5, H, W, 2)).astype(np.float32) * np.linspace(0.2, 3.0, W, dtype=np.float32)[None, None, :, None]
    return raw, torch.from_numpy(flow).cuda()


@pytest.mark.parametrize('n', [0, 1, CAP])
@pytest.mark.parametrize('window', sorted(WINDOWS))
@pytest.mark.parametrize('C', [1, 3])
def test_stream_cut_equals_cube_cut_and_cube_energy(C, window, n):
    from vec_vad_amd.extract import cube_cut, cube_energy
    from vec_vad_amd.stream import stream_cut
    raw, flow = _rings(C)
    wr, wf = (np.array(w, np.int32) for w in WINDOWS[window])
    all_e, _ = cube_energy(flow, CROPS, np.tile(wf, (CAP, 1)), P, 0.0)
    e_sorted = np.sort(all_e.cpu().numpy())
    assert e_sorted[1] < e_sorted[2]
    thr = float((e_sorted[1] + e_sorted[2]) / 2)                     # keeps two of the four boxes and drops two
    # reference: the batch route's kernels on the same frames, crops and windows, into a poisoned store
    ref_raw = torch.full((CAP, 5, P, P, C), 201, dtype=torch.uint8, device='cuda')
    ref_flow = torch.full((CAP, 5, P, P, 2), -7.5, device='cuda')
    cube_cut(raw, CROPS[:n], np.tile(wr, (n, 1)), np.arange(n, dtype=np.int32), P, ref_raw)
    cube_cut(flow, CROPS[:n], np.tile(wf, (n, 1)), np.arange(n, dtype=np.int32), P, ref_flow)
    ref_e, ref_keep = cube_energy(flow, CROPS[:n], np.tile(wf, (n, 1)), P, thr)
    got_raw, got_flow = torch.full_like(ref_raw, 201), torch.full_like(ref_flow, -7.5)
    keep = torch.full((CAP,), 9, dtype=torch.uint8, device='cuda')
    energy = torch.full((CAP,), -3.0, dtype=torch.float64, device='cuda')
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    stream_cut(raw, flow, dv([n]), dv(CROPS), dv(wr), dv(wf), thr, got_raw, got_flow, keep, energy)
    assert torch.equal(got_raw, ref_raw)                             # the cubes, and the poison in slots >= n
    assert torch.equal(got_flow, ref_flow)
    assert torch.equal(keep[:n], ref_keep) and torch.equal(energy[:n], ref_e)
    assert bool((keep[n:] == 9).all()) and bool((energy[n:] == -3.0).all())
    if n == CAP:
        assert sorted(keep.tolist()) == [0, 0, 1, 1]                 # both classes occur
        assert bool((got_raw != 201).any()) and bool((got_flow != -7.5).any())


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def test_stream_scores_equals_the_numpy_restatement():
    """A 1x2 grid, 5 boxes in 8 slots: boxes 0-2 in block 0, boxes 2-4 in block 1 (box 2 in both), box 1 dropped by the motion test.
    NaN and 1e30 sit in the padded slots and in the dropped box.  Launch by launch the box rows and the frame cell must be the
    restatement's, bit for bit; then a block without a model, and a frame with nothing kept."""
    from vec_vad_amd.stream import stream_scores
    rng = np.random.default_rng(3)
    cap, n = 8, 5
    raw = (rng.random(cap) * 40).astype(np.float32)
    of = (rng.random(cap) * 9).astype(np.float32)
    raw[[1, 5, 6, 7]] = [np.nan, 1e30, np.nan, np.inf]
    of[[1, 5, 6, 7]] = [1e30, np.nan, np.inf, np.nan]
    keep = np.array([1, 0, 1, 1, 1, 1, 1, 1], np.uint8)
    masks = [np.array([1, 1, 1, 0, 0, 1, 1, 1], np.uint8), np.array([0, 0, 1, 1, 1, 1, 1, 1], np.uint8)]
    stats = [(17.3, 4.1, 3.9, 1.7), (21.0, 3.3, 5.2, 2.9)]
    w_raw, w_of = 0.7, 1.3
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def run(keep, blocks, use_of=True):
        """blocks: (mask, stats | None) per launch.  Returns the device results and the restated ones."""
        rows = torch.full((len(blocks), cap), 55.5, dtype=torch.float64, device='cuda')
        cell = torch.full((1,), -float(BIG), dtype=torch.float64, device='cuda')
        want_rows, want_cell = [], -float(BIG)
        for i, (mask, st) in enumerate(blocks):
            stream_scores(cu(raw), cu(of) if use_of else None, cu(np.array(st, np.float64)) if st is not None else None, w_raw, w_of,
                          cu(keep), cu(np.array([n], np.int32)), cu(mask), rows[i], cell)
            row, want_cell = restated(raw, of if use_of else None, st, w_raw, w_of, keep, n, mask, np.full(cap, 55.5), want_cell)
            want_rows.append(row)
        return rows.cpu().numpy(), float(cell.cpu()[0]), np.stack(want_rows), want_cell

    for use_of in (True, False):
        got_rows, got_cell, want_rows, want_cell = run(keep, [(masks[0], stats[0]), (masks[1], stats[1])], use_of)
        assert np.array_equal(_bits(got_rows), _bits(want_rows)) and _bits(got_cell) == _bits(want_cell)
        assert np.isfinite(got_rows).all() and (got_rows[:, n:] == 55.5).all()          # nothing of the padded slots got anywhere
        assert got_rows[0, 1] == -BIG and got_rows[0, 3] == -BIG and got_rows[1, 0] == -BIG
        assert got_cell == max(got_rows[0, [0, 2]].max(), got_rows[1, [2, 3, 4]].max()) and -BIG < got_cell < BIG
        assert got_rows[0, 2] != got_rows[1, 2]                                          # the box in both blocks: one score per model
    # block 1 has no model: its kept boxes score +BIG, and so does the frame
    got_rows, got_cell, want_rows, want_cell = run(keep, [(masks[0], stats[0]), (masks[1], None)])
    assert np.array_equal(_bits(got_rows), _bits(want_rows)) and got_cell == want_cell == BIG
    assert got_rows[1, :n].tolist() == [-BIG, -BIG, BIG, BIG, BIG]
    # nothing kept: the cell stays at -BIG and every box below n reads -BIG
    got_rows, got_cell, want_rows, want_cell = run(np.zeros(cap, np.uint8), [(masks[0], stats[0]), (masks[1], None)])
    assert np.array_equal(_bits(got_rows), _bits(want_rows)) and got_cell == want_cell == -BIG
    assert (got_rows[:, :n] == -BIG).all()


# ---- the scorer against the existing API ------------------------------------------------------------------------------------------------
N_VIDEO = (4, 3)                          # two videos; the first has context_frame_num frames, as context_range needs at the head of a split
COUNTS = (3, 2, 0, 5, 1, 3, 2)            # boxes per frame: an empty frame, and one with more boxes than the small launch size


@pytest.fixture(scope='module')
def net():
    from FlowNet2_src import FlowNet2
    torch.manual_seed(0)
    return FlowNet2().cuda().eval()


@pytest.fixture(scope='module')
def tree(tmp_path_factory, net):
    """The synthetic tree trained by ``train.main`` (2x2 grid, as test_gpu_direct_flow.py's ``staged`` does), then its test split
    replaced by two videos of grey 48x72 frames cut from a pattern that slides 2 px per frame, with boxes inside them and a
    ``motionThr`` picked from the boxes' flow energies (at one pair per launch) so that the motion test keeps some and drops others."""
    from PIL import Image
    from test_gpu_scripts import _synthetic_ped2_tree
    import train as T
    import test as S
    from calc_optical_flow import chunk_flows, flow_pairs
    from vec_vad_amd.extract import boxes_to_crops, cube_energy
    root = tmp_path_factory.mktemp('stream')
    back = os.getcwd()
    os.chdir(root)
    try:
        _synthetic_ped2_tree(np.random.default_rng(11))
        # 48x72 frames lie in block (0, 0) of the 2x2 grid over the nominal 240x360 frame: two moving boxes per training frame there,
        # so that this block gets a model
        path = os.path.join('raw_datasets', 'UCSDped2', 'bboxes_train_obj_det_with_motion.npy')
        train_boxes = np.load(path, allow_pickle=True)
        for i in range(len(train_boxes)):
            train_boxes[i] = np.concatenate([train_boxes[i], [[100.0, 70.0, 140.0, 110.0, 0.9], [110.0, 66.0, 160.0, 100.0, 0.9]]])
        np.save(path, train_boxes, allow_pickle=True)
        cfg = small_config()
        T.main('config.cfg')
        shutil.rmtree('raw_datasets/UCSDped2/Test')
        shutil.rmtree('optical_flow/UCSDped2/Test')
        rng = np.random.default_rng(4)
        n = sum(N_VIDEO)
        base = rng.integers(0, 256, (H, W + 2 * n), dtype=np.uint8)
        frames, boxes, k = [], [], 0
        for v, length in enumerate(N_VIDEO, start=1):
            name = 'Test%03d' % v
            os.makedirs(os.path.join('raw_datasets', 'UCSDped2', 'Test', name))
            os.makedirs(os.path.join('raw_datasets', 'UCSDped2', 'Test', name + '_gt'))
            for j in range(length):
                g = np.ascontiguousarray(base[:, 2 * k:2 * k + W])
                Image.fromarray(g).save(os.path.join('raw_datasets', 'UCSDped2', 'Test', name, '%03d.tif' % (j + 1)))
                gt = np.zeros((H, W), np.uint8)
                if k % 2:
                    gt[10:20, 10:30] = 255
                Image.fromarray(gt).save(os.path.join('raw_datasets', 'UCSDped2', 'Test', name + '_gt', '%03d.bmp' % (j + 1)))
                bb = []
                for _ in range(COUNTS[k]):
                    x0, y0 = rng.uniform(0, W - 40), rng.uniform(0, H - 30)
                    bb.append([x0, y0, x0 + rng.uniform(8, 38), y0 + rng.uniform(8, 28), rng.random()])
                boxes.append(np.array(bb).reshape(-1, 5))
                frames.append(g)
                k += 1
        arr = np.empty(n, dtype=object)
        for i, b in enumerate(boxes):
            arr[i] = b
        np.save(os.path.join('raw_datasets', 'UCSDped2', 'bboxes_test_obj_det_with_motion.npy'), arr, allow_pickle=True)
        # the flow energy of every box, as the direct route forms it at one pair per launch and context_of_num = 4
        c = T.read_config('config.cfg')
        assert c['cp'].getint('SelfComplete', 'context_of_num') == 4
        from vad_datasets import context_range
        fvi = [v for v, length in enumerate(N_VIDEO, start=1) for _ in range(length)]
        fr = torch.from_numpy(np.stack(frames)[..., None].repeat(3, axis=3)).cuda()
        fl = torch.empty((n, H, W, 2), device='cuda')
        chunk_flows(net, fr, flow_pairs(fvi, range(n)), np.arange(n), fl, 1)
        crops = np.concatenate([boxes_to_crops(b, H, W) for b in boxes if len(b)])
        win = np.concatenate([np.tile(context_range(i, 'predict', 4, n, fvi), (len(b), 1)) for i, b in enumerate(boxes) if len(b)])
        e = np.sort(cube_energy(fl, crops, win.astype(np.int32), P, 0.0)[0].cpu().numpy())
        q = len(e) // 3                                              # the weakest third of the boxes is dropped
        assert e[q - 1] < e[q]
        thr = float((e[q - 1] + e[q]) / 2)
        cfg = cfg.replace('[UCSDped2]\n', '[UCSDped2]\nmotionThr = %r\n' % thr)
        cfg = cfg.replace('direct_test = False', 'direct_test = True').replace('direct_flow = False', 'direct_flow = True')
        cfg = cfg.replace('direct_flow_pairs = 4', 'direct_flow_pairs = 1')
        open('config.cfg', 'w').write(cfg)
        c = T.read_config('config.cfg')
        assert c['direct_test'] and c['direct_flow'] and c['direct_flow_pairs'] == 1 and c['h_block'] == 2
        arts = S.load_artifacts(os.path.join('data', 'raw2flow', 'UCSDped2_'), c['mode_fg'], c['method'], False, lambda: T.build_network(c),
                                torch.device('cuda'))
        assert len(arts[0][0][0]) == 1                               # block (0, 0), where every test box lies, has a model
    finally:
        os.chdir(back)
    return dict(root=str(root), c=c, arts=arts, frames=[np.repeat(f[..., None], 3, axis=2) for f in frames], boxes=boxes, fvi=fvi)


def _stream(tree, net, max_boxes, sync_error_after=None):
    from vec_vad_amd.stream import StreamScorer
    sc = StreamScorer(tree['c'], *tree['arts'], (H, W, 3), flownet2=net, max_boxes=max_boxes)
    res = []
    try:
        for i, (f, b) in enumerate(zip(tree['frames'], tree['boxes'])):
            if i and tree['fvi'][i] != tree['fvi'][i - 1]:
                res += sc.end_video()
            if sync_error_after is not None and i == sync_error_after:
                torch.cuda.set_sync_debug_mode('error')
            res += sc.push(f, b)
        res += sc.end_video()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert [r.frame for r in res] == list(range(len(tree['frames'])))
    return [r.wait() for r in res]


def _reference(tree, net, B):
    """Per frame (score, box scores, kept) from ``foreground.extract_device`` (direct_flow, one pair per launch), ``score_index_list``
    at launches of exactly ``B`` cubes (= ``trainer.score_cubes`` on the frame's cubes padded to ``B``), ``scoring.cube_scores`` and the
    maximum over the boxes that paint a pixel."""
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
    frame = np.full(n, -float(BIG))
    cube = {}
    trainers = {}
    per_frame = [set() for _ in range(n)]
    for (key, hh, ww), (idx, off) in part['groups'].items():
        models = net_set[hh][ww]
        for f in range(n):
            ids = idx[off[f]:off[f + 1]]
            if not len(ids):
                continue
            per_frame[f].update(ids.tolist())
            if models:
                tr = trainers.setdefault(id(models[0]), FusedTrainer(models[0]))
                r, o = S.score_index_list(tr, part['raw'], part['flow'], ids, c['score_batch'], batch=B)
                so = st_o[hh][ww] if c['useFlow'] else (0.0, 1.0)
                stats, cube_stat = np.array([[st_r[hh][ww][0], st_r[hh][ww][1], so[0], so[1]]], np.float64), np.zeros(len(ids), np.int32)
            else:
                r, o, stats, cube_stat = torch.zeros(len(ids), device='cuda'), None, np.array([[0.0, 1.0, 0.0, 1.0]]), np.full(len(ids), -1, np.int32)
            sc = scoring.cube_scores(r, o if c['useFlow'] else None, cube_stat, stats, c['w_raw'], c['w_of']).cpu().numpy()
            for s, v, p in zip(ids.tolist(), sc, scoring.box_paints(part['boxes'][ids], h, w)):
                if p:
                    cube[s] = max(cube.get(s, -float(BIG)), float(v))
                    frame[f] = max(frame[f], float(v))
    out = []
    for f in range(n):
        boxes = np.asarray(tree['boxes'][f], np.float64).reshape(-1, 5)[:, :4]
        kept, score = np.zeros(len(boxes), bool), np.full(len(boxes), -float(BIG))
        j = 0
        for s in sorted(per_frame[f]):                  # the kept cubes of a frame stand in box order
            while not np.array_equal(boxes[j], part['boxes'][s]):
                j += 1
            kept[j], score[j] = True, cube.get(s, -float(BIG))
            j += 1
        out.append((float(frame[f]), score, kept))
    return out


@pytest.mark.parametrize('max_boxes', [8, 2], ids=['one-round', 'rounds'])
def test_stream_scorer_equals_the_batch_api_at_the_same_launch_size(tree, net, monkeypatch, max_boxes):
    """8 holds every frame's boxes; 2 is below the largest count (5 boxes: three rounds)."""
    monkeypatch.chdir(tree['root'])
    assert max(COUNTS) > 2 and max(COUNTS) <= 8
    got, want = _stream(tree, net, max_boxes), _reference(tree, net, max_boxes)
    kept_all = np.concatenate([k for _, _, k in want])
    assert kept_all.any() and not kept_all.all()                     # the motion test keeps some boxes and drops others
    for f, ((gs, gb, gk), (ws, wb, wk)) in enumerate(zip(got, want)):
        assert gk.tolist() == wk.tolist(), f
        assert np.array_equal(_bits(gb), _bits(wb)), (f, gb, wb)
        assert _bits(gs) == _bits(ws), (f, gs, ws)
    assert got[2][0] == -BIG and len(got[2][1]) == 0                 # the frame without boxes
    assert sum(-BIG < s < BIG for s, _, _ in got) >= 3                # frames scored by a trained model


def test_push_does_not_synchronise(tree, net, monkeypatch):
    """From the second video on every ``push`` and ``end_video`` runs under ``torch.cuda.set_sync_debug_mode('error')``: a synchronising
    call would raise.  ``wait()`` is called after the mode is back to its default.  The scores are those of the run without the mode."""
    monkeypatch.chdir(tree['root'])
    plain = _stream(tree, net, 8)
    strict = _stream(tree, net, 8, sync_error_after=N_VIDEO[0])
    assert [s for s, _, _ in strict] == [s for s, _, _ in plain]


def test_stream_main_equals_test_main(tree, net, monkeypatch, capsys):
    """``stream.main`` against ``test.main`` (direct_test, direct_flow, one pair per launch) on the same tree.  ``test.py`` sizes its
    launches from its whole index lists, the stream from ``stream_max_boxes``: the same cubes through launches of another size."""
    import stream as STREAM
    import test as S
    from utils import save_roc_pr_curve_data
    monkeypatch.chdir(tree['root'])
    S.main('config.cfg', flownet2=net)
    A = np.load('results/UCSDped2/frame_scores_obj_det_with_motion_SelfComplete.npy')
    capsys.readouterr()
    B = STREAM.main('config.cfg', flownet2=net)
    out = capsys.readouterr().out
    written = np.load('results/UCSDped2/stream_scores_obj_det_with_motion_SelfComplete.npy')
    assert written.dtype == np.float64 and np.array_equal(written, B) and B.shape == A.shape == (sum(N_VIDEO),)
    labels = np.load('data/raw2flow/UCSDped2_frame_labels_test.npy')
    auc = save_roc_pr_curve_data(written, labels, 'own.npz', verbose=False)
    assert 'Frame-level AUC of the stream is {}'.format(auc) in out.splitlines()
    assert float(np.load('results/UCSDped2/raw2flow_obj_det_with_motion_SelfComplete_stream_results.npz')['roc_auc']) == auc
    diff = np.abs(A - B).max()
    print('stream.main against test.main: largest |difference| of a frame score = %.3e' % diff)
    assert (A > -BIG).sum() >= 3 and ((A > -BIG) == (B > -BIG)).all()
    assert np.array_equal(A, B), (A, B)
