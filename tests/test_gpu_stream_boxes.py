"""GPU: the stream scorer that finds its own motion boxes (``StreamScorer(boxes='motion')``, vec_vad_amd/stream.py) -- ``vv_stream_boxes``
against the numpy restatement of tests/stream_boxes_restatement.py, the scorer against ``motion.motion_boxes`` and a second scorer that
is given those boxes, the one-round overflow rule, ``push`` under torch's sync debug mode, ``stream.main`` against ``test.main`` without
a box file, and the refusals.  Every comparison is exact: both sides run the same arithmetic on the same inputs."""
import glob
import os
import shutil

import numpy as np
import pytest
import torch

import stream_boxes_restatement as R
from _util import small_config

pytestmark = pytest.mark.gpu

def _big():
    from vec_vad_amd.scoring import BIG as b
    return float(b)


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------------------------
GRID = dict(H=48, W=72, grid_h=96, grid_w=144, hb=2, wb=3)      # a 48x72 frame in a 2x3 grid of 48x48 cells
CAP = 8
BOXES = np.array([[40, 4, 70, 20],        # centre in column 1, its left corners and left edge mid-point in column 0
                  [24, 8, 72, 48],        # touches the right and the bottom frame edge; centre x = 48: 48 / 48 is exactly column 1
                  [40, 10, 56, 30],       # centre x = 48 again, both corners' probes (44, 52) on either side of the boundary
                  [10, 10, 30, 30],
                  [0, 0, 4, 4],
                  [60, 30, 72, 48],
                  [20, 20, 50, 46],       # centre x = 35; its right probes (50 + 35) / 2 = 42.5 stay in column 0
                  [47, 0, 49, 48],        # two pixels wide across the boundary: centre 48 -> column 1, left probe 47.5 -> column 0
                  [1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], np.int32)      # rows 8.. lie behind mcap = 8 and are never read


def _run_kernel(count, mcap, n_ap, block_mode, GRID=GRID, BOXES=BOXES):
    from vec_vad_amd.stream import stream_boxes
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    poison = dict(crops=np.full((CAP, 4), -77, np.int32), masks=np.full((GRID['hb'] * GRID['wb'], CAP), 9, np.uint8),
                  boxes_out=np.full((CAP, 4), -55, np.int32))
    n, dropped = cu(np.array([-5], np.int32)), cu(np.array([-6], np.int32))
    crops, masks, out = cu(poison['crops']), cu(poison['masks']), cu(poison['boxes_out'])
    table = cu(BOXES)                                                # the whole table is there; the kernel is told mcap rows
    stream_boxes(cu(np.array([count], np.int32)), table[:mcap], n_ap, GRID['H'], GRID['W'], GRID['grid_h'], GRID['grid_w'], GRID['hb'],
                 GRID['wb'], GRID['grid_h'] / GRID['hb'], GRID['grid_w'] / GRID['wb'], block_mode, n, dropped, crops, masks, out)
    want = R.stream_boxes(count, BOXES[:mcap], n_ap, CAP, block_mode=block_mode, **GRID, **poison)
    got = (int(n.cpu()[0]), int(dropped.cpu()[0]), crops.cpu().numpy(), masks.cpu().numpy(), out.cpu().numpy())
    return got, want


@pytest.mark.parametrize('n_ap', [0, 3])
@pytest.mark.parametrize('block_mode', [1, 5, 9])
def test_stream_boxes_kernel_equals_the_restatement(block_mode, n_ap):
    free = CAP - n_ap
    cases = [(0, 8), (1, 8), (free, 8), (free + 2, 8), (11, 8), (7, 4)]      # (count, mcap); the last: mcap binds before the free slots
    seen_multi = False
    for count, mcap in cases:
        (n, dropped, crops, masks, out), want = _run_kernel(count, mcap, n_ap, block_mode)
        m = min(count, mcap, free)
        assert (n, dropped) == (want[0], want[1]) == (n_ap + m, count - m), (count, mcap)
        assert np.array_equal(crops, want[2]) and np.array_equal(masks, want[3]) and np.array_equal(out, want[4]), (count, mcap)
        # the poison: appearance slots and slots at or above n keep it; the motion columns of the masks at or above n read 0
        assert (crops[:n_ap] == -77).all() and (crops[n:] == -77).all() and (out[:n_ap] == -55).all() and (out[n:] == -55).all()
        assert (masks[:, :n_ap] == 9).all() and not masks[:, n:].any() and masks[:, n_ap:].max(initial=0) <= 1
        assert np.array_equal(out[n_ap:n], BOXES[:m]) and np.array_equal(crops[n_ap:n], BOXES[:m])
        assert not masks[GRID['wb']:, n_ap:].any()                   # the frame lies in the first row of cells
        seen_multi |= bool((masks[:, n_ap:n].sum(axis=0) > 1).any())
    assert seen_multi == (block_mode > 1)                            # a box in two cells, once the probes leave the centre


# a 96x72 frame that fills both rows of a 2x3 grid of 48 (high) x 40 (wide) cells: the steps differ, and so do hb and wb
TALL = dict(H=96, W=72, grid_h=96, grid_w=120, hb=2, wb=3)
TALL_BOXES = np.array([[10, 50, 30, 90],      # row 1, column 0
                       [30, 40, 60, 60],      # centre (50, 45): row 1, column 1; its upper probes (40 + 50) / 2 = 45 in row 0, left 37.5 in column 0
                       [50, 4, 72, 96],       # the full height at the right edge: centre (50, 61) -> row 1, column 1; top probes row 0
                       [42, 70, 70, 96]], np.int32)      # centre x = 56 -> column 1, right probe (70 + 56) / 2 = 63 too, left probe 49 too


@pytest.mark.parametrize('block_mode', [1, 5, 9])
def test_stream_boxes_kernel_rows_and_unequal_steps(block_mode):
    """Mask bits below the first row of cells, with h_step != w_step and hb != wb: an exchange of the two steps or of the two grid
    sizes, in the kernel or in the wrapper, changes the expected bytes."""
    wb = TALL['wb']
    for n_ap in (0, 3):
        (n, dropped, crops, masks, out), want = _run_kernel(4, 4, n_ap, block_mode, TALL, TALL_BOXES)
        assert (n, dropped) == (want[0], want[1]) == (n_ap + 4, 0)
        assert np.array_equal(crops, want[2]) and np.array_equal(masks, want[3]) and np.array_equal(out, want[4])
        assert masks[0 * wb + 0:, n_ap + 0].tolist() == [0, 0, 0, 1, 0, 0]                 # the first box: cell (1, 0) alone
        assert masks[1 * wb + 1, n_ap + 1] == 1 and masks[1 * wb + 1, n_ap + 2] == 1
        assert bool(masks[0 * wb + 0, n_ap + 1]) == (block_mode >= 9)                      # the upper left corner's probe
        assert bool(masks[0 * wb + 1, n_ap + 2]) == (block_mode > 1)                       # the upper edge's mid-point
        assert not masks[:, n_ap:n][[2, 5]].any()                                          # nothing reaches column 2 (x >= 80)


def test_stream_boxes_bad_arguments_return_without_a_launch():
    from vec_vad_amd import _lib
    l = _lib.lib()
    t = torch.zeros(64, dtype=torch.int32, device='cuda')
    p, st = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    good = [p, p, 8, 0, 8, 48, 72, 96, 144, 2, 3, 48.0, 48.0, 9, p, p, p, p, p, st]
    for i, v in ((0, None), (1, None), (14, None), (15, None), (16, None), (17, None), (18, None), (2, -1), (3, -1), (3, 9), (4, 0),
                 (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 0.0), (12, float('nan')), (13, 0)):
        args = list(good)
        args[i] = v
        assert l.vv_stream_boxes(*args) == 1, i                       # VV_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert not t.any()                                               # and nothing was written


# ---- the synthetic tree ----------------------------------------------------------------------------------------------------------------
H, W, P = R.H, R.W, 32


@pytest.fixture(scope='module')
def net():
    from FlowNet2_src import FlowNet2
    torch.manual_seed(0)
    return FlowNet2().cuda().eval()


@pytest.fixture(scope='module')
def tree(tmp_path_factory, net):
    """The synthetic tree of tests/test_gpu_stream.py (2x2 grid, trained by ``train.main``) with the test split replaced by the two
    videos of ``stream_boxes_restatement.synthetic_frames``, no test box file at all and ``test_bbox_saved = False``.  ``motionThr``
    is picked from the flow energies (one pair per launch) of the boxes of both runs -- the motion boxes alone, and one appearance
    box per frame with the motion boxes that remain -- so that the motion test keeps some boxes and drops others."""
    from PIL import Image
    from test_gpu_scripts import _synthetic_ped2_tree
    import train as T
    import test as S
    from calc_optical_flow import chunk_flows, flow_pairs
    from vad_datasets import context_range
    from vec_vad_amd.extract import boxes_to_crops, cube_energy
    from vec_vad_amd.motion import motion_boxes
    root = tmp_path_factory.mktemp('stream_boxes')
    back = os.getcwd()
    os.chdir(root)
    try:
        _synthetic_ped2_tree(np.random.default_rng(11))
        path = os.path.join('raw_datasets', 'UCSDped2', 'bboxes_train_obj_det_with_motion.npy')
        train_boxes = np.load(path, allow_pickle=True)
        for i in range(len(train_boxes)):      # two boxes per training frame in block (0, 0), where the 48x72 frames lie: it gets a model
            train_boxes[i] = np.concatenate([train_boxes[i], [[100.0, 70.0, 140.0, 110.0, 0.9], [110.0, 66.0, 160.0, 100.0, 0.9]]])
        np.save(path, train_boxes, allow_pickle=True)
        cfg = small_config()
        T.main('config.cfg')
        shutil.rmtree('raw_datasets/UCSDped2/Test')
        shutil.rmtree('optical_flow/UCSDped2/Test')
        os.remove(os.path.join('raw_datasets', 'UCSDped2', 'bboxes_test_obj_det_with_motion.npy'))
        frames, fvi = R.synthetic_frames()
        n = len(frames)
        for k, (g, v) in enumerate(zip(frames, fvi)):
            name, j = 'Test%03d' % v, fvi[:k].count(v)
            os.makedirs(os.path.join('raw_datasets', 'UCSDped2', 'Test', name), exist_ok=True)
            os.makedirs(os.path.join('raw_datasets', 'UCSDped2', 'Test', name + '_gt'), exist_ok=True)
            Image.fromarray(g).save(os.path.join('raw_datasets', 'UCSDped2', 'Test', name, '%03d.tif' % (j + 1)))
            gt = np.zeros((H, W), np.uint8)
            if k % 2:
                gt[10:20, 10:30] = 255
            Image.fromarray(gt).save(os.path.join('raw_datasets', 'UCSDped2', 'Test', name + '_gt', '%03d.bmp' % (j + 1)))
        c = T.read_config('config.cfg')
        assert c['cp'].getint('SelfComplete', 'context_of_num') == 4
        # the boxes of both runs, from the batch route's own function on the same three frames
        fr = torch.from_numpy(np.stack(frames)[..., None].repeat(3, axis=3)).cuda()
        wins = R.motion_windows(fvi)
        ap = R.appearance_boxes()
        found = {'plain': motion_boxes(fr, wins, None, 'UCSDped2'), 'covered': motion_boxes(fr, wins, [a[:, :4] for a in ap], 'UCSDped2')}
        boxes = {'plain': [np.asarray(m, np.float64).reshape(-1, 4) for m in found['plain']],
                 'covered': [np.concatenate([a[:, :4], np.asarray(m, np.float64).reshape(-1, 4)]) for a, m in zip(ap, found['covered'])]}
        # the flow energy of every box, as the direct route forms it at one pair per launch and context_of_num = 4
        fl = torch.empty((n, H, W, 2), device='cuda')
        chunk_flows(net, fr, flow_pairs(fvi, range(n)), np.arange(n), fl, 1)
        every = [(i, b) for run in ('plain', 'covered') for i, bb in enumerate(boxes[run]) for b in bb]
        crops = boxes_to_crops([b for _, b in every], H, W)
        win = np.array([context_range(i, 'predict', 4, n, fvi) for i, _ in every], np.int32)
        e = np.unique(cube_energy(fl, crops, win, P, 0.0)[0].cpu().numpy())
        q = len(e) // 3                                              # the weakest third of the energies is dropped
        assert q >= 1 and e[q - 1] < e[q]
        thr = float((e[q - 1] + e[q]) / 2)
        cfg = cfg.replace('[UCSDped2]\n', '[UCSDped2]\nmotionThr = %r\ntest_bbox_saved = False\n' % thr)
        cfg = cfg.replace('direct_test = False', 'direct_test = True').replace('direct_flow = False', 'direct_flow = True')
        cfg = cfg.replace('direct_flow_pairs = 4', 'direct_flow_pairs = 1')
        cfg = cfg.replace('\nstream_max_boxes = 64\n', '\nstream_max_boxes = %d\n' % R.CAP)
        open('config.cfg', 'w').write(cfg)
        c = T.read_config('config.cfg')
        assert c['direct_test'] and c['direct_flow'] and c['direct_flow_pairs'] == 1 and c['h_block'] == 2 and c['stream_max_boxes'] == R.CAP
        assert c['stream_boxes'] == 'given' and not c['cp'].getboolean('UCSDped2', 'test_bbox_saved')
        arts = S.load_artifacts(os.path.join('data', 'raw2flow', 'UCSDped2_'), c['mode_fg'], c['method'], False, lambda: T.build_network(c),
                                torch.device('cuda'))
        assert len(arts[0][0][0]) == 1                               # block (0, 0), where every test box lies, has a model
    finally:
        os.chdir(back)
    return dict(root=str(root), c=c, arts=arts, frames=[np.repeat(f[..., None], 3, axis=2) for f in frames], fvi=fvi, ap=ap, boxes=boxes,
                cfg=cfg)


@pytest.fixture(scope='module')
def scorer(tree, net):
    """``scorer(mode, max_boxes)``: one ``StreamScorer`` per mode and launch size for the whole module (a scorer starts over with every
    video, so the runs of several tests go through it one after the other)."""
    from vec_vad_amd.stream import StreamScorer
    made = {}

    def get(mode, max_boxes):
        if (mode, max_boxes) not in made:
            made[(mode, max_boxes)] = StreamScorer(tree['c'], *tree['arts'], (H, W, 3), flownet2=net, max_boxes=max_boxes, boxes=mode)
        return made[(mode, max_boxes)]

    return get


def _run(sc, tree, boxes, sync_error_after=None):
    """All frames of the tree through ``sc``; ``boxes``: per frame what goes into ``push`` behind the frame (None: nothing).  Returns per
    frame ``(score, box_scores, kept, boxes, dropped)``."""
    res, first = [], sc.frames
    try:
        for i, f in enumerate(tree['frames']):
            if i and tree['fvi'][i] != tree['fvi'][i - 1]:
                res += sc.end_video()
            if sync_error_after is not None and i == sync_error_after:
                torch.cuda.set_sync_debug_mode('error')
            res += sc.push(f) if boxes is None else sc.push(f, boxes[i])
        res += sc.end_video()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert [r.frame - first for r in res] == list(range(len(tree['frames'])))
    return [r.wait() + (r.boxes, r.dropped) for r in res]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _same(got, want, f):
    assert got[2].tolist() == want[2].tolist(), f
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (f, got[1], want[1])
    assert _bits(got[0]) == _bits(want[0]), (f, got[0], want[0])


# ---- 2. the scorer against motion_boxes and a scorer that is given the boxes -----------------------------------------------------------------
@pytest.mark.parametrize('run', ['plain', 'covered'])
def test_motion_scorer_equals_motion_boxes_and_the_given_scorer(tree, scorer, monkeypatch, run):
    monkeypatch.chdir(tree['root'])
    big = _big()
    want_boxes = tree['boxes'][run]
    got = _run(scorer('motion', R.CAP), tree, None if run == 'plain' else tree['ap'])
    want = _run(scorer('given', R.CAP), tree, want_boxes)
    n_ap = 0 if run == 'plain' else 1
    for f, (g, w, b) in enumerate(zip(got, want, want_boxes)):
        assert g[3].dtype == np.float64 and np.array_equal(g[3], b), (f, g[3], b)      # the boxes read back: appearance rows first
        assert g[4] == 0 and isinstance(g[4], int) and w[4] == 0 and np.array_equal(w[3], b)
        assert len(g[1]) == len(g[2]) == len(b)
        _same(g, w, f)
    counts = [len(b) - n_ap for b in want_boxes]
    assert sum(k >= 2 for k in counts) >= 2 and counts[-1] == 0      # frames with several motion boxes, and one with none
    kept = np.concatenate([g[2] for g in got])
    assert kept.any() and not kept.all()                             # the motion test keeps some boxes and drops others
    assert sum(-big < g[0] < big for g in got) >= 3                  # frames scored by a trained model
    if run == 'plain':
        assert got[-1][0] == -big and len(got[-1][1]) == 0           # no box at all
    else:
        plain = tree['boxes']['plain']
        assert sum(len(p) == len(c) for p, c in zip(plain, want_boxes)) >= 4          # a motion box left, the appearance box came: slot 0
        assert all(np.array_equal(c[0], a[0, :4]) for c, a in zip(want_boxes, tree['ap']))
        assert any(g[2][0] and g[1][0] > -big for g in got)          # an appearance box in slot 0 that was kept and scored


# ---- 3. overflow -----------------------------------------------------------------------------------------------------------------------
def test_overflow_drops_the_last_motion_boxes_and_counts_them(tree, scorer, monkeypatch):
    monkeypatch.chdir(tree['root'])
    boxes = tree['boxes']['plain']
    most = max(len(b) for b in boxes)
    cap = most - 1
    assert cap >= 1
    got = _run(scorer('motion', cap), tree, None)
    first = [b[:cap] for b in boxes]                                 # the first of motion_boxes' list: vv_mask_boxes' emission order
    want = _run(scorer('given', cap), tree, first)
    for f, (g, w, b) in enumerate(zip(got, want, boxes)):
        assert g[4] == (1 if len(b) == most else 0), f
        assert np.array_equal(g[3], first[f]), f
        _same(g, w, f)
    assert sum(g[4] for g in got) >= 1


def test_given_mode_still_cuts_a_frame_whose_only_box_paints_no_pixel(tree, net, monkeypatch):
    """The mode that is off: a lone box with a negative x1 paints no pixel of the score mask (the slice wraps to nothing) and belongs
    to no block, but its crop is valid, so its cube is cut and ``kept`` is the motion test's answer -- that of the same crop under a
    box that does paint.  Its score and the frame's stay at -BIG.  ``motionThr = 0`` here, so that the motion test keeps the cube of
    every frame whose flow is not zero throughout the crop."""
    import re
    import train as T
    from vec_vad_amd.stream import StreamScorer
    monkeypatch.chdir(tree['root'])
    big = _big()
    n = len(tree['frames'])
    cfg, subs = re.subn(r'\nmotionThr = [^\n]*\ntest_bbox_saved', '\nmotionThr = 0\ntest_bbox_saved', tree['cfg'])
    assert subs == 1
    open('config_thr0.cfg', 'w').write(cfg)
    c = T.read_config('config_thr0.cfg')
    assert c['cp'].getfloat('UCSDped2', 'motionThr') == 0.0
    sc = StreamScorer(c, *tree['arts'], (H, W, 3), flownet2=net, max_boxes=R.CAP, boxes='given')
    off = _run(sc, tree, [np.array([[-3.0, 5.0, 40.0, 40.0]])] * n)
    on = _run(sc, tree, [np.array([[0.0, 5.0, 40.0, 40.0]])] * n)
    assert [g[2].tolist() for g in off] == [g[2].tolist() for g in on]
    assert any(g[2][0] for g in off) and all(len(g[2]) == 1 for g in off)
    assert all(g[0] == -big and g[1].tolist() == [-big] for g in off)
    assert any(g[0] > -big for g in on)


# ---- 4. no synchronisation -------------------------------------------------------------------------------------------------------------
def test_push_does_not_synchronise_in_motion_mode(tree, scorer, monkeypatch):
    """From the second video on every ``push`` and ``end_video`` runs under ``torch.cuda.set_sync_debug_mode('error')``; ``wait()`` is
    called after the mode is back to its default.  With and without appearance boxes."""
    monkeypatch.chdir(tree['root'])
    sc = scorer('motion', R.CAP)
    second = tree['fvi'].index(2)
    for given in (None, tree['ap']):
        plain = _run(sc, tree, given)
        strict = _run(sc, tree, given, sync_error_after=second)
        assert [_bits(s[0]).tolist() for s in strict] == [_bits(s[0]).tolist() for s in plain]
        assert all(np.array_equal(a[3], b[3]) for a, b in zip(strict, plain))


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------
def test_stream_main_in_motion_mode_equals_test_main_without_a_box_file(tree, net, monkeypatch, capsys):
    import stream as STREAM
    import test as S
    monkeypatch.chdir(tree['root'])
    assert not glob.glob('raw_datasets/UCSDped2/bboxes_test_*')
    open('config.cfg', 'w').write(tree['cfg'].replace('\nstream_boxes = given\n', '\nstream_boxes = motion\n'))
    try:
        B = STREAM.main('config.cfg', flownet2=net)                   # first: test.main writes the box file it computes
        out = capsys.readouterr().out
        assert not glob.glob('raw_datasets/UCSDped2/bboxes_test_*')  # neither loaded nor written
        assert 'dropped' not in out and 'motion boxes only' in out
        S.main('config.cfg', flownet2=net)
        A = np.load('results/UCSDped2/frame_scores_obj_det_with_motion_SelfComplete.npy')
        saved = np.load('raw_datasets/UCSDped2/bboxes_test_obj_det_with_motion.npy', allow_pickle=True)
        assert max(len(b) for b in saved) <= R.CAP and [len(b) for b in saved] == [len(b) for b in tree['boxes']['plain']]
        big = _big()
        assert B.shape == A.shape == (len(tree['frames']),) and (A > -big).sum() >= 3
        assert np.array_equal(A, B), (A, B)
    finally:
        for p in glob.glob('raw_datasets/UCSDped2/bboxes_test_*'):   # the other tests of the module run without a box file
            os.remove(p)
        open('config.cfg', 'w').write(tree['cfg'])


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(tree, scorer, net, monkeypatch):
    from vec_vad_amd import _lib
    from vec_vad_amd.stream import StreamScorer
    monkeypatch.chdir(tree['root'])
    with pytest.raises(ValueError, match='larger than the nominal') as e:
        StreamScorer(tree['c'], *tree['arts'], (240, 361, 3), flownet2=net, max_boxes=4, boxes='motion')
    assert '\n' not in str(e.value)
    sc = scorer('motion', R.CAP)
    count, frames = sc.sched.count, sc.frames
    many = np.tile(np.array([[4.0, 4.0, 30.0, 30.0]]), (R.CAP + 1, 1))

    def launched(*a, **k):
        raise AssertionError('a kernel was launched')

    l = _lib.lib()
    for name in ('vv_stream_boxes', 'vv_stream_cut', 'vv_motion_mask', 'vv_mask_boxes', 'vv_flow_pairs_prep'):
        monkeypatch.setattr(l, name, launched)
    with pytest.raises(ValueError, match='appearance boxes') as e:
        sc.push(tree['frames'][0], ap_boxes=many)
    assert '\n' not in str(e.value)
    assert (sc.sched.count, sc.frames, sc.held) == (count, frames, None)      # no ring was touched
    # a scorer that is given its boxes has no box-free push
    with pytest.raises(ValueError, match='stream_boxes = motion'):
        scorer('given', R.CAP).push(tree['frames'][0])
