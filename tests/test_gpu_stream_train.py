"""GPU: training from pushed frames (vec_vad_amd/stream_train.py, stream_train.py) -- ``vv_stream_append`` against the numpy restatement
of tests/stream_train_restatement.py, ``StreamCollector`` against ``foreground.extract_train_device`` on the synthetic tree of
tests/test_gpu_direct_train.py (given boxes and motion boxes), ``stream_train.main`` against ``train.main`` with direct_train, direct_flow
and one pair per launch, ``push`` under torch's sync debug mode, and a store that is too small.  Every comparison is bit for bit: a copy
has no round-off, and both routes run the same arithmetic on the same frames in the same order."""
import glob
import os
import shutil

import numpy as np
import pytest
import torch

from stream_train_restatement import stream_append as restated
from test_gpu_direct_train import (HB, MODEL, OF_SC, RAW_SC, WB, _assert_same_outputs, _cfg, _outputs, _quiet, _remove_outputs, _train,
                                   _tree)

pytestmark = pytest.mark.gpu

CAP, CAPACITY, T = 5, 7, 5
# (keep, n) per launch: three of five kept | all of three: the cursor goes to 6 | all of four: cube 6 is written and three cubes fall past
# the capacity, the cursor goes to 10 | nothing | the cursor at or past the capacity and n = 9 clamped to cap: only the cursor moves |
# n = -3 clamped to 0
SEQUENCE = (([1, 0, 1, 1, 0], 5), ([1, 1, 1, 1, 1], 3), ([1, 1, 1, 1, 1], 4), ([1, 1, 1, 1, 1], 0), ([1, 1, 0, 1, 1], 9), ([1, 1, 1, 1, 1], -3))
CURSORS = (3, 6, 10, 10, 14, 14)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _sentinels(C, Tf, P, cells):
    return dict(raw=np.full((CAPACITY, T, P, P, C), 201, np.uint8), flow=np.full((CAPACITY, Tf, P, P, 2), -7.5, np.float32),
                meta=np.full((CAPACITY, 2), -9, np.int32), mbox=np.full((CAPACITY, 4), -9, np.int32),
                cells=np.full((CAPACITY, max(cells, 1)), 77, np.uint8))


def _round(rng, C, Tf, P, cells, keep, n):
    """The slots of one round: random bytes and values, NaN and Inf in every flow slot that is not kept (unkept, or at or above n)."""
    raw = rng.integers(0, 256, (CAP, T, P, P, C), dtype=np.uint8)
    flow = rng.standard_normal((CAP, Tf, P, P, 2)).astype(np.float32)
    for b in range(CAP):
        if not (b < n and keep[b]):
            flow[b] = np.nan
            flow[b].reshape(-1)[::3] = np.inf
    masks = rng.integers(0, 2, (cells, CAP), dtype=np.uint8)
    boxes = rng.integers(-5, 400, (CAP, 4)).astype(np.int32)
    return raw, flow, masks, boxes


# C, Tf, P, cells, boxes given: P = 32 always takes the 16-byte path; P = 6 with C = 3 has 540-byte raw cubes and P = 5 200-byte flow cubes
CASES = [(1, 1, 32, 0, False), (3, 5, 32, 4, True), (1, 5, 32, 1, True), (3, 1, 32, 4, False), (3, 1, 6, 1, True), (3, 1, 5, 4, False)]


@pytest.mark.parametrize('C,Tf,P,cells,with_boxes', CASES)
def test_stream_append_equals_the_numpy_restatement(C, Tf, P, cells, with_boxes):
    from vec_vad_amd.stream_train import stream_append

    def sequence():
        rng = np.random.default_rng(100 * C + 10 * Tf + P + cells)
        want = _sentinels(C, Tf, P, cells)
        got = {k: _cu(v) for k, v in want.items()}
        state = torch.zeros(2, dtype=torch.int32, device='cuda')
        cursor = 0
        for i, (keep, n) in enumerate(SEQUENCE):
            raw, flow, masks, boxes = _round(rng, C, Tf, P, cells, keep, n)
            keep = np.array(keep, np.uint8)
            stream_append(_cu(raw), _cu(flow), _cu(keep), _cu(np.array([n], np.int32)), _cu(masks), _cu(boxes) if with_boxes else None,
                          40 + i, 5 * i, state[i % 2:i % 2 + 1], state[(i + 1) % 2:(i + 1) % 2 + 1], got['raw'], got['flow'], got['meta'],
                          got['mbox'], got['cells'])
            new = restated(raw, flow, keep, n, masks, boxes if with_boxes else None, 40 + i, 5 * i, cursor, want['raw'], want['flow'],
                           want['meta'], want['mbox'], want['cells'][:, :cells])
            assert new == CURSORS[i]
            assert state.tolist()[(i + 1) % 2] == new and state.tolist()[i % 2] == cursor, i      # the cell that was read is not written
            cursor = new
            for k in want:                                             # cubes, tables and every sentinel outside the written cubes
                assert np.array_equal(_bytes(got[k]), _bytes(want[k])), (i, k)
        return {k: _bytes(v) for k, v in got.items()}, want

    first, want = sequence()
    again, _ = sequence()
    assert all(np.array_equal(first[k], again[k]) for k in first)     # a repeated sequence gives the same bytes
    assert np.isfinite(want['flow']).all()                             # no NaN or Inf of an unkept slot reached the store
    assert (want['raw'][:CAPACITY] != 201).any() and want['meta'][6].tolist() == [42, 10] and want['meta'][5].tolist() == [41, 7]
    if cells == 0:
        assert (want['cells'] == 77).all()
    if not with_boxes:
        assert (want['mbox'] == 0).all()


def test_refused_calls_return_their_status_and_write_nothing():
    from vec_vad_amd import _lib
    from vec_vad_amd.stream_train import stream_append
    rng = np.random.default_rng(1)
    raw, flow, masks, boxes = _round(rng, 3, 1, 32, 4, [1] * CAP, CAP)
    S = {k: _cu(v) for k, v in _sentinels(3, 1, 32, 4).items()}
    before = {k: _bytes(v) for k, v in S.items()}
    state = torch.tensor([0, -1], dtype=torch.int32, device='cuda')
    dv = dict(raw=_cu(raw), flow=_cu(flow), keep=_cu(np.ones(CAP, np.uint8)), n=_cu(np.array([CAP], np.int32)), masks=_cu(masks))
    f = _lib.lib().vv_stream_append
    p = lambda t: t.data_ptr()                                         # noqa: E731

    def call(cap=CAP, rb=int(raw[0].size), fb=4 * int(flow[0].size), masks=p(dv['masks']), cells=4, cin=p(state), cout=p(state) + 4,
             capacity=CAPACITY, n=p(dv['n']), keep=p(dv['keep']), meta=p(S['meta'])):
        return f(p(dv['raw']), p(dv['flow']), keep, n, cap, rb, fb, masks, cells, None, 0, 0, cin, cout, capacity, p(S['raw']), p(S['flow']),
                 meta, p(S['mbox']), p(S['cells']), torch.cuda.current_stream().cuda_stream)

    for kw in (dict(cap=0), dict(cells=-1), dict(capacity=-1), dict(rb=-1), dict(fb=-1), dict(masks=None), dict(cout=p(state)),
               dict(n=None), dict(keep=None), dict(cin=None), dict(cout=None), dict(meta=None)):
        assert call(**kw) == 1, kw                                     # VV_ERR_BAD_ARG
    with pytest.raises(ValueError):                                    # the wrapper's own checks: mask rows of another cap
        stream_append(dv['raw'], dv['flow'], dv['keep'], dv['n'], dv['masks'][:, :4].contiguous(), None, 0, 0, state[0:1], state[1:2],
                      S['raw'], S['flow'], S['meta'], S['mbox'], S['cells'])
    with pytest.raises(_lib.VecVadHipError, match='VV_ERR_BAD_ARG'):
        stream_append(dv['raw'], dv['flow'], dv['keep'], dv['n'], dv['masks'], None, 0, 0, state[0:1], state[0:1], S['raw'], S['flow'],
                      S['meta'], S['mbox'], S['cells'])
    torch.cuda.synchronize()
    assert state.tolist() == [0, -1] and all(np.array_equal(_bytes(S[k]), before[k]) for k in S)
    assert call() == 0 and state.tolist() == [0, CAP]                  # the good call, last


# ---- the collector against extract_train_device ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net():
    from FlowNet2_src import FlowNet2
    torch.manual_seed(0)
    return FlowNet2().cuda().eval()


def _reference(c, net):
    """The store and groups of ``extract_train_device`` and the boxes of its cubes (``extract_device`` hands them out), computed once."""
    import foreground as FG
    st = FG.extract_train_device(c, 'cuda', log=_quiet, flownet2=net)
    info, parts = FG.extract_device(c, 'train', 'cuda', log=_quiet, flownet2=net)
    part = next(parts)
    assert part['n'] == st['n'] and info['n_frames'] == st['n_frames']
    n = st['n']
    return dict(n=n, n_frames=st['n_frames'], raw=st['raw'][:n].clone(), flow=st['flow'][:n].clone(), groups=st['groups'],
                boxes=part['boxes'].copy())


@pytest.fixture(scope='module')
def tree(tmp_path_factory, net):
    """The 7-frame tree of tests/test_gpu_direct_train.py without its ``optical_flow/`` directory, the configuration with direct_train,
    direct_flow and one pair per launch, the three output files of ``train.main`` on it (removed again), and the reference store."""
    root = tmp_path_factory.mktemp('stream_train')
    back = os.getcwd()
    os.chdir(root)
    try:
        cfg = _tree()
        shutil.rmtree('optical_flow')
        c = _cfg(cfg, direct_train=True, direct_flow=True, direct_flow_pairs=1)
        cfg = open('config.cfg').read()
        _train(flownet2=net)
        out = _outputs()
        _remove_outputs()
        ref = _reference(c, net)
        assert _no_staged_file()
    finally:
        os.chdir(back)
    return dict(root=str(root), cfg=cfg, c=c, out=out, ref=ref)


def _no_staged_file():
    return not os.path.exists('optical_flow') and glob.glob('data/raw2flow/*foreground_*') == []


def _split(c, motion=False):
    """The frames of the training split, the video of each, and what goes into ``push`` behind each frame."""
    import foreground as FG
    from vad_datasets import get_inputs
    if motion:
        indexer = FG._datasets(c, 'train', None, direct_flow=True)[0]
        boxes = [None] * len(indexer)
    else:
        st = FG._stage(c, 'train', direct_flow=True)
        indexer, boxes = st.raw_ds, list(st.boxes)
    frames = [get_inputs(indexer.all_frame_addr[i]) for i in range(len(indexer))]
    return frames, list(indexer.frame_video_idx), boxes


def _collect(c, net, max_boxes, boxes='given', max_cubes=64, sync_error_after=None, finish=True):
    from vec_vad_amd.stream_train import StreamCollector
    frames, fvi, given = _split(c, boxes == 'motion')
    col = StreamCollector(c, frames[0].shape, flownet2=net, max_boxes=max_boxes, max_cubes=max_cubes, boxes=boxes)
    try:
        for i, f in enumerate(frames):
            if i and fvi[i] != fvi[i - 1]:
                assert col.end_video() is None
            if sync_error_after is not None and i == sync_error_after:
                torch.cuda.set_sync_debug_mode('error')
            assert (col.push(f) if given[i] is None else col.push(f, given[i])) is None
        col.end_video()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return (col, col.finish()) if finish else col


def _assert_same_store(got, ref):
    n = ref['n']
    assert got['n'] == n and got['n_frames'] == ref['n_frames'] and got['raw'].dtype == torch.uint8 and got['flow'].dtype == torch.float32
    assert torch.equal(got['raw'][:n], ref['raw']) and torch.equal(got['flow'][:n].view(torch.int32), ref['flow'].view(torch.int32))
    assert sorted(got['groups']) == sorted(ref['groups'])
    for k, (idx, off) in ref['groups'].items():
        assert got['groups'][k][0].dtype == np.int64 and got['groups'][k][1].dtype == np.int32
        assert np.array_equal(got['groups'][k][0], idx) and np.array_equal(got['groups'][k][1], off), k
    assert got['boxes'].dtype == np.float64 and np.array_equal(got['boxes'], ref['boxes'])


@pytest.mark.parametrize('max_boxes', [64, 1], ids=['one-round', 'rounds'])
def test_collector_equals_extract_train_device(tree, net, monkeypatch, max_boxes):
    """64 slots hold every frame's boxes; with 1 every box is a round of its own."""
    monkeypatch.chdir(tree['root'])
    ref = tree['ref']
    _, got = _collect(tree['c'], net, max_boxes)
    _assert_same_store(got, ref)
    assert got['dropped_boxes'] == 0 and ref['n_frames'] == 7
    boxes = np.load('raw_datasets/UCSDped2/bboxes_train_obj_det_with_motion.npy', allow_pickle=True)
    print('kept cubes:', ref['n'], 'of', [len(b) for b in boxes], 'boxes per frame')
    assert 4 < ref['n'] <= sum(len(b) for b in boxes) and max(len(b) for b in boxes) > 1     # several rounds with one slot
    both = set(ref['groups'][(None, 0, 0)][0]) & set(ref['groups'][(None, 0, 1)][0])
    assert both and ref['groups'][(None, 0, 0)][1][2] == ref['groups'][(None, 0, 0)][1][3]   # the two-block box; frame 2 has no box
    assert _no_staged_file()


def test_collector_equals_extract_train_device_when_the_motion_test_drops_boxes(tree, net, monkeypatch):
    """FlowNet2's fields leave no box of the tree below ``motionThr = 0``, so the run above keeps every slot of every round.  Here the
    threshold lies between the energies of the weakest third of the cubes and the rest (taken from the reference store's flow cubes;
    the gap is checked), so that rounds with unkept slots in front of kept ones occur: the same store and lists again."""
    import train as T
    monkeypatch.chdir(tree['root'])
    flow = tree['ref']['flow'].double()
    e = np.sort((flow * flow).sum(dim=(1, 2, 3, 4)).cpu().numpy() / flow.shape[1])
    q = len(e) // 3
    assert q >= 1 and e[q] - e[q - 1] > 1e-6 * e[q]
    try:
        open('config.cfg', 'w').write(tree['cfg'].replace('[UCSDped2]\n', '[UCSDped2]\nmotionThr = %r\n' % float((e[q - 1] + e[q]) / 2)))
        c = T.read_config('config.cfg')
        ref = _reference(c, net)
        assert ref['n'] == len(e) - q
        for max_boxes in (64, 2):
            _assert_same_store(_collect(c, net, max_boxes)[1], ref)
    finally:
        open('config.cfg', 'w').write(tree['cfg'])


def test_motion_collector_equals_extract_train_device_on_the_boxes_load_bboxes_forms(tree, net, monkeypatch):
    import foreground as FG
    import train as T
    monkeypatch.chdir(tree['root'])
    path = 'raw_datasets/UCSDped2/bboxes_train_obj_det_with_motion.npy'
    saved = path + '.given'
    os.rename(path, saved)
    try:
        open('config.cfg', 'w').write(tree['cfg'].replace('[UCSDped2]\n', '[UCSDped2]\ntrain_bbox_saved = False\n'))
        c = T.read_config('config.cfg')
        assert not c['cp'].getboolean('UCSDped2', 'train_bbox_saved') and c['direct_flow_pairs'] == 1
        boxes = FG.load_bboxes(c, 'train', log=_quiet)                 # the motion boxes of the batch route, written to `path`
        counts = [len(b) for b in boxes]
        print('motion boxes per frame:', counts)
        assert len(counts) == 7 and max(counts) >= 1
        ref = _reference(c, net)
        assert ref['n'] >= 1
        os.remove(path)                                                # the collector reads no box file
        _, got = _collect(c, net, max(counts), boxes='motion')
        assert not os.path.exists(path)
        _assert_same_store(got, ref)
        assert got['dropped_boxes'] == 0 and isinstance(got['dropped_boxes'], int)
    finally:
        if os.path.exists(path):
            os.remove(path)
        os.rename(saved, path)
        open('config.cfg', 'w').write(tree['cfg'])


# ---- no synchronisation, capacity --------------------------------------------------------------------------------------------------------
def test_push_and_end_video_do_not_synchronise(tree, net, monkeypatch):
    """From the second video on every ``push`` and ``end_video`` runs under ``torch.cuda.set_sync_debug_mode('error')``: a synchronising
    call would raise.  ``finish()`` is called after the mode is back to its default.  The store is that of the run without the mode."""
    monkeypatch.chdir(tree['root'])
    _, fvi, _ = _split(tree['c'])
    second = fvi.index(fvi[-1])
    assert 0 < second < len(fvi) - 1
    for mode, max_boxes in (('given', 2), ('motion', 8)):
        _, plain = _collect(tree['c'], net, max_boxes, boxes=mode)
        _, strict = _collect(tree['c'], net, max_boxes, boxes=mode, sync_error_after=second)
        n = plain['n']
        assert strict['n'] == n and torch.equal(strict['raw'][:n], plain['raw'][:n])
        assert torch.equal(strict['flow'][:n].view(torch.int32), plain['flow'][:n].view(torch.int32))
        assert np.array_equal(strict['boxes'], plain['boxes']) and strict['dropped_boxes'] == plain['dropped_boxes']
    _assert_same_store(_collect(tree['c'], net, 2)[1], tree['ref'])


def test_a_store_too_small_raises_in_finish_with_the_number_needed(tree, net, monkeypatch):
    monkeypatch.chdir(tree['root'])
    n = tree['ref']['n']
    col = _collect(tree['c'], net, 3, max_cubes=n - 1, finish=False)
    with pytest.raises(ValueError, match='collect_max_cubes') as e:
        col.finish()
    assert '\n' not in str(e.value) and str(n) in str(e.value) and str(n - 1) in str(e.value)      # needed, allowed
    assert col.store is None
    frames, _, given = _split(tree['c'])
    for call in (lambda: col.push(frames[0], given[0]), col.end_video, col.finish, col.train):
        with pytest.raises(ValueError):                                # no partial set, and no way on
            call()
    col, got = _collect(tree['c'], net, 3, max_cubes=n)               # exactly enough: fine
    _assert_same_store(got, tree['ref'])
    with pytest.raises(ValueError, match='finished'):
        col.push(frames[0], given[0])
    assert col.finish() is got


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_stream_train_main_equals_train_main_and_its_models_score_alike(tree, net, monkeypatch, capsys):
    """``stream_train.main`` writes the three files of ``train.main`` with direct_train, direct_flow and one pair per launch; no
    ``optical_flow/`` directory and no ``foreground_*`` file before or after.  A ``StreamScorer`` built from what it returns gives, on
    the test split, the scores of one built by ``load_artifacts`` from those files."""
    import foreground as FG
    import stream_train as ST
    import test as S
    import train as T
    from vad_datasets import get_inputs
    from vec_vad_amd.stream import StreamScorer
    monkeypatch.chdir(tree['root'])
    _remove_outputs()
    assert _no_staged_file()
    torch.manual_seed(5)                                               # as test_gpu_direct_train._train seeds the initial weights
    arts = ST.main('config.cfg', flownet2=net)
    assert _no_staged_file() and all(os.path.exists(p) for p in (MODEL, RAW_SC, OF_SC))
    trained = _assert_same_outputs(tree['out'], _outputs())
    out = capsys.readouterr().out
    assert 'training scores saved!' in out and 'dropped' not in out
    c = tree['c']
    filed = S.load_artifacts(os.path.join('data', 'raw2flow', 'UCSDped2_'), c['mode_fg'], c['method'], False, lambda: T.build_network(c),
                             torch.device('cuda'))
    assert sum(len(arts[0][h][w]) for h in range(HB) for w in range(WB)) == trained
    for a, b in zip(arts[1:], filed[1:]):                              # the statistics: the same numbers
        assert np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64))
    st = FG._stage(c, 'test', direct_flow=True)
    frames = [get_inputs(st.raw_ds.all_frame_addr[i]) for i in range(len(st.raw_ds))]
    scores = []
    for art in (arts, filed):
        sc = StreamScorer(c, *art, frames[0].shape, flownet2=net, max_boxes=8)
        res = []
        for f, b in zip(frames, st.boxes):
            res += sc.push(f, b)
        res += sc.end_video()
        scores.append([r.wait() for r in res])
    assert len(scores[0]) == len(frames) == 4
    for (sa, ba, ka), (sb, bb, kb) in zip(*scores):
        assert np.float64(sa).tobytes() == np.float64(sb).tobytes() and ba.tobytes() == bb.tobytes() and ka.tolist() == kb.tolist()
    assert any(-1e5 < s < 1e5 for s, _, _ in scores[0])               # a frame scored by a trained model
    _remove_outputs()
