"""GPU: the direct train path ([mi355x] direct_train) -- the store and index lists of ``foreground.extract_train_device`` against
the cube files of ``extract_train``, ``train.train_block`` from a device store against the same loop on numpy segments, and
``train.main`` (then ``test.main``) with and without cube and flow files.  Every comparison is bit for bit: both routes run the same
arithmetic on the same cubes in the same order."""
import glob
import os
import shutil

import numpy as np
import pytest
import torch

from _util import small_config

pytestmark = pytest.mark.gpu

HB = WB = 2
MODEL = 'data/raw2flow/UCSDped2_model_obj_det_with_motion_SelfComplete.npy'
RAW_SC = 'data/raw2flow/UCSDped2_raw_training_scores_obj_det_with_motion_SelfComplete.npy'
OF_SC = 'data/raw2flow/UCSDped2_of_training_scores_obj_det_with_motion_SelfComplete.npy'
CUBES = 'data/raw2flow/UCSDped2_foreground_train_obj_det_with_motion-%s.npy'
SCORES = 'results/UCSDped2/frame_scores_obj_det_with_motion_SelfComplete.npy'
TRAIN_FLOW = 'optical_flow/UCSDped2/Train'
TWO_BLOCK_BOX = [150.0, 70.0, 215.0, 110.0, 0.9]             # centre in block (0, 1), left edge probe in block (0, 0)


def _quiet(*a):
    pass


def _tree():
    """The synthetic UCSDped2 tree (7 training frames in videos of 4 and 3, 4 test frames) on a 2x2 block grid with
    ``train_block_mode = 9``.  Frame 0 keeps its box in the still corner (zero flow: fails ``motionThr``); frame 1 gets a box that
    lies in blocks (0, 0) and (0, 1); frame 2 loses its boxes."""
    from test_gpu_scripts import _synthetic_ped2_tree
    _synthetic_ped2_tree(np.random.default_rng(11))
    path = 'raw_datasets/UCSDped2/bboxes_train_obj_det_with_motion.npy'
    boxes = np.load(path, allow_pickle=True)
    boxes[1] = np.concatenate([np.asarray(boxes[1]).reshape(-1, 5), np.array([TWO_BLOCK_BOX])])
    boxes[2] = np.zeros((0, 5))
    np.save(path, boxes, allow_pickle=True)
    cfg = small_config()
    return cfg


def _cfg(base, **keys):
    """``base`` with ``[mi355x]`` keys set; writes config.cfg and returns the parsed dict."""
    import train as T
    stock = dict(direct_train='False', direct_test='False', direct_flow='False', direct_flow_pairs='4', direct_frames_per_chunk='64',
                 direct_max_cubes='524288')
    cfg = base
    for k, v in keys.items():
        old = '%s = %s' % (k, stock[k])
        assert old in cfg, k
        cfg = cfg.replace(old, '%s = %s' % (k, v))
    open('config.cfg', 'w').write(cfg)
    c = T.read_config('config.cfg')
    for k, v in keys.items():
        assert str(c[k]) == str(v), k
    return c


def _train(**kw):
    """``train.main`` on ./config.cfg with the networks' random initial weights seeded: every run starts from the same model."""
    import train as T
    torch.manual_seed(5)
    return T.main('config.cfg', **kw)


def _outputs():
    load = lambda p: torch.load(p, map_location='cpu', weights_only=False)      # noqa: E731
    return load(MODEL), load(RAW_SC), load(OF_SC)


def _remove_outputs():
    for p in (MODEL, RAW_SC, OF_SC):
        if os.path.exists(p):
            os.remove(p)


def _assert_same_outputs(a, b):
    """The three files of two runs: same nesting, equal tensors (dtype included), equal score arrays; at least one trained block."""
    trained = 0
    for x, y in zip(a, b):
        assert len(x) == len(y) == HB and all(len(x[h]) == len(y[h]) == WB for h in range(HB))
    for h in range(HB):
        for w in range(WB):
            ma, mb = a[0][h][w], b[0][h][w]
            assert len(ma) == len(mb) <= 1, (h, w)
            if ma:
                trained += 1
                assert list(ma[0]) == list(mb[0]) and all(k.startswith('module.') for k in ma[0])
                for k in ma[0]:
                    assert ma[0][k].dtype == mb[0][k].dtype and torch.equal(ma[0][k], mb[0][k]), (h, w, k)
            for sa, sb in ((a[1][h][w], b[1][h][w]), (a[2][h][w], b[2][h][w])):
                assert type(sa) is type(sb), (h, w)
                if isinstance(sa, np.ndarray):
                    assert sa.dtype == sb.dtype and np.array_equal(sa, sb), (h, w)
                    assert np.isfinite(sa).all() and (len(sa) > 1) == bool(ma)
                else:
                    assert sa == sb == [] and not ma
    assert trained >= 1
    return trained


def _cube_files(kind='train'):
    return glob.glob('data/raw2flow/*foreground_%s*' % kind) + (glob.glob('data/raw2flow/*foreground_bbox_test*') if kind != 'train' else [])


# ---- 1: the store against the cube files ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def staged(tmp_path_factory):
    """The tree, ``train.main`` on the staged route (cube files written and read), its three output files."""
    root = tmp_path_factory.mktemp('direct_train')
    back = os.getcwd()
    os.chdir(root)
    try:
        cfg = _tree()
        _train()
        out = _outputs()
        assert len(_cube_files()) == 2
    finally:
        os.chdir(back)
    return dict(root=str(root), cfg=cfg, out=out)


def test_store_and_groups_equal_the_files_of_extract_train(staged, monkeypatch):
    import foreground as FG
    monkeypatch.chdir(staged['root'])
    c = _cfg(staged['cfg'])
    FG.extract_train(c, 'cuda', log=_quiet)
    fset = np.load(CUBES % 'raw', allow_pickle=True)
    fset2 = np.load(CUBES % 'flow', allow_pickle=True)
    boxes = np.load('raw_datasets/UCSDped2/bboxes_train_obj_det_with_motion.npy', allow_pickle=True)
    assert fset.shape == (HB, WB) and len(boxes) == 7 and len(boxes[2]) == 0
    for chunk in (64, 2):
        c['direct_frames_per_chunk'] = chunk
        st = FG.extract_train_device(c, 'cuda', log=_quiet)
        assert st['n_frames'] == 7 and st['raw'].dtype == torch.uint8 and st['flow'].dtype == torch.float32
        n_boxes = sum(len(b) for b in boxes)
        assert 0 < st['n'] < n_boxes                                   # the still-corner boxes failed the motion test
        named = 0
        for h in range(HB):
            for w in range(WB):
                want_r, want_f = np.asarray(fset[h][w]), np.asarray(fset2[h][w])
                if (None, h, w) not in st['groups']:
                    assert len(want_r) == 0 and len(want_f) == 0, (h, w)
                    continue
                idx, off = st['groups'][(None, h, w)]
                assert idx.dtype == np.int64 and idx.max() < st['n'] and off[2] == off[3]        # frame 2 has no box
                sel = torch.from_numpy(idx).cuda()
                got_r, got_f = st['raw'][sel].cpu().numpy(), st['flow'][sel].cpu().numpy()
                assert got_r.dtype == want_r.dtype and got_r.shape == want_r.shape and np.array_equal(got_r, want_r), (h, w)
                assert got_f.dtype == want_f.dtype and got_f.shape == want_f.shape and np.array_equal(got_f, want_f), (h, w)
                named += len(idx)
        both = set(st['groups'][(None, 0, 0)][0]) & set(st['groups'][(None, 0, 1)][0])
        assert both and named > st['n']                                # the two-block box: one slot, two lists
        assert named == sum(len(np.asarray(fset[h][w])) for h in range(HB) for w in range(WB))
    assert len(_cube_files()) == 2                                     # the device route wrote no cube file of its own


# ---- 2: the loop on a store against the loop on numpy segments -------------------------------------------------------------------
def _net4(seed):
    from oracle import unet_oracle as O
    from model.unet import SelfCompleteNet4
    net = SelfCompleteNet4(features_root=32, tot_raw_num=5, tot_of_num=1, border_mode='predict', rawRange=None, useFlow=True,
                           padding=False)
    net.load_state_dict(O.seeded_state_dict('net4', nf=32, padding=False, seed=seed))
    return net


def test_train_block_from_a_store_equals_train_block_from_arrays():
    """11 cubes of a store of 16 (two full batches of 4 and a kept partial one of 3), two epochs, so that eager, capturing and
    replayed steps all occur: the state_dict and both score vectors of the two forms are equal."""
    import train as T
    from oracle import unet_oracle as O
    raw, flow = O.seeded_cubes(16, 1, 77)
    block_idx = np.array([0, 2, 3, 5, 6, 7, 9, 10, 12, 13, 15], np.int64)
    logs = [], []
    sd_a, r_a, o_a = T.train_block(_net4(0), [lambda: (raw[block_idx], flow[block_idx])], 2, 4, shuffle_seed=0, log=logs[0].append)
    store = (torch.from_numpy(raw).cuda(), torch.from_numpy(flow).cuda())
    sd_b, r_b, o_b = T.train_block(_net4(0), [(store[0], store[1], block_idx)], 2, 4, shuffle_seed=0, log=logs[1].append)
    assert list(sd_a) == list(sd_b) and len(sd_a) > 0
    for k in sd_a:
        assert sd_a[k].dtype == sd_b[k].dtype and torch.equal(sd_a[k], sd_b[k]), k
    assert r_a.shape == (11,) and o_a.shape == (11,) and np.isfinite(r_a).all() and np.isfinite(o_a).all()
    assert torch.equal(torch.from_numpy(r_a), torch.from_numpy(r_b)) and torch.equal(torch.from_numpy(o_a), torch.from_numpy(o_b))
    assert logs[0] == logs[1] and len(logs[0]) == 2                    # the same running losses were logged
    # the training moved the weights, and the scores are those of the block's cubes in list order, not of the store's first 11
    init = _net4(0).state_dict()
    assert any(not torch.equal(sd_a['module.' + k].cpu(), v) for k, v in init.items() if v.dtype.is_floating_point)
    sd_c, r_c, _ = T.train_block(_net4(0), [(store[0], store[1], np.arange(11))], 2, 4, shuffle_seed=0, log=_quiet)
    assert not np.array_equal(r_a, r_c)


# ---- 3: train.main, staged flow --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', [64, 2], ids=['stock', 'chunks-of-2'])
def test_main_direct_train_equals_staged(staged, monkeypatch, chunk):
    """``direct_train = True`` with no ``foreground_train_*`` file on disk: the three output files of the staged run, and still no
    cube file afterwards; also with chunks of 2 frames (context windows cross chunk borders)."""
    monkeypatch.chdir(staged['root'])
    for p in _cube_files():
        os.remove(p)
    _remove_outputs()
    _cfg(staged['cfg'], direct_train=True, direct_frames_per_chunk=chunk)
    _train()
    assert _cube_files() == []
    _assert_same_outputs(staged['out'], _outputs())


def test_direct_flow_without_direct_train_is_the_staged_route(staged, monkeypatch):
    """``direct_flow = True`` alone changes nothing in training: ``train.main`` cuts and reads the cube files from the staged flow
    files and never asks for the network it is handed."""

    class Unused:
        def __getattr__(self, name):
            raise AssertionError('the staged route asked FlowNet2 for %s' % name)

    monkeypatch.chdir(staged['root'])
    for p in _cube_files():
        os.remove(p)
    _remove_outputs()
    _cfg(staged['cfg'], direct_flow=True)
    _train(flownet2=Unused())
    assert len(_cube_files()) == 2
    _assert_same_outputs(staged['out'], _outputs())


# ---- 6: capacity -----------------------------------------------------------------------------------------------------------------
def test_a_store_too_small_for_the_split_is_an_error(staged, monkeypatch):
    import foreground as FG
    monkeypatch.chdir(staged['root'])
    c = _cfg(staged['cfg'], direct_train=True)
    kept = FG.extract_train_device(c, 'cuda', log=_quiet)['n']
    assert kept > 4
    _remove_outputs()
    _cfg(staged['cfg'], direct_train=True, direct_max_cubes=kept - 1)
    with pytest.raises(ValueError, match='direct_max_cubes') as e:
        _train()
    assert str(kept) in str(e.value) and str(kept - 1) in str(e.value)           # needed, allowed
    assert not os.path.exists(MODEL) and not os.path.exists(RAW_SC) and not os.path.exists(OF_SC)
    c = _cfg(staged['cfg'], direct_train=True, direct_max_cubes=kept)            # exactly enough: fine
    assert FG.extract_train_device(c, 'cuda', log=_quiet)['n'] == kept


# ---- 4 + 5: direct flow ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net():
    from FlowNet2_src import FlowNet2
    torch.manual_seed(0)
    return FlowNet2().cuda().eval()


@pytest.fixture(scope='module')
def flow_staged(tmp_path_factory, net):
    """The fully staged legs on a tree of their own: ``calc_optical_flow(pairs_per_launch=1)`` with the seeded FlowNet2 over both
    splits, ``train.main`` and ``test.main`` through flow and cube files.  Afterwards ``optical_flow/`` and every ``foreground_*``
    file are removed."""
    import calc_optical_flow as COF
    import test as S
    from vad_datasets import unified_dataset_interface
    root = tmp_path_factory.mktemp('direct_train_flow')
    back = os.getcwd()
    os.chdir(root)
    try:
        cfg = _tree()
        shutil.rmtree('optical_flow')                                  # the synthetic fields: the staged leg reads FlowNet2's
        for mode in ('train', 'test'):
            ds = unified_dataset_interface('UCSDped2', os.path.join('raw_datasets', 'UCSDped2'), context_frame_num=1, mode=mode,
                                           border_mode='hard')
            COF.calc_optical_flow(ds, flownet2=net, log=_quiet, pairs_per_launch=1)
        assert len(glob.glob(TRAIN_FLOW + '/Train00*/*.npy')) == 7
        _train()
        out = _outputs()
        auc = S.main('config.cfg')
        fs = np.load(SCORES)
        assert len(_cube_files()) == 2 and len(_cube_files('test')) == 3 and fs.shape == (4,) and np.isfinite(fs).all()
        shutil.rmtree('optical_flow')
        for p in glob.glob('data/raw2flow/*foreground_*'):
            os.remove(p)
        os.remove(SCORES)
        _remove_outputs()
    finally:
        os.chdir(back)
    return dict(root=str(root), cfg=cfg, out=out, fs=fs, auc=auc)


def _no_staged_file():
    return not os.path.exists('optical_flow') and glob.glob('data/raw2flow/*foreground_*') == []


@pytest.mark.parametrize('chunk', [64, 2], ids=['stock', 'chunks-of-2'])
def test_main_direct_train_direct_flow_equals_flow_files(flow_staged, net, monkeypatch, chunk):
    """``direct_train`` + ``direct_flow`` at one pair per launch, with no ``optical_flow/UCSDped2/Train*`` on disk: the output files
    of the staged run on the flow files ``calc_optical_flow(pairs_per_launch=1)`` wrote with the same network."""
    monkeypatch.chdir(flow_staged['root'])
    _remove_outputs()
    _cfg(flow_staged['cfg'], direct_train=True, direct_flow=True, direct_flow_pairs=1, direct_frames_per_chunk=chunk)
    _train(flownet2=net)
    assert glob.glob(TRAIN_FLOW + '*') == [] and _no_staged_file()
    _assert_same_outputs(flow_staged['out'], _outputs())


def test_main_direct_flow_four_pairs_does_not_depend_on_the_chunk(flow_staged, net, monkeypatch):
    """direct_flow_pairs = 4: chunks of 64 frames and of 2 train the same models (not compared with the one-pair run: a layer's
    split-K choice depends on the batch)."""
    monkeypatch.chdir(flow_staged['root'])
    outs = []
    for chunk in (64, 2):
        _remove_outputs()
        c = _cfg(flow_staged['cfg'], direct_train=True, direct_flow=True, direct_frames_per_chunk=chunk)
        assert c['direct_flow_pairs'] == 4
        _train(flownet2=net)
        assert _no_staged_file()
        outs.append(_outputs())
    _assert_same_outputs(outs[0], outs[1])


def test_frames_to_scores_without_a_cube_or_flow_file(flow_staged, net, monkeypatch):
    """``train.main`` then ``test.main`` with direct_train, direct_test and direct_flow on (one pair per launch), no ``optical_flow/``
    directory and no ``foreground_*`` file before, between or after: the frame scores and AUC of the fully staged run."""
    import test as S
    monkeypatch.chdir(flow_staged['root'])
    _remove_outputs()
    if os.path.exists(SCORES):
        os.remove(SCORES)
    _cfg(flow_staged['cfg'], direct_train=True, direct_test=True, direct_flow=True, direct_flow_pairs=1)
    assert _no_staged_file()
    _train(flownet2=net)
    assert _no_staged_file()
    auc = S.main('config.cfg', flownet2=net)
    assert _no_staged_file()
    fs = np.load(SCORES)
    assert np.array_equal(fs, flow_staged['fs']), (fs, flow_staged['fs'])
    assert auc == flow_staged['auc']
