"""GPU: the direct flow path ([mi355x] direct_flow) -- vv_flow_pairs_prep / vv_flow_resize_back against the ``crop_resize``
composition of ``calc_optical_flow.flow_of_frames``, ``FlowNet2.graph_entry`` against ``forward_graphed``, ``chunk_flows`` against the
staged driver's per-frame functions, and ``test.main`` with the flow computed per chunk against the same run on flow files.
Every comparison is bit for bit: both sides run the same arithmetic in the same order."""
import glob
import os
import shutil

import numpy as np
import pytest
import torch

from _util import small_config

pytestmark = pytest.mark.gpu

OH, OW = 64, 128
PAIRS = np.array([[0, 1], [2, 2], [3, 0], [1, 3]], np.int32)
# (H, W) of the frames: general / upscaling | exact 2x area branch | copy branch | downscaling, non-integer ratio
SIZES = [(48, 72), (128, 256), (64, 128), (100, 150)]


def _whole(W, H):
    return np.array([[0, 0, W, H]], np.int32)


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('H,W', SIZES, ids=['up', 'area2x', 'copy', 'down'])
def test_flow_pairs_prep_equals_the_crop_resize_composition(H, W, C):
    from vec_vad_amd.extract import crop_resize, flow_pairs_prep
    frames = torch.from_numpy(np.random.default_rng(H + C).integers(0, 256, (4, H, W, C), dtype=np.uint8)).cuda()
    got = flow_pairs_prep(frames, PAIRS, OH, OW)
    assert got.shape == (4, 3, 2, OH, OW) and got.dtype == torch.float32
    for n, (a, b) in enumerate(PAIRS.tolist()):
        small = crop_resize(frames[[a, b]].contiguous(), _whole(W, H), OH, OW)[0]         # [2,oh,ow,C]
        if C == 1:
            small = small.expand(-1, -1, -1, 3)
        assert torch.equal(got[n], small.permute(3, 0, 1, 2).float()), n
    # into a given buffer: the same values, nothing else needed
    out = torch.full((4, 3, 2, OH, OW), -1.0, device='cuda')
    assert flow_pairs_prep(frames, PAIRS, OH, OW, out=out) is out and torch.equal(out, got)


@pytest.mark.parametrize('H,W', [(48, 72), (32, 64), (64, 128), (100, 150)], ids=['down', 'area2x', 'copy', 'up'])
def test_flow_resize_back_equals_crop_resize_of_the_interleaved_field(H, W):
    from vec_vad_amd.extract import crop_resize, flow_resize_back
    flow = (torch.randn((4, 2, OH, OW), generator=torch.Generator().manual_seed(3)) * 3).cuda()
    rows = np.array([2, -1, 0, 5], np.int32)
    sentinel = -123.5
    out = torch.full((6, H, W, 2), sentinel, device='cuda')
    assert flow_resize_back(flow, rows, H, W, out) is out
    for n, r in enumerate(rows):
        if r >= 0:
            ref = crop_resize(flow[n].permute(1, 2, 0).contiguous()[None], _whole(OW, OH), H, W)[0, 0]
            assert torch.equal(out[r], ref), n
    for r in (1, 3, 4):
        assert bool((out[r] == sentinel).all()), r


def test_no_pairs_write_nothing():
    """N = 0 through both wrappers and through the bare C entries with null tables: status 0, the buffers keep their sentinel."""
    from vec_vad_amd import _lib
    from vec_vad_amd.extract import flow_pairs_prep, flow_resize_back
    frames = torch.zeros((4, 48, 72, 1), dtype=torch.uint8, device='cuda')
    assert flow_pairs_prep(frames, np.zeros((0, 2), np.int32), OH, OW).shape == (0, 3, 2, OH, OW)
    out = torch.full((2, 48, 72, 2), 7.0, device='cuda')
    flow_resize_back(torch.zeros((0, 2, OH, OW), device='cuda'), np.zeros(0, np.int32), 48, 72, out)
    buf = torch.full((1, 3, 2, OH, OW), 7.0, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    assert _lib.lib().vv_flow_pairs_prep(frames.data_ptr(), 4, 48, 72, 1, None, 0, OH, OW, buf.data_ptr(), st) == 0
    assert _lib.lib().vv_flow_resize_back(buf.data_ptr(), 0, OH, OW, None, 48, 72, out.data_ptr(), 2, st) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((buf == 7.0).all())


# ---- chunk_flows against the staged driver ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net():
    from FlowNet2_src import FlowNet2
    torch.manual_seed(0)
    return FlowNet2().cuda().eval()


@pytest.fixture(scope='module')
def chunk():
    """6 grey 48x72 frames cut from a pattern that slides 2 px per frame (as in test_calc_optical_flow_driver), as videos of 4 and 2
    frames: the staged driver's pairs are (0,0) (1,2) (2,3) (2,3) (4,4) (4,5) -- border frames, (f,f) pairs, a pair used twice."""
    from calc_optical_flow import flow_pairs
    from vad_datasets import context_range
    base = np.random.default_rng(0).integers(0, 256, (48, 72 + 12), dtype=np.uint8)
    frames = np.stack([np.ascontiguousarray(base[:, 2 * k:2 * k + 72]) for k in range(6)])            # [6,H,W]
    fvi = [1, 1, 1, 1, 2, 2]
    ranges = [context_range(i, 'hard', 1, 6, fvi) for i in range(6)]
    pairs = flow_pairs(fvi, range(6))
    assert pairs == [(0, 0), (1, 2), (2, 3), (2, 3), (4, 4), (4, 5)]
    items = [(frames[r][:, None], r) for r in ranges]                                               # ([3,1,H,W], range)
    return dict(frames=torch.from_numpy(frames[..., None]).cuda(), pairs=pairs, items=items)


def test_graph_entry_is_forward_graphed(net):
    shape = (1, 3, 2, 384, 512)
    si, so, g = net.graph_entry(shape)
    assert tuple(si.shape) == shape and tuple(so.shape) == (1, 2, 384, 512) and si.dtype == so.dtype == torch.float32
    x = torch.rand(shape, generator=torch.Generator().manual_seed(1)).cuda() * 255
    si.copy_(x)
    g.replay()
    mine = so.clone()
    assert torch.equal(mine, net.forward_graphed(x))
    si2, so2, g2 = net.graph_entry(shape)
    assert si2 is si and so2 is so and g2 is g
    assert bool(torch.isfinite(mine).all())


def test_chunk_flows_one_pair_per_launch_is_flow_of_frames(net, chunk):
    from calc_optical_flow import chunk_flows, flow_of_frames
    out = torch.full((6, 48, 72, 2), float('nan'), device='cuda')
    chunk_flows(net, chunk['frames'], chunk['pairs'], np.arange(6), out, 1)
    for f, (stack, r) in enumerate(chunk['items']):
        assert torch.equal(out[f], flow_of_frames(net, stack, r)), f
    assert bool(torch.isfinite(out).all())
    assert float(out.abs().max()) > 0


def test_chunk_flows_four_pairs_per_launch(net, chunk):
    """5 pairs at 4 per launch: the first launch is ``flows_of_frames`` of the same four; the tail launch (one pair + 3 padding
    slots) writes its one row.  Then per-sample independence, on which the chunk invariance of scores at 4 pairs per launch rests:
    one pair gives the same flow in slot 0 and in slot 3, among different companions."""
    from calc_optical_flow import chunk_flows, flows_of_frames
    out = torch.full((5, 48, 72, 2), float('nan'), device='cuda')
    chunk_flows(net, chunk['frames'], chunk['pairs'][:5], np.arange(5), out, 4)
    for f, ref in enumerate(flows_of_frames(net, chunk['items'][:4])):
        assert torch.equal(out[f], ref), f
    assert bool(torch.isfinite(out).all())
    X = (1, 2)
    a = torch.full((4, 48, 72, 2), float('nan'), device='cuda')
    b = torch.full((4, 48, 72, 2), float('nan'), device='cuda')
    chunk_flows(net, chunk['frames'], [X, (0, 0), (2, 3), (4, 5)], np.arange(4), a, 4)
    chunk_flows(net, chunk['frames'], [(5, 4), (3, 1), (4, 4), X], np.arange(4), b, 4)
    diff = float((a[0] - b[3]).abs().max())
    print('pair (1,2) in slot 0 vs slot 3 of a 4-pair launch: max |difference| = %.3e' % diff)
    assert torch.equal(a[0], b[3])
    assert torch.equal(a[0], out[1])                    # and in slot 1 of the first launch above
    assert torch.equal(b[2], out[4])                    # (4,4): slot 2 here, slot 0 of the padded tail launch there


# ---- script level ----------------------------------------------------------------------------------------------------------------
SCORES = 'results/UCSDped2/frame_scores_obj_det_with_motion_SelfComplete.npy'


def _masks():
    return [torch.load('results/UCSDped2/score_mask/%d' % f, weights_only=False) for f in range(4)]


def _cube_files():
    return glob.glob('data/raw2flow/*foreground_test*') + glob.glob('data/raw2flow/*foreground_bbox_test*')


@pytest.fixture(scope='module')
def staged(tmp_path_factory, net):
    """The synthetic tree, ``train.main`` on its staged flows, then the comparison leg: the test split's flow files rewritten by
    ``calc_optical_flow`` with the seeded network, one pair per launch, and ``test.main`` with direct_test on them -> scores A,
    masks, AUC.  After that ``optical_flow/UCSDped2/Test`` is removed."""
    from test_gpu_scripts import _synthetic_ped2_tree
    import calc_optical_flow as COF
    import train as T
    import test as S
    from vad_datasets import unified_dataset_interface
    root = tmp_path_factory.mktemp('direct_flow')
    back = os.getcwd()
    os.chdir(root)
    try:
        _synthetic_ped2_tree(np.random.default_rng(11))
        cfg = small_config()
        T.main('config.cfg')
        ds = unified_dataset_interface('UCSDped2', os.path.join('raw_datasets', 'UCSDped2'), context_frame_num=1, mode='test',
                                       border_mode='hard')
        before = np.load('optical_flow/UCSDped2/Test/Test001/001.npy')
        COF.calc_optical_flow(ds, flownet2=net, log=lambda *a: None, pairs_per_launch=1)
        assert len(glob.glob('optical_flow/UCSDped2/Test/Test001/*.npy')) == 4
        assert not np.array_equal(before, np.load('optical_flow/UCSDped2/Test/Test001/001.npy'))
        cfg = cfg.replace('direct_test = False', 'direct_test = True')
        open('config.cfg', 'w').write(cfg)
        auc = S.main('config.cfg')
        A, masks = np.load(SCORES), _masks()
        assert _cube_files() == [] and auc is not None
        shutil.rmtree('optical_flow/UCSDped2/Test')
    finally:
        os.chdir(back)
    return dict(root=str(root), cfg=cfg, A=A, masks=masks, auc=auc)


def _run(staged, net, edits):
    import train as T
    import test as S
    cfg = staged['cfg'].replace('direct_flow = False', 'direct_flow = True')
    for old, new in edits:
        assert old in cfg
        cfg = cfg.replace(old, new)
    open('config.cfg', 'w').write(cfg)
    c = T.read_config('config.cfg')
    assert c['direct_test'] and c['direct_flow']
    if os.path.exists(SCORES):
        os.remove(SCORES)
    auc = S.main('config.cfg', flownet2=net)
    assert not os.path.exists('optical_flow/UCSDped2/Test') and _cube_files() == []
    return np.load(SCORES), auc, c


@pytest.mark.parametrize('edits', [(), (('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = 2'),),
                                   (('direct_max_cubes = 524288', 'direct_max_cubes = 3'),)], ids=['stock', 'chunks-of-2', 'store-of-3'])
def test_main_direct_flow_equals_flow_files(staged, net, monkeypatch, edits):
    """direct_flow at one pair per launch, with no ``optical_flow/UCSDped2/Test`` on disk: the frame scores, masks and AUC of the run on
    the flow files that ``calc_optical_flow(pairs_per_launch=1)`` wrote; also with chunks of 2 frames (windows and pairs cross chunk
    borders) and with a store of 3 cubes."""
    monkeypatch.chdir(staged['root'])
    B, auc, c = _run(staged, net, (('direct_flow_pairs = 4', 'direct_flow_pairs = 1'),) + tuple(edits))
    assert c['direct_flow_pairs'] == 1
    A = staged['A']
    assert A.shape == (4,) and np.isfinite(A).all()
    assert np.array_equal(A, B), (A, B)
    assert auc == staged['auc']
    for ma, mb in zip(staged['masks'], _masks()):
        assert ma.dtype == mb.dtype and np.array_equal(ma, mb)


def test_main_direct_flow_four_pairs_does_not_depend_on_the_chunk(staged, net, monkeypatch):
    """direct_flow_pairs = 4: chunks of 64 frames and of 2 give the same scores (not compared with the one-pair scores: a layer's
    split-K choice depends on the batch).  At least one cube is scored, so an empty run cannot pass."""
    import foreground as FG
    import test as S
    monkeypatch.chdir(staged['root'])
    big, _, c = _run(staged, net, ())
    assert c['direct_flow_pairs'] == 4 and c['direct_frames_per_chunk'] == 64
    small, _, c2 = _run(staged, net, (('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = 2'),))
    assert c2['direct_frames_per_chunk'] == 2
    assert np.isfinite(big).all() and np.array_equal(big, small), (big, small)
    info, parts = FG.extract_device(c, 'test', 'cuda', log=lambda *msg: None, flownet2=net)
    cubes = 0
    for p in parts:
        cubes += p['n']
        assert bool(torch.isfinite(p['flow'][:p['n']]).all())
    assert cubes > 0 and info['n_frames'] == 4
    assert (big > -S.BIG).any()


def test_main_direct_flow_needs_direct_test(staged, net, monkeypatch):
    import test as S
    monkeypatch.chdir(staged['root'])
    cfg = staged['cfg'].replace('direct_test = True', 'direct_test = False').replace('direct_flow = False', 'direct_flow = True')
    open('config.cfg', 'w').write(cfg)
    with pytest.raises(ValueError, match='direct_flow.*direct_test'):
        S.main('config.cfg', flownet2=net)
