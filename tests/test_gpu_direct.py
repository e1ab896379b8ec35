"""GPU: the direct test path ([mi355x] direct_test) -- vv_cube_cut / vv_cube_energy against per-box ``extract.crop_resize``,
``test.score_store`` against ``test.score_frames`` on the same cubes, and ``test.main`` with and without cube files."""
import glob
import os

import numpy as np
import pytest
import torch

from _util import small_config

pytestmark = pytest.mark.gpu

F, H, W, P = 4, 72, 80, 32
# x_min, y_min, x_max, y_max: copy | exact 2x area (left, top edge) | 1 px wide | 1 px high | 45x23 (right, bottom edge) |
# left + bottom edge | top + right edge | whole frame | inside the all-zero flow region
CROPS = np.array([[10, 8, 42, 40], [0, 0, 64, 64], [5, 3, 6, 50], [7, 20, 60, 21], [35, 49, 80, 72], [0, 30, 13, 72],
                  [50, 0, 80, 17], [0, 0, 80, 72], [62, 52, 78, 70]], np.int32)
WIN5 = np.array([[0, 0, 0, 1, 2], [0, 1, 2, 3, 3], [3, 2, 1, 0, 0], [1, 1, 1, 1, 1], [0, 1, 2, 3, 0], [2, 2, 3, 3, 3],
                 [0, 0, 0, 1, 2], [1, 2, 3, 3, 3], [3, 0, 3, 0, 3]], np.int32)
WIN1 = np.array([[0], [3], [1], [2], [2], [0], [3], [1], [2]], np.int32)


@pytest.fixture(scope='module')
def frames():
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    flow = (rng.standard_normal((F, H, W, 2)) * 2).astype(np.float32)
    flow[:, 50:, 60:] = 0                                   # a still corner: CROPS[8] lies inside it
    return torch.from_numpy(raw).cuda(), torch.from_numpy(flow).cuda()


@pytest.fixture(scope='module')
def reference(frames):
    """Per-box ``crop_resize`` of the frames each window names: {(dtype name, T): [n,T,P,P,C]}, computed once."""
    from vec_vad_amd.extract import crop_resize
    out = {}
    for name, fr, win in (('raw', frames[0], WIN5), ('flow', frames[1], WIN5), ('flow', frames[1], WIN1)):
        idx = torch.from_numpy(win).long().cuda()
        out[(name, win.shape[1])] = torch.cat([crop_resize(fr[idx[i]].contiguous(), CROPS[i:i + 1], P, P) for i in range(len(CROPS))])
    return out


@pytest.mark.parametrize('name,win', [('raw', WIN5), ('flow', WIN5), ('flow', WIN1)], ids=['uint8-T5', 'float32-T5', 'float32-T1'])
def test_cube_cut_equals_per_box_crop_resize(frames, reference, name, win):
    from vec_vad_amd.extract import cube_cut
    fr = frames[0] if name == 'raw' else frames[1]
    ref = reference[(name, win.shape[1])]
    sentinel = 7 if name == 'raw' else -123.5
    n, slots = len(CROPS), 14
    # a permutation with gaps and skipped boxes, then the complement so that every box is cut once
    slot_a = np.array([5, -1, 0, 9, -1, 2, 13, -1, 3], np.int32)
    slot_b = np.array([-1, 12, -1, -1, 1, -1, -1, 6, -1], np.int32)
    for slot in (slot_a, slot_b):
        out = torch.full((slots, win.shape[1], P, P, fr.shape[3]), sentinel, dtype=fr.dtype, device='cuda')
        cube_cut(fr, CROPS, win, slot, P, out)
        written = set()
        for i in range(n):
            if slot[i] >= 0:
                assert torch.equal(out[slot[i]], ref[i]), (name, i)
                written.add(int(slot[i]))
        for s in range(slots):
            if s not in written:
                assert bool((out[s] == sentinel).all()), (name, s)
    # N = 0: OK, nothing written
    out = torch.full((2, win.shape[1], P, P, fr.shape[3]), sentinel, dtype=fr.dtype, device='cuda')
    cube_cut(fr, np.zeros((0, 4), np.int32), np.zeros((0, win.shape[1]), np.int32), np.zeros(0, np.int32), P, out)
    from vec_vad_amd import _lib
    assert _lib.lib().vv_cube_cut(fr.data_ptr(), int(name != 'raw'), F, H, W, fr.shape[3], None, None, None, 0, win.shape[1], P,
                                  out.data_ptr(), 2, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())


def test_bad_tables_raise_before_any_launch(frames):
    """A slot past the store, a window outside the chunk, a crop outside the frame: the wrappers raise (numpy tables and device
    tables alike) and the store keeps its sentinel -- the kernels alone would skip or clamp without a word."""
    from vec_vad_amd.extract import cube_cut, cube_energy
    raw, flow = frames
    out = torch.full((4, 5, P, P, 3), 7, dtype=torch.uint8, device='cuda')
    crops, win, slot = CROPS[:3], WIN5[:3], np.array([2, -1, 0], np.int32)
    for to in (lambda a: a, lambda a: torch.from_numpy(a).cuda()):
        with pytest.raises(ValueError, match='names slot 4'):
            cube_cut(raw, to(crops), to(win), to(np.array([2, -1, 4], np.int32)), P, out)
        w = win.copy()
        w[1, 4] = F
        with pytest.raises(ValueError, match='window 1'):
            cube_cut(raw, to(crops), to(w), to(slot), P, out)
        with pytest.raises(ValueError, match='window 1'):
            cube_energy(flow, to(crops), to(w), P, 0.0)
        c = crops.copy()
        c[2, 3] = H + 1
        with pytest.raises(ValueError, match='crop 2'):
            cube_cut(raw, to(c), to(win), to(slot), P, out)
        with pytest.raises(ValueError, match='crop 2'):
            cube_energy(flow, to(c), to(win), P, 0.0)
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    with pytest.raises(ValueError, match='below 2\\^31'):
        cube_energy(flow, crops, np.zeros((3, 2100), np.int32), 1024, 0.0)        # T * P * P = 2 100 * 2^20 > 2^31


@pytest.mark.parametrize('win', [WIN5, WIN1], ids=['T5', 'T1'])
def test_cube_energy_against_resized_patch(frames, reference, win):
    """Both sides sum at most 5*32*32*2 = 10 240 non-negative doubles, so each is within n * 2^-53 = 1.14e-12 (relative) of the exact
    sum whatever its order: the two differ by at most 2.5e-12."""
    from vec_vad_amd.extract import cube_energy
    fl = frames[1]
    ref = (reference[('flow', win.shape[1])].double() ** 2).sum((2, 3, 4)).mean(1).cpu().numpy()
    e, keep0 = cube_energy(fl, CROPS, win, P, 0.0)
    e2, _ = cube_energy(fl, CROPS, win, P, 0.0)
    assert torch.equal(e, e2)                                # bit-identical run to run
    e = e.cpu().numpy()
    rel = np.abs(e - ref) / np.maximum(ref, 1e-300)
    print('cube_energy T=%d: max relative difference %.3e' % (win.shape[1], rel.max()))
    assert (np.abs(e - ref) <= 2.5e-12 * ref).all(), rel
    assert ref[8] == 0.0 and e[8] == 0.0 and (ref[:8] > 0).all()
    assert np.array_equal(keep0.cpu().numpy().astype(bool), ref > 0.0)
    # a threshold at least 1 % away from every energy of the test: the geometric middle of the widest gap
    srt = np.sort(ref[ref > 0])
    k = int(np.argmax(srt[1:] / srt[:-1]))
    thr = float(np.sqrt(srt[k] * srt[k + 1]))
    assert (np.abs(ref - thr) >= 0.01 * thr).all()
    _, keep = cube_energy(fl, CROPS, win, P, thr)
    want = ref > thr
    assert want.any() and not want.all()
    assert np.array_equal(keep.cpu().numpy().astype(bool), want)
    en, kn = cube_energy(fl, np.zeros((0, 4), np.int32), np.zeros((0, win.shape[1]), np.int32), P, 0.0)
    assert en.numel() == 0 and kn.numel() == 0


# ---- scoring level ------------------------------------------------------------------------------------------------------------
COUNTS = [3, 0, 9, 1, 0, 4, 7]
HB = WB = 2
FH, FW = 240, 360


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
    model --, cube 5 lies in (1, 0) and (0, 1).  Returns the cubes, their frames / blocks / boxes, and the host lists of score_frames."""
    from oracle import unet_oracle as O
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
    assert raw.shape == (24, 5, 32, 32, 3) and flow.shape == (24, 1, 32, 32, 2)
    fset = [[[[] for _ in range(WB)] for _ in range(HB)] for _ in COUNTS]
    for k, (f, blocks) in enumerate(zip(cube_frame, cube_blocks)):
        for (hi, wi) in blocks:
            fset[f][hi][wi].append(k)

    def lists(pick, empty):
        return [[[pick(np.array(cell, np.int64)) if cell else empty for cell in row] for row in fr] for fr in fset]

    host = (lists(lambda i: raw[i], np.zeros((0, 5, 32, 32, 3), np.uint8)),
            lists(lambda i: flow[i, 0], np.zeros((0, 32, 32, 2), np.float32)), lists(lambda i: boxes[i], np.zeros((0, 4))))
    return dict(raw=raw, flow=flow, boxes=boxes, cube_frame=cube_frame, cube_blocks=cube_blocks, host=host)


@pytest.fixture(scope='module')
def models():
    n0, n1 = _net(0), _net(1)
    one = dict(net_set=[[[n0], [n0]], [[n0], []]],
               st_r=[[(900.0, 35.0), (880.0, 40.0)], [(910.0, 30.0), (0.0, 1.0)]],
               st_o=[[(50.0, 4.0), (52.0, 5.0)], [(49.0, 3.0), (0.0, 1.0)]])
    two = dict(net_set=[one['net_set'], [[[n1], [n1]], [[n1], []]]],
               st_r=[one['st_r'], [[(700.0, 25.0), (720.0, 20.0)], [(690.0, 30.0), (0.0, 1.0)]]],
               st_o=[one['st_o'], [[(40.0, 3.0), (41.0, 2.0)], [(39.0, 3.5), (0.0, 1.0)]]])
    return one, two


def _masks_equal(a, b, n):
    for f in range(n):
        ma, mb = torch.load(os.path.join(a, str(f)), weights_only=False), torch.load(os.path.join(b, str(f)), weights_only=False)
        assert ma.dtype == mb.dtype and np.array_equal(ma, mb), f
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))


@pytest.mark.parametrize('scenes', [None, [1, 1, 1, 2, 2, 2, 2]], ids=['one-model-set', 'two-scenes'])
def test_score_store_equals_score_frames(tmp_path, cube_set, models, scenes):
    import test as S
    from foreground import block_groups
    m = models[0] if scenes is None else models[1]
    fset, fset2, bset = cube_set['host']
    da, db = str(tmp_path / 'staged'), str(tmp_path / 'direct')
    fs_a = S.score_frames(m['net_set'], m['st_r'], m['st_o'], fset, fset2, bset, FH, FW, 1.0, 0.5, True, 'cuda', score_batch=4,
                          scene_idx=scenes, result_dir=da)
    store = (torch.from_numpy(cube_set['raw']).cuda(), torch.from_numpy(cube_set['flow']).cuda())
    groups = block_groups(cube_set['cube_frame'], cube_set['cube_blocks'], len(COUNTS), scenes)
    assert sum(len(i) for i, _ in groups.values()) == 25            # 24 cubes, one of them in two lists
    fs_b = S.score_store(m['net_set'], m['st_r'], m['st_o'], store, groups, cube_set['boxes'], FH, FW, 1.0, 0.5, True, 'cuda', 4,
                         scenes, db)
    assert fs_a.shape == (7,) and np.array_equal(fs_a, fs_b)
    assert fs_a[1] == -S.BIG and (fs_a == S.BIG).any()              # a frame without cubes; a cube in the block without a model
    _masks_equal(da, db, 7)


def test_score_store_in_parts_equals_score_frames(tmp_path, cube_set, models):
    """The test set in two parts through ONE reused store (what [mi355x] direct_max_cubes below the set size does): frames 0-2
    (12 cubes), then frames 3-6 (12 cubes) written over them; the frame scores are max-accumulated."""
    import test as S
    from foreground import block_groups
    m = models[0]
    fset, fset2, bset = cube_set['host']
    da, db = str(tmp_path / 'staged'), str(tmp_path / 'parts')
    fs_a = S.score_frames(m['net_set'], m['st_r'], m['st_o'], fset, fset2, bset, FH, FW, 1.0, 0.5, True, 'cuda', score_batch=4,
                          result_dir=da)
    store = (torch.zeros((12, 5, 32, 32, 3), dtype=torch.uint8, device='cuda'), torch.zeros((12, 1, 32, 32, 2), device='cuda'))
    out = torch.full((7,), -float(S.BIG), dtype=torch.float64, device='cuda')
    trainers = {}
    for (lo, hi), frames_ in (((0, 12), (0, 3)), ((12, 24), (3, 7))):
        store[0].copy_(torch.from_numpy(cube_set['raw'][lo:hi]))
        store[1].copy_(torch.from_numpy(cube_set['flow'][lo:hi]))
        groups = block_groups(cube_set['cube_frame'][lo:hi], cube_set['cube_blocks'][lo:hi], 7)
        S.score_store(m['net_set'], m['st_r'], m['st_o'], store, groups, cube_set['boxes'][lo:hi], FH, FW, 1.0, 0.5, True, 'cuda', 4,
                      None, db, out=out, frame_range=frames_, trainers=trainers)
    assert len(trainers) == 1
    assert np.array_equal(fs_a, out.cpu().numpy())
    _masks_equal(da, db, 7)


# ---- script level -------------------------------------------------------------------------------------------------------------
def test_main_direct_equals_staged(tmp_path, monkeypatch):
    """train.main once, test.main with the stock config (cube files), then with direct_test = True after the cube files are gone:
    same frame scores, same AUC, no cube file; again with chunks of 2 frames (context windows cross chunk borders) and with a
    store of 3 cubes (the 4 test frames come in several parts)."""
    from test_gpu_scripts import _synthetic_ped2_tree
    import train as T
    import test as S
    monkeypatch.chdir(tmp_path)
    _synthetic_ped2_tree(np.random.default_rng(11))
    cfg = small_config()
    scores = 'results/UCSDped2/frame_scores_obj_det_with_motion_SelfComplete.npy'

    def cube_files():
        return glob.glob('data/raw2flow/*foreground_test*') + glob.glob('data/raw2flow/*foreground_bbox_test*')

    def masks():
        return [torch.load('results/UCSDped2/score_mask/%d' % f, weights_only=False) for f in range(4)]

    T.main('config.cfg')
    a = S.main('config.cfg')
    A, masks_a = np.load(scores), masks()
    assert len(cube_files()) == 3 and a is not None
    for p in cube_files():
        os.remove(p)
    os.remove(scores)
    os.remove('data/raw2flow/UCSDped2_frame_labels_test.npy')
    for key, stock, value in ((None, None, None), ('direct_frames_per_chunk', 64, 2), ('direct_max_cubes', 524288, 3)):
        c2 = cfg.replace('direct_test = False', 'direct_test = True')
        if key:
            c2 = c2.replace('%s = %d' % (key, stock), '%s = %d' % (key, value))
        open('config.cfg', 'w').write(c2)
        c = T.read_config('config.cfg')
        assert c['direct_test'] and (key is None or c[key] == value)
        b = S.main('config.cfg')
        B = np.load(scores)
        assert np.array_equal(A, B), (key, A, B)
        assert a == b, key
        assert np.load('data/raw2flow/UCSDped2_frame_labels_test.npy').tolist() == [False, True, False, True]
        assert cube_files() == []
        for ma, mb in zip(masks_a, masks()):
            assert np.array_equal(ma, mb), key
    assert np.isfinite(A).all() and A.shape == (4,)
    # a store of 3 cubes really comes in several parts: ranges tile the frames, no frame is split
    import foreground as FG
    open('config.cfg', 'w').write(cfg.replace('direct_test = False', 'direct_test = True').replace('direct_max_cubes = 524288',
                                                                                                   'direct_max_cubes = 3'))
    c3 = T.read_config('config.cfg')
    assert c3['direct_max_cubes'] == 3
    info, parts = FG.extract_device(c3, 'test', 'cuda', log=lambda *msg: None)
    ranges, counts = [], []
    for p in parts:                  # the store is reused: look at a part before asking for the next one
        ranges.append(p['frames'])
        counts.append(p['n'])
        assert len(p['boxes']) == p['n']
        for idx, off in p['groups'].values():
            assert off[p['frames'][0]] == 0 and off[p['frames'][1]] == len(idx) and idx.max() < p['n']
    assert len(ranges) > 1 and ranges[0][0] == 0 and ranges[-1][1] == 4 == info['n_frames']
    assert all(prev[1] == nxt[0] for prev, nxt in zip(ranges, ranges[1:])) and all(0 < k <= 3 for k in counts[:-1]) and counts[-1] <= 3
    assert info['scene_idx'] is None and info['labels'].tolist() == [False, True, False, True]


def test_a_short_list_under_a_forced_launch_size_is_padded_not_shrunk(cube_set, models):
    """``score_index_list(..., batch=4)`` on 2 cubes is ONE launch of 4 cubes, the last one repeated -- what the staged route's
    tail chunk relies on: bit for bit the first two scores of that 4-cube launch (a launch of 2 takes other kernels)."""
    import test as S
    from vec_vad_amd.trainer import FusedTrainer
    tr = FusedTrainer(models[0]['net_set'][0][0][0])
    store = (torch.from_numpy(cube_set['raw']).cuda(), torch.from_numpy(cube_set['flow']).cuda())
    calls = []
    score_cubes = tr.score_cubes
    tr.score_cubes = lambda raw, flow, idx: calls.append(idx.cpu().tolist()) or score_cubes(raw, flow, idx)
    r4, o4 = (t.clone() for t in score_cubes(*store, torch.tensor([7, 3, 3, 3], device='cuda')))        # the launch itself
    for idx in (np.array([7, 3]), torch.tensor([7, 3], device='cuda')):          # host list | device list
        r, o = S.score_index_list(tr, *store, idx, score_batch=4, batch=4)
        assert r.shape == o.shape == (2,) and torch.equal(r, r4[:2]) and torch.equal(o, o4[:2])
    assert calls == [[7, 3, 3, 3]] * 2
    r2, _ = S.score_index_list(tr, *store, np.array([7, 3]), score_batch=4)         # the default rule: a launch of n = 2 cubes
    assert calls[-1] == [7, 3] and r2.shape == (2,)


def test_score_store_equals_score_frames_with_masks_and_without_flow(tmp_path, cube_set, models):
    """``result_dir`` set and ``useFlow=False`` on the set that has a block without a trained model: same frame scores, same masks."""
    import test as S
    from foreground import block_groups
    m = models[0]
    fset, fset2, bset = cube_set['host']
    da, db = str(tmp_path / 'staged'), str(tmp_path / 'direct')
    fs_a = S.score_frames(m['net_set'], m['st_r'], m['st_o'], fset, fset2, bset, FH, FW, 1.0, 0.5, False, 'cuda', score_batch=4,
                          result_dir=da)
    store = (torch.from_numpy(cube_set['raw']).cuda(), torch.from_numpy(cube_set['flow']).cuda())
    groups = block_groups(cube_set['cube_frame'], cube_set['cube_blocks'], len(COUNTS))
    fs_b = S.score_store(m['net_set'], m['st_r'], m['st_o'], store, groups, cube_set['boxes'], FH, FW, 1.0, 0.5, False, 'cuda', 4,
                         None, db)
    assert fs_a.shape == (7,) and np.array_equal(fs_a, fs_b)
    assert fs_a[1] == -S.BIG and (fs_a == S.BIG).any()              # a frame without cubes; a cube in the block without a model
    _masks_equal(da, db, 7)
