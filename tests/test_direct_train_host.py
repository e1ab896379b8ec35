"""Host side of the direct train path ([mi355x] direct_train): the config key, the ShanghaiTech refusal before any GPU work, and the
order of the per-block index lists that training consumes (foreground.block_groups against the filing of extract_train).  No GPU."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


def test_direct_train_is_off_in_the_stock_file_and_parses(tmp_path):
    import train as T
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    assert c['cp'].has_option('mi355x', 'direct_train') and c['direct_train'] is False
    assert 'direct_train = False' in _config_text()
    p = tmp_path / 'config.cfg'
    p.write_text(_config_text().replace('direct_train = False', 'direct_train = True'))
    assert T.read_config(str(p))['direct_train'] is True
    # a file from before the key: the staged route
    p.write_text('\n'.join(l for l in _config_text().splitlines() if not l.startswith('direct_train')) + '\n')
    c = T.read_config(str(p))
    assert not c['cp'].has_option('mi355x', 'direct_train') and c['direct_train'] is False


def test_shanghaitech_is_refused_before_the_gpu_is_touched(tmp_path, monkeypatch):
    """``train.main`` and ``foreground.extract_train_device`` raise before ``torch.cuda`` is asked for anything (this test runs
    without a GPU; every ``torch.cuda`` entry the route would touch first is made to fail loudly)."""
    import torch
    import foreground as FG
    import train as T

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')

    monkeypatch.setattr(torch.cuda, 'set_device', touched)
    monkeypatch.setattr(torch.cuda, 'current_device', touched)
    monkeypatch.setattr(FG, 'load_bboxes', touched)
    monkeypatch.chdir(tmp_path)
    cfg = _config_text().replace('dataset_name = UCSDped2', 'dataset_name = ShanghaiTech')
    cfg = cfg.replace('direct_train = False', 'direct_train = True')
    open('config.cfg', 'w').write(cfg)
    c = T.read_config('config.cfg')
    assert c['dataset_name'] == 'ShanghaiTech' and c['direct_train']
    with pytest.raises(NotImplementedError, match='ShanghaiTech') as e:
        T.main('config.cfg')
    assert '\n' not in str(e.value)                      # a one-line reason
    with pytest.raises(NotImplementedError, match='ShanghaiTech'):
        FG.extract_train_device(c, 'cuda')
    assert os.listdir('.') == ['config.cfg']             # nothing written either


def test_block_lists_keep_the_order_extract_train_files_cubes_in():
    """``extract_train`` visits frames in order and a frame's kept boxes in order, and appends each cube to every block
    ``calc_block_idx`` names.  The store holds the kept cubes in that same frame-then-box order, once each; ``block_groups`` must
    then name, per block, exactly the sequence of cubes the staged filing appended.  3 frames on a 2x2 grid of a 240x360 frame,
    ``train_block_mode = 9``; frame 1 keeps nothing; box B straddles the vertical block border."""
    from foreground import block_groups
    from utils import calc_block_idx
    h_step, w_step = 240 / 2, 360 / 2
    A, B, C, D = [20, 20, 60, 60], [150, 30, 215, 90], [200, 130, 264, 194], [30, 150, 70, 200]
    kept = {0: [A, B, C], 1: [], 2: [D, B, A]}             # frame -> kept boxes, in box order
    staged = {}                                            # block -> [(frame, box position)], appended as extract_train does
    cube_frame, cube_blocks, cube_id = [], [], {}
    for f in sorted(kept):
        for k, bb in enumerate(kept[f]):
            blocks = calc_block_idx(bb[0], bb[2], bb[1], bb[3], h_step, w_step, mode=9)
            for hw in blocks:
                staged.setdefault(hw, []).append((f, k))
            cube_id[(f, k)] = len(cube_frame)              # one store slot per kept box
            cube_frame.append(f)
            cube_blocks.append(blocks)
    assert len(cube_frame) == 6
    two = [s for s, b in enumerate(cube_blocks) if len(b) == 2]
    assert two == [1, 4] and sorted(cube_blocks[1]) == [(0, 0), (0, 1)]      # box B, in frames 0 and 2
    groups = block_groups(cube_frame, cube_blocks, 3)
    assert sorted(groups) == sorted((None,) + hw for hw in staged)
    for hw, seq in staged.items():
        idx, off = groups[(None,) + hw]
        assert idx.dtype == np.int64
        assert idx.tolist() == [cube_id[fk] for fk in seq], hw               # the staged array's order, as store slots
        assert idx.tolist() == sorted(idx.tolist())                          # = frame, then box
        assert off.tolist() == [0] + np.cumsum([sum(1 for f, _ in seq if f == g) for g in range(3)]).tolist()
    # the two-block box: one slot, named by both lists
    assert 1 in groups[(None, 0, 0)][0] and 1 in groups[(None, 0, 1)][0]
    assert sum(len(i) for i, _ in groups.values()) == 6 + 2
    assert groups[(None, 0, 0)][0].tolist() == [0, 1, 4, 5] and groups[(None, 0, 1)][0].tolist() == [1, 4]
    assert groups[(None, 1, 1)][0].tolist() == [2] and groups[(None, 1, 0)][0].tolist() == [3]


def test_store_view_composes_indices_like_slicing_the_block_array():
    """``train_block`` on ``(store_raw, store_flow, block_idx)``: cube ``j`` of the block is store cube ``block_idx[j]``, so a batch
    ``perm[a:b]`` of the block gathers ``store[block_idx[perm[a:b]]]`` = ``store[block_idx][perm[a:b]]``, and a rank's contiguous
    shard of the composed batch is the composed shard.  ``CubeStore`` (the staged form) maps a batch to itself."""
    import torch
    import train as T
    from vec_vad_amd.trainer import shard_batch
    store = torch.arange(10 * 3).reshape(10, 3)
    block_idx = np.array([1, 4, 5, 8, 9], np.int64)
    v = T.StoreView(store, store, block_idx, device='cpu')
    assert len(v) == 5 and v.idx.dtype == torch.int64
    perm = torch.from_numpy(np.random.default_rng(0).permutation(5))
    block = store[torch.from_numpy(block_idx)]
    for a, b in ((0, 4), (4, 8)):                          # a full batch of 4, then the kept partial one
        got = v.take(perm[a:b])
        assert torch.equal(store[got], block[perm[a:b]])
    full = v.take(perm[0:4])
    for r in range(2):
        assert torch.equal(shard_batch(full, r, 2), v.take(shard_batch(perm[0:4], r, 2)))
    assert torch.equal(v.take(torch.arange(0, 5)), torch.from_numpy(block_idx))      # the scoring pass: in list order
    with pytest.raises(IndexError):
        T.StoreView(store, store, np.array([3, 10], np.int64), device='cpu')
    from vad_datasets import CubeStore
    cs = CubeStore(np.zeros((3, 5, 32, 32, 3), np.uint8), np.zeros((3, 32, 32, 2), np.float32), device='cpu')
    assert cs.take(perm[:2]) is not None and torch.equal(cs.take(perm[:2]), perm[:2]) and len(cs) == 3
