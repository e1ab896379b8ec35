"""Host side of the direct flow path ([mi355x] direct_flow): config keys, which frame pair stands behind each flow file
(calc_optical_flow.flow_pairs), the launch tables of calc_optical_flow.chunk_flows, and the refusals of the two wrappers in
vec_vad_amd/extract.py, which come before anything touches a device.  No GPU."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('direct_flow', 'direct_flow_pairs', 'direct_flow_fp16', 'flownet2_checkpoint')


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


def _fvi(lengths):
    return [v for v, n in enumerate(lengths, start=1) for _ in range(n)]


def test_flow_pairs_are_the_staged_drivers_pairs():
    """Videos of 3, 2, 1 and 5 frames: wherever the 'hard' context of one frame each side exists, flow_pairs gives pair_of of it;
    where ``context_range`` raises (the one-frame video between two others: the staged driver stops there too) flow_pairs raises the
    same error.  Hand answers (calc_optical_flow.py:43,61 matches the FIRST two entries of a clipped context): first frame of a video
    (f, f), inside (f, f + 1), last frame (f - 1, f); a dataset of one single frame: (f, f)."""
    from calc_optical_flow import flow_pairs, pair_of
    from vad_datasets import context_range
    fvi = _fvi((3, 2, 1, 5))
    n = len(fvi)
    assert n == 11
    defined = 0
    for i in range(n):
        try:
            r = context_range(i, 'hard', 1, n, fvi)
        except NotImplementedError:
            assert i == 5                                   # the one-frame video
            with pytest.raises(NotImplementedError):
                flow_pairs(fvi, [i])
            continue
        a, b = pair_of(r)
        assert flow_pairs(fvi, [i]) == [(r[a], r[b])], i
        defined += 1
    assert defined == 10
    rest = [i for i in range(n) if i != 5]
    assert flow_pairs(fvi, rest) == [(0, 0), (1, 2), (1, 2), (3, 3), (3, 4), (6, 6), (7, 8), (8, 9), (9, 10), (9, 10)]
    # first / last frame of the first, a middle and the last video
    assert flow_pairs(fvi, [0, 2, 3, 4, 6, 10]) == [(0, 0), (1, 2), (3, 3), (3, 4), (6, 6), (9, 10)]
    assert flow_pairs(fvi, []) == []
    # a one-frame video where its context is defined: the pair is (f, f)
    assert context_range(0, 'hard', 1, 1, [1]) == [0, 0, 0]
    assert flow_pairs([1], [0]) == [(0, 0)]

    class DS:                                               # a dataset is read for its video structure only
        frame_video_idx = fvi
        context_frame_num, border_mode = 4, 'predict'
    assert flow_pairs(DS(), [2, 3]) == [(1, 2), (3, 3)]


def test_stock_config_has_the_four_keys_and_leaves_the_path_off():
    import train as T
    from calc_optical_flow import CHECKPOINT
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    for k in KEYS:
        assert c['cp'].has_option('mi355x', k), k
    assert c['direct_flow'] is False and c['direct_flow_pairs'] == 4 and c['direct_flow_fp16'] is False
    assert c['flownet2_checkpoint'] == CHECKPOINT


def test_the_four_keys_parse(tmp_path):
    import train as T
    cfg = _config_text().replace('direct_flow = False', 'direct_flow = True').replace('direct_flow_pairs = 4', 'direct_flow_pairs = 1')
    cfg = cfg.replace('direct_flow_fp16 = False', 'direct_flow_fp16 = True')
    cfg = cfg.replace('flownet2_checkpoint = FlowNet2_src/pretrained/FlowNet2_checkpoint.pth.tar', 'flownet2_checkpoint = weights/fn2.pth')
    p = tmp_path / 'config.cfg'
    p.write_text(cfg)
    c = T.read_config(str(p))
    assert c['direct_flow'] is True and c['direct_flow_pairs'] == 1 and c['direct_flow_fp16'] is True
    assert c['flownet2_checkpoint'] == 'weights/fn2.pth'
    assert c['direct_test'] is False                        # the other keys keep their values


def test_defaults_apply_without_the_keys(tmp_path):
    import train as T
    from calc_optical_flow import CHECKPOINT
    lines = [l for l in _config_text().splitlines() if not l.startswith(('direct_flow', 'flownet2_checkpoint'))]
    p = tmp_path / 'config.cfg'
    p.write_text('\n'.join(lines) + '\n')
    c = T.read_config(str(p))
    for k in KEYS:
        assert not c['cp'].has_option('mi355x', k), k
    assert c['direct_flow'] is False and c['direct_flow_pairs'] == 4 and c['direct_flow_fp16'] is False
    assert c['flownet2_checkpoint'] == CHECKPOINT
    assert c['cp'].has_option('mi355x', 'direct_test')


def test_config_edit_rules_hold():
    """Tests edit config.cfg by text replacement: every ``key = value`` text still occurs exactly once."""
    text = _config_text()
    pairs = [l.strip() for l in text.splitlines() if l.strip() and l.lstrip()[0] not in ';[' and '=' in l]
    for kv in pairs:
        assert text.count(kv) == 1, kv


def test_launch_tables_pad_the_tail():
    """5 pairs at 4 per launch: two launches of exactly 4; the tail repeats its last pair with row -1; every real row once."""
    from calc_optical_flow import launch_tables
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 4)]
    rows = [3, 0, 4, 1, 2]
    t = launch_tables(pairs, rows, 4)
    assert len(t) == 2
    for p, r in t:
        assert p.shape == (4, 2) and r.shape == (4,) and p.dtype == np.int32 and r.dtype == np.int32
        assert p.flags['C_CONTIGUOUS'] and r.flags['C_CONTIGUOUS']
    assert t[0][0].tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]] and t[0][1].tolist() == [3, 0, 4, 1]
    assert t[1][0].tolist() == [[4, 4]] * 4 and t[1][1].tolist() == [2, -1, -1, -1]
    real = np.concatenate([r for _, r in t])
    assert sorted(real[real >= 0].tolist()) == [0, 1, 2, 3, 4]
    # exact multiples get no padding, one pair per launch never pads, nothing gives no launch
    assert [r.tolist() for _, r in launch_tables(pairs[:4], rows[:4], 2)] == [[3, 0], [4, 1]]
    assert [(p.tolist(), r.tolist()) for p, r in launch_tables(pairs, rows, 1)] == [([list(p)], [r]) for p, r in zip(pairs, rows)]
    assert launch_tables(np.zeros((0, 2), np.int32), [], 4) == []
    with pytest.raises(ValueError):
        launch_tables(pairs, rows[:4], 4)
    with pytest.raises(ValueError):
        launch_tables(pairs, rows, 0)


def test_wrappers_refuse_bad_tables_before_any_device_work():
    """A pair index >= F (or < 0) and a row >= out_rows raise ValueError: the checks come before the tensors are even asked where
    they live, so host tensors do here."""
    from vec_vad_amd.extract import flow_pairs_prep, flow_resize_back
    frames = torch.zeros((4, 6, 8, 1), dtype=torch.uint8)
    with pytest.raises(ValueError, match='pair 1'):
        flow_pairs_prep(frames, np.array([[0, 1], [2, 4]], np.int32), 64, 128)
    with pytest.raises(ValueError, match='pair 0'):
        flow_pairs_prep(frames, np.array([[-1, 1]], np.int32), 64, 128)
    with pytest.raises(ValueError, match=r'\[N,2\]'):
        flow_pairs_prep(frames, np.array([0, 1, 2], np.int32), 64, 128)
    flow = torch.zeros((3, 2, 64, 128))
    out = torch.zeros((6, 6, 8, 2))
    with pytest.raises(ValueError, match='row 6'):
        flow_resize_back(flow, np.array([2, -1, 6], np.int32), 6, 8, out)
    with pytest.raises(ValueError, match='same row'):
        flow_resize_back(flow, np.array([2, 2, -1], np.int32), 6, 8, out)
    with pytest.raises(ValueError, match='one row per pair'):
        flow_resize_back(flow, np.array([0, 1], np.int32), 6, 8, out)
    # good tables on host tensors: there is no CPU path
    from vec_vad_amd._lib import VecVadHipError
    with pytest.raises(VecVadHipError):
        flow_pairs_prep(frames, np.array([[0, 3]], np.int32), 64, 128)
    with pytest.raises(VecVadHipError):
        flow_resize_back(flow, np.array([2, -1, 5], np.int32), 6, 8, out)
    assert not out.any()


def test_direct_flow_without_direct_test_is_refused(tmp_path):
    import test as S
    p = tmp_path / 'config.cfg'
    p.write_text(_config_text().replace('direct_flow = False', 'direct_flow = True'))
    with pytest.raises(ValueError, match='direct_flow.*direct_test'):
        S.main(str(p))
