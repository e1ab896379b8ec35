"""Host side of the region- and track-based detection criteria ([mi355x] region_criterion): the config keys, the refusals before any
GPU work, ``scoring.link_tracks`` / ``track_scores`` and ``scoring.region_curves`` against the threshold sweep of
tests/region_restatement.py.  No GPU."""
import os

import numpy as np
import pytest
import torch

import region_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('region_criterion', 'region_iou_percent', 'track_percent')


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


# ---- config keys and refusals -------------------------------------------------------------------------------------------------------
def test_the_three_keys_parse_with_defaults_and_bad_percents_are_rejected(tmp_path):
    import train as T
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    for key in KEYS:
        assert c['cp'].has_option('mi355x', key), key
    assert c['region_criterion'] is False and c['region_iou_percent'] == 10 and c['track_percent'] == 10
    assert c['pixel_criterion'] is False                                   # independent keys, both off in the stock file
    p = tmp_path / 'config.cfg'
    p.write_text(_config_text().replace('region_criterion = False', 'region_criterion = True')
                 .replace('region_iou_percent = 10', 'region_iou_percent = 1').replace('track_percent = 10', 'track_percent = 100'))
    c = T.read_config(str(p))
    assert c['region_criterion'] is True and c['region_iou_percent'] == 1 and c['track_percent'] == 100 and c['pixel_criterion'] is False
    # a file from before the keys
    p.write_text('\n'.join(l for l in _config_text().splitlines() if not l.startswith(KEYS)) + '\n')
    c = T.read_config(str(p))
    assert not any(c['cp'].has_option('mi355x', k) for k in KEYS)
    assert c['region_criterion'] is False and c['region_iou_percent'] == 10 and c['track_percent'] == 10
    for key in KEYS[1:]:
        for bad in ('0', '101', '-5', '10.5'):
            p.write_text(_config_text().replace(key + ' = 10', key + ' = ' + bad))
            with pytest.raises(ValueError):
                T.read_config(str(p))
    text = _config_text()
    assert 'derived from the per-pixel ground truth' in text               # the caveat the stock file must state


def test_shanghaitech_is_refused_before_the_gpu_is_touched(tmp_path, monkeypatch):
    import foreground as FG
    import test as S
    import train as T

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')

    monkeypatch.setattr(torch.cuda, 'set_device', touched)
    monkeypatch.setattr(torch.cuda, 'current_device', touched)
    monkeypatch.setattr(FG, 'load_bboxes', touched)
    monkeypatch.chdir(tmp_path)
    cfg = _config_text().replace('dataset_name = UCSDped2', 'dataset_name = ShanghaiTech')
    for saved in ('False', 'True'):
        open('config.cfg', 'w').write(cfg.replace('region_criterion = False', 'region_criterion = True')
                                      .replace('scores_saved = False', 'scores_saved = ' + saved))
        c = T.read_config('config.cfg')
        assert c['dataset_name'] == 'ShanghaiTech' and c['region_criterion'] and not c['pixel_criterion']
        with pytest.raises(ValueError, match='ShanghaiTech') as e:
            S.main('config.cfg')
        assert '\n' not in str(e.value)
    assert os.listdir('.') == ['config.cfg']


def test_a_tree_without_pixel_ground_truth_is_refused_and_the_source_tells_the_videos(tmp_path, monkeypatch):
    import foreground as FG
    import test as S
    import train as T
    from PIL import Image

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')

    monkeypatch.setattr(torch.cuda, 'set_device', touched)
    monkeypatch.chdir(tmp_path)
    for v, n in ((1, 2), (2, 3)):
        os.makedirs('raw_datasets/UCSDped2/Test/Test%03d' % v)
        for k in range(n):
            Image.fromarray(np.zeros((240, 360), np.uint8)).save('raw_datasets/UCSDped2/Test/Test%03d/%03d.tif' % (v, k + 1))
    open('config.cfg', 'w').write(_config_text().replace('region_criterion = False', 'region_criterion = True'))
    with pytest.raises(ValueError, match='ground truth') as e:
        S.main('config.cfg')                                               # region_criterion alone opens the source
    assert '\n' not in str(e.value)
    for v, n in ((1, 2), (2, 3)):
        os.makedirs('raw_datasets/UCSDped2/Test/Test%03d_gt' % v)
        for k in range(n):
            Image.fromarray(np.zeros((240, 360), np.uint8)).save('raw_datasets/UCSDped2/Test/Test%03d_gt/%03d.bmp' % (v, k + 1))
    gt = FG.gt_source(T.read_config('config.cfg'))
    assert len(gt) == 5 and list(gt.frame_video_idx) == [1, 1, 2, 2, 2]


def test_pixel_eval_keeps_its_old_signature_and_checks_the_region_arguments():
    import test as S
    p = S.PixelEval()                                                      # today's call
    assert p.regions is False and p.criterion is True
    out = torch.zeros(3, dtype=torch.float64)
    p = S.PixelEval(lambda i: None, 40, out, None, False, 2)
    assert p.regions is False and p.frames_per_chunk == 2
    with pytest.raises(ValueError):
        S.PixelEval(None, regions=True, video_idx=[1, 1])                  # no ground truth
    with pytest.raises(ValueError):
        S.PixelEval(lambda i: None, out=out, regions=True)                 # no video index
    p = S.PixelEval(lambda i: None, criterion=False, regions=True, region_iou=25, video_idx=[1, 1, 2])
    assert p.out is None and p.region_iou == 25
    st = p.region_state(10)                                                # nothing seen yet: empty lists, no exception
    assert st['region_score'].shape == (0,) and st['track_score'].shape == (0,) and st['fp_score'].shape == (0,) and st['n_frames'] == 0


# ---- tracks -------------------------------------------------------------------------------------------------------------------------
def _words(F, bits):
    w = np.zeros((F, 64), np.uint64)
    for (f, r), qs in bits.items():
        for q in qs:
            w[f, r - 1] |= np.uint64(1) << np.uint64(q - 1)
    return w


def test_link_tracks_chain_split_and_video_boundary():
    from vec_vad_amd import scoring
    # a chain over 4 frames, next to a region that appears in frame 2 only
    n = [1, 1, 2, 1]
    w = _words(4, {(1, 1): [1], (2, 1): [1], (3, 1): [1]})
    track, length, k = scoring.link_tracks(n, w, 10)
    assert track.tolist() == [0, 0, 0, 1, 0] and length.tolist() == [4, 1] and k.tolist() == [1, 1]
    # a split: region 1 of frame 0 links to both regions of frame 1, which stay apart in frame 2 -- one track
    n = [1, 2, 2]
    w = _words(3, {(1, 1): [1], (1, 2): [1], (2, 1): [1], (2, 2): [2]})
    track, length, k = scoring.link_tracks(n, w, 50)
    assert track.tolist() == [0, 0, 0, 0, 0] and length.tolist() == [5] and k.tolist() == [3]
    # a merge, with region 64 in play: bit 63 must survive the int64 the device hands over
    n = [64, 1]
    w = _words(2, {(1, 1): [1, 64]})
    track, length, _ = scoring.link_tracks(n, w.view(np.int64), 10)
    assert track[0] == track[63] == track[64] == 0 and length[0] == 3 and len(length) == 63
    # a video boundary: the same position in frames 1 and 2, but no link word (region_links writes zeros there) -> two tracks
    n = [1, 1, 1, 1]
    w = _words(4, {(1, 1): [1], (3, 1): [1]})
    track, length, _ = scoring.link_tracks(n, w, 10)
    assert track.tolist() == [0, 0, 1, 1] and length.tolist() == [2, 2]
    # equal to the restatement's label propagation on random link words
    rng = np.random.default_rng(4)
    for trial in range(20):
        F = int(rng.integers(1, 9))
        n = rng.integers(0, 5, F)
        w = np.zeros((F, 64), np.uint64)
        for f in range(1, F):
            for r in range(n[f]):
                for q in range(n[f - 1]):
                    if rng.random() < 0.3:
                        w[f, r] |= np.uint64(1) << np.uint64(q)
        pct = int(rng.integers(1, 101))
        track, length, k = scoring.link_tracks(n, w, pct)
        want_track, want_k = R.tracks(n, w, pct)
        assert track.tolist() == want_track.tolist() and k.tolist() == want_k.tolist(), trial
    # empty, bad percent, a bit that names a region the frame before does not have
    track, length, k = scoring.link_tracks([], np.zeros((0, 64), np.uint64), 10)
    assert track.shape == (0,) and length.shape == (0,) and k.shape == (0,)
    for bad in (0, 101, 10.5):
        with pytest.raises(ValueError):
            scoring.link_tracks([1], np.zeros((1, 64), np.uint64), bad)
    with pytest.raises(ValueError):
        scoring.link_tracks([1, 1], _words(2, {(1, 1): [2]}), 10)


def test_k_for_lengths_1_9_10_11_at_10_percent():
    from vec_vad_amd import scoring
    for length, want in ((1, 1), (9, 1), (10, 1), (11, 2)):
        n = [1] * length
        w = _words(length, {(f, 1): [1] for f in range(1, length)})
        track, lens, k = scoring.link_tracks(n, w, 10)
        assert lens.tolist() == [length] and k.tolist() == [want], length
        scores = np.arange(length, dtype=np.float64)
        assert scoring.track_scores(scores, track, k).tolist() == [float(length - want)]      # the k-th largest of 0..length-1
    assert scoring.link_tracks([1] * 11, _words(11, {(f, 1): [1] for f in range(1, 11)}), 100)[2].tolist() == [11]


# ---- curves -------------------------------------------------------------------------------------------------------------------------
def _quiet(*a):
    pass


def test_region_curves_known_answers():
    from vec_vad_amd import scoring
    # the example of the definition: thresholds 3, 2, 1 -> (0, .5), (.5, .5), (.5, 1), flat to 1
    fpr, rbdr, tbdr, rbdc, tbdc = scoring.region_curves([3, 1], [3, 1], [2], 2, log=_quiet)
    assert fpr.tolist() == [0, 0, 0.5, 0.5] and rbdr.tolist() == [0, 0.5, 0.5, 1.0] and rbdc == 0.75 and tbdc == 0.75
    # one track of both regions with k = 1: found with the first
    assert scoring.region_curves([3, 1], [3], [2], 2, log=_quiet)[4] == 1.0
    # the cut at fpr = 1: 4 false positives above the only region in 2 frames -> the curve reaches the region at fpr = 2
    fpr, rbdr, _, rbdc, _ = scoring.region_curves([1], [1], [5, 4, 3, 2], 2, log=_quiet)
    assert fpr.tolist() == [0, 0.5, 1.0, 1.5, 2.0, 2.0] and rbdr.tolist() == [0, 0, 0, 0, 0, 1.0] and rbdc == 0.0
    # ... and by interpolation: 3 equal false positives in 2 frames tie with the region: one segment (0,0) -> (1.5, 1), cut at 1
    fpr, rbdr, _, rbdc, _ = scoring.region_curves([2], [2], [2, 2, 2], 2, log=_quiet)
    assert fpr.tolist() == [0, 1.5] and rbdr.tolist() == [0, 1.0] and abs(rbdc - (1.0 / 1.5) / 2) < 1e-15
    # the flat extension: the last point lies at fpr = 0.25 with half of the regions found
    _, _, _, rbdc, _ = scoring.region_curves([4, -R.BIG], [4, -R.BIG], [5], 4, log=_quiet)
    assert rbdc == 0.75 * 0.5
    # a region no detection matches is never detected: nothing found, no false positive -> 0, not 1
    assert scoring.region_curves([-R.BIG], [-R.BIG], [], 3, log=_quiet)[3:] == (0.0, 0.0)
    # the empty case: nan and a line, no exception
    said = []
    fpr, rbdr, tbdr, rbdc, tbdc = scoring.region_curves([], [], [1.0, 2.0], 5, log=said.append)
    assert np.isnan(rbdc) and np.isnan(tbdc) and len(said) == 1 and '\n' not in said[0] and fpr.tolist() == [0, 0.2, 0.4]
    with pytest.raises(ValueError):
        scoring.region_curves([1.0], [], [], 5, log=_quiet)
    with pytest.raises(ValueError):
        scoring.region_curves([1.0], [1.0], [], 0, log=_quiet)
    with pytest.raises(ValueError):
        scoring.region_curves([float('nan')], [1.0], [], 2, log=_quiet)


def test_region_curves_equal_the_threshold_sweep_on_random_inputs_with_ties():
    from vec_vad_amd import scoring
    rng = np.random.default_rng(11)
    cut = flat = 0
    for trial in range(60):
        F = int(rng.integers(1, 12))
        n = rng.integers(0, 4, F)
        n[int(rng.integers(0, F))] = max(1, n[0])                                # at least one region
        w = np.zeros((F, 64), np.uint64)
        for f in range(1, F):
            for r in range(n[f]):
                for q in range(n[f - 1]):
                    if rng.random() < 0.5:
                        w[f, r] |= np.uint64(1) << np.uint64(q)
        pct = (10, 50, 100)[trial % 3]
        track, _, k = scoring.link_tracks(n, w, pct)
        scores = np.round(rng.standard_normal(int(n.sum())) * 2, 0)              # ties everywhere
        scores[rng.random(scores.size) < 0.25] = -R.BIG                          # regions nothing matched
        fp = np.round(rng.standard_normal(int(rng.integers(0, 4 * F))) * 2, 0)
        n_frames = F if trial % 2 else max(1, F // 3)                            # more false positives than frames in every other trial
        ts = scoring.track_scores(scores, track, k)
        fpr, rbdr, tbdr, rbdc, tbdc = scoring.region_curves(scores, ts, fp, n_frames, log=_quiet)
        thr, w_fpr, w_rbdr, w_tbdr, w_rbdc, w_tbdc = R.sweep(scores, track, k, fp, n_frames)
        assert fpr[0] == rbdr[0] == tbdr[0] == 0.0
        assert fpr[1:].tolist() == w_fpr and rbdr[1:].tolist() == w_rbdr and tbdr[1:].tolist() == w_tbdr, trial
        assert abs(rbdc - w_rbdc) < 1e-12 and abs(tbdc - w_tbdc) < 1e-12, (trial, rbdc, w_rbdc, tbdc, w_tbdc)
        assert 0.0 <= rbdc <= 1.0 and 0.0 <= tbdc <= 1.0
        cut += bool(len(w_fpr) and w_fpr[-1] > 1.0)
        flat += bool(not len(w_fpr) or w_fpr[-1] < 1.0)
        # a detected track count never exceeds what its regions allow: every detected track owns at least k >= 1 detected regions
        n_tracks = len(k)
        for i, t in enumerate(thr):
            det_tracks = round(w_tbdr[i] * n_tracks)
            det_regions = int((scores >= t).sum())
            assert round(tbdr[i + 1] * n_tracks) == det_tracks <= det_regions
            by_track = np.bincount(track[scores >= t], minlength=n_tracks)
            assert det_tracks == int((by_track >= k).sum()) and int(k[by_track >= k].sum()) <= det_regions
    assert cut >= 5 and flat >= 5
