"""Host side of test.py's shared stage helpers: the ShanghaiTech per-scene evaluation walked through ``main`` from saved scores, the
score-vector table against the literal file names, the frame chunks with their temporal halo, the per-frame mask writer and the gatherer
of launch results.  No GPU."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shanghaitech_is_evaluated_per_scene_from_saved_scores(tmp_path, monkeypatch, capsys):
    import test as S
    from utils import save_roc_pr_curve_data
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a, **k: None)
    monkeypatch.chdir(tmp_path)
    text = open(os.path.join(ROOT, 'config.cfg')).read()
    for old, new in (('dataset_name = UCSDped2', 'dataset_name = ShanghaiTech'), ('\nscores_saved = False', '\nscores_saved = True'),
                     ('smooth_masks = False', 'smooth_masks = True')):
        assert text.count(old) == 1
        text = text.replace(old, new)
    open('config.cfg', 'w').write(text)
    fg, method = 'obj_det_with_motion', 'SelfComplete'
    rng = np.random.default_rng(11)
    scene_idx = np.repeat([1, 2], 20)
    labels = np.concatenate([rng.permutation(np.arange(20) < k) for k in (7, 12)])      # both classes in each scene
    fs, fs_smooth = rng.standard_normal(40), rng.standard_normal(40)
    data, res = os.path.join('data', 'raw2flow'), os.path.join('results', 'ShanghaiTech')
    os.makedirs(data)
    os.makedirs(res)
    np.save(os.path.join(data, 'ShanghaiTech_scene_idx.npy'), scene_idx)
    np.save(os.path.join(data, 'ShanghaiTech_frame_labels_test.npy'), labels)
    inputs = ['frame_scores_{}_{}.npy'.format(fg, method), 'frame_scores_smooth_{}_{}.npy'.format(fg, method)]
    np.save(os.path.join(res, inputs[0]), fs)
    np.save(os.path.join(res, inputs[1]), fs_smooth)

    got = S.main('config.cfg')
    out = capsys.readouterr().out

    def per_scene(scores):
        return float(np.mean([save_roc_pr_curve_data(scores[scene_idx == si], labels[scene_idx == si], str(tmp_path / 'own.npz'),
                                                     verbose=False) for si in (1, 2)]))

    want, want_smooth = per_scene(fs), per_scene(fs_smooth)
    os.remove(str(tmp_path / 'own.npz'))
    assert got == want
    assert sorted(os.listdir(res)) == sorted(inputs + ['raw2flow_{}_{}_{}_results_scene_{}.npz'.format(fg, method, name, si)
                                                       for name in ('frame', 'frame_smooth') for si in (1, 2)])
    lines = ['Evaluating ShanghaiTech by frame-criterion:', 'Average frame-level AUC is {}'.format(want),
             'Average frame-level AUC of the smoothed masks (5 frames x 9 x 9 pixels) is {}'.format(want_smooth)]
    printed = out.splitlines()
    at = [printed.index(line) for line in lines]
    assert at == sorted(at)


def test_the_vector_table_names_the_files_the_script_has_always_written():
    import test as S
    assert list(S.VECTORS) == ['frame', 'frame_smooth', 'pixel', 'pixel_fine', 'pixel_smooth']
    scores = {name: v.scores_path('D', 'a', 'b') for name, v in S.VECTORS.items()}
    results = {name: v.results_path('D', 'm', 'a', 'b') for name, v in S.VECTORS.items()}
    j = os.path.join
    assert scores == {'frame': j('results', 'D', 'frame_scores_a_b.npy'),
                      'frame_smooth': j('results', 'D', 'frame_scores_smooth_a_b.npy'),
                      'pixel': j('results', 'D', 'pixel_scores_a_b.npy'),
                      'pixel_fine': j('results', 'D', 'pixel_scores_fine_a_b.npy'),
                      'pixel_smooth': j('results', 'D', 'pixel_scores_smooth_a_b.npy')}
    assert results == {'frame': j('results', 'D', 'm_a_b_frame_results.npz'),
                       'frame_smooth': j('results', 'D', 'm_a_b_frame_smooth_results.npz'),
                       'pixel': j('results', 'D', 'm_a_b_pixel_results.npz'),
                       'pixel_fine': j('results', 'D', 'm_a_b_pixel_fine_results.npz'),
                       'pixel_smooth': j('results', 'D', 'm_a_b_pixel_smooth_results.npz')}
    assert S.VECTORS['frame_smooth'].results_path('D', 'm', 'a', 'b', scene=3) == j('results', 'D', 'm_a_b_frame_smooth_results_scene_3.npz')
    assert {name: v.plain for name, v in S.VECTORS.items() if v.plain} == {'frame_smooth': 'frame', 'pixel_fine': 'pixel', 'pixel_smooth': 'pixel'}


def test_frame_chunks_clamp_their_halo_to_the_frames_that_exist():
    import test as S
    assert list(S._frame_chunks(0, 10, 4, halo=2)) == [(0, 4, 0, 6), (4, 8, 2, 10), (8, 10, 6, 10)]
    assert list(S._frame_chunks(0, 10, 4)) == [(0, 4, 0, 4), (4, 8, 4, 8), (8, 10, 8, 10)]
    assert list(S._frame_chunks(5, 12, 3, halo=0)) == [(5, 8, 5, 8), (8, 11, 8, 11), (11, 12, 11, 12)]
    assert list(S._frame_chunks(3, 7, 64)) == [(3, 7, 3, 7)]
    assert list(S._frame_chunks(4, 4, 8, halo=2)) == []


def test_save_frames_writes_one_owned_array_per_frame(tmp_path):
    import test as S
    masks = torch.arange(60, dtype=torch.float64).reshape(3, 5, 4).transpose(1, 2)      # [3,4,5], not contiguous
    for sub, given in (('tensor', masks), ('array', masks.numpy())):
        out_dir = tmp_path / sub
        out_dir.mkdir()
        S._save_frames(str(out_dir), 7, given)
        assert sorted(os.listdir(out_dir)) == ['7', '8', '9']
        for k in range(3):
            got = torch.load(str(out_dir / str(7 + k)), weights_only=False)
            assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (4, 5)
            assert got.flags['C_CONTIGUOUS'] and got.base is None
            assert np.array_equal(got, masks[k].numpy())


def test_gathered_launch_results_keep_the_flow_tensors_lazy():
    import test as S
    r = torch.arange(5, dtype=torch.float32)
    e = torch.arange(5 * 32 * 32, dtype=torch.float32).reshape(5, 32, 32)
    pad = lambda x, m, B: torch.cat([x[:m], x[m - 1:m].expand((B - m,) + tuple(x.shape[1:]))])      # noqa: E731 -- a padded tail launch
    for flow in (True, False):
        for maps in (True, False):
            g = S._Gathered(5, maps, 'cpu')
            for s0, m in ((0, 3), (3, 2)):
                sl = slice(s0, s0 + m)
                launch = (pad(r[sl], m, 3), pad(-r[sl], m, 3) if flow else None)
                if maps:
                    launch += (pad(e[sl], m, 3), pad(-e[sl], m, 3) if flow else None)
                g.put(s0, m, *launch)
            got = g.result()
            assert len(got) == (4 if maps else 2)
            assert got[0].dtype == torch.float32 and torch.equal(got[0], r)
            assert torch.equal(got[1], -r) if flow else got[1] is None
            if maps:
                assert got[2].dtype == torch.float32 and torch.equal(got[2], e)
                assert torch.equal(got[3], -e) if flow else got[3] is None
