"""Macro AUROC and bootstrap intervals on the GPU ([mi355x] auc_statistics): the raw ABI (vv_auc_boot_counts), ``scoring.auc_counts``,
``auc_bootstrap`` and ``auc_paired`` against the plain-numpy restatement (tests/auc_bootstrap_restatement.py), then the script level
(``test.main`` staged, direct and from saved scores).  The device returns integers and the host forms one quotient per group, so every
comparison is exact: ``np.array_equal`` on the int64 counts and on the float64 statistics, no tolerance anywhere."""
import glob
import os
import sys
import zipfile

import numpy as np
import pytest
import torch

from _util import small_config
import auc_bootstrap_restatement as R

pytestmark = pytest.mark.gpu

BIG = 100000.0
SENT = -7                                     # sentinel rows behind the output
GUARD = 4096                                  # guard bytes behind the work buffer
UNIT = {'none': 0, 'video': 1, 'block': 2}
SEEDS = (0, (1 << 63) + 12345)
# group lengths 1, 2, 63, 64, 65, 257, 1500 (longer than the 1024-position tile of the count kernel) and 4200 (longer than the 4096-frame
# difference array of the block weights); strata of 1, 3 and 4 videos
LENS = [1, 2, 63, 64, 65, 257, 1500, 4200]
STRATA = [0, 1, 1, 1, 2, 2, 2, 2]
REPS = 3


def _inputs():
    rng = np.random.default_rng(5)
    n = sum(LENS)
    video = np.repeat(np.arange(len(LENS)) + 3, LENS)
    scores = np.round(rng.standard_normal(n), 1)
    scores[rng.random(n) < 0.3] = -BIG                                    # many ties at the background, in every group
    scores[rng.random(n) < 0.01] = BIG
    labels = rng.random(n) < 0.35
    labels[0] = True                                                      # the one-frame video: no negative
    labels[1:3] = False                                                   # the two-frame video: no positive
    scores[2] = scores[3] = 0.5                                           # equal scores on both sides of a group boundary
    for a in (scores, labels, video):
        a.setflags(write=False)
    return scores, labels, video, np.repeat(STRATA, LENS)


_cache = {}


def inputs():
    if 'in' not in _cache:
        _cache['in'] = _inputs()
    return _cache['in']


def grouping(kind):
    scores, labels, video, scene = inputs()
    return {'one': None, 'scene': scene, 'video': video}[kind]


def tables(kind, strata=True, dataset=None):
    """Host tables and their uploaded copy, built once per grouping."""
    from vec_vad_amd import scoring
    key = ('t', kind, strata, dataset is not None and id(dataset))
    if key not in _cache:
        scores, labels, video, scene = dataset or inputs()
        groups = {'one': None, 'scene': scene, 'video': video}[kind]
        t = scoring.auc_tables(scores, labels, video, groups, scene if strata else None)
        _cache[key] = (t, scoring.auc_tables_device(t, 'cuda'))
    return _cache[key]


def reference(kind, unit, block, seed, r0, reps, strata=True):
    """The restatement's counts, computed once and left unchanged."""
    key = ('r', kind, unit, block, seed, r0, reps, strata)
    if key not in _cache:
        scores, labels, video, scene = inputs()
        c = R.counts(scores, labels, video, grouping(kind), unit, block, seed, r0, reps, scene if strata else None)
        c.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def raw_call(t, unit, block, seed, r0, reps, group_off=None):
    """vv_auc_boot_counts through ctypes with a work buffer of exactly the size the companion reports, guard bytes behind it and
    sentinel rows behind the output: host int64 [reps, G, 3], after checking that neither was touched."""
    from vec_vad_amd import _lib
    l = _lib.lib()
    goff = t['group_off'] if group_off is None else torch.tensor(group_off, dtype=torch.int32, device='cuda')
    G = goff.numel() - 1
    nb = int(l.vv_auc_boot_work(t['n'], t['V'], reps, UNIT[unit]))
    assert nb % 8 == 0 and nb >= (0 if unit == 'none' else reps * t['n'] * 4)
    work = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    out = torch.full((reps + 1, G, 3), SENT, dtype=torch.int64, device='cuda')
    rc = l.vv_auc_boot_counts(t['order'].data_ptr(), t['tie'].data_ptr(), t['label'].data_ptr(), goff.data_ptr(), t['video_off'].data_ptr(),
                              t['stratum_off'].data_ptr(), t['n'], G, t['V'], t['S'], seed, r0, reps, UNIT[unit], block, out.data_ptr(),
                              work.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((work[nb:] == 0xA5).all()), 'the kernels wrote behind the work buffer'
    assert bool((out[-1] == SENT).all()), 'the kernels wrote behind the output'
    return out[:-1].cpu().numpy()


@pytest.mark.parametrize('seed', SEEDS, ids=['seed0', 'seedtop'])
@pytest.mark.parametrize('unit,block', [('block', 1), ('block', 7), ('block', 5000), ('video', 1)])
@pytest.mark.parametrize('kind', ['one', 'scene', 'video'])
def test_raw_abi_equals_the_restatement(kind, unit, block, seed):
    host, dev = tables(kind)
    want = reference(kind, unit, block, seed, 1, REPS)
    got = raw_call(dev, unit, block, seed, 1, REPS)
    print('%s groups, unit %s, block %d: %d of %d counts differ from the restatement' % (kind, unit, block, int((got != want).sum()), want.size))
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(raw_call(dev, unit, block, seed, 1, REPS), got)          # run to run
    if kind == 'video':
        assert got[:, 0, 2].max() == 0 and got[:, 1, 1].max() == 0 and (got[:, :2, 0] == 0).all()      # a group without a negative / a positive
    if unit == 'block' and block >= max(LENS):                             # one block that is the video: every replicate is the full sample
        assert all(np.array_equal(g, reference(kind, 'none', 1, 0, 1, 1)[0]) for g in got)
    else:
        assert not np.array_equal(got[0], got[1])                          # replicates differ
    # an empty group in front, in the middle and at the end gives zeros and moves nothing
    goff = host['group_off'].tolist()
    wide = [goff[0]] + goff[:2] + goff[1:] + [goff[-1]]
    got_wide = raw_call(dev, unit, block, seed, 1, REPS, group_off=wide)
    keep = [k for k in range(len(wide) - 1) if k not in (0, 2, len(wide) - 2)]
    assert np.array_equal(got_wide[:, keep], want) and (got_wide[:, [0, 2, len(wide) - 2]] == 0).all()


def test_one_stratum_one_video_and_one_frame():
    from vec_vad_amd import scoring
    scores, labels, video, scene = inputs()
    host, dev = tables('one', strata=False)
    assert host['S'] == 1
    for unit in ('video', 'block'):
        assert np.array_equal(raw_call(dev, unit, 7, 11, 1, REPS), reference('one', unit, 7, 11, 1, REPS, strata=False))
    for a, b in ((452, 1952), (0, 1), (0, 3)):                               # V = 1 (1500 frames); a one-frame set; a one-frame and a two-frame video
        s, lab, vid = scores[a:b], labels[a:b], video[a:b]
        t = scoring.auc_tables_device(scoring.auc_tables(s, lab, vid, vid), 'cuda')
        for unit in ('video', 'block'):
            assert np.array_equal(raw_call(t, unit, 7, 0, 1, REPS), R.counts(s, lab, vid, vid, unit, 7, 0, 1, REPS))
    # V = 1: the video bootstrap can only pick the video once -- every replicate is the full sample
    s, lab, vid = scores[452:1952], labels[452:1952], video[452:1952]
    assert np.array_equal(scoring.auc_counts(s, lab, vid, None, 'video', 1, 3, 1, 2)[1], scoring.auc_counts(s, lab, vid, None, 'none', 1, 0, 1, 1)[0])


def test_all_scores_equal_give_p_times_n():
    scores, labels, video, scene = inputs()
    flat = (np.zeros(scores.size), labels, video, scene)
    for kind in ('one', 'video'):
        _, dev = tables(kind, dataset=flat)
        for unit, block in (('none', 1), ('video', 1), ('block', 7)):
            got = raw_call(dev, unit, block, 1, 1, 1 if unit == 'none' else REPS)
            assert np.array_equal(got[:, :, 0], got[:, :, 1] * got[:, :, 2]) and got[:, :, 0].max() > 0


def test_replicates_split_over_calls():
    from vec_vad_amd import scoring
    scores, labels, video, scene = inputs()
    for unit in ('video', 'block'):
        _, dev = tables('scene')
        whole = raw_call(dev, unit, 7, SEEDS[1], 1, 7)
        assert np.array_equal(whole, np.concatenate([raw_call(dev, unit, 7, SEEDS[1], 1, 3), raw_call(dev, unit, 7, SEEDS[1], 4, 4)]))
        assert np.array_equal(whole[:REPS], reference('scene', unit, 7, SEEDS[1], 1, REPS))
        # the wrapper splits by itself when the scratch of one call would pass its bound
        old = scoring.AUC_WORK_BYTES
        try:
            scoring.AUC_WORK_BYTES = 2 * 4 * (dev['n'] + dev['V']) + 64      # two replicates per call
            got = scoring.auc_counts(scores, labels, video, scene, unit, 7, SEEDS[1], 1, 7, strata=scene)
        finally:
            scoring.AUC_WORK_BYTES = old
        assert got.dtype == np.int64 and np.array_equal(got, whole)


@pytest.mark.parametrize('kind', ['one', 'scene', 'video'])
def test_full_sample_equals_vv_roc_auc_counts_on_every_group(kind):
    from vec_vad_amd import _lib, scoring
    scores, labels, video, scene = inputs()
    _, dev = tables(kind)
    got = raw_call(dev, 'none', 1, 0, 1, 1)
    assert np.array_equal(got, reference(kind, 'none', 1, 0, 1, 1))
    assert np.array_equal(scoring.auc_counts(scores, labels, video, grouping(kind), 'none', 1, 0, 1, 1, strata=scene), got)
    for g, idx in enumerate(R.group_members(grouping(kind), scores.size)):
        out3 = torch.zeros(3, dtype=torch.int64, device='cuda')
        s, lab = torch.from_numpy(scores[idx]).cuda(), torch.from_numpy(labels[idx].astype(np.uint8)).cuda()
        _lib.check(_lib.lib().vv_roc_auc_counts(s.data_ptr(), lab.data_ptr(), idx.size, out3.data_ptr(), torch.cuda.current_stream().cuda_stream))
        assert out3.tolist() == got[0, g].tolist(), g


def test_bad_arguments_and_empty_shapes_return_the_codes_stated():
    from vec_vad_amd import _lib
    l = _lib.lib()
    OK, BAD, UNSUPPORTED = 0, 1, 3
    _, t = tables('video')
    n, G, V, S = t['n'], t['G'], t['V'], t['S']
    reps = 2
    out = torch.full((reps, G, 3), SENT, dtype=torch.int64, device='cuda')
    work = torch.full((int(l.vv_auc_boot_work(n, V, reps, 1)),), 9, dtype=torch.uint8, device='cuda')
    P = dict(order=t['order'].data_ptr(), tie=t['tie'].data_ptr(), label=t['label'].data_ptr(), goff=t['group_off'].data_ptr(),
             voff=t['video_off'].data_ptr(), soff=t['stratum_off'].data_ptr(), out=out.data_ptr(), work=work.data_ptr())
    st = torch.cuda.current_stream().cuda_stream

    def call(n=n, G=G, V=V, S=S, seed=0, r0=1, R=reps, unit=2, block=7, **ptr):
        p = dict(P)
        p.update(ptr)
        return l.vv_auc_boot_counts(p['order'], p['tie'], p['label'], p['goff'], p['voff'], p['soff'], n, G, V, S, seed, r0, R, unit, block,
                                    p['out'], p['work'], st)

    for kw in (dict(order=None), dict(tie=None), dict(label=None), dict(goff=None), dict(voff=None), dict(out=None), dict(work=None),
               dict(unit=1, soff=None), dict(unit=1, work=None),                              # NULL pointers with something to do
               dict(n=-1), dict(G=-1), dict(V=-1), dict(S=-1), dict(R=-1),                    # negative sizes
               dict(r0=0), dict(r0=-5), dict(block=0), dict(block=-7), dict(unit=3), dict(unit=-1), dict(unit=0, R=2)):
        assert call(**kw) == BAD, kw
    assert call(V=65537) == UNSUPPORTED and call(unit=1, V=65537) == UNSUPPORTED
    for a in ((-1, V, 1, 2), (n, -1, 1, 2), (n, V, -1, 2), (n, V, 1, 3), (n, 65537, 1, 2)):
        assert l.vv_auc_boot_work(*a) == -1, a
    assert l.vv_auc_boot_work(n, V, 5, 0) == 0 and l.vv_auc_boot_work(n, V, 0, 2) == 0
    assert l.vv_auc_boot_work(n, V, 3, 2) == (3 * n * 4 + 7) // 8 * 8 and l.vv_auc_boot_work(n, V, 3, 1) == (3 * n * 4 + 7) // 8 * 8 + 3 * V * 4
    # nothing to do: R == 0 or G == 0, whatever the pointers
    none = dict(order=None, tie=None, label=None, goff=None, voff=None, soff=None, out=None, work=None)
    assert call(R=0) == OK and call(R=0, **none) == OK and call(G=0) == OK and call(G=0, **none) == OK
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((work == 9).all())           # nothing was launched by any call above
    # n == 0: every group is empty, the output is zeroed
    assert call(n=0, V=0, order=None, tie=None, label=None, goff=None, voff=None, soff=None, work=None) == OK
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((work == 9).all())
    # the full sample needs neither the video tables nor work
    assert call(unit=0, R=1, voff=None, soff=None, work=None) == OK


def test_wrapper_refusals():
    from vec_vad_amd import scoring
    scores, labels, video, scene = inputs()
    for kw, text in ((dict(unit='frame'), "unit must be 'none', 'video' or 'block'"), (dict(r0=0), 'r0 >= 1'), (dict(block=0), 'block'),
                     (dict(seed=-1), 'seed must be an integer in 0..2.64-1'), (dict(seed=2 ** 64), 'seed must be'), (dict(unit='none', R=2), 'R must be 1'),
                     (dict(R=-1), 'R >= 0')):
        a = dict(scores=scores, labels=labels, video_idx=video, groups=None, unit='block', block=7, seed=0, r0=1, R=2)
        a.update(kw)
        with pytest.raises(ValueError, match=text) as e:
            scoring.auc_counts(**a)
        assert '\n' not in str(e.value)
    assert scoring.auc_counts(scores, labels, video, None, 'block', 7, 0, 1, 0).shape == (0, 1, 3)


def _flat(res, prefix=''):
    return {'%s%s_%s' % (prefix, kind, k): v for kind in ('micro', 'macro') for k, v in res[kind].items()}


def test_auc_bootstrap_and_auc_paired_equal_the_restatement():
    from vec_vad_amd import scoring
    scores, labels, video = R.array_set()
    scene = np.repeat([4, 4, 9, 9, 9, 9], [120, 180, 150, 200, 90, 170])
    other = np.round(scores + 0.3 * np.random.default_rng(1).standard_normal(scores.size), 2)
    for sc in (None, scene):
        for unit in ('block', 'video'):
            kw = dict(replicates=100, unit=unit, block=25, seed=SEEDS[1], confidence=90)
            got = scoring.auc_bootstrap(torch.from_numpy(scores).cuda(), labels, video, sc, **kw)
            want = R.bootstrap(scores, labels, video, sc, **kw)
            for kind in ('micro', 'macro'):
                print(unit, 'scenes' if sc is not None else 'one group', kind, got[kind]['auc'], got[kind]['lo'], got[kind]['hi'],
                      got[kind]['n_invalid'])
                assert R.entries_equal(got[kind], want[kind]), (unit, kind)
                assert got[kind]['replicates'].dtype == np.float64 and got[kind]['lo'] < got[kind]['hi']
            assert got['macro']['n_groups_valid'] == 4 and got['micro']['n_groups_valid'] == (1 if sc is None else 2)
            got_b = scoring.auc_bootstrap(other, labels, video, sc, **kw)      # host scores are uploaded
            assert R.entries_equal(_flat(got_b), _flat(R.bootstrap(other, labels, video, sc, **kw)))
            pair = scoring.auc_paired(got_b, got)
            for kind in ('micro', 'macro'):
                assert R.entries_equal(pair[kind], R.paired(got_b[kind], got[kind]))
            assert R.entries_equal(_flat(scoring.auc_paired(got, got)), _flat({k: R.paired(got[k], got[k]) for k in got}))
            assert scoring.auc_paired(got, got)['macro']['frac_le0'] == 1.0
    none = scoring.auc_bootstrap(scores, labels, video, replicates=0)      # the statistics alone
    assert R.entries_equal(_flat(none), _flat(R.bootstrap(scores, labels, video, None, 0)))
    for kind in ('micro', 'macro'):
        assert none[kind]['replicates'].shape == (0,) and np.isnan(none[kind]['lo']) and none[kind]['n_invalid'] == 0


# ---- script level -------------------------------------------------------------------------------------------------------------------
TEST_VIDEOS = (7, 5)
N_TEST = sum(TEST_VIDEOS)
RES = 'results/UCSDped2/'
TAIL = 'obj_det_with_motion_SelfComplete'
NAMES = ('frame', 'frame_smooth', 'pixel', 'pixel_fine', 'pixel_smooth')
PLAIN = {'frame_smooth': 'frame', 'pixel_fine': 'pixel', 'pixel_smooth': 'pixel'}
VECTOR = {'frame': 'frame_scores_%s.npy', 'frame_smooth': 'frame_scores_smooth_%s.npy', 'pixel': 'pixel_scores_%s.npy',
          'pixel_fine': 'pixel_scores_fine_%s.npy', 'pixel_smooth': 'pixel_scores_smooth_%s.npy'}


def _tree():
    return sorted(os.path.relpath(os.path.join(d, f), 'results') for d, _, files in os.walk('results') for f in files)


def _content(path):
    """The bytes of a result file; for an .npz the bytes of every member (the zip container stamps the time of writing)."""
    if path.endswith('.npz'):
        with zipfile.ZipFile(path) as z:
            return {name: z.read(name) for name in z.namelist()}
    return open(path, 'rb').read()


def test_main_auc_statistics_staged_direct_and_from_saved_scores(tmp_path, monkeypatch, capsys):
    import train as T
    import test as S
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from synthetic_tree import make_tree
    monkeypatch.chdir(tmp_path)
    make_tree({'train': (4, 3), 'test': TEST_VIDEOS}, 3)
    # one cube per launch on every route, so the scores are equal bit for bit between the routes (as in tests/test_gpu_smooth.py)
    cfg = small_config().replace('score_batch = 2048', 'score_batch = 1').replace('pixel_criterion = False', 'pixel_criterion = True')
    cfg = cfg.replace('smooth_masks = False', 'smooth_masks = True').replace('save_score_masks = True', 'save_score_masks = False')
    cfg = cfg.replace('pixel_maps = False', 'pixel_maps = True')
    assert 'pixel_maps = True' in cfg and 'smooth_masks = True' in cfg and 'pixel_criterion = True' in cfg
    assert 'auc_statistics = False' in cfg and 'auc_bootstrap = 1000' in cfg and 'auc_bootstrap_block = 25' in cfg
    cfg = cfg.replace('auc_bootstrap = 1000', 'auc_bootstrap = 50').replace('auc_bootstrap_block = 25', 'auc_bootstrap_block = 2')
    open('config.cfg', 'w').write(cfg)
    boots = ['raw2flow_%s_%s_bootstrap.npz' % (TAIL, name) for name in NAMES]

    def clear():
        for p in glob.glob(RES + '*.np?'):
            os.remove(p)

    T.main('config.cfg')
    before = set(_tree())

    # ---- key off: no bootstrap file, nothing printed about it
    S.main('config.cfg')
    assert 'bootstrap' not in capsys.readouterr().out
    off_tree = _tree()
    assert not any('bootstrap' in p for p in off_tree) and set(off_tree) > before
    off = {p: _content(os.path.join('results', p)) for p in off_tree if p not in before}
    labels = np.load('data/raw2flow/UCSDped2_frame_labels_test.npy').astype(bool)
    video = np.repeat(np.arange(1, len(TEST_VIDEOS) + 1), TEST_VIDEOS)

    def expected():
        """The restatement applied to the saved score files."""
        want, done = {}, {}
        for name in NAMES:
            done[name] = R.bootstrap(np.load(RES + VECTOR[name] % TAIL), labels, video, None, 50, 'block', 2, 0, 95)
            want[name] = _flat(done[name])
            if name in PLAIN:
                want[name].update(_flat({k: R.paired(done[name][k], done[PLAIN[name]][k]) for k in ('micro', 'macro')}, 'paired_'))
        return want

    on = cfg.replace('auc_statistics = False', 'auc_statistics = True').replace('test_foreground_saved = False', 'test_foreground_saved = True')
    direct = on.replace('direct_test = False', 'direct_test = True').replace('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = 5')
    got = {}
    for route, text in (('staged', on), ('direct', direct)):
        clear()
        open('config.cfg', 'w').write(text)
        c = T.read_config('config.cfg')
        assert c['auc_statistics'] and c['auc_bootstrap'] == 50 and c['auc_bootstrap_block'] == 2 and c['direct_test'] == (route == 'direct')
        S.main('config.cfg')
        printed = capsys.readouterr().out
        for name in NAMES:
            assert '%s micro AUROC is ' % name in printed and '%s macro AUROC is ' % name in printed
        assert 'frame_smooth - frame macro AUROC is ' in printed and 'pixel_smooth - pixel micro AUROC is ' in printed
        assert _tree() == sorted(off_tree + ['UCSDped2/' + p for p in boots]), route       # the bootstrap files and no other
        for p, content in off.items():                                                     # every other file: byte for byte the key-off run's
            assert _content(os.path.join('results', p)) == content, (route, p)
        want = expected()
        got[route] = {name: dict(np.load(RES + p)) for name, p in zip(NAMES, boots)}
        for name in NAMES:
            assert ('paired_micro_diff' in got[route][name]) == (name in PLAIN)
            assert R.entries_equal(got[route][name], want[name]), (route, name)
            assert got[route][name]['macro_replicates'].shape == (50,) and got[route][name]['macro_n_groups_valid'] == 2
    for name in NAMES:                                                     # the same files on both routes
        assert R.entries_equal(got['staged'][name], got['direct'][name]), name

    # ---- scores_saved = True: the same files from the saved vectors, nothing is scored
    for p in boots:
        os.remove(RES + p)
    open('config.cfg', 'w').write(on.replace('scores_saved = False', 'scores_saved = True'))

    def scored(*a, **k):
        raise AssertionError('scores_saved = True must not score')

    for fn in ('score_frames', 'score_direct', '_smooth_stage'):
        monkeypatch.setattr(S, fn, scored)
    S.main('config.cfg')
    for name, p in zip(NAMES, boots):
        assert R.entries_equal(dict(np.load(RES + p)), got['staged'][name]), name

    # ---- tools/compare_scores.py on two of the saved vectors: the paired entries of the stage
    import compare_scores as CS
    capsys.readouterr()
    res_a, res_b, pair = CS.main([RES + VECTOR['frame_smooth'] % TAIL, RES + VECTOR['frame'] % TAIL, '--config', 'config.cfg'])
    printed = capsys.readouterr().out
    assert 'A micro AUROC is ' in printed and 'B macro AUROC is ' in printed and 'A - B macro AUROC is ' in printed
    stage = got['staged']['frame_smooth']
    assert R.entries_equal(_flat(pair, 'paired_'), {k: v for k, v in stage.items() if k.startswith('paired_')})
    assert R.entries_equal(_flat(res_a), {k: v for k, v in stage.items() if not k.startswith('paired_')})
    assert R.entries_equal(_flat(res_b), got['staged']['frame'])
