"""Macro AUROC and bootstrap statistics ([mi355x] auc_statistics) on the host: the plain-numpy restatement
(tests/auc_bootstrap_restatement.py) against independent forms -- a brute-force O(n^2) pair count, ``utils.frame_roc_auc``, the
quadratic form over per-video-pair counts --, the weight invariants of both resampling units, the interval and 5 % rules, the host
half of ``vec_vad_amd.scoring`` (tables, statistic, interval, paired rule, settings), the config keys, and the share of invalid
replicates on the inputs the GPU tests use.  No GPU is needed."""
import os
import sys
import warnings

import numpy as np
import pytest

import auc_bootstrap_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
KEYS = ('auc_statistics', 'auc_bootstrap', 'auc_bootstrap_unit', 'auc_bootstrap_block', 'auc_bootstrap_seed', 'auc_confidence')
SEEDS = (0, (1 << 63) + 12345)


def brute(scores, labels, w):
    """(U2, P, N) by looking at every (positive, negative) pair."""
    scores, labels, w = np.asarray(scores, np.float64), np.asarray(labels).astype(bool), [int(v) for v in w]
    u2 = 0
    for i in np.nonzero(labels)[0]:
        for j in np.nonzero(~labels)[0]:
            u2 += w[i] * w[j] * (2 if scores[j] < scores[i] else (1 if scores[j] == scores[i] else 0))
    return u2, sum(w[i] for i in np.nonzero(labels)[0]), sum(w[j] for j in np.nonzero(~labels)[0])


def small_set(seed=3):
    """5 videos of 9 / 1 / 30 / 17 / 12 frames, scores with many ties, video 1 (one frame) all-normal."""
    rng = np.random.default_rng(seed)
    lens = np.array([9, 1, 30, 17, 12])
    video = np.repeat(np.arange(lens.size) + 4, lens)
    scores = np.round(rng.standard_normal(lens.sum()), 1)
    labels = rng.random(lens.sum()) < 0.4
    labels[9] = False
    scene = np.repeat([2, 2, 7, 7, 7], lens)
    return scores, labels, video, scene


def test_mix_is_splitmix64_and_draw_stays_below_m():
    assert R.mix(0) == 0xE220A8397B1DCDAF                                 # the first output of SplitMix64 seeded with 0
    assert R.mix(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4                # ... and its second
    for seed in SEEDS:
        for m in (1, 2, 7, 65536, (1 << 31) - 1):
            d = [R.draw(seed, r, s, j, m) for r in (1, 2, 1000) for s in (0, 3, 1 << 32) for j in range(20)]
            assert all(isinstance(v, int) and 0 <= v < m for v in d)
            assert m == 1 or len(set(d)) > 1
    assert R.draw(0, 1, 0, 0, 1 << 32) == R.mix(R.mix(R.mix(R.mix(0) ^ 1) ^ 0) ^ 0) >> 32
    # every argument matters
    base = R.draw(5, 1, 2, 3, 1 << 30)
    assert len({base, R.draw(6, 1, 2, 3, 1 << 30), R.draw(5, 2, 2, 3, 1 << 30), R.draw(5, 1, 3, 3, 1 << 30), R.draw(5, 1, 2, 4, 1 << 30)}) == 5


def test_full_sample_counts_equal_the_brute_force_and_frame_roc_auc():
    from utils import frame_roc_auc
    scores, labels, video, scene = small_set()
    for groups in (None, scene, video):
        c = R.counts(scores, labels, video, groups, 'none', 1, 0, 1, 1)
        members = R.group_members(groups, scores.size)
        assert c.shape == (1, len(members), 3) and c.dtype == np.int64
        for g, idx in enumerate(members):
            assert tuple(c[0, g]) == brute(scores[idx], labels[idx], np.ones(idx.size, int))
            u2, p, q = (int(v) for v in c[0, g])
            if p and q:
                assert abs(u2 / (2.0 * p * q) - frame_roc_auc(scores[idx], labels[idx])) < 1e-12
    flat = np.zeros(7)
    assert tuple(R.counts(flat, [1, 0, 1, 0, 0, 1, 1], np.zeros(7, int), None, 'none', 1, 0, 1, 1)[0, 0]) == (12, 4, 3)    # all tied: U2 = P * N


@pytest.mark.parametrize('seed', SEEDS)
def test_video_unit_is_the_quadratic_form_over_per_video_pair_counts(seed):
    scores, labels, video, scene = small_set()
    off = R.runs(video)
    V = off.size - 1
    C = np.zeros((V, V), np.int64)
    Pv, Nv = np.zeros(V, np.int64), np.zeros(V, np.int64)
    for a in range(V):
        ia = np.arange(off[a], off[a + 1])
        Pv[a], Nv[a] = labels[ia].sum(), (~labels[ia]).sum()
        for b in range(V):
            ib = np.arange(off[b], off[b + 1])
            pos, neg = ia[labels[ia]], ib[~labels[ib]]
            C[a, b] = sum(2 * int(scores[j] < scores[i]) + int(scores[j] == scores[i]) for i in pos for j in neg)
    for strata, stratum_off in ((None, [0, V]), (scene, [0, 2, 5])):
        for r in (1, 2, 77):
            m = R.multiplicities(seed, r, stratum_off)
            assert all(m[stratum_off[s]:stratum_off[s + 1]].sum() == stratum_off[s + 1] - stratum_off[s] for s in range(len(stratum_off) - 1))
            w = R.weights('video', seed, r, off, stratum_off)
            assert np.array_equal(w, np.repeat(m, np.diff(off)))
            got = R.counts(scores, labels, video, None, 'video', 1, seed, r, 1, strata)[0, 0]
            assert tuple(int(v) for v in got) == (int(m @ C @ m), int(m @ Pv), int(m @ Nv))
            per_scene = R.counts(scores, labels, video, scene, 'video', 1, seed, r, 1, strata)[0]
            for g, vs in enumerate(([0, 1], [2, 3, 4])):
                mg = np.zeros(V, np.int64)
                mg[vs] = m[vs]
                assert tuple(int(v) for v in per_scene[g]) == (int(mg @ C @ mg), int(mg @ Pv), int(mg @ Nv))
    mults = {tuple(R.multiplicities(seed, r, [0, V])) for r in range(1, 30)}
    assert len(mults) > 5                                                  # replicates differ


@pytest.mark.parametrize('block', [1, 7, 25, 1000])
def test_block_unit_equals_the_brute_force_weighted_count_and_keeps_k_times_b(block):
    scores, labels, video, scene = small_set()
    off = R.runs(video)
    for seed in SEEDS:
        for r in (1, 5):
            w = R.weights('block', seed, r, off, None, block)
            for v in range(off.size - 1):
                L = int(off[v + 1] - off[v])
                b = min(block, L)
                assert int(w[off[v]:off[v + 1]].sum()) == -(-L // b) * b >= L                # the weighted length is k * b: not trimmed
                if block >= L:
                    assert (w[off[v]:off[v + 1]] == 1).all()                                  # one block that is the video
            for groups in (None, scene, video):
                c = R.counts(scores, labels, video, groups, 'block', block, seed, r, 1)[0]
                for g, idx in enumerate(R.group_members(groups, scores.size)):
                    assert tuple(int(x) for x in c[g]) == brute(scores[idx], labels[idx], w[idx])
    assert not np.array_equal(R.weights('block', 0, 1, off, None, 7), R.weights('block', 0, 2, off, None, 7))


def test_replicates_split_over_calls_and_do_not_depend_on_the_scores():
    scores, labels, video, scene = small_set()
    for unit in ('video', 'block'):
        whole = R.counts(scores, labels, video, video, unit, 7, 9, 1, 6, scene)
        parts = np.concatenate([R.counts(scores, labels, video, video, unit, 7, 9, 1, 2, scene),
                                R.counts(scores, labels, video, video, unit, 7, 9, 3, 4, scene)])
        assert np.array_equal(whole, parts)
        other = R.counts(-scores, labels, video, video, unit, 7, 9, 1, 6, scene)
        assert np.array_equal(whole[:, :, 1:], other[:, :, 1:])            # P and N: the weights are the same
        assert np.array_equal(whole[:, :, 0] + other[:, :, 0], 2 * whole[:, :, 1] * whole[:, :, 2])      # mirrored scores: U2' = 2 P N - U2


def test_statistic_skips_one_class_groups_and_interval_follows_the_index_rule():
    from vec_vad_amd import scoring
    for S, I in ((R.statistic, R.interval), (scoring.auc_statistic, scoring.auc_interval)):
        assert S(np.array([[3, 2, 3], [0, 0, 5], [7, 4, 0], [4, 2, 2]])) == ((3 / 12.0 + 4 / 8.0) / 2, 2)
        stat, valid = S(np.array([[0, 0, 5], [0, 3, 0]]))
        assert np.isnan(stat) and valid == 0
        reps = np.arange(1000, dtype=np.float64)[::-1].copy()
        assert I(reps, 95) == (24.0, 975.0, 0)                             # k = (5 * 999) // 200 = 24
        assert I(reps, 50) == (249.0, 750.0, 0) and I(reps, 99) == (4.0, 995.0, 0)
        assert I(reps[:1], 95) == (0.0 + 999.0, 999.0, 0)
        reps[:50] = np.nan                                                 # exactly 5 %: still an interval, over the 950 valid ones
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            lo, hi, bad = I(reps, 95)
        assert bad == 50 and (lo, hi) == (23.0, 926.0)                     # k = (5 * 949) // 200 = 23, a = 0..949
        reps[50] = np.nan                                                  # 51 of 1000: more than 5 %
        with pytest.warns(UserWarning, match='51 of 1000'):
            lo, hi, bad = I(reps, 95)
        assert bad == 51 and np.isnan(lo) and np.isnan(hi)


def test_paired_rule():
    from vec_vad_amd import scoring
    st = dict(n_replicates=6, unit='block', block=25, seed=0, confidence=95)
    a = dict(auc=0.75, replicates=np.array([0.5, 0.625, np.nan, 0.75, 0.25, 0.5]), **st)
    b = dict(auc=0.5, replicates=np.array([0.25, 0.625, 0.5, np.nan, 0.5, 0.25]), **st)
    for P in (R.paired, scoring.auc_paired):
        with pytest.warns(UserWarning):                                    # 2 of 6 invalid: no interval, but the differences stand
            p = P(a, b)
        assert p['diff'] == 0.25 and p['n_invalid'] == 2 and np.isnan(p['lo']) and np.isnan(p['hi'])
        assert np.array_equal(p['replicates'], [0.25, 0.0, np.nan, np.nan, -0.25, 0.25], equal_nan=True)
        assert p['frac_le0'] == 2 / 4.0
    c = dict(a, replicates=np.linspace(0.5, 0.75, 6))
    d = dict(b, replicates=np.linspace(0.25, 0.625, 6))
    for P in (R.paired, scoring.auc_paired):
        p = P(c, d)
        assert (p['lo'], p['hi'], p['n_invalid'], p['frac_le0']) == (0.125, 0.25, 0, 0.0)
    with pytest.warns(UserWarning, match='1 of 6'):
        both = scoring.auc_paired({'micro': c, 'macro': a}, {'micro': d, 'macro': a})
    assert sorted(both) == ['macro', 'micro'] and both['macro']['diff'] == 0.0 and both['macro']['frac_le0'] == 1.0
    with pytest.raises(ValueError, match='different settings'):
        scoring.auc_paired(a, dict(b, seed=1))
    flat = scoring.auc_flatten(both, 'paired_')
    assert 'paired_micro_frac_le0' in flat and 'paired_macro_replicates' in flat and len(flat) == 12


def test_tables_follow_the_contract_and_refuse_what_the_kernel_cannot_take():
    from vec_vad_amd import scoring
    scores, labels, video, scene = small_set()
    n = scores.size
    for groups in (None, scene, video):
        t = scoring.auc_tables(scores, labels, video, groups, scene)
        members = R.group_members(groups, n)
        assert (t['n'], t['G'], t['V'], t['S']) == (n, len(members), 5, 2)
        assert all(t[k].dtype == np.int32 for k in ('order', 'tie', 'group_off', 'video_off', 'stratum_off')) and t['label'].dtype == np.uint8
        assert t['video_off'].tolist() == [0, 9, 10, 40, 57, 69] and t['stratum_off'].tolist() == [0, 2, 5]
        assert np.array_equal(t['label'], labels.astype(np.uint8)) and sorted(t['order'].tolist()) == list(range(n))
        ranks = set()
        for g, idx in enumerate(members):
            seg = slice(t['group_off'][g], t['group_off'][g + 1])
            o, tie = t['order'][seg], t['tie'][seg]
            assert sorted(o.tolist()) == idx.tolist()
            s = scores[o]
            assert (np.diff(s) >= 0).all() and all(o[k] < o[k + 1] for k in range(len(o) - 1) if s[k] == s[k + 1])       # ascending, stable
            assert np.array_equal(np.diff(tie), (np.diff(s) != 0).astype(int))                                              # dense ranks
            assert not ranks & set(tie.tolist())                                                                            # never shared
            ranks |= set(tie.tolist())
    assert scoring.auc_tables(scores, labels, video)['stratum_off'].tolist() == [0, 5]
    empty = scoring.auc_tables(np.zeros(0), np.zeros(0), np.zeros(0, int))
    assert (empty['n'], empty['G'], empty['V']) == (0, 1, 0) and empty['group_off'].tolist() == [0, 0]
    half = scene.copy()
    half[3] = 7                                                            # a group that cuts a video
    for kw, text in ((dict(groups=half), 'groups must be a union of whole videos'), (dict(strata=half), 'strata must be a union of whole videos'),
                     (dict(video_idx=np.where(np.arange(n) == 50, 4, video)), 'frames of one video must be contiguous'),
                     (dict(strata=np.repeat([2, 7, 2, 7, 7], [9, 1, 30, 17, 12])), 'must follow one another'),
                     (dict(scores=np.where(np.arange(n) == 3, np.nan, scores)), 'NaN'), (dict(labels=labels[:-1]), 'labels for'),
                     (dict(video_idx=video.astype(float)), 'with an integer')):
        a = dict(scores=scores, labels=labels, video_idx=video, groups=None, strata=None)
        a.update(kw)
        with pytest.raises(ValueError, match=text) as e:
            scoring.auc_tables(**a)
        assert '\n' not in str(e.value)
    big = 70000
    with pytest.raises(ValueError, match='70000 videos, at most 65536'):
        scoring.auc_tables(np.zeros(big), np.zeros(big), np.arange(big))
    with pytest.raises(ValueError, match='U2 would not fit int64'):
        scoring.auc_tables(np.zeros(60000), np.zeros(60000), np.arange(60000))          # 60000 * 60000 >= 2^31
    assert scoring.auc_tables(np.zeros(60000), np.zeros(60000), np.arange(60000), strata=np.arange(60000) // 10)['S'] == 6000


def test_settings_and_config_keys(tmp_path):
    import train as T
    from vec_vad_amd import scoring
    assert scoring.auc_settings() == dict(n_replicates=1000, unit='block', block=25, seed=0, confidence=95)
    assert scoring.auc_settings(0, 'Video', 1, 2 ** 64 - 1, 50)['seed'] == 2 ** 64 - 1
    for kw in (dict(replicates=-1), dict(replicates=2.5), dict(unit='frame'), dict(block=0), dict(seed=-1), dict(seed=2 ** 64),
               dict(confidence=49), dict(confidence=100), dict(confidence=True)):
        with pytest.raises(ValueError):
            scoring.auc_settings(**kw)
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    for key in KEYS:
        assert c['cp'].has_option('mi355x', key), key
    assert [c[k] for k in KEYS] == [False, 1000, 'block', 25, 0, 95]
    text = open(os.path.join(ROOT, 'config.cfg')).read()
    p = tmp_path / 'config.cfg'
    p.write_text(text.replace('auc_statistics = False', 'auc_statistics = True').replace('auc_bootstrap = 1000', 'auc_bootstrap = 0')
                 .replace('auc_bootstrap_unit = block', 'auc_bootstrap_unit = Video').replace('auc_confidence = 95', 'auc_confidence = 50')
                 .replace('auc_bootstrap_seed = 0', 'auc_bootstrap_seed = 18446744073709551615'))
    c = T.read_config(str(p))
    assert [c[k] for k in KEYS] == [True, 0, 'video', 25, 2 ** 64 - 1, 50]
    p.write_text('\n'.join(l for l in text.splitlines() if not l.startswith('auc_')) + '\n')      # a file from before the keys
    c = T.read_config(str(p))
    assert not any(c['cp'].has_option('mi355x', k) for k in KEYS) and [c[k] for k in KEYS] == [False, 1000, 'block', 25, 0, 95]
    # checked whatever the switch says
    for key, stock, bads in (('auc_bootstrap', '1000', ('-1', '2.5', 'many')), ('auc_bootstrap_unit', 'block', ('frame', 'none', '')),
                             ('auc_bootstrap_block', '25', ('0', '-25', '1.5')), ('auc_bootstrap_seed', '0', ('-1', '18446744073709551616')),
                             ('auc_confidence', '95', ('49', '100', '0', '95.0'))):
        for bad in bads:
            p.write_text(text.replace('%s = %s' % (key, stock), '%s = %s' % (key, bad)))
            with pytest.raises(ValueError):
                T.read_config(str(p))


def test_auc_stage_refuses_an_indexer_of_another_length():
    import test as S
    with pytest.raises(ValueError, match='indexes 3 frames, 4 frame labels'):
        S._auc_stage({}, {}, [0, 1, 0, 1], [1, 1, 2], None, '{}', 'cpu')


@pytest.mark.parametrize('unit', ['block', 'video'])
def test_invalid_share_stays_below_the_cap_on_the_inputs_the_gpu_tests_use(unit):
    """The 5 % rule on the committed inputs: the script-level tree (test videos of 7 and 5 frames, every odd frame anomalous) and the
    array set of six videos (one all-normal, one all-anomalous).  Validity depends on the labels and the weights alone."""
    sets = {'tree': (np.zeros(12), np.array([k % 2 for k in range(7)] + [k % 2 for k in range(5)], bool), np.repeat([1, 2], [7, 5]))}
    sets['arrays'] = R.array_set()
    for name, (scores, labels, video) in sets.items():
        for kind, groups in (('micro', None), ('macro', video)):
            c = R.counts(scores, labels, video, groups, unit, 25, 0, 1, 400)
            invalid = sum(R.statistic(x)[1] == 0 for x in c)
            print('%s, %s, unit %s: %d of 400 replicates invalid' % (name, kind, unit, invalid))
            assert invalid * 20 <= 400, (name, kind, invalid)
