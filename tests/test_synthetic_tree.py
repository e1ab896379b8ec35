"""CPU: ``tools/synthetic_tree.make_tree`` builds, for a given seed, the files the two builders it replaced did
(``time_direct_test.make_tree`` / ``time_direct_train.make_train_tree``; values recorded by golden/make_synthetic_tree_golden.py)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from _util import GOLDEN, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('tag', ['test_tool', 'train_tool'])
def test_make_tree_builds_the_files_of_the_builders_it_replaced(tmp_path, monkeypatch, tag):
    rec = _load(os.path.join(GOLDEN, 'make_synthetic_tree_golden.py'), 'make_synthetic_tree_golden')
    tree = _load(os.path.join(ROOT, 'tools', 'synthetic_tree.py'), 'synthetic_tree')
    a = rec.TREE_ARGS
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, 'path', list(sys.path))            # summarise() puts tests/ on the path
    if tag == 'test_tool':                                      # the calls of time_direct_test / _flow and of time_direct_train
        tree.make_tree({'train': (6, 6), 'test': (a['test_frames'],)}, a['boxes'])
    else:
        tree.make_tree({'train': a['train_videos']}, a['boxes'], flow=False)
    got = rec.summarise('.')
    want = {k[len(tag) + 1:]: v for k, v in load_golden('synthetic_tree').items() if k.startswith(tag + '/')}
    assert sorted(got) == sorted(want) and 'frames' in want and ('flow' in want) == (tag == 'test_tool')
    for k, v in want.items():
        assert got[k].shape == v.shape, k
        if k in ('frames', 'gt', 'flow'):
            # digest rows: float64 sums over <= 172800 values of magnitude <= 255, whose order of summation is the library's --
            # round-off <= 1e-16 * sum|x| < 1e-8, while one changed pixel moves the weighted sum by its own size
            assert np.allclose(got[k], v, rtol=1e-12, atol=1e-6), k
        else:
            assert np.array_equal(got[k], v), k                 # paths, counts and seeded float64 box draws: exact
    assert all(os.path.basename(p) == '%04d.tif' % (int(os.path.basename(p)[:4])) for p in got['frames_paths'])
    assert not os.path.exists('optical_flow') or tag == 'test_tool'
