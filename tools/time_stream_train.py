"""The figures of profiles/stream_train.md.

    python tools/time_stream_train.py [--short] [--out FILE.json]

One process: a ``StreamScorer`` (stock configuration, a 1x1 grid, a model with its initial weights) and a ``StreamCollector`` are
pushed the same 90 frames of 240x360 with 12 boxes each, twice in turn; per frame the host clock around ``push`` and around ``push`` +
``torch.cuda.synchronize()`` (the frame's last enqueued launch has completed), medians over frames 10.. of the second pass.  Then the
wall time of ``train.main`` (direct_train, direct_flow, one pair per launch) and of ``stream_train.main`` on the 7-frame synthetic tree
of tests/test_gpu_direct_train.py, three times in turn.  FlowNet2 carries seeded random weights.  ``--short``: 24 frames and the
pushes only -- the run to put under ``rocprofv3 --kernel-trace --stats`` for the device time of ``vv_stream_append``."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import train as T  # noqa: E402
from FlowNet2_src import FlowNet2  # noqa: E402
from test import artifacts_from  # noqa: E402
from vec_vad_amd.stream import StreamScorer  # noqa: E402
from vec_vad_amd.stream_train import StreamCollector  # noqa: E402

short = '--short' in sys.argv
OUT = os.path.abspath(sys.argv[sys.argv.index('--out') + 1]) if '--out' in sys.argv else None
out = {}
torch.manual_seed(0)
flownet = FlowNet2().cuda().eval()
c = T.read_config(os.path.join(ROOT, 'config.cfg'))
H, W, NB, N = 240, 360, 12, (24 if short else 90)
rng = np.random.default_rng(0)
base = rng.integers(0, 256, (H, W + 2 * N, 3), dtype=np.uint8)
frames = [np.ascontiguousarray(base[:, 2 * k:2 * k + W]) for k in range(N)]
boxes = []
for k in range(N):
    x0, y0 = rng.uniform(0, W - 70, NB), rng.uniform(0, H - 70, NB)
    boxes.append(np.stack([x0, y0, x0 + rng.uniform(10, 64, NB), y0 + rng.uniform(10, 64, NB)], axis=1))

net = T.build_network(c)
sd = {'module.' + k: v.detach().clone() for k, v in net.state_dict().items()}
arts = artifacts_from([[[sd]]], [[rng.random(100).astype(np.float32) + 1]], [[rng.random(100).astype(np.float32) + 1]], False,
                      lambda: T.build_network(c), torch.device('cuda'))


def run(obj):
    host, done = [], []
    for f, b in zip(frames, boxes):
        t0 = time.perf_counter()
        obj.push(f, b)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.append(t1 - t0)
        done.append(t2 - t0)
    obj.end_video()
    torch.cuda.synchronize()
    w = 10
    return dict(push_host_us=float(np.median(host[w:]) * 1e6), push_done_us=float(np.median(done[w:]) * 1e6))


scorer = StreamScorer(c, *arts, (H, W, 3), flownet2=flownet)
col = StreamCollector(c, (H, W, 3), flownet2=flownet, max_cubes=4096)
for rep in range(2):                      # alternate, the second pass is reported
    out['scorer'] = run(scorer)
    out['collector'] = run(col)
st = col.finish()
out['collector_cubes'] = st['n']
print(json.dumps(out))
if short:
    if OUT:
        json.dump(out, open(OUT, 'w'), indent=1)
    sys.exit(0)

# wall time on the synthetic tree
from test_gpu_direct_train import _cfg, _tree  # noqa: E402
import stream_train as ST  # noqa: E402
os.chdir(tempfile.mkdtemp())
cfg = _tree()
_cfg(cfg, direct_train=True, direct_flow=True, direct_flow_pairs=1)
wall = {'train_main': [], 'stream_train_main': []}
for rep in range(3):
    for name, fn in (('train_main', T.main), ('stream_train_main', ST.main)):
        torch.manual_seed(5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn('config.cfg', flownet2=flownet)
        torch.cuda.synchronize()
        wall[name].append(time.perf_counter() - t0)
out['wall_s'] = wall
print(json.dumps(out))
if OUT:
    json.dump(out, open(OUT, 'w'), indent=1)
