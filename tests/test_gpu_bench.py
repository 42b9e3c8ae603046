"""GPU (-m gpu): the plain `bench.py --gpus 1 --steps K --warmup W` run and its `--dump-outputs DIR`.

A plain run does the headline only: its line has the headline fields, counts exactly K steps and carries none of what
`--full` measures (roofline, also, cpu_baseline).  The dump holds what the last timed step computed -- every head's heat maps,
the loss, the module's state after the update -- in float32 / float64, within 64 MB.  The dumped heat maps are the ones the dumped
loss was computed from (their MSE against the seeded targets).  In a dumping run the last train step starts from the seeded state
again, so two runs with the same arguments agree: forward outputs, loss and BatchNorm buffers to rounding, the parameters after the
update to the order-dependent last bits of the heads' weight-gradient atomics (a near-zero gradient whose sign they flip moves its
parameter by 2 x 10 x lr in RMSprop's first step: a few such elements at most).  Different inputs or weights would be O(1) apart."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir, steps=3, warmup=1):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
           '--dump-outputs', str(out_dir)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_line_and_output_dump(tmp_path):
    a, b = tmp_path / 'a', tmp_path / 'b'
    out = _plain_run(a)
    assert out['steps'] == 3 and out['warmup'] == 1 and out['n_gpus'] == 1
    assert out['unit'] == 'images/sec' and out['higher_is_better'] is True and out['dtype'] == 'f32'
    assert out['metric'].startswith('images/sec train step')
    assert out['value'] > 0 and abs(out['value'] - 24 * 3 / (out['ms_per_step'] * 3e-3)) <= 1e-2 * out['value']
    for key in ('roofline', 'also', 'cpu_baseline'):
        assert key not in out, key

    files = sorted(os.listdir(a))
    assert files == sorted(['heatmap_0.npy', 'heatmap_1.npy', 'loss.npy', 'params.npy', 'buffers.npy', 'counters.npy']), files
    assert sum(os.path.getsize(a / f) for f in files) <= 64 * 10 ** 6
    got = {f[:-4]: np.load(a / f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got['heatmap_0'].shape == (24, 68, 64, 64) and got['heatmap_1'].shape == (24, 68, 64, 64)
    assert all(np.isfinite(v).all() for v in got.values())
    assert abs(float(got['loss']) - out['final_loss']) <= 1e-6 * abs(out['final_loss'])
    assert got['counters'].max() > 0 and (got['counters'] == np.round(got['counters'])).all()      # num_batches_tracked

    # the dump belongs to the last step: its heat maps give its loss (sum over heads of the pixelwise MSE against the seeded targets)
    sys.path.insert(0, ROOT)
    from bench import synthetic_batch
    _, target = synthetic_batch(24, 68, 256, seed=1000, device='cpu')
    tgt = target.numpy().astype(np.float64)
    mse = sum(float(np.mean((got[f'heatmap_{i}'].astype(np.float64) - tgt) ** 2)) for i in range(2))
    assert abs(mse - float(got['loss'])) <= 1e-5 * abs(mse), (mse, float(got['loss']))

    _plain_run(b)                            # same arguments -> same inputs -> the same last step
    for name, v in got.items():
        w = np.load(b / (name + '.npy'))
        assert w.shape == v.shape and w.dtype == v.dtype, name
        v64, w64 = v.astype(np.float64), w.astype(np.float64)
        if name == 'counters':
            assert np.array_equal(w, v), name
        elif name == 'params':
            rel = np.linalg.norm(w64 - v64) / np.linalg.norm(v64)
            moved = int((np.abs(w64 - v64) > 1e-6).sum())
            assert rel <= 1e-3 and moved <= 1e-3 * v.size, (name, rel, moved)
        else:
            assert np.allclose(w64, v64, rtol=1e-5, atol=1e-7), (name, float(np.abs(w64 - v64).max()))
