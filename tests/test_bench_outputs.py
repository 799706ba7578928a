"""bench.py --dump-outputs: what the last timed step computed, written as .npy within 64 MB, the same inputs on every run; and a
plain run (no --full) that carries the headline fields and nothing that needs runs of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 4000)
    g = torch.Generator().manual_seed(3)
    arrays = {'small': torch.randn(10, 5, generator=g), 'big': torch.randn(3000, generator=g),
              'wide': torch.randn(7, generator=g, dtype=torch.float64), 'half': torch.randn(40, generator=g).half()}
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), arrays)
    a = {n: np.load(tmp_path / 'a' / f'{n}.npy') for n in arrays}
    b = {n: np.load(tmp_path / 'b' / f'{n}.npy') for n in arrays}
    assert sum(v.nbytes for v in a.values()) <= 4000
    assert a['wide'].dtype == np.float64 and all(a[n].dtype == np.float32 for n in ('small', 'big', 'half'))
    np.testing.assert_array_equal(a['small'], arrays['small'].numpy())              # within its share: whole, same shape
    np.testing.assert_array_equal(a['half'], arrays['half'].float().numpy())
    assert 0 < a['big'].size < 3000                                                 # over its share: a sample of the elements
    assert np.isin(a['big'], arrays['big'].numpy()).all()
    for n in arrays:                                                                # the same sample on every run
        np.testing.assert_array_equal(a[n], b[n])


def test_plain_flags():
    import bench
    args = bench.parse(['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert args.steps == 7 and not args.full and args.dump_outputs == ''
    assert bench.parse(['--full', '--dump-outputs', 'd']).full
    with pytest.raises(SystemExit):
        bench.parse(['--steps', '0'])
    assert bench.parse(['--dump-kernels', 'k.json']).full                          # the per-kernel table is a --full measurement


def _bench(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '2',
                        '--height', '64', '--width', '96', '--dump-outputs', str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-1000:]
    return json.loads(lines[0]), {f[:-4]: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    line, a = _bench(tmp_path / 'a')
    assert line['steps'] == 4 and line['ms_per_step'] > 0 and line['value'] > 0 and line['finite'] is True
    assert line['unit'] == 'images/sec' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    for k in ('fwd_ms_per_img', 'eager_autograd', 'roofline', 'stage_roofline', 'cpu_baseline', 'neck', 'extract_feat'):
        assert line[k] is None, k                                                   # measured with --full only
    assert sorted(a) == ['grads', 'out0', 'out1', 'out2', 'out3', 'params']
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a['out0'].shape == (2, 16, 24, 18) and float(np.abs(a['grads']).max()) > 0
    # same arguments: same inputs and weights, and every one of the 8 steps (2 eager ones of the hipGraph capture, 2 warm-up,
    # 4 timed) starts from the same weights, so the last step computes the same as in any other run, up to the rounding of
    # the atomic gradient reductions
    _, b = _bench(tmp_path / 'b')
    for n in a:
        assert a[n].shape == b[n].shape, n
        err = np.linalg.norm(a[n].astype(np.float64) - b[n]) / max(np.linalg.norm(a[n].astype(np.float64)), 1e-30)
        assert err < 1e-5, (n, err)
