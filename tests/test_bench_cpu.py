"""bench.py's self-launcher on a host without a GPU: `--gpus N` must fail cleanly, naming the visible device count, before anything is started."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_without_enough_devices_names_the_visible_count():
    import torch
    n_vis = torch.cuda.device_count()
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(n_vis + 2)], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode != 0
    assert 'only %d GPU(s) visible' % n_vis in out.stderr and 'nothing launched' in out.stderr


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs (bench.dump_outputs on host tensors): float32 / float64 files within the byte budget, small tensors whole, a larger one as a
    sample of its elements drawn the same way on every call."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 1 << 20)
    big = torch.arange(1 << 20, dtype=torch.float32).reshape(1024, 1024)
    outs = {'loss': torch.tensor(0.5), 'n_pair': torch.tensor([7], dtype=torch.int64), 'grad.a/kernel': torch.ones(3, 4), 'dx': big, 'none': None}
    for d in ('one', 'two'):
        bench.dump_outputs(str(tmp_path / d), outs)
    names = sorted(p.name for p in (tmp_path / 'one').iterdir())
    assert names == ['dx.npy', 'grad.a.kernel.npy', 'loss.npy', 'n_pair.npy']
    assert sum(np.load(tmp_path / 'one' / n).nbytes for n in names) <= 1 << 20
    assert np.load(tmp_path / 'one' / 'loss.npy').dtype == np.float32 and float(np.load(tmp_path / 'one' / 'loss.npy')) == 0.5
    assert np.load(tmp_path / 'one' / 'n_pair.npy').dtype == np.float64 and np.load(tmp_path / 'one' / 'n_pair.npy').tolist() == [7.0]
    assert np.load(tmp_path / 'one' / 'grad.a.kernel.npy').shape == (3, 4)
    dx = np.load(tmp_path / 'one' / 'dx.npy')
    assert dx.dtype == np.float32 and 0.8 * (1 << 18) < dx.size < (1 << 18)            # distinct draws of 2^18 from the 2^20 elements: ~88 % of them
    assert np.all(np.diff(dx) > 0) and np.array_equal(dx, np.load(tmp_path / 'two' / 'dx.npy'))        # distinct, ascending, the same each call


def test_steps_below_one_is_refused():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode != 0 and '--steps must be at least 1' in out.stderr


def test_full_is_an_option_off_by_default():
    """--full (everything besides the headline figure) is parsed and documented (off unless given: tests/test_bench_gpu.py)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--full', '--steps', '0'], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode != 0 and '--steps must be at least 1' in out.stderr and 'unrecognized' not in out.stderr
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and '--full' in out.stdout
