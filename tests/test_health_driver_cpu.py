"""The training driver without ``training.health``: nothing changes -- no recorder is attached to the trainer and the log lines
have exactly the form they had before the flight recorder existed.  (With the key present the driver needs the GPU:
tests/test_health_gpu.py.)  The kernels are emulated by tests/cpu_shim.py; the driver is the product code."""
import re

import torch

from tests import synth
from tests.test_drivers_cpu import _driver_cfg, _dataset, shim  # noqa: F401  (the shim fixture)
from tests.test_model_cpu import V

# f'epoch {epoch} step {step} loss {loss:.4f} lr {lr:.3e} {seconds:.1f}s' -- and nothing behind it
LINE = re.compile(r'epoch \d+ step \d+ loss (\d+\.\d{4}|nan) lr \d\.\d{3}e[-+]\d{2} \d+\.\d{1}s')


def test_without_the_key_the_driver_logs_and_launches_as_before(shim, tmp_path, monkeypatch):
    from gpv1_amd import health, train_distr as td
    from gpv1_amd.default_config import default_tree
    assert 'health' not in default_tree()['training']              # opt-in: not part of the default configuration
    made = []
    monkeypatch.setattr(health.FlightRecorder, '__init__', lambda self, *a, **k: made.append(1))
    torch.manual_seed(0)
    logs = []
    cfg = _driver_cfg(tmp_path)
    model, tr, step = td.train_worker(cfg, dataset=_dataset(synth.make_vocab(V)), device='cpu', log=logs.append)
    lines = [l for l in logs if l.startswith('epoch')]
    assert step == 4 and len(lines) == 4
    for i, l in enumerate(lines):
        assert LINE.fullmatch(l), l
        assert l.startswith(f'epoch {i // 2} step {i + 1} loss '), l
    assert tr.recorder is None and not made

