"""bench.py --dump-outputs: what the last timed step left behind, written as .npy files -- checked here on a host-side parameter store (no GPU)."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from iseg_amd.param_store import ParamStore  # noqa: E402


class _Metric:
    def __init__(self, cm):
        self.total_cm = cm


class _Wrapper:
    def __init__(self, cm):
        self.metric = _Metric(cm)


class _Trainer:
    def __init__(self, params, cm):
        self.store = ParamStore(params)
        self._cm = cm

    def _metrics_for(self, i):
        return [_Wrapper(self._cm)] if i == 0 else []


def _trainer(seed):
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((37, 5), (300,), (3, 3, 7, 11), (1,))]
    cm = torch.arange(21 * 21, dtype=torch.int64) * (1 << 26)
    return _Trainer(params, cm), params


def _dump(tmp_path, monkeypatch, sample, seed=0):
    monkeypatch.setattr(bench, "DUMP_WEIGHT_SAMPLE", sample)
    tr, params = _trainer(seed)
    out = tmp_path / f"dump_{sample}_{seed}"
    bench.dump_outputs(str(out), tr, [torch.tensor(2.5, requires_grad=True)])
    return out, params


def test_dump_writes_loss_weights_and_confusion_matrix(tmp_path, monkeypatch):
    out, params = _dump(tmp_path, monkeypatch, sample=1 << 20)      # more than there are elements: every weight, in parameter order
    assert sorted(os.listdir(out)) == ["confusion_matrix_output_1_0.npy", "loss.npy", "weights_sample.npy"]
    loss = np.load(out / "loss.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [2.5]
    w = np.load(out / "weights_sample.npy")
    assert w.dtype == np.float32
    np.testing.assert_array_equal(w, torch.cat([p.detach().reshape(-1) for p in params]).numpy())
    cm = np.load(out / "confusion_matrix_output_1_0.npy")
    assert cm.dtype == np.float64 and cm[-1] == 440 * (1 << 26)


def test_dump_sample_is_fixed_and_taken_from_real_elements(tmp_path, monkeypatch):
    a, params = _dump(tmp_path, monkeypatch, sample=200)
    b, _ = _dump(tmp_path, monkeypatch, sample=200, seed=0)
    wa, wb = np.load(a / "weights_sample.npy"), np.load(b / "weights_sample.npy")
    assert wa.shape == (200,)
    np.testing.assert_array_equal(wa, wb)
    flat = torch.cat([p.detach().reshape(-1) for p in params]).numpy()
    assert np.isin(wa, flat).all()      # never the store's alignment padding


def test_the_flagship_dump_stays_under_64_mb():
    assert bench.DUMP_WEIGHT_SAMPLE * 4 + 21 * 21 * 8 + 8 <= 64 << 20


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
