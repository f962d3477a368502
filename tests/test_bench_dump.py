"""not-gpu: bench.py --dump-outputs writes the last step's logged losses and model state as DIR/<name>.npy in float32 / float64,
and an output above the size budget is replaced by a fixed sample.  No kernel is launched here."""
import os

import numpy as np
import torch

import bench


class _Trainer:
    def __init__(self, n):
        torch.manual_seed(0)
        self.model = torch.nn.Sequential(torch.nn.Conv2d(1, n, 3), torch.nn.BatchNorm2d(n))
        self.losses = {"loss_ae": [torch.tensor(0.5), torch.tensor(0.25)], "loss_latent_1": [0.125], "loss_unused": []}


def test_dump_outputs_names_and_dtypes(tmp_path):
    tr = _Trainer(4)
    bench.dump_outputs(tr, str(tmp_path))
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(["loss_ae.npy", "loss_latent_1.npy"] + ["state.%s.npy" % k for k in tr.model.state_dict()])
    assert np.load(tmp_path / "loss_ae.npy").tolist() == [0.25]             # the LAST step's value
    assert np.load(tmp_path / "loss_ae.npy").dtype == np.float64
    w = np.load(tmp_path / "state.0.weight.npy")
    assert w.dtype == np.float32 and np.array_equal(w, tr.model[0].weight.detach().numpy())
    assert np.load(tmp_path / "state.1.num_batches_tracked.npy").dtype == np.float64


def test_dump_outputs_samples_above_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 256)
    tr = _Trainer(64)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(tr, str(a))
    bench.dump_outputs(tr, str(b))
    assert sum(np.load(a / f).nbytes for f in os.listdir(a)) <= 256 + 8 * len(os.listdir(a))      # one element at most over each share
    assert "state.0.weight.sample.npy" in os.listdir(a) and "state.0.weight.npy" not in os.listdir(a)
    for f in os.listdir(a):                                                  # the sample is the same from run to run
        assert np.array_equal(np.load(a / f), np.load(b / f))
    s = np.load(a / "state.0.weight.sample.npy")
    assert 0 < s.size < 64 * 9 and np.isin(s, tr.model[0].weight.detach().numpy().ravel()).all()
