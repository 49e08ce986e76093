"""``bin_device`` of the two GPU trainers: validation and where "auto" lands
when no GPU is visible."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from creditcore.models import hgbt
from creditcore.models.hgbt import HistGBTClassifier
from creditcore.models.hrf import HistForestClassifier

ESTIMATORS = [HistGBTClassifier, HistForestClassifier]


@pytest.fixture
def no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def _xy():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(200, 4)).astype(np.float32)
    return x, (x[:, 0] + x[:, 1] > 0).astype(np.int64)


@pytest.mark.parametrize("cls", ESTIMATORS)
def test_bin_device_is_validated(cls):
    with pytest.raises(ValueError, match="bin_device must be"):
        cls(n_estimators=2, device="cpu", bin_device="gpu").fit(*_xy())


@pytest.mark.parametrize("cls", ESTIMATORS)
def test_cpu_fit_refuses_device_bins(cls):
    with pytest.raises(ValueError, match="numpy bins"):
        cls(n_estimators=2, device="cpu", bin_device="cuda").fit(*_xy())


@pytest.mark.parametrize("cls", ESTIMATORS)
def test_auto_bins_on_the_host_without_a_gpu(cls, no_gpu, monkeypatch):
    monkeypatch.setattr(hgbt, "bin_features_gpu", None)  # would fail if called
    auto = cls(n_estimators=2, max_depth=3).fit(*_xy())
    host = cls(n_estimators=2, max_depth=3, device="cpu", bin_device="cpu").fit(*_xy())
    assert auto.fit_device_ == "cpu"
    np.testing.assert_array_equal(auto.threshold_, host.threshold_)
    assert hgbt.resolve_bin_device("auto", "auto", "cpu", 10**7) == "cpu"
    assert hgbt.resolve_bin_device("auto", "auto", "cuda", 10**7) == "cuda"


@pytest.mark.parametrize("cls", ESTIMATORS)
def test_cuda_bins_raise_without_a_gpu(cls, no_gpu):
    with pytest.raises(RuntimeError, match="no GPU is visible"):
        cls(n_estimators=2, device="auto", bin_device="cuda").fit(*_xy())
