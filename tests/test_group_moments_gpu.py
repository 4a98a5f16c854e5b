"""K14d on the GPU: the checks of tests/test_group_moments.py (the pure-Python
model, ``int_moments`` over the selected rows) on the gfx950 kernel, every
output ``torch.equal`` to the host twin's, and one further case with a DP of
70,000 rows (uniform keys, then all in one group).  Run with -m gpu."""
import pytest
import torch

import test_group_moments as tg

pytestmark = pytest.mark.gpu


def _same(dev, host):
    assert len(dev) == len(host) and all(torch.equal(a, b) for a, b in zip(dev, host))


def test_small_shapes_equal_the_model_and_the_host(gpu_device):
    _same(tg.check_small(gpu_device), tg.check_small("cpu"))


def test_products_wrap(gpu_device):
    _same(tg.check_wrap(gpu_device), tg.check_wrap("cpu"))


def test_two_windows(gpu_device):
    _same(tg.check_windows(gpu_device), tg.check_windows("cpu"))


def test_wide_pair_list(gpu_device):
    _same(tg.check_wide(gpu_device), tg.check_wide("cpu"))


def test_counts(gpu_device):
    _same(tg.check_counts(gpu_device), tg.check_counts("cpu"))


def test_one_large_dp(gpu_device):
    dev = tg.check_large(gpu_device)
    assert len(dev) == 4
    _same(dev, tg.check_large("cpu"))
