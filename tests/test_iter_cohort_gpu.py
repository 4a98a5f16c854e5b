"""Iterative rounds over SQL cohorts on the GPU: the grouped digit histogram
(dx_iter_round_cells in dx_iter_round.hip) against the pure-Python model and,
bit for bit, its host twin -- per-cell prefixes over a strided table, group
windows (b = 4096 over two windows, b = 2 over 4096 groups and over two
windows), one DP of 70000 rows with every row on one counter -- and the
per-cell quantile and extreme searches end to end over 100 values in base 10,
without and with (16, 2) proofs.  Run with -m gpu."""
import pytest
import torch

import test_iter_cohort as tc
from drynx_amd.services.api import DrynxClient
from drynx_amd.services.local import local_cluster

pytestmark = pytest.mark.gpu


def _same(dev, host):
    assert len(dev) == len(host) and all(torch.equal(a, b) for a, b in zip(dev, host))


def test_rows_equal_the_model_and_the_host(gpu_device):
    _same(tc.check_rows(gpu_device), tc.check_rows("cpu"))


def test_windows(gpu_device):
    _same(tc.check_windows(gpu_device), tc.check_windows("cpu"))


def test_contention_and_tiles(gpu_device):
    _same(tc.check_contention(gpu_device), tc.check_contention("cpu"))


@pytest.fixture(scope="module")
def genv(gpu_device, tmp_path_factory):
    torch.cuda.set_device(gpu_device)
    cl, node = local_cluster(3, 5, 3, device=gpu_device, workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node, device=gpu_device)
    node.close(remove=True)


def test_search_fixed_tables_gpu(genv, gpu_device):
    cl, node, client = genv
    tc.check_search_fixed(cl, node, client, gpu_device, 0, 99, 10)


def test_search_with_proofs_gpu(genv, gpu_device):
    cl, node, client = genv
    assert len(tc.check_search_with_proofs(cl, node, client, gpu_device, 10)) == 2
