"""Iterative quantiles on the GPU: the K14c kernel pair (dx_iter_round.hip)
against the pure-Python model, the classic histogram and, bit for bit, its host
twin -- also with one DP of 70000 rows at b = 1000 (68 tiles of 1024 rows and a
ragged one; uniform records, then all in one bin) -- and rank walks end to end
over 100 values in base 10 (two rounds), without and with (16, 2) proofs.  Run
with -m gpu."""
import pytest
import torch

import test_iter_quantile as tq
from drynx_amd.services.api import DrynxClient
from drynx_amd.services.local import local_cluster

pytestmark = pytest.mark.gpu


def test_rows_equal_the_model_and_the_host(gpu_device):
    dev = tq.check_rows(gpu_device)
    host = tq.check_rows("cpu")
    assert len(dev) == len(host) and all(torch.equal(a, b) for a, b in zip(dev, host))


def test_one_large_dp(gpu_device):
    dev = tq.check_large(gpu_device)
    host = tq.check_large("cpu")
    assert len(dev) == len(host) == 4 and all(torch.equal(a, b) for a, b in zip(dev, host))


@pytest.fixture(scope="module")
def genv(gpu_device, tmp_path_factory):
    torch.cuda.set_device(gpu_device)
    cl, node = local_cluster(3, 5, 3, device=gpu_device, workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node, device=gpu_device)
    node.close(remove=True)


def test_search_fixed_records_gpu(genv, gpu_device):
    cl, node, client = genv
    tq.check_search_fixed(cl, node, client, gpu_device, 0, 99, 10)
    tq.check_search_fixed(cl, node, client, gpu_device, -40, 59, 10)


def test_search_generated_records_gpu(genv):
    cl, node, client = genv
    tq.check_search_generated(cl, node, client, 0, 99, 10)


def test_search_with_proofs_gpu(genv, gpu_device):
    cl, node, client = genv
    rounds = tq.check_search_with_proofs(cl, node, client, gpu_device, 99, 10)
    assert len(rounds) == 2
