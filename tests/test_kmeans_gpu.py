"""K-means on the GPU: the K14f kernel (dx_kmeans.hip) against the pure-Python
model and, bit for bit, its host twin -- every (d, k) case of the CPU suite, the
ties and the largest distances, and one DP of 70000 rows at k = 17, d = 5 (many
tiles and a ragged one; uniform records, then every row in one cluster) -- and
the runs end to end (fixed and generated records, (16, 2) proofs).  Run with
-m gpu."""
import pytest
import torch

import test_kmeans as tk
from drynx_amd.services.api import DrynxClient
from drynx_amd.services.local import local_cluster

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", tk.DIMS)
def test_rows_equal_the_model_and_the_host(gpu_device, d):
    dev = tk.check_rows(gpu_device, d)
    host = tk.check_rows("cpu", d)
    assert len(dev) == len(host) == 5 and all(torch.equal(a, b) for a, b in zip(dev, host))


def test_ties_and_largest_distances_gpu(gpu_device):
    dev = tk.check_edges(gpu_device)
    host = tk.check_edges("cpu")
    assert dev.keys() == host.keys() and all(torch.equal(dev[n], host[n]) for n in dev)


def test_one_large_dp(gpu_device):
    dev = tk.check_large(gpu_device)
    host = tk.check_large("cpu")
    assert len(dev) == len(host) == 2 and all(torch.equal(a, b) for a, b in zip(dev, host))


@pytest.fixture(scope="module")
def genv(gpu_device, tmp_path_factory):
    torch.cuda.set_device(gpu_device)
    cl, node = local_cluster(3, 5, 3, device=gpu_device, workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node, device=gpu_device)
    node.close(remove=True)


def test_run_fixed_records_gpu(genv, gpu_device):
    cl, node, client = genv
    tk.check_run_fixed(cl, node, client, gpu_device)
    tk.check_run_fixed(cl, node, client, gpu_device, lo=-60)


def test_run_generated_records_gpu(genv, gpu_device):
    cl, node, client = genv
    tk.check_run_generated(cl, node, client, gpu_device)


def test_run_with_proofs_gpu(genv, gpu_device):
    cl, node, client = genv
    rounds = tk.check_run_with_proofs(cl, node, client, gpu_device)
    assert len(rounds) == 2
