"""SQL WHERE / GROUP BY surveys on the GPU: the checks of tests/test_sql_query.py
with the cluster, the DPs' records and the K14d kernel on the device.  Run with
-m gpu."""
import pytest
import torch

import test_sql_query as ts
from drynx_amd.services.api import DrynxClient
from drynx_amd.services.local import local_cluster

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def genv(gpu_device, tmp_path_factory):
    torch.cuda.set_device(gpu_device)
    cl, node = local_cluster(3, 5, 3, device=gpu_device, workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node, device=gpu_device)
    node.close(remove=True)


def test_mean_and_variance_by_group_gpu(genv, gpu_device):
    ts.check_mean_variance(*genv, gpu_device)


def test_counting_operations_by_two_columns_gpu(genv, gpu_device):
    ts.check_counting(*genv, gpu_device)


def test_where_without_group_by_gpu(genv, gpu_device):
    ts.check_where_only(*genv, gpu_device)


def test_grouped_mean_with_proofs_gpu(genv, gpu_device):
    plain = ts.check_mean_variance(*genv, gpu_device)["mean"]
    ts.check_proofs(*genv, gpu_device, plain)


def test_empty_sql_replicates_gpu(genv):
    ts.check_empty_sql(*genv)


def test_generated_tables_gpu(genv):
    ts.check_generated(*genv)
