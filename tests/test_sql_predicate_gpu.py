"""``QuerySQL.Predicate`` on the GPU: the checks of tests/test_sql_predicate.py
(this suite's own per-row model) on the gfx950 kernels, every output
``torch.equal`` to the host twin's; the binding's refusals through the GPU-only
cohort encoder; the mean with proofs and the per-cell median end to end with
the cluster on the device.  Run with -m gpu."""
import pytest
import torch

import test_sql_predicate as tp
from drynx_amd import native as nt
from drynx_amd.services.api import DrynxClient
from drynx_amd.services.local import local_cluster

pytestmark = pytest.mark.gpu


def _same(dev, host):
    assert len(dev) == len(host) and all(torch.equal(a, b) for a, b in zip(dev, host))


def test_atoms_equal_the_model_and_the_host(gpu_device):
    _same(tp.check_atoms(gpu_device), tp.check_atoms("cpu"))


def test_formulas_equal_the_model_and_the_host(gpu_device):
    _same(tp.check_formulas(gpu_device), tp.check_formulas("cpu"))


def test_plans(gpu_device):
    _same(tp.check_plans(gpu_device), tp.check_plans("cpu"))


def test_two_windows_and_a_strided_view(gpu_device):
    _same(tp.check_windows(gpu_device), tp.check_windows("cpu"))


def test_cohort_encoder_cells(gpu_device):
    _same(tp.check_lr_cells(gpu_device), tp.check_lr_cells("cpu"))


def test_cohort_encoder_refusals(gpu_device):
    _, K = tp.tables()
    X = torch.zeros((tp.N, 2), dtype=torch.float64, device=gpu_device)
    y = torch.zeros(tp.N, dtype=torch.int64, device=gpu_device)
    for f in (nt.lr_encode_cells_many, nt.lr_encode_cells_packed_many):
        for predicate, text in (((("~",), 1), "unknown operator"), ((("==", "<"), 1), "2 operators for 1"),
                                ((("==",), 4), "truth table outside")):
            with pytest.raises(ValueError, match=text):
                f([X], [y], [K.to(gpu_device)], [0.0, 0.0], [1.0, 1.0], -1.0, tp.KEYS, [(3, 1)], predicate=predicate)
        with pytest.raises(ValueError, match="predicate without filter terms"):
            f([X], [y], [K.to(gpu_device)], [0.0, 0.0], [1.0, 1.0], -1.0, tp.KEYS, [], predicate=((), 1))


@pytest.fixture(scope="module")
def genv(gpu_device, tmp_path_factory):
    torch.cuda.set_device(gpu_device)
    cl, node = local_cluster(3, 5, 3, device=gpu_device, workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node, device=gpu_device)
    node.close(remove=True)


def test_mean_with_proofs_end_to_end_gpu(genv, gpu_device):
    tp.check_mean(*genv, gpu_device, True)


def test_median_per_cell_end_to_end_gpu(genv):
    tp.check_median(*genv)
