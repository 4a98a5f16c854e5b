"""Iterative min/max on the GPU: the K14b kernel pair (dx_iter_round.hip) against
the pure-Python model and, bit for bit, against its host twin -- also with one
DP of 200000 rows, where the tile plan's chunk is 128 rows -- and searches end
to end at range 1000 in base 10 (three rounds), without and with proofs.  Run
with -m gpu."""
import pytest
import torch

import test_iter_extreme as ti
from drynx_amd import native as nt
from drynx_amd.services.api import DrynxClient
from drynx_amd.services.local import local_cluster

pytestmark = pytest.mark.gpu


def test_rows_equal_the_model_and_the_host(gpu_device):
    dev = ti.check_rows(gpu_device)
    host = ti.check_rows("cpu")
    assert len(dev) == len(host) and all(torch.equal(a, b) for a, b in zip(dev, host))


def test_rows_at_the_widest_base(gpu_device):
    dev = ti.check_rows(gpu_device, **ti.WIDEST)
    host = ti.check_rows("cpu", **ti.WIDEST)
    assert len(dev) == len(host) == 4 and all(torch.equal(a, b) for a, b in zip(dev, host))


def test_one_large_dp(gpu_device):
    """200000 + 0 + 70 rows: chunk = 128, 1563 tiles for DP 0 (stage 2 strides its partials)."""
    seg = [200_000, 0, 70]
    plan, first = nt._tile_plan(torch.tensor(seg).numpy())
    assert plan[0, 2] - plan[0, 1] == 128 and first.tolist() == [0, 1563, 1563, 1564]
    qmin, qmax, b = -50, 10 ** 6 - 51, 100
    L = ti.model_rounds(qmax - qmin + 1, b)
    g = torch.Generator().manual_seed(5)
    Z = torch.randint(qmin + 1000, qmax - 1000, (sum(seg), 1), generator=g)
    Zd = Z.to(gpu_device)
    for name in ("max", "min"):
        is_max = name == "max"
        ext = [int(Z[:200_000].max() if is_max else Z[:200_000].min()), None,
               int(Z[200_000:].max() if is_max else Z[200_000:].min())]
        o = ext[0] - qmin
        for k in range(L):
            for prefix in {o // b ** (L - k), (ext[2] - qmin) // b ** (L - k)}:
                got = nt.iter_round(name, Zd, seg, qmin, qmax, b, k, prefix)
                want = [ti.model_row([e] if e is not None else [], is_max, qmin, qmax, b, L, k, prefix) for e in ext]
                assert got.cpu().tolist() == want
                assert torch.equal(got.cpu(), nt.iter_round(name, Z, seg, qmin, qmax, b, k, prefix))


@pytest.fixture(scope="module")
def genv(gpu_device, tmp_path_factory):
    torch.cuda.set_device(gpu_device)
    cl, node = local_cluster(3, 5, 3, device=gpu_device, workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node, device=gpu_device)
    node.close(remove=True)


def test_search_fixed_records_gpu(genv, gpu_device):
    cl, node, client = genv
    ti.check_search_fixed(cl, node, client, gpu_device, 0, 999, 10)


def test_search_generated_records_gpu(genv):
    cl, node, client = genv
    ti.check_search_generated(cl, node, client, 0, 999, 10)


def test_search_with_proofs_gpu(genv, gpu_device):
    cl, node, client = genv
    rounds = ti.check_search_with_proofs(cl, node, client, gpu_device, 999, 10)
    assert len(rounds) == 3
