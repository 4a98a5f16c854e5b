"""GT chains on torus images on the GPU (csrc/bn254/gt_torus.h: a lane pair per
item) against the host path of the same ops, bit for bit: the GLS-8 table
builder (Fp12 powers, then one shared inversion per 16 entries), the 16-bit gT
table, and the three prover passes of dx_rp_prove_a_gls8 (numerator of gT^t,
numerator of E^e times it, canonical value).  Item counts are not multiples of
the 32 pairs per wave, and (3, 1, 11) puts a single pair into a second wave."""
import random

import pytest
import torch

from drynx_amd import native as nt
from drynx_amd.crypto import bn254 as bn
from drynx_amd.crypto import oracle as O

pytestmark = pytest.mark.gpu
RNG = random.Random(20262)


@pytest.fixture(scope="module")
def tables(gpu_device):
    g = O.pairing(O.G1_GEN, O.G2_GEN)
    # four bases of the order-r group and the unit (a set's padding point: marked rows, skipped steps)
    bases = bn.gt_tensor([g ** RNG.randrange(1, O.R) for _ in range(4)] + [O.Fp12.one()], "cpu")
    return nt.gt_gls8_table(bases), nt.gt_gls8_table(bases.to(gpu_device))


def test_gls8_table_builder_matches_host(tables):
    host, dev = tables
    assert dev.shape == (5 * nt.GLS8_ENTRIES, 48)
    assert torch.equal(dev.cpu(), host)
    assert bool((host[4 * nt.GLS8_ENTRIES:] == -1).all())


def test_gls8_table_rejects_a_base_without_image(gpu_device):
    with pytest.raises(RuntimeError):
        nt.gt_gls8_table(bn.gt_tensor([-O.Fp12.one()], gpu_device))


def test_gt16_table_entries_are_images_of_the_powers(gpu_device):
    g = O.pairing(O.G1_GEN, O.G2_GEN)
    tab = nt.gt16_table(gpu_device)
    assert tab.shape == (17 * 32768, 48)
    wd = [(0, 1), (0, 2), (0, 32768), (1, 17), (7, 32767), (16, 1), (16, 32768)]
    rows = torch.tensor([w * 32768 + d - 1 for w, d in wd], device=gpu_device)
    got = nt.gt_t2_decompress(tab.index_select(0, rows).contiguous())
    assert torch.equal(got.cpu(), bn.gt_tensor([g ** (d << (16 * w)) for w, d in wd], "cpu"))


@pytest.mark.parametrize("S,L,n_p", [(3, 5, 3), (1, 1, 1), (3, 1, 11)])
def test_gls8_prover_pairs_match_host(tables, gpu_device, S, L, n_p):
    from drynx_amd.proofs.range_proof import gt_generator_table

    host, dev = tables
    n = n_p * S * L
    tidx = torch.tensor([RNG.randrange(5) for _ in range(n)], dtype=torch.int32)
    es = ([RNG.randrange(O.R) for _ in range(n)] + [0, O.R - 1])[-n:]
    ts = ([RNG.randrange(O.R) for _ in range(n_p * L)] + [O.R - 1, 0])[-n_p * L:]
    e_sc, t_sc = bn.scalars_tensor(es, "cpu"), bn.scalars_tensor(ts, "cpu")
    _, comb = gt_generator_table("cpu")
    got = nt.rp_prove_a_tab(dev, tidx.to(gpu_device), e_sc.to(gpu_device), t_sc.to(gpu_device), None, S, L, 7)
    ref = nt.rp_prove_a_tab(host, tidx, e_sc, t_sc, comb, S, L, 7)
    assert torch.equal(got.cpu(), ref)
