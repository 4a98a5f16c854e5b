"""The torus first pass of the verifier's GT multi-exponentiation
(csrc/kernels/dx_me_torus.hip) on the GPU against the host path of the same
ops, bit for bit: the image rows for chunk lengths that leave ragged last
chunks, the lane-pair slice products for slice counts around the 32 pairs of
a wave with lengths 0..17 and skip rows, and a small plan of the headline's
shape."""
import random

import pytest
import torch

from drynx_amd import native as nt
from drynx_amd.crypto import bn254 as bn
from drynx_amd.crypto import oracle as O

pytestmark = pytest.mark.gpu
RNG = random.Random(20262)


@pytest.fixture(scope="module")
def gt_pool(gpu_device):
    """(host, device) copies of 200 random GT elements with rows of 1 at 0, 77
    and 199; shared and never modified."""
    g = O.pairing(O.G1_GEN, O.G2_GEN)
    base = bn.gt_tensor([g ** RNG.randrange(1, O.R) for _ in range(4)], gpu_device)
    k = bn.scalars_tensor([RNG.randrange(O.R) for _ in range(200)], gpu_device)
    a = nt.gt_pow(base.repeat(50, 1).contiguous(), k)
    for i in (0, 77, 199):
        a[i] = nt.gt_one(gpu_device)[0]
    return a.cpu(), a


@pytest.mark.parametrize("rows_per_inv", [1, 4, 8])
@pytest.mark.parametrize("m", [1, 63, 200])
def test_beta_rows_device_matches_host(gt_pool, m, rows_per_inv):
    host, dev = gt_pool
    off = 200 - m                                              # every m ends on the row of 1
    got = nt.gt_beta_rows(dev[off:].contiguous(), rows_per_inv)
    ref = nt.gt_beta_rows(host[off:].contiguous(), rows_per_inv)
    assert not ref[m - 1].any() and not ref[2 * m - 1].any()
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("n_slices", [1, 31, 32, 33, 70])
def test_beta_slice_prod_device_matches_host(gt_pool, gpu_device, n_slices):
    """A lone pair, a wave one pair short, a full wave, one pair into a second
    wave, a ragged third wave; lengths drawn from 0..17 per slice."""
    host, _ = gt_pool
    beta = nt.gt_beta_rows(host, 8)                            # [400, 48], skip rows at 0, 77, 199 (+ 200)
    rnd = random.Random(n_slices)
    lens = [rnd.randrange(18) for _ in range(n_slices)]
    if n_slices > 2:
        lens[1], lens[2] = 0, 17
    start = torch.tensor([rnd.randrange(400 - 17) for _ in range(n_slices)], dtype=torch.int64)
    start[0] = 70                                              # row 77 inside the first slice when it is long enough
    length = torch.tensor(lens, dtype=torch.int32)
    idx = torch.tensor([rnd.randrange(400) for _ in range(400)], dtype=torch.int64)
    idx[::7] = 77                                              # skip rows all over the gathered slices
    for ix in (None, idx):
        got = nt.gt_beta_slice_prod(beta.to(gpu_device), None if ix is None else ix.to(gpu_device),
                                    start.to(gpu_device), length.to(gpu_device))
        ref = nt.gt_beta_slice_prod(beta, ix, start, length)
        assert torch.equal(got.cpu(), ref)
        assert torch.equal(nt.gt_pi(got).cpu(), nt.gt_pi(ref))


def test_multi_exp_device_on_images_device_matches_host(gpu_device):
    """The headline's plan shape (G = 3, the 16-bit windows me_window picks at
    its size: one lane per bucket) at m = 1,000 items, and 5-bit windows, where
    a bucket has 8 lanes and the tree passes run over the numerators."""
    m, G = 1000, 3
    rnd = random.Random(7)
    g = O.pairing(O.G1_GEN, O.G2_GEN)
    base = bn.gt_tensor([g ** rnd.randrange(1, O.R) for _ in range(4)], gpu_device)
    A = nt.gt_pow(base.repeat(m // 4, 1).contiguous(),
                  bn.scalars_tensor([rnd.randrange(O.R) for _ in range(m)], gpu_device))
    A[11] = nt.gt_one(gpu_device)[0]
    gen = torch.Generator().manual_seed(3)
    k = torch.zeros((3 * G * m, 8), dtype=torch.int64)
    k[:, 0] = torch.randint(0, 1 << 32, (3 * G * m,), generator=gen)
    k[2 * G * m:, 1] = torch.randint(0, 1 << 8, (G * m,), generator=gen)
    k = k.to(torch.int32)
    e = torch.arange(3 * G * m)
    grp = torch.where(e < 2 * G * m, e // (2 * m), G + (e - 2 * G * m) // m).to(torch.int32)
    groups = ((2 * m, 32),) * G + ((m, 40),) * G
    for W, c in ((3, 16), (8, 5)):
        out = []
        for dev in (gpu_device, torch.device("cpu")):
            beta2 = nt.gt_beta_rows(A.to(dev))
            h = nt.multi_exp_device(beta2, k.to(dev), grp.to(dev), groups, W, c, item_split=(2 * G * m, m))
            out.append(nt.multi_exp_grouped_finish(h))
            nt.check_overflow(h)
        assert torch.equal(out[0], out[1]), (W, c)
