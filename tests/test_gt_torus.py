"""GT chains on torus images (csrc/bn254/gt_torus.h), host paths against the
Python oracle: the GLS-8 GT table holds beta = (1 + g) / h of each power, the
table prover (mode 7) runs y <- y (+-beta + w) and maps the numerator to the
canonical Fp12 value at the end.

Scalars cover an empty GLV half (k < 6u^2 leaves k1 = 0; k = 6u^2 leaves
k0 = 0), the carry out of the top byte window and both digit signs (r - 1,
6u^2 - 1), and 0 (an empty chain: the result must be the limbs of 1)."""
import random

import pytest
import torch

from drynx_amd import native as nt
from drynx_amd.crypto import bn254 as bn
from drynx_amd.crypto import oracle as O

RNG = random.Random(20261)
LAM = 6 * O.U * O.U
SCALARS = [0, 1, O.R - 1, LAM, LAM - 1, RNG.randrange(O.R)]


@pytest.fixture(scope="module")
def material():
    g = O.pairing(O.G1_GEN, O.G2_GEN)
    E = [g ** RNG.randrange(1, O.R) for _ in range(2)]
    return g, E, nt.gt_gls8_table(bn.gt_tensor(E, "cpu"))


def test_table_entries_decompress_to_powers(material):
    _, E, tabs = material
    assert tabs.shape == (2 * nt.GLS8_ENTRIES, 48)
    rows, want = [], []
    for b in range(2):
        for w in (0, 8, 16):
            for d in (1, 2, 127, 128):
                rows.append(b * nt.GLS8_ENTRIES + w * 128 + d - 1)
                want.append(E[b] ** (d << (8 * w)))
    got = nt.gt_t2_decompress(tabs[rows].contiguous())
    assert torch.equal(got, bn.gt_tensor(want, "cpu"))


def test_table_rejects_a_base_without_image():
    with pytest.raises(RuntimeError):
        nt.gt_gls8_table(bn.gt_tensor([-O.Fp12.one()], "cpu"))


def test_unit_base_is_skipped_by_the_prover():
    """E = 1 (a set's padding point at infinity) has no image: its rows are
    marked, and a chain over them leaves gT^t."""
    from drynx_amd.proofs.range_proof import gt_generator_table

    g = O.pairing(O.G1_GEN, O.G2_GEN)
    tabs = nt.gt_gls8_table(bn.gt_tensor([O.Fp12.one()], "cpu"))
    assert bool((tabs == -1).all())
    _, comb = gt_generator_table("cpu")
    es, ts = [O.R - 1, 5], [7, 0]
    got = nt.rp_prove_a_tab(tabs, torch.zeros(2, dtype=torch.int32), bn.scalars_tensor(es, "cpu"),
                            bn.scalars_tensor(ts, "cpu"), comb, 1, 1, 7)
    assert torch.equal(got, bn.gt_tensor([g ** 7, O.Fp12.one()], "cpu"))


def test_prover_mode7_matches_oracle(material):
    from drynx_amd.proofs.range_proof import gt_generator_table

    g, E, tabs = material
    _, comb = gt_generator_table("cpu")
    S, L, n_p = 2, 6, 6                                                    # item (p, i, j): t = SCALARS[j]
    k = len(SCALARS)
    ts = [SCALARS[j] for _ in range(n_p) for j in range(L)]
    es, tidx = [], []
    for p in range(n_p):
        for i in range(S):
            for j in range(L):
                es.append(SCALARS[(p + i * (j + 1)) % k])                  # server 0: every (e, t) pair
                tidx.append((p + i + j) % 2)
    got = nt.rp_prove_a_tab(tabs, torch.tensor(tidx, dtype=torch.int32), bn.scalars_tensor(es, "cpu"),
                            bn.scalars_tensor(ts, "cpu"), comb, S, L, 7)
    pe = {(b, e): E[b] ** e for b in range(2) for e in SCALARS}
    pt = {t: g ** t for t in SCALARS}
    want = [pe[(tidx[n], es[n])] * pt[ts[(n // (S * L)) * L + n % L]] for n in range(len(es))]
    assert torch.equal(got, bn.gt_tensor(want, "cpu"))
    # e = t = 0 (p = 0, server 0, j = 0): exactly the limbs of 1
    assert es[0] == 0 and ts[0] == 0
    assert torch.equal(got[0], bn.gt_tensor([O.Fp12.one()], "cpu")[0])
