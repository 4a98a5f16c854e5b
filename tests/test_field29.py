"""The 9 x 29-bit-limb Montgomery core (csrc/bn254/field.h, tower.h) on the host
path, through the probe binding, against Python integers: every result is the
canonical a b R^-1 mod the modulus (Fp2: both coefficients), R = 2^256.

The file also carries the limb model of each primitive (unpack with a pre-shift,
the REDC column loop with R' = 2^261, pack).  The model proves the bounds the
header states -- no column reaches 2^64 with every limb at its contract maximum,
the value before the conditional subtraction stays below twice the modulus --
and picks, for every reduction of every opcode, a vector whose value before
the subtraction is at least the modulus and one whose value is below it, so both
branches of the conditional subtraction are exercised."""
import random

import numpy as np
import pytest
import torch

from drynx_amd import native as nt
from drynx_amd.crypto import bn254 as bn
from drynx_amd.crypto import oracle as O

P, R = O.P, O.R
RM = 1 << 256
M29 = (1 << 29) - 1
OPS = [nt.PROBE_FP_MUL, nt.PROBE_FP_SQR, nt.PROBE_FR_MUL, nt.PROBE_FP2_MUL, nt.PROBE_FP2_SQR, nt.PROBE_FP2_MUL_FP]
N_RANDOM = 10000


def modulus(opc):
    return R if opc == nt.PROBE_FR_MUL else P


def fixed_operands(q):
    """The edge values of the issue, all below the modulus q."""
    v = [0, 1, q - 1, q - 2, RM % q, RM * RM % q]
    for k in range(1, 9):
        v += [(1 << (29 * k)) - 1, 1 << (29 * k), (1 << (29 * k)) + 1]
    for k in range(1, 8):
        v += [(1 << (32 * k)) - 1, (1 << (32 * k)) + 1]
    v += [q - (1 << (29 * k)) for k in range(1, 9)]
    assert all(0 <= x < q for x in v)
    return v


def fixed_vectors(opc):
    """Operand rows (a, b) of an opcode over every pairing of the edge values.
    An Fp operand is an int, an Fp2 operand a pair of ints; b is None for the
    squarings."""
    v = fixed_operands(modulus(opc))
    n = len(v)
    pairs = [(i, j) for i in range(n) for j in range(n)]
    if opc in (nt.PROBE_FP_MUL, nt.PROBE_FR_MUL):
        return [(v[i], v[j]) for i, j in pairs]
    if opc == nt.PROBE_FP_SQR:
        return [(x, None) for x in v]
    if opc == nt.PROBE_FP2_SQR:
        return [((v[i], v[j]), None) for i, j in pairs]
    if opc == nt.PROBE_FP2_MUL_FP:
        return [((v[i], v[(i + 1) % n]), v[j]) for i, j in pairs]
    # Fp2 mul: every pairing inside an operand, and every pairing across the two
    return ([((v[i], v[j]), (v[j], v[i])) for i, j in pairs]
            + [((v[i], v[(i + 1) % n]), (v[j], v[(j + 1) % n])) for i, j in pairs])


def random_vectors(opc, n, rng):
    q = modulus(opc)

    def fp():
        return rng.randrange(q)

    def fp2():
        return (fp(), fp())

    if opc in (nt.PROBE_FP_MUL, nt.PROBE_FR_MUL):
        return [(fp(), fp()) for _ in range(n)]
    if opc == nt.PROBE_FP_SQR:
        return [(fp(), None) for _ in range(n)]
    if opc == nt.PROBE_FP2_SQR:
        return [(fp2(), None) for _ in range(n)]
    if opc == nt.PROBE_FP2_MUL_FP:
        return [(fp2(), fp()) for _ in range(n)]
    return [(fp2(), fp2()) for _ in range(n)]


def expected(opc, a, b):
    """a b R^-1 mod q on Python integers, as a flat tuple of coefficients."""
    q = modulus(opc)
    ri = pow(RM, -1, q)
    if opc in (nt.PROBE_FP_MUL, nt.PROBE_FR_MUL):
        return (a * b * ri % q,)
    if opc == nt.PROBE_FP_SQR:
        return (a * a * ri % q,)
    if opc == nt.PROBE_FP2_MUL:
        return ((a[0] * b[0] - a[1] * b[1]) * ri % q, (a[0] * b[1] + a[1] * b[0]) * ri % q)
    if opc == nt.PROBE_FP2_SQR:
        return ((a[0] * a[0] - a[1] * a[1]) * ri % q, 2 * a[0] * a[1] * ri % q)
    return (a[0] * b * ri % q, a[1] * b * ri % q)


def flat(x):
    return list(x) if isinstance(x, tuple) else [x]


def tensors(opc, vecs, device="cpu"):
    wa = 2 if opc >= nt.PROBE_FP2_MUL else 1
    a = bn.ints_to_limbs([c for x, _ in vecs for c in flat(x)]).reshape(len(vecs), 8 * wa)
    ta = bn.to_tensor(a, device)
    if vecs[0][1] is None:
        return ta, None
    wb = 1 if opc == nt.PROBE_FP2_MUL_FP else wa
    b = bn.ints_to_limbs([c for _, y in vecs for c in flat(y)]).reshape(len(vecs), 8 * wb)
    return ta, bn.to_tensor(b, device)


def probe_ints(opc, vecs, device="cpu"):
    """Rows of coefficient tuples the native probe returns for the vectors."""
    a, b = tensors(opc, vecs, device)
    out = bn.to_numpy(nt.field_probe(opc, a, b))
    w = out.shape[1] // 8
    ints = bn.limbs_to_ints(out.reshape(-1, 8))
    return [tuple(ints[w * i: w * i + w]) for i in range(len(vecs))]


# ----------------------------------------------------------------------------- limb model
def unpack(x, sh):
    """Nine 29-bit limbs of x << sh (x < 2^256, sh in {0, 5})."""
    x <<= sh
    assert x < 1 << 261
    return [(x >> (29 * k)) & M29 for k in range(9)]


def redc_cols(q, prods, limbs_m=None):
    """The column loop of l29::redc_cols on limb lists: prods is a list of
    (A, B) limb vectors whose products are summed.  Returns (value before the
    conditional subtraction, largest column).  limbs_m forces every Montgomery
    digit to a given value (the bound run); the value is then meaningless."""
    pl = unpack(q, 0)
    ninv = (-pow(q, -1, 1 << 29)) % (1 << 29)
    m, u = [0] * 9, [0] * 9
    acc = top = 0
    for i in range(9):
        for j in range(i + 1):
            for A, B in prods:
                acc += A[j] * B[i - j]
            if j < i:
                acc += m[j] * pl[i - j]
        m[i] = ((acc & 0xFFFFFFFF) * ninv) & M29 if limbs_m is None else limbs_m
        acc += m[i] * pl[0]
        top = max(top, acc)
        if limbs_m is None:
            assert acc & M29 == 0
        acc >>= 29
    for i in range(9, 17):
        for j in range(i - 8, 9):
            for A, B in prods:
                acc += A[j] * B[i - j]
            acc += m[j] * pl[i - j]
        top = max(top, acc)
        u[i - 9] = acc & M29
        acc >>= 29
    u[8] = acc
    return sum(x << (29 * k) for k, x in enumerate(u)), top


def pack(q, val):
    """pack(): the 8 x 32 words of a value below 2^256, one conditional subtraction."""
    assert val < RM and val < 2 * q
    return val - q if val >= q else val


def model_pre(q, *ab):
    """Value before the subtraction of REDC(sum of a_i b_i), operands as ints."""
    val, top = redc_cols(q, [(unpack(a, 5), unpack(b, 0)) for a, b in zip(ab[0::2], ab[1::2])])
    assert top < 1 << 64
    return val


def model(opc, a, b):
    """(result coefficients, values before each conditional subtraction of a
    product) of an opcode, following field.h / tower.h step by step."""
    q = modulus(opc)
    if opc in (nt.PROBE_FP_MUL, nt.PROBE_FR_MUL):
        pre = [model_pre(q, a, b)]
        return (pack(q, pre[0]),), pre
    if opc == nt.PROBE_FP_SQR:
        pre = [model_pre(q, a, a)]
        return (pack(q, pre[0]),), pre
    if opc == nt.PROBE_FP2_MUL:
        pre = [model_pre(q, a[0], b[0], a[1], q - b[1]), model_pre(q, a[0], b[1], a[1], b[0])]
        return (pack(q, pre[0]), pack(q, pre[1])), pre
    if opc == nt.PROBE_FP2_SQR:
        pre = [model_pre(q, (a[0] + a[1]) % q, (a[0] - a[1]) % q), model_pre(q, a[0], a[1])]
        return (pack(q, pre[0]), 2 * pack(q, pre[1]) % q), pre
    pre = [model_pre(q, a[0], b), model_pre(q, a[1], b)]
    return (pack(q, pre[0]), pack(q, pre[1])), pre


# ----------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def fixed():
    return {opc: fixed_vectors(opc) for opc in OPS}


@pytest.mark.parametrize("opc", OPS)
def test_fixed_vectors_match_python_integers(opc, fixed):
    vecs = fixed[opc]
    got = probe_ints(opc, vecs)
    q = modulus(opc)
    for (a, b), g in zip(vecs, got):
        assert all(c < q for c in g), (opc, a, b, g)
        assert g == expected(opc, a, b), (opc, a, b)


@pytest.mark.parametrize("opc", OPS)
def test_random_pairs_match_python_integers(opc):
    vecs = random_vectors(opc, N_RANDOM, random.Random(2900 + opc))
    got = probe_ints(opc, vecs)
    want = [expected(opc, a, b) for a, b in vecs]
    assert got == want


@pytest.mark.parametrize("q", [P, R])
def test_model_bounds_at_contract_maximum(q):
    """Every operand limb at the largest value its contract allows (and every
    Montgomery digit at 2^29 - 1): no column reaches 2^64, for one product and
    for a sum of two.  Operands at the largest VALUES the contracts allow: the
    value before the subtraction stays below 2 q."""
    amax = [M29] * 9                      # limbs of a value << 5
    bmax = [M29] * 8 + [(1 << 24) - 1]    # limbs of a value below 2^256
    for prods in ([(amax, bmax)], [(amax, bmax), (amax, bmax)]):
        _, top = redc_cols(q, prods, limbs_m=M29)
        assert top < 1 << 63
    # fmul: a < 2^256, b < q
    assert model_pre(q, RM - 1, q - 1) < 2 * q
    assert model_pre(q, q - 1, q - 1) < 2 * q
    # fmul2: a, b, c, d <= q
    pre = model_pre(q, q, q, q, q)
    assert pre < 2 * q and pre < RM
    assert 5 * pre < 7 * q  # the stated 1.4 q


@pytest.mark.parametrize("opc", OPS)
def test_both_branches_of_the_conditional_subtraction(opc, fixed):
    """The model agrees with the integers on a slice of the fixed vectors and
    on random ones; among them it finds, for each reduction of the opcode, a
    vector at or above the modulus before the subtraction and one below it, and
    the native result is right on exactly those."""
    q = modulus(opc)
    rng = random.Random(2929 + opc)
    vecs = fixed[opc][::7] + random_vectors(opc, 400, rng)
    hi, lo = {}, {}
    for a, b in vecs:
        res, pre = model(opc, a, b)
        assert res == expected(opc, a, b), (opc, a, b)
        for k, v in enumerate(pre):
            (hi if v >= q else lo).setdefault(k, (a, b))
    n_red = len(model(opc, *vecs[0])[1])
    assert sorted(hi) == sorted(lo) == list(range(n_red)), (sorted(hi), sorted(lo))
    picked = list(hi.values()) + list(lo.values())
    assert probe_ints(opc, picked) == [expected(opc, a, b) for a, b in picked]


def test_probe_rejects_an_unknown_opcode():
    a = torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        nt._call("dx_field_probe", 0, None, 99, nt._ptr(a), nt._ptr(a), nt._ptr(torch.empty_like(a)), 1)


def test_operand_set_has_the_listed_values():
    v = fixed_operands(P)
    assert len(v) == 6 + 24 + 14 + 8
    assert np.unique(bn.ints_to_limbs(v), axis=0).shape[0] == len(set(v))
