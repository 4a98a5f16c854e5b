"""Distinct-coefficient packing of logistic-regression queries
(LogisticRegressionParameters.Packing = 1): level 2, the symmetric matrix
sum_i w_i xa_i xa_i^T, travels as its row-major upper triangle -- D(D+1)/2
values instead of D^2 (D = d + 1).  The packed values are the cartesian values
at (i, j), i <= j; the querier mirrors them and runs the same descent.  Host
side of the extension: counts, layout, query rules, wire, one query end to end."""
import pytest
import torch

import test_lr_highdim as hd
from drynx_amd import query as Q
from drynx_amd.models import logistic_regression as lr
from drynx_amd.query import LogisticRegressionParameters


def packed_params(lp: LogisticRegressionParameters, packing: int = 1) -> LogisticRegressionParameters:
    out = LogisticRegressionParameters(**lp.__dict__)
    out.Packing = packing
    return out


def upper_gather(cart: torch.Tensor, d: int) -> torch.Tensor:
    """Level 1, then level 2's entries (i, j), i <= j, row by row, from a cartesian vector."""
    D = d + 1
    A2 = cart[D:].reshape(D, D)
    return torch.cat([cart[:D]] + [A2[i, i:] for i in range(D)])


def run_packed_query(dataset: str, device, workdir: str, packing: int = 1, precision: float = 1e0):
    """``test_lr_highdim.run_query`` (3 CNs / 3 DPs, proofs off) with a chosen
    layout -> (weights, clear responses per DP, parameters)."""
    from drynx_amd.services.api import DrynxClient
    from drynx_amd.services.local import local_cluster, make_survey

    X, y = hd.load(dataset, "training")
    lp = packed_params(hd.lr_parameters(dataset, X, precision), packing)
    cl, node = local_cluster(3, hd.N_DPS, 0, device=device, workdir=workdir)
    client = DrynxClient(node, device=device)
    node.dp_data = {dp.id: (Xi.to(device), yi.to(device)) for dp, (Xi, yi) in zip(cl.dps, hd.dp_splits(X, y))}
    sq = make_survey(client, cl, "logistic regression", lr_params=lp)
    assert sq.Query.Operation.NbrOutput == lr.n_coeffs(lp.NbrFeatures, lp.K, packing)
    _, vals, res = client.send_survey_query(sq)
    clear = [list(v[0]) for v in res.clear_dp.values()]
    node.close(remove=True)
    return list(vals[0]), clear, lp


def test_counts():
    for f in (Q.lr_nbr_outputs, lr.n_coeffs):
        assert f(44, 2, 1) == 1080 and f(44, 2, packing=1) == 1080
        assert f(100, 2, 1) == 5252
        assert f(44, 1, 1) == 45 and f(100, 1, 1) == 101  # K = 1: the same vector as today
        assert f(5, 2, 1) == 27
        assert f(44, 2) == f(44, 2, 0) == 2070 and f(100, 2) == 10302 and f(3, 3) == 4 + 16 + 64
        with pytest.raises(ValueError):
            f(3, 3, 1)
        with pytest.raises(ValueError):
            f(3, 2, 2)


@pytest.mark.parametrize("d", [1, 4, 44])
def test_pack_unpack_round_trip(d):
    D = d + 1
    g = torch.Generator().manual_seed(d)
    lvl1 = torch.randint(-1000, 1000, (D,), generator=g)
    A = torch.randint(-10 ** 6, 10 ** 6, (D, D), generator=g)
    A2 = torch.triu(A) + torch.triu(A, 1).T
    assert torch.equal(A2, A2.T)
    cart = torch.cat([lvl1, A2.reshape(-1)])
    packed = lr.pack(cart, d, 2)
    assert packed.numel() == lr.n_coeffs(d, 2, 1) and torch.equal(packed, upper_gather(cart, d))
    assert lr.pack(cart.tolist(), d, 2) == packed.tolist()
    for (i, j) in ((0, 0), (0, d), (1, 1), (d, d)):
        e = lr.packed_index(i, j, D)
        assert e == i * D - i * (i - 1) // 2 + (j - i)
        assert int(packed[D + e]) == int(A2[i, j])
    assert lr.packed_index(0, 0, D) == 0 and lr.packed_index(0, d, D) == d
    assert lr.packed_index(1, 1, D) == D and lr.packed_index(d, d, D) == D * (D + 1) // 2 - 1
    back = lr.unpack(packed.tolist(), d, 2, 1)
    ref = lr.unpack(cart.tolist(), d, 2)
    assert len(back) == 2 and all(torch.equal(a, b) for a, b in zip(back, ref))
    # K = 1: one level, the same vector in both layouts
    assert lr.pack(lvl1.tolist(), d, 1) == lvl1.tolist()
    assert torch.equal(lr.unpack(lvl1.tolist(), d, 1, 1)[0], lr.unpack(lvl1.tolist(), d, 1)[0])
    with pytest.raises(ValueError):
        lr.unpack(packed.tolist(), d, 2, 2)


@pytest.mark.parametrize("dataset", hd.DATASETS)
@pytest.mark.parametrize("precision", [1e0, 1e2])
def test_layout_agreement_fixtures(dataset, precision):
    """Packing = 1 == the upper-triangle gather of the Packing = 0 vector, for
    every DP split (these inputs sit at least 5.8e-6 from a rounding boundary,
    tests/test_lr_highdim_gpu.py)."""
    X, y = hd.load(dataset, "training")
    lp0 = hd.lr_parameters(dataset, X, precision)
    lp1 = packed_params(lp0)
    for Xi, yi in hd.dp_splits(X, y):
        cart = lr.encode_coefficients_int(Xi, yi, lp0)
        packed = lr.encode_coefficients_int(Xi, yi, lp1)
        assert cart.numel() == 10302 and packed.numel() == 5252 and packed.dtype == torch.int64
        assert torch.equal(packed, upper_gather(cart, 100))


def test_layout_agreement_k1():
    X, y = hd.load("BC", "training")
    lp0 = hd.lr_parameters("BC", X, 1e2)
    lp0.K = 1
    assert torch.equal(lr.encode_coefficients_int(X, y, packed_params(lp0)), lr.encode_coefficients_int(X, y, lp0))


def test_slab_rule_is_the_two_drivers_rules():
    """``native._lr_slab_uninit`` against the two expressions it replaced (the
    batch driver's and the grouped driver's, copied here as they stood), on the
    (upper plan, packed reader) combinations each driver reaches; a slab with
    an unwritten record block is never left uninitialised."""
    from drynx_amd import native as nt

    for D in range(2, 121):
        for T in (1, 2, 5, 64):
            P = nt._lr_padded(D + T)
            for upper in (False, True):  # the batch driver: the upper plan goes with the packed reader
                assert nt._lr_slab_uninit(D, T, upper, upper, True) == \
                    (upper or P == 48 or (D + 15) // 16 == P // 16), (D, T, upper)
            for upper, packed in ((False, False), (True, True), (True, False)):  # the grouped driver
                assert nt._lr_slab_uninit(D, T, upper, packed, True) == \
                    ((upper and packed) or P == 48 or ((D + 15) // 16 == P // 16 and not upper)), (D, T, upper, packed)
            for upper in (False, True):
                for packed in (False, True):
                    assert nt._lr_slab_uninit(D, T, upper, packed, False) is False


def test_packed_query_cpu(tmp_path):
    w, clear, lp = run_packed_query("BC", "cpu", str(tmp_path / "p1"))
    assert len(clear) == hd.N_DPS and all(len(v) == 5252 for v in clear)
    tot = [sum(v[i] for v in clear) for i in range(5252)]
    assert len(w) == 101 and w == list(lr.decode_logistic_regression_values(tot, lp))
    w0, clear0, _ = run_packed_query("BC", "cpu", str(tmp_path / "p0"), packing=0)
    assert all(len(v) == 10302 for v in clear0)
    assert w == pytest.approx(w0, rel=1e-9, abs=1e-12)
    hd.check_metrics("BC", w, lp)


def _lr_survey(packing: int, k: int = 2, proofs: int = 0, n_ranges=None):
    from drynx_amd.services.api import DrynxClient
    from drynx_amd.services.local import local_cluster, make_survey

    d = 2
    cl, node = local_cluster(2, 2, 1, device="cpu")
    client = DrynxClient(node, device="cpu")
    lp = LogisticRegressionParameters(NbrRecords=20, NbrFeatures=d, Means=[0.5] * d, StandardDeviations=[1.1] * d,
                                      Lambda=1.0, Step=0.1, MaxIterations=5, InitialWeights=[0.1] * (d + 1), K=k,
                                      PrecisionApproxCoefficients=1e1, Packing=packing)
    if packing in (0, 1) and k <= 2:
        n_out = Q.lr_nbr_outputs(d, k, packing)
    else:  # make_survey sizes the query from the parameters: size a refused one by hand
        lp_ok = LogisticRegressionParameters(**{**lp.__dict__, "Packing": 0})
        n_out = Q.lr_nbr_outputs(d, k, 0)
    ranges = None
    if proofs:
        ranges = [[4, 4, 128]] * (n_ranges if n_ranges is not None else n_out)
    if packing in (0, 1) and k <= 2:
        sq = make_survey(client, cl, "logistic regression", lr_params=lp, proofs=proofs, ranges=ranges)
    else:
        sq = make_survey(client, cl, "logistic regression", lr_params=lp_ok, proofs=proofs, ranges=ranges)
        sq.Query.Operation.LRParameters = lp
    node.close(remove=True)
    return sq


def test_check_parameters_packing_rules():
    for packing, k in ((0, 2), (1, 2), (1, 1), (0, 3)):
        assert Q.check_parameters(_lr_survey(packing, k), False), (packing, k)
    assert not Q.check_parameters(_lr_survey(2), False)
    assert not Q.check_parameters(_lr_survey(-1), False)
    assert not Q.check_parameters(_lr_survey(1, 3), False)


def test_proofs_need_packed_range_count():
    """With proofs on, NbrOutput (packed: 3 + 6 = 9 at d = 2) must match
    len(Ranges) and the signatures per CN, as for every query."""
    ok = _lr_survey(1, proofs=1)
    assert ok.Query.Operation.NbrOutput == 9 and len(ok.Query.Ranges) == 9
    assert len(ok.Query.IVSigs.InputValidationSigs[0]) == 9
    assert Q.check_parameters(ok, False)
    assert Q.query_to_proofs_nbrs(ok) == Q.query_to_proofs_nbrs(_lr_survey(0, proofs=1))
    bad = _lr_survey(1, proofs=1, n_ranges=12)  # the cartesian count
    assert bad.Query.Operation.NbrOutput == 9 and len(bad.Query.Ranges) == 12
    assert not Q.check_parameters(bad, False)


def test_wire_carries_packing():
    from drynx_amd.wire import messages as M
    from drynx_amd.wire import onet
    from drynx_amd.wire import protobuf as pb

    assert onet.LR_PARAMETERS[-1] == ("Packing", "sint")  # appended after the reference's fields
    sq = _lr_survey(1)
    back = M.survey_query_from_wire(M.survey_query_to_wire(sq))
    assert back.Query.Operation.LRParameters.Packing == 1
    assert back.Query.Operation.LRParameters == sq.Query.Operation.LRParameters
    assert back.Query.Operation.NbrOutput == 9
    assert M.survey_query_from_wire(M.survey_query_to_wire(_lr_survey(0))).Query.Operation.LRParameters.Packing == 0
    # a sender that does not know the field: the body encoded with the reference's schema decodes to 0
    body = {k: v for k, v in sq.Query.Operation.LRParameters.__dict__.items() if k != "Packing"}
    old = pb.encode(onet.LR_PARAMETERS[:-1], body)
    dec = pb.decode(onet.LR_PARAMETERS, old)
    assert dec["Packing"] == 0 and dec["K"] == 2 and dec["NbrFeatures"] == 2
    assert LogisticRegressionParameters(**dec).Packing == 0
    # JSON form of a survey written before the extension
    dd = sq.to_dict()
    del dd["Query"]["Operation"]["LRParameters"]["Packing"]
    assert Q.SurveyQuery.from_dict(dd).Query.Operation.LRParameters.Packing == 0
    assert Q.SurveyQuery.from_dict(sq.to_dict()).Query.Operation.LRParameters.Packing == 1


def test_simul_runfile_column(tmp_path, monkeypatch):
    """The optional runfile column LRPacking reaches the query: 3 + 6 outputs
    at 2 features (the DPs' records are seeded by the survey id, so the two
    runs' weights are not comparable)."""
    from drynx_amd.parallel.comm import LocalComm
    from drynx_amd.simul import simul

    seen = []
    make = simul.make_survey

    def recording(*a, **kw):
        sq = make(*a, **kw)
        seen.append((sq.Query.Operation.LRParameters.Packing, sq.Query.Operation.NbrOutput))
        return sq

    monkeypatch.setattr(simul, "make_survey", recording)
    row = {"NbrServers": 2, "NbrDPs": 2, "NbrVNs": 0, "Proofs": 0, "OperationName": "logistic regression",
           "NbrRecords": 20, "MaxIterations": 5}
    glob = {"NbrFeatures": 2, "Rounds": 1}
    w1 = simul.run_row(glob, dict(row, LRPacking=1), LocalComm("cpu"), "cpu", str(tmp_path / "a"), netem="off")
    w0 = simul.run_row(glob, dict(row), LocalComm("cpu"), "cpu", str(tmp_path / "b"), netem="off")
    assert seen == [(1, 9), (0, 12)]
    assert len(w1[0]) == 3 and len(w0[0]) == 3


def test_find_minimum_weights_with_encryption_packed():
    from drynx_amd.crypto import elgamal as eg

    d, n = 3, 45
    g = torch.Generator().manual_seed(3)
    X = torch.rand(n, d, dtype=torch.float64, generator=g) * 4
    y = torch.randint(0, 2, (n,), generator=g)
    p = LogisticRegressionParameters(NbrRecords=n, NbrFeatures=d, Lambda=1.0, Step=0.1, MaxIterations=50,
                                     InitialWeights=[0.1] * (d + 1), K=2, PrecisionApproxCoefficients=100.0,
                                     Means=[2.0] * d, StandardDeviations=[1.1] * d, Packing=1)
    vals = lr.encode_coefficients_int(X, y, p)
    assert vals.numel() == 4 + 10
    kp = eg.KeyPair.generate()
    pk = eg.pk_table(kp.public)
    enc = [eg.encrypt_ints(pk, vals[:4])[0], eg.encrypt_ints(pk, vals[4:])[0]]
    w, approx = lr.find_minimum_weights_with_encryption(enc, kp.secret, p.InitialWeights, n, 1.0, 0.1, 50, 100.0,
                                                        packing=1)
    assert w == lr.decode_logistic_regression_values(vals.tolist(), p)
    assert len(approx[1]) == 16
