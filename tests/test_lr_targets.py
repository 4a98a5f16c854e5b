"""Multi-target logistic regression (LogisticRegressionParameters.NbrTargets =
T): T binary models over the same features in one query.  Level 2's weight
y - y(-1)^2 - 1 = -1 does not depend on the label, so a DP sends T level-1
vectors (target-major) and ONE level 2: T*D + D^2 values (T*D + D(D+1)/2
packed) instead of T*(D + D^2).  Host side: counts, query rules, wire, the
encoding against the single-label one, queries end to end, loaders."""
import pytest
import torch

from drynx_amd import query as Q
from drynx_amd.models import logistic_regression as lr
from drynx_amd.query import LogisticRegressionParameters


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def lr_params(d, n, T=0, packing=0, k=2, init=None, precision=1e1, max_iter=25):
    return LogisticRegressionParameters(NbrRecords=n, NbrFeatures=d, Means=[2.0] * d, StandardDeviations=[1.15] * d,
                                        Lambda=1.0, Step=0.05, MaxIterations=max_iter,
                                        InitialWeights=list(init) if init is not None else [0.1] * (d + 1), K=k,
                                        PrecisionApproxCoefficients=precision, Packing=packing, NbrTargets=T)


def dp_records(rows, d, T, seed=0):
    """Per DP (X float64 [n, d] in [0, 4), Y int64 [n, T] in {0, 1})."""
    return [((torch.rand(n, d, dtype=torch.float64, generator=_gen(seed + i)) * 4),
             torch.randint(0, 2, (n, T), generator=_gen(seed + 100 + i))) for i, n in enumerate(rows)]


def run_query(data, lp, device, workdir, n_vns=0, **survey):
    """One query over len(data) DPs on 3 CNs -> (weights, clear responses per DP, survey, result, client)."""
    from drynx_amd.services.api import DrynxClient
    from drynx_amd.services.local import local_cluster, make_survey

    cl, node = local_cluster(3, len(data), n_vns, device=device, workdir=workdir)
    client = DrynxClient(node, device=device)
    node.dp_data = {dp.id: (X.to(device), y.to(device)) for dp, (X, y) in zip(cl.dps, data)}
    sq = make_survey(client, cl, "logistic regression", lr_params=lp, **survey)
    assert sq.Query.Operation.NbrOutput == lr.n_coeffs(lp.NbrFeatures, lp.K, lp.Packing, lp.NbrTargets)
    _, vals, res = client.send_survey_query(sq)
    clear = [list(v[0]) for v in res.clear_dp.values()]
    out = (list(vals[0]), clear, sq, res, [int(x) for x in client.last_plaintexts[0]])
    node.close(remove=True)
    return out


def check_targets_query(device, tmp_path):
    """T = 3 in one query == three single-label queries on Y[:, t], as floats
    with ==: the integers are the single-label ones by construction and the
    descent of target t runs on [level 1 of t, the shared level 2]."""
    d, T, rows = 6, 3, (60, 57, 63)
    D = d + 1
    data = dp_records(rows, d, T, seed=20)
    n = sum(rows)
    per_target = [0.1 * (t + 1) * (-1) ** j for t in range(T) for j in range(D)]
    for case, init in (("one", [0.1] * D), ("each", per_target)):
        w, clear, _, _, plain = run_query(data, lr_params(d, n, T, init=init), device, str(tmp_path / case))
        assert len(w) == T * D and all(len(v) == T * D + D * D for v in clear)
        tot = [sum(v[i] for v in clear) for i in range(T * D + D * D)]
        assert plain == tot and w == list(lr.decode_logistic_regression_values(tot, lr_params(d, n, T, init=init)))
        exp = []
        for t in range(T):
            init_t = init if len(init) == D else init[t * D:(t + 1) * D]
            wt, clear_t, _, _, _ = run_query([(X, Y[:, t]) for X, Y in data], lr_params(d, n, 0, init=init_t), device,
                                             str(tmp_path / f"{case}{t}"))
            assert len(wt) == D
            for v, vt in zip(clear, clear_t):  # the DPs' integers: level 1 of target t, the shared level 2
                assert v[t * D:(t + 1) * D] == vt[:D] and v[T * D:] == vt[D:]
            exp += wt
        assert w == exp
        assert lr.split_targets(w, T) == [exp[t * D:(t + 1) * D] for t in range(T)]


def check_proofs_query(device, tmp_path, packing):
    """d = 3, T = 2 through every layer with proofs on (3 CNs, 3 VNs, 3 DPs):
    ranges (4, 4, offset 128) as in test_lr_packed's proof case.  |standardised
    feature| <= 2 / 2.5, so |coefficient| <= 6 records * 1 * precision 10 < 128."""
    d, T, rows = 3, 2, (5, 6, 4)
    D = d + 1
    data = dp_records(rows, d, T, seed=40)
    lp = lr_params(d, sum(rows), T, packing=packing)
    lp.StandardDeviations = [2.5] * d
    n_out = T * D + (D * D if packing == 0 else D * (D + 1) // 2)
    w, clear, sq, res, plain = run_query(data, lp, device, str(tmp_path), n_vns=3, proofs=1, ranges=[4, 4, 128],
                                         thresholds=[1.0, 1.0, 1.0, 0.0, 1.0], sig_device=device)
    assert sq.Query.Operation.NbrOutput == n_out == len(sq.Query.Ranges)
    assert len(sq.Query.IVSigs.InputValidationSigs[0]) == n_out
    assert Q.check_parameters(sq, False)
    codes = res.block.data_block().Proofs
    assert set(codes.values()) == {1} and len(codes) == 3 * (3 + 3 + 3)
    assert all(len(v) == n_out and max(abs(x) for x in v) < 128 for v in clear)
    tot = [sum(v[i] for v in clear) for i in range(n_out)]
    assert plain == tot
    assert len(w) == T * D and w == list(lr.decode_logistic_regression_values(tot, lp))


# ----------------------------------------------------------------------------- counts and refusals
def test_counts():
    for f in (Q.lr_nbr_outputs, lr.n_coeffs):
        for d in (1, 5, 44, 100):
            D = d + 1
            for T in (0, 1):  # today's values
                assert f(d, 1, 0, T) == f(d, 1) == D and f(d, 2, 0, T) == f(d, 2) == D + D * D
                assert f(d, 1, 1, T) == f(d, 1, 1) == D and f(d, 2, 1, T) == f(d, 2, 1) == D + D * (D + 1) // 2
                assert f(d, 3, 0, T) == f(d, 3) == D + D ** 2 + D ** 3
            for T in (2, 3, 64):
                assert f(d, 1, 0, T) == f(d, 1, 1, T) == T * D
                assert f(d, 2, 0, T) == f(d, 2, targets=T) == T * D + D * D
                assert f(d, 2, 1, T) == f(d, 2, packing=1, targets=T) == T * D + D * (D + 1) // 2
        assert f(44, 2, 0, 3) == 2160 and 3 * f(44, 2) == 6210  # the headline shape
        for bad in ((3, 3, 0, 2), (3, 2, 0, 65), (3, 2, 0, -1), (3, 2, 2, 2)):
            with pytest.raises(ValueError):
                f(*bad)


def _survey(T, k=2, init_len=None, d=2):
    from drynx_amd.services.api import DrynxClient
    from drynx_amd.services.local import local_cluster, make_survey

    cl, node = local_cluster(2, 2, 0, device="cpu")
    client = DrynxClient(node, device="cpu")
    ok = lr_params(d, 20, 0)
    sq = make_survey(client, cl, "logistic regression", lr_params=ok)  # sized by hand below when refused
    lp = lr_params(d, 20, T, k=k, init=[0.1] * (init_len if init_len is not None else d + 1))
    sq.Query.Operation.LRParameters = lp
    try:
        sq.Query.Operation.NbrOutput = Q.lr_nbr_outputs(d, k, 0, T)
    except ValueError:
        pass
    node.close(remove=True)
    return sq


def test_check_parameters_target_rules():
    for T, k, n_init in ((0, 2, 3), (1, 2, 3), (2, 2, 3), (2, 2, 6), (3, 1, 9), (64, 2, 3), (0, 3, 3), (2, 2, 0)):
        assert Q.check_parameters(_survey(T, k, n_init), False), (T, k, n_init)
    assert not Q.check_parameters(_survey(65), False)
    assert not Q.check_parameters(_survey(-1), False)
    assert not Q.check_parameters(_survey(2, k=3), False)
    assert not Q.check_parameters(_survey(2, init_len=4), False)  # neither 0, D = 3 nor T*D = 6
    assert not Q.check_parameters(_survey(3, init_len=6), False)
    assert not Q.check_parameters(_survey(0, init_len=6), False)


# ----------------------------------------------------------------------------- wire
def test_wire_carries_targets():
    from drynx_amd.wire import messages as M
    from drynx_amd.wire import onet
    from drynx_amd.wire import protobuf as pb

    assert onet.SURVEY_QUERY[-1] == ("LRTargets", "sint")  # appended after every stored field
    assert onet.SURVEY_QUERY[-2] == ("RangeProofMode", "sint")
    assert onet.LR_PARAMETERS == (
        ("DatasetName", "string"), ("FilePath", "string"), ("NbrRecords", "sint"), ("NbrFeatures", "sint"),
        ("Means", ("rep", "double")), ("StandardDeviations", ("rep", "double")), ("Lambda", "double"),
        ("Step", "double"), ("MaxIterations", "sint"), ("InitialWeights", ("rep", "double")), ("K", "sint"),
        ("PrecisionApproxCoefficients", "double"), ("Packing", "sint"))
    sq = _survey(3)
    assert sq.Query.Operation.NbrOutput == 3 * 3 + 9
    back = M.survey_query_from_wire(M.survey_query_to_wire(sq))
    assert back.Query.Operation.LRParameters.NbrTargets == 3
    assert back.Query.Operation.LRParameters == sq.Query.Operation.LRParameters
    assert back.Query.Operation.NbrOutput == 18
    assert M.survey_query_from_wire(M.survey_query_to_wire(_survey(0))).Query.Operation.LRParameters.NbrTargets == 0
    # a sender that does not know the field: the body encoded without it decodes to 0 targets
    msg = M.survey_query_to_msg(sq)
    assert msg["LRTargets"] == 3
    old = onet.message_type_id("libdrynx.SurveyQuery") + pb.encode(onet.SURVEY_QUERY[:-1], msg)
    dec = M.survey_query_from_wire(old)
    assert dec.Query.Operation.LRParameters.NbrTargets == 0 and dec.Query.Operation.LRParameters.NbrFeatures == 2
    assert dec.RangeProofMode == sq.RangeProofMode and dec.SurveyID == sq.SurveyID
    # JSON form
    jd = sq.to_dict()
    assert jd["Query"]["Operation"]["LRParameters"]["NbrTargets"] == 3
    assert Q.SurveyQuery.from_dict(jd).Query.Operation.LRParameters == sq.Query.Operation.LRParameters
    del jd["Query"]["Operation"]["LRParameters"]["NbrTargets"]
    assert Q.SurveyQuery.from_dict(jd).Query.Operation.LRParameters.NbrTargets == 0


# ----------------------------------------------------------------------------- encoding
@pytest.mark.parametrize("packing", [0, 1])
@pytest.mark.parametrize("k", [1, 2])
def test_encoding_is_the_single_label_one_per_target(packing, k):
    d, N, T = 5, 40, 3
    D = d + 1
    X, Y = dp_records((N,), d, T, seed=5)[0]
    vals = lr.encode_coefficients_int(X, Y, lr_params(d, N, T, packing, k, precision=1e2))
    assert vals.dtype == torch.int64 and vals.numel() == lr.n_coeffs(d, k, packing, T)
    for t in range(T):
        one = lr.encode_coefficients_int(X, Y[:, t], lr_params(d, N, 1, packing, k, precision=1e2))
        assert torch.equal(vals[t * D:(t + 1) * D], one[:D])
        assert torch.equal(vals[T * D:], one[D:])
        assert torch.equal(one, lr.encode_coefficients_int(X, Y[:, t:t + 1], lr_params(d, N, 0, packing, k,
                                                                                      precision=1e2)))
    # unpack: the T level-1 vectors and the one level-2 matrix, cartesian in both layouts
    lv = lr.unpack(vals.tolist(), d, k, packing, T)
    assert len(lv) == k and lv[0].shape == (T, D)
    assert lv[0].reshape(-1).tolist() == [float(v) for v in vals[:T * D]]
    if k == 2:
        cart = lr.encode_coefficients_int(X, Y[:, 0], lr_params(d, N, 1, 0, 2, precision=1e2))
        assert lv[1].tolist() == [float(v) for v in cart[D:]]
    with pytest.raises(ValueError):
        lr.encode_coefficients_int(X, Y[:, :2], lr_params(d, N, T, packing, k))  # two columns for three targets
    with pytest.raises(ValueError):
        lr.encode_coefficients_int(X, Y, lr_params(d, N, T, 0, 3))


def test_predict_targets_and_class():
    d, T = 4, 3
    X = torch.rand(30, d, dtype=torch.float64, generator=_gen(1)) * 4
    w = (torch.rand(T * (d + 1), dtype=torch.float64, generator=_gen(2)) - 0.5).tolist()
    parts = lr.split_targets(w, T)
    assert [len(p) for p in parts] == [d + 1] * T and sum(parts, []) == w
    m, s = [2.0] * d, [1.15] * d
    P = lr.predict_targets(X, w, T, m, s)
    assert P.shape == (30, T)
    for t in range(T):
        assert torch.equal(P[:, t], lr.predict(X, parts[t], m, s))
    assert torch.equal(lr.predict_class(X, w, T, m, s), P.argmax(1))
    y = (P >= 0.5).to(torch.int64)
    assert all(lr.metrics(P[:, t], y[:, t])["accuracy"] == 1.0 for t in range(T))
    with pytest.raises(ValueError):
        lr.split_targets(w[:-1], T)


# ----------------------------------------------------------------------------- queries
def test_targets_query_cpu(tmp_path):
    check_targets_query("cpu", tmp_path)


def test_complement_target_negates_the_weights(tmp_path):
    """Y[:, 1] = 1 - Y[:, 0] and zero initial weights: level 1 and the gradient
    are odd in (a0, w), the cost is even and every operation is
    sign-symmetric, so target 1's weights are exactly target 0's negated: an
    exact check that both descents ran on the same level 2."""
    d, rows = 6, (60, 57, 63)
    D = d + 1
    data = [(X, torch.stack([Y[:, 0], 1 - Y[:, 0]], 1)) for X, Y in dp_records(rows, d, 1, seed=30)]
    w, _, _, _, _ = run_query(data, lr_params(d, sum(rows), 2, init=[0.0] * D), "cpu", str(tmp_path))
    assert len(w) == 2 * D and any(v != 0.0 for v in w)
    assert w[D:] == [-v for v in w[:D]]


@pytest.mark.parametrize("packing", [0, 1])
def test_targets_query_with_proofs_cpu(tmp_path, packing):
    check_proofs_query("cpu", tmp_path, packing)


# ----------------------------------------------------------------------------- simul, loaders, generated data
def test_simul_runfile_column(tmp_path, monkeypatch):
    from drynx_amd.parallel.comm import LocalComm
    from drynx_amd.simul import simul

    seen = []
    make = simul.make_survey

    def recording(*a, **kw):
        sq = make(*a, **kw)
        seen.append((sq.Query.Operation.LRParameters.NbrTargets, sq.Query.Operation.NbrOutput))
        return sq

    monkeypatch.setattr(simul, "make_survey", recording)
    row = {"NbrServers": 2, "NbrDPs": 2, "NbrVNs": 0, "Proofs": 0, "OperationName": "logistic regression",
           "NbrRecords": 20, "MaxIterations": 5}
    glob = {"NbrFeatures": 2, "Rounds": 1}
    w3 = simul.run_row(glob, dict(row, LRTargets=3), LocalComm("cpu"), "cpu", str(tmp_path / "a"), netem="off")
    w0 = simul.run_row(glob, dict(row), LocalComm("cpu"), "cpu", str(tmp_path / "b"), netem="off")
    wp = simul.run_row(glob, dict(row, LRTargets=2, LRPacking=1), LocalComm("cpu"), "cpu", str(tmp_path / "c"),
                       netem="off")
    assert seen == [(3, 9 + 9), (0, 12), (2, 6 + 6)]
    assert len(w3[0]) == 9 and len(w0[0]) == 3 and len(wp[0]) == 6


def test_file_loader_with_two_label_columns(tmp_path):
    from drynx_amd.models.datasets import load_dp_file

    rows = [[1, 0, 0.5, 2.0, 3.25], [0, 0, 1.5, 0.0, 1.0], [1, 1, 2.5, 4.0, 0.75]]
    path = str(tmp_path / "dp.txt")
    with open(path, "w") as f:
        for r in rows:
            f.write(",".join(str(v) for v in r) + "\n")
    op = Q.Operation(NameOp="logistic regression", LRParameters=lr_params(3, 3, 2))
    X, Y = load_dp_file(path, op)
    assert X.dtype == torch.float64 and X.tolist() == [r[2:] for r in rows]
    assert Y.dtype == torch.int64 and Y.tolist() == [r[:2] for r in rows]
    X2, Y2 = lr.load_csv_dataset(path, targets=2)
    assert torch.equal(X2, X) and torch.equal(Y2, Y)
    # the same file read by a single-label query: one label, four features
    X1, y1 = load_dp_file(path, Q.Operation(NameOp="logistic regression", LRParameters=lr_params(4, 3, 0)))
    assert X1.shape == (3, 4) and y1.tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        load_dp_file(path, Q.Operation(NameOp="logistic regression", LRParameters=lr_params(4, 3, 2)))


def test_generated_labels():
    from drynx_amd.protocols.data_collection import generate_lr_data

    X3, Y3 = generate_lr_data(lr_params(4, 25, 3), "cpu", _gen(9))
    assert X3.shape == (25, 4) and Y3.shape == (25, 3) and set(Y3.unique().tolist()) <= {0, 1}
    X0, y0 = generate_lr_data(lr_params(4, 25, 0), "cpu", _gen(9))
    X1, y1 = generate_lr_data(lr_params(4, 25, 1), "cpu", _gen(9))
    assert y0.shape == (25,) and torch.equal(y0, y1) and torch.equal(X0, X1) and torch.equal(X0, X3)
    # today's draws: features, then n labels from the same generator
    g = _gen(9)
    Xe = torch.randint(0, 4, (25, 4), generator=g).to(torch.float64)
    assert torch.equal(X0, Xe) and torch.equal(y0, torch.randint(0, 2, (25,), generator=g))
