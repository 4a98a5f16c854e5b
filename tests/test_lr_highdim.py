"""Logistic regression on the reference's 100-feature datasets (BC, GSE).

Reference: services/service_test.go:1460-1923 runs both end to end on 3 CNs
and 3 DPs with proofs off: K = 2, lambda 1, the training file's means and
standard deviations, initial weights from a previous run, and
PrecisionApproxCoefficients 1e0.  101 + 101^2 = 10,302 encrypted outputs per DP.
The reference only logs the metrics; here the weights are pinned to the
clear-text descent on the clear aggregate and the held-out metrics to bounds.
The datasets (tests/golden/datasets/*.npy: what np.loadtxt reads from the
reference's text files, label in column 0) and the initial weights
(tests/golden/lr_highdim_weights.json) are stored with the suite."""
import json
import os

import numpy as np
import pytest
import torch

from drynx_amd.models import logistic_regression as lr
from drynx_amd.query import LogisticRegressionParameters

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "lr_highdim_weights.json")) as _f:
    PARAMS = json.load(_f)
DATASETS = ["BC", "GSE"]
N_DPS = 3
# held-out bounds: measured on the host path BC accuracy 1.0 / AUC 1.0, GSE accuracy 38/47 = 0.809 / AUC 0.936
BOUNDS = {"BC": {"accuracy": 0.95}, "GSE": {"accuracy": 0.80, "auc": 0.93}}


def load(dataset: str, split: str):
    """(X [n, 100] float64, y [n] int64) of a fixture."""
    data = np.load(os.path.join(GOLDEN, "datasets", f"{dataset}_dataset_{split}.npy"))
    assert data.dtype == np.float64 and data.shape[1] == 101
    return torch.tensor(data[:, 1:]), torch.tensor(data[:, 0]).to(torch.int64)


def lr_parameters(dataset: str, X: torch.Tensor, precision: float) -> LogisticRegressionParameters:
    p = PARAMS[dataset]
    m, s = lr.compute_means_sds(X)
    assert len(p["initial_weights"]) == X.shape[1] + 1
    return LogisticRegressionParameters(NbrRecords=X.shape[0], NbrFeatures=X.shape[1], Means=m.tolist(),
                                        StandardDeviations=s.tolist(), Lambda=p["lambda"], Step=p["step"],
                                        MaxIterations=p["max_iterations"], InitialWeights=p["initial_weights"], K=2,
                                        PrecisionApproxCoefficients=precision)


def dp_splits(X: torch.Tensor, y: torch.Tensor) -> list:
    return [lr.partition_for_dp(X, y, i, N_DPS) for i in range(N_DPS)]


def run_query(dataset: str, device, workdir: str, precision: float = 1e0):
    """The reference's query on 3 CNs / 3 DPs, proofs off, the DPs' records on
    ``device`` -> (weights, clear-text descent on the clear aggregate, parameters)."""
    from drynx_amd.services.api import DrynxClient
    from drynx_amd.services.local import local_cluster, make_survey

    X, y = load(dataset, "training")
    lp = lr_parameters(dataset, X, precision)
    cl, node = local_cluster(3, N_DPS, 0, device=device, workdir=workdir)
    client = DrynxClient(node, device=device)
    node.dp_data = {dp.id: (Xi.to(device), yi.to(device)) for dp, (Xi, yi) in zip(cl.dps, dp_splits(X, y))}
    sq = make_survey(client, cl, "logistic regression", lr_params=lp)
    _, vals, res = client.send_survey_query(sq)
    n = lr.n_coeffs(lp.NbrFeatures, lp.K)
    assert n == 10302 and len(res.clear_dp) == N_DPS
    assert all(len(v[0]) == n for v in res.clear_dp.values())
    tot = [sum(v[0][i] for v in res.clear_dp.values()) for i in range(n)]
    exp = lr.decode_logistic_regression_values(tot, lp)
    node.close(remove=True)
    return list(vals[0]), list(exp), lp


def check_metrics(dataset: str, weights, lp) -> None:
    Xt, yt = load(dataset, "testing")
    met = lr.metrics(lr.predict(Xt, weights, lp.Means, lp.StandardDeviations), yt)
    for k, bound in BOUNDS[dataset].items():
        assert met[k] >= bound, (dataset, met)


def test_fixture_shapes():
    for ds, n_train, n_test in (("BC", 211, 29), ("GSE", 180, 47)):
        X, y = load(ds, "training")
        assert X.shape == (n_train, 100) and set(y.tolist()) == {0, 1}
        assert load(ds, "testing")[0].shape == (n_test, 100)
        assert sum(len(Xi) for Xi, _ in dp_splits(X, y)) == n_train


@pytest.mark.parametrize("dataset", DATASETS)
def test_highdim_query_cpu(dataset, tmp_path):
    w, exp, lp = run_query(dataset, "cpu", str(tmp_path))
    assert len(w) == 101
    assert w == exp
    check_metrics(dataset, w, lp)
