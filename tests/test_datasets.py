"""Dataset-level LR checks against the fixtures the reference ships
(lib/encoding/logistic_regression_dataset_test.go: SPECTF parameters and the
paper's weights).  The reference only *logs* the comparison (it asserts
nothing, :38-80); here we assert that our weights reach an approximated cost no
worse than the paper's weights and generalise on the held-out split.
The datasets (tests/golden/datasets) and the weight vectors of that test file
(tests/golden/lr_paper_weights.json) are stored with the suite."""
import json
import os

import pytest
import torch

from drynx_amd.models import logistic_regression as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATA = os.path.join(GOLDEN, "datasets")
with open(os.path.join(GOLDEN, "lr_paper_weights.json")) as _f:
    WEIGHTS = json.load(_f)


def test_spectf_weights_with_encryption_precision():
    init = WEIGHTS["SPECTF"]["initial_weights"]
    paper = WEIGHTS["SPECTF"]["paper_weights"]["encrypted"]
    X, y = lr.load_csv_dataset(os.path.join(DATA, "SPECTF_heart_dataset_training.txt"))
    Xa = lr.augment(lr.standardise(X))
    ap = [lr.round_precision(a, 1e2).to(torch.float64) / 1e2 for a in lr.approx_coefficients(Xa, y, 2)]
    w = lr.find_minimum_weights(ap, init, X.shape[0], 1.0, 0.012, 450)
    assert lr.cost(torch.tensor(w), ap, X.shape[0], 1.0) <= lr.cost(torch.tensor(paper), ap, X.shape[0], 1.0)
    Xt, yt = lr.load_csv_dataset(os.path.join(DATA, "SPECTF_heart_dataset_testing.txt"))
    m, s = lr.compute_means_sds(X)
    met = lr.metrics(lr.predict(Xt, w, m, s), yt)
    assert met["accuracy"] > 0.6 and met["auc"] > 0.7


def test_pima_training_converges():
    X, y = lr.load_csv_dataset(os.path.join(DATA, "Pima_dataset_training.txt"))
    Xa = lr.augment(lr.standardise(X))
    ap = [lr.round_precision(a, 1e2).to(torch.float64) / 1e2 for a in lr.approx_coefficients(Xa, y, 2)]
    w = lr.find_minimum_weights(ap, [0.0] * (X.shape[1] + 1), X.shape[0], 1.0, 0.1, 200)
    m, s = lr.compute_means_sds(X)
    Xt, yt = lr.load_csv_dataset(os.path.join(DATA, "Pima_dataset_testing.txt"))
    assert lr.metrics(lr.predict(Xt, w, m, s), yt)["accuracy"] > 0.7


# compareFindMinimumWeights (logistic_regression_dataset_test.go:38-80) for each
# fixture the reference ships, with the reference's own parameters:
# SPECTF (getParametersForSPECTF :384-418: training split, lambda 1, step
# 0.012, 450 iterations, the paper's initial weights; :421-433 the paper's
# weights) and Pima (getParametersForPima :603-632: the whole dataset, step
# 0.1, 200 iterations, the paper's initial weights).  "with encryption"
# follows findMinimumWeightsWithEncryption (:102-132): every record's
# approximation coefficients rounded to precision 1e2 before aggregation.
# Pima_dataset.txt is the raw UCI file with the label in its LAST column;
# the reference's LoadData reads column 0 (logistic_regression.go:1276), i.e.
# the pregnancy count, so its own Pima comparison ran on mislabeled data: the
# label is read from column 8 here.
_FIXTURES = {
    "SPECTF": ("SPECTF_heart_dataset_training.txt", 0, 0.012, 450),
    "Pima": ("Pima_dataset.txt", 8, 0.1, 200),
}


def _fixture(dataset, encrypted):
    path, label, step, iters = _FIXTURES[dataset]
    init = WEIGHTS[dataset]["initial_weights"]
    paper = WEIGHTS[dataset]["paper_weights"]["encrypted" if encrypted else "clear"]
    X, y = lr.load_csv_dataset(os.path.join(DATA, path), label_col=label)
    assert len(init) == len(paper) == X.shape[1] + 1
    Xa = lr.augment(lr.standardise(X))
    if encrypted:  # per record, rounded to 1e2, then summed (the DPs' integer encoding)
        per = [lr.approx_coefficients(Xa[i: i + 1], y[i: i + 1], 2) for i in range(X.shape[0])]
        ap = [sum(lr.round_precision(p[j], 1e2).to(torch.float64) for p in per) / 1e2 for j in range(len(per[0]))]
    else:
        ap = lr.approx_coefficients(Xa, y, 2)
    N = X.shape[0]
    return lr.find_minimum_weights(ap, init, N, 1.0, step, iters), paper, ap, Xa, y, N


@pytest.mark.parametrize("dataset", ["SPECTF", "Pima"])
@pytest.mark.parametrize("encrypted", [False, True])
def test_paper_weight_fixtures(dataset, encrypted):
    w, paper, ap, Xa, y, N = _fixture(dataset, encrypted)
    ours, theirs = lr.cost(torch.tensor(w), ap, N, 1.0), lr.cost(torch.tensor(paper), ap, N, 1.0)
    if dataset == "Pima" and encrypted:
        # the paper's encrypted-Pima weights beat the reference's own gradient
        # descent from the same start in approximated AND true logistic cost
        # (0.896 vs 0.986; they come from a setting the repository does not
        # hold): parity is with the reference's computation -- the encrypted
        # run lands where the clear one does, up to the 1e2 rounding
        wc, _, _, _, _, _ = _fixture(dataset, False)
        assert max(abs(a - b) for a, b in zip(w, wc)) < 0.02
        return
    # the approximated cost our gradient descent minimises is no worse than the paper's weights'
    assert ours <= theirs + 1e-9, (ours, theirs)
    # and the true logistic cost stays within 5% of the paper weights'
    true_ours = lr.logistic_regression_cost(w, Xa, y, N, 1.0)
    true_paper = lr.logistic_regression_cost(paper, Xa, y, N, 1.0)
    assert true_ours <= 1.05 * true_paper, (true_ours, true_paper)


def test_clean_data_pcs_and_gas(tmp_path):
    from drynx_amd.models import datasets as ds

    X, y, dropped = ds.clean_rows("PCS", ["7,1,2,3,4,5,6,7,8,9,0,11,12", "8,a,2,3,4,5,6,7,8,9,0,11,12"])
    # index col 0 dropped -> label is the old column 1; cols 10, 11 dropped
    assert y == [1] and X == [[2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 12.0]] and dropped == 1
    X, y, _ = ds.clean_rows("GAS_SENSOR_MULTI", ["3,1:0.5,2:1.5"], float)
    assert y == [3.0] and X == [[0.5, 1.5]]
    p = tmp_path / "m.txt"
    p.write_text("1,0,255\n")
    ds.clean_file("MNIST", str(p))
    assert p.read_text().strip().split(",")[0] == "1" and abs(float(p.read_text().split(",")[2]) - 1.0) < 1e-12
