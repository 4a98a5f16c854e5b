"""K14d (csrc/kernels/dx_group_moments.hip) through ``native.group_moments`` on
the host path: filtered, grouped exact int64 moments against a pure-Python
model (Python ints reduced mod 2^64), against ``native.int_moments`` over the
rows selected in torch, and the binding's argument checks and window loop.

Shapes: DPs of 0, 1, 64, 65 and 200 rows in one batch (330 rows: the plan's
chunk is 64, so the 200-row DP spans 4 tiles and the 65-row DP has a ragged
second tile), 3 value columns, (3, 2) groups with the key values -1 and V_i
present.  The ``check_*`` functions take the device and return their outputs:
tests/test_group_moments_gpu.py runs them on the GPU and compares the outputs
with the host's bit for bit."""
import numpy as np
import pytest
import torch

from drynx_amd import native as nt
from drynx_amd.ops.encoding import moment_pairs

ROWS = [0, 1, 64, 65, 200]
N = sum(ROWS)
M64 = 1 << 64
KEYS = [(0, 0, 3), (1, 0, 2)]  # K columns 0 and 1: 3 x 2 groups


def _signed(v: int) -> int:
    v %= M64
    return v - M64 if v >= 1 << 63 else v


def model(Z, K, rows, pairs, keys, filters):
    """out[dp][g][p] with Python ints, record by record."""
    z, k = Z.tolist(), (K.tolist() if K is not None else [[]] * Z.shape[0])
    G = int(np.prod([c for _, _, c in keys])) if keys else 1
    out = [[[0] * len(pairs) for _ in range(G)] for _ in rows]
    i = 0
    for dp, cnt in enumerate(rows):
        for _ in range(cnt):
            zi, ki = z[i] + [1], k[i]
            i += 1
            if any(ki[c] != v for c, v in filters):
                continue
            g = 0
            for c, off, card in keys:
                d = ki[c] - off
                if not 0 <= d < card:
                    g = -1
                    break
                g = g * card + d
            if g < 0:
                continue
            for p, (a, b) in enumerate(pairs):
                out[dp][g][p] += zi[a] * zi[b]
    return torch.tensor([[[_signed(v) for v in grp] for grp in dp] for dp in out], dtype=torch.int64).reshape(
        len(rows), G, len(pairs))


def _tables(seed=7, lo=-9, hi=9):
    g = torch.Generator().manual_seed(seed)
    Z = torch.randint(lo, hi + 1, (N, 3), generator=g, dtype=torch.int64)
    # key columns over (3, 2) groups with -1 and V_i present, a filter column in [0, 2], a counted column
    K = torch.stack([torch.randint(-1, 4, (N,), generator=g), torch.randint(-1, 3, (N,), generator=g),
                     torch.randint(0, 3, (N,), generator=g), torch.randint(-2, 9, (N,), generator=g)], dim=1)
    assert (K[:, 0] == -1).any() and (K[:, 0] == 3).any() and (K[:, 1] == -1).any() and (K[:, 1] == 2).any()
    return Z, K


def _selected(Z, K, rows, pairs, keys, filters, device):
    """Every group's slice from ``int_moments`` over the rows selected in torch."""
    keep = torch.ones(Z.shape[0], dtype=torch.bool)
    for c, v in filters:
        keep &= K[:, c] == v
    key = torch.zeros(Z.shape[0], dtype=torch.int64)
    G = 1
    for c, off, card in keys:
        d = K[:, c] - off
        keep &= (d >= 0) & (d < card)
        key = key * card + d
        G *= card
    seg = torch.repeat_interleave(torch.arange(len(rows)), torch.tensor(rows))
    out = []
    for g in range(G):
        m = keep & (key == g)
        counts = torch.bincount(seg[m], minlength=len(rows)).tolist()
        out.append(nt.int_moments(Z[m].contiguous().to(device), counts, pairs).cpu())
    return torch.stack(out, dim=1)


def check_small(device):
    """cosim and lin_reg (d = 2) pairs x 0, 1, 2 filter terms (one that no row
    passes) over (3, 2) groups; all rows in one group; no keys at all."""
    Z, K = _tables()
    outs = []
    for pairs in (moment_pairs("cosim", 3), moment_pairs("lin_reg", 3)):
        for filters in ([], [(2, 1)], [(2, 1), (3, 4)], [(2, 7)]):
            got = nt.group_moments(Z.to(device), K.to(device), ROWS, pairs, KEYS, filters).cpu()
            assert got.shape == (len(ROWS), 6, len(pairs))
            assert torch.equal(got, model(Z, K, ROWS, pairs, KEYS, filters))
            assert torch.equal(got, _selected(Z, K, ROWS, pairs, KEYS, filters, device))
            if filters == [(2, 7)]:
                assert not got.any()
            outs.append(got)
    pairs = moment_pairs("cosim", 3)
    # in-range keys, no filter: the groups partition every DP
    Kin = torch.stack([K[:, 0].clamp(0, 2), K[:, 1].clamp(0, 1)], dim=1)
    got = nt.group_moments(Z.to(device), Kin.to(device), ROWS, pairs, KEYS, []).cpu()
    assert torch.equal(got, model(Z, Kin, ROWS, pairs, KEYS, []))
    assert torch.equal(got.sum(1), nt.int_moments(Z.to(device), ROWS, pairs).cpu())
    outs.append(got)
    # all rows in one group: every lane adds to the same cell
    Kone = torch.tensor([[2, 1]]).expand(N, 2).contiguous()
    got = nt.group_moments(Z.to(device), Kone.to(device), ROWS, pairs, KEYS, []).cpu()
    whole = nt.int_moments(Z.to(device), ROWS, pairs).cpu()
    assert torch.equal(got[:, 5], whole) and not got[:, :5].any()
    outs.append(got)
    # no key and no filter: one group, int_moments itself; K as a strided view of a wider table
    got = nt.group_moments(Z.to(device), None, ROWS, pairs).cpu()
    assert got.shape == (len(ROWS), 1, len(pairs)) and torch.equal(got[:, 0], whole)
    outs.append(got)
    wide = torch.cat([K, K], dim=1).to(device)
    view = wide[:, 4:]
    assert view.stride(0) == 8
    got = nt.group_moments(Z.to(device), view, ROWS, pairs, KEYS, [(2, 1)]).cpu()
    assert torch.equal(got, outs[1])
    outs.append(got)
    return outs


def check_wrap(device):
    """Magnitudes near 2^31 (products near 2^62) and near 2^62 (products wrap), both signs."""
    outs = []
    _, K = _tables()
    g = torch.Generator().manual_seed(11)
    for bits in (31, 62):
        Z = torch.randint((1 << bits) - 1000, (1 << bits) + 1000, (N, 3), generator=g, dtype=torch.int64)
        Z = Z * (torch.randint(0, 2, (N, 3), generator=g) * 2 - 1)
        for pairs in (moment_pairs("cosim", 3), moment_pairs("lin_reg", 3)):
            got = nt.group_moments(Z.to(device), K.to(device), ROWS, pairs, KEYS, [(2, 1)]).cpu()
            assert torch.equal(got, model(Z, K, ROWS, pairs, KEYS, [(2, 1)]))
            assert torch.equal(got, _selected(Z, K, ROWS, pairs, KEYS, [(2, 1)], device))
            outs.append(got)
    return outs


def over_cap_groups(P: int) -> int:
    """One group more than a launch's cells hold for P pairs."""
    return nt.GROUP_MOMENTS_MAX_CELLS // P + 1


def check_windows(device):
    """Cells exceed GROUP_MOMENTS_MAX_CELLS by one group: two windows."""
    pairs = moment_pairs("cosim", 3)
    G = over_cap_groups(len(pairs))
    assert (G - 1) * len(pairs) <= nt.GROUP_MOMENTS_MAX_CELLS < G * len(pairs)
    Z, _ = _tables()
    g = torch.Generator().manual_seed(13)
    K = torch.randint(0, G, (N, 1), generator=g, dtype=torch.int64)
    K[-3:, 0] = G - 1  # the one group of the second window is populated
    K[5, 0] = G        # and one row is out of range
    keys = [(0, 0, G)]
    got = nt.group_moments(Z.to(device), K.to(device), ROWS, pairs, keys, []).cpu()
    assert got.shape == (len(ROWS), G, len(pairs)) and got[:, G - 1].any()
    assert torch.equal(got, model(Z, K, ROWS, pairs, keys, []))
    return [got]


def check_wide(device):
    """lin_reg over 64 columns (d = 63, 2144 pairs): a window is 2 groups, 3
    groups take two launches, and a workgroup's LDS passes 64 KiB."""
    g = torch.Generator().manual_seed(19)
    Z = torch.randint(-(1 << 20), 1 << 20, (N, 64), generator=g, dtype=torch.int64)
    K = torch.randint(-1, 4, (N, 1), generator=g, dtype=torch.int64)
    pairs = moment_pairs("lin_reg", 64)
    assert len(pairs) == 2144 and nt.GROUP_MOMENTS_MAX_CELLS // len(pairs) == 2
    keys = [(0, 0, 3)]
    got = nt.group_moments(Z.to(device), K.to(device), ROWS, pairs, keys, []).cpu()
    assert torch.equal(got, model(Z, K, ROWS, pairs, keys, []))
    return [got]


def check_counts(device):
    """frequencyCount through the extra innermost key: 7 bins x 6 groups,
    records outside the domain [0, 6] (-2, -1, 7, 8) dropped."""
    Z, K = _tables()
    assert (K[:, 3] < 0).any() and (K[:, 3] > 6).any()
    outs = []
    for filters in ([], [(2, 1)]):
        got = nt.group_moments(Z[:, :0].to(device), K.to(device), ROWS, [(0, 0)], KEYS, filters, bins=(3, 0, 7)).cpu()
        assert got.shape == (len(ROWS), 42, 1)
        assert torch.equal(got, model(Z[:, :0], K, ROWS, [(0, 0)], KEYS + [(3, 0, 7)], filters))
        keep = ((K[:, 0] >= 0) & (K[:, 0] < 3) & (K[:, 1] >= 0) & (K[:, 1] < 2) & (K[:, 3] >= 0) & (K[:, 3] < 7))
        for c, v in filters:
            keep &= K[:, c] == v
        assert int(got.sum()) == int(keep.sum())
        outs.append(got)
    return outs


def check_large(device):
    """One more DP of 70,000 rows: uniform keys, then all in one group."""
    rows = ROWS + [70000]
    n = sum(rows)
    g = torch.Generator().manual_seed(17)
    Z = torch.randint(-(1 << 40), 1 << 40, (n, 3), generator=g, dtype=torch.int64)
    K = torch.stack([torch.randint(0, 3, (n,), generator=g), torch.randint(0, 2, (n,), generator=g),
                     torch.randint(0, 2, (n,), generator=g)], dim=1)
    pairs = moment_pairs("cosim", 3)
    outs = []
    for Kc in (K, torch.tensor([[1, 1, 1]]).expand(n, 3).contiguous()):
        for filters in ([], [(2, 1)]):
            got = nt.group_moments(Z.to(device), Kc.to(device), rows, pairs, KEYS, filters).cpu()
            assert torch.equal(got, _selected(Z, Kc, rows, pairs, KEYS, filters, device))
            outs.append(got)
    assert torch.equal(outs[0].sum(1), nt.int_moments(Z.to(device), rows, pairs).cpu())
    return outs


# ----------------------------------------------------------------------------- the host path
def test_max_cells_is_the_kernels():
    assert nt.lib().dx_group_moments_max_cells() == nt.GROUP_MOMENTS_MAX_CELLS
    # half of a CU's 160 KiB of LDS holds the cells and the widest staging area: two workgroups stay resident
    assert nt.GROUP_MOMENTS_MAX_CELLS * 8 + 64 * 66 * 8 + 64 * 4 <= 80 * 1024
    assert nt.GROUP_MOMENTS_MAX_CELLS >= 2145  # one group of lin_reg at 64 columns


def test_small_shapes_host():
    assert len(check_small("cpu")) == 12


def test_products_wrap_host():
    assert len(check_wrap("cpu")) == 4


def test_wide_pair_list_host():
    assert len(check_wide("cpu")) == 1


def test_counts_host():
    assert len(check_counts("cpu")) == 2


def test_window_loop_runs_twice(monkeypatch):
    calls = []
    raw = nt._raw_call

    def spy(name, *args):
        if name == "dx_group_moments":
            calls.append((args[-3], args[-2], args[11]))  # g0, gw, P
        return raw(name, *args)

    monkeypatch.setattr(nt, "_raw_call", spy)
    check_windows("cpu")
    P = 5
    G = over_cap_groups(P)
    assert calls == [(0, G - 1, P), (G - 1, 1, P)]
    assert all(gw * p <= nt.GROUP_MOMENTS_MAX_CELLS for _, gw, p in calls)


def test_entry_refuses_a_window_above_the_cap():
    """The C entry itself returns an error code for cells above the cap (and
    for the other limits) instead of running."""
    P = 5
    G = over_cap_groups(P)
    Z = torch.zeros((4, 3), dtype=torch.int64)
    K = torch.zeros((4, 1), dtype=torch.int64)
    tiles = torch.tensor([[0, 0, 4]], dtype=torch.int64)
    pairs = torch.tensor(moment_pairs("cosim", 3), dtype=torch.int16)
    out = torch.zeros((1, G, P), dtype=torch.int64)

    def entry(keys, filters, g0, gw, ck=1):
        kd, fd = np.asarray(keys, dtype=np.int64).reshape(-1), np.asarray(filters, dtype=np.int64).reshape(-1)
        return nt._raw_call("dx_group_moments", 0, None, nt._ptr(Z), 3, 3, nt._ptr(K), 1, ck, nt._ptr(tiles), 1,
                            nt._ptr(pairs), P, kd.ctypes.data_as(nt._P), len(keys), fd.ctypes.data_as(nt._P),
                            len(filters), g0, gw, nt._ptr(out))

    assert entry([(0, 0, G)], [], 0, G - 1) == 0
    assert entry([(0, 0, G)], [], 0, G) == -2            # cells above the cap
    assert entry([(0, 0, G)], [], G - 1, 2) == -2        # window past the last group
    assert entry([(0, 0, 0)], [], 0, 1) == -2            # cardinality 0
    assert entry([(1, 0, 2)], [], 0, 1) == -2            # key column >= width
    assert entry([], [(1, 0)], 0, 1) == -2               # filter column >= width
    assert entry([(0, 0, 1)] * 6, [], 0, 1) == -2        # too many key columns
    assert entry([], [(0, 0)] * 9, 0, 1) == -2           # too many filters
    assert not out.any()  # (zeros in, zeros out)


def test_invalid_arguments_raise():
    Z, K = _tables()
    pairs = moment_pairs("cosim", 3)
    with pytest.raises(ValueError, match="key columns"):
        nt.group_moments(Z, K, ROWS, pairs, [(0, 0, 1)] * 5, [])
    with pytest.raises(ValueError, match="filter terms"):
        nt.group_moments(Z, K, ROWS, pairs, KEYS, [(2, 1)] * 9)
    with pytest.raises(ValueError, match="cardinality"):
        nt.group_moments(Z, K, ROWS, pairs, [(0, 0, 0)], [])
    with pytest.raises(ValueError, match="column 4"):
        nt.group_moments(Z, K, ROWS, pairs, [(4, 0, 2)], [])
    with pytest.raises(ValueError, match="column 4"):
        nt.group_moments(Z, K, ROWS, pairs, KEYS, [(4, 1)])
    with pytest.raises(ValueError, match="column 0"):
        nt.group_moments(Z, None, ROWS, pairs, [(0, 0, 2)], [])
    with pytest.raises(ValueError, match="pairs out of range"):
        nt.group_moments(Z, K, ROWS, [(0, 4)], KEYS, [])
    with pytest.raises(ValueError, match="segments cover"):
        nt.group_moments(Z, K, ROWS[:-1], pairs, KEYS, [])
    with pytest.raises(ValueError, match="groups"):
        nt.group_moments(Z, K, ROWS, pairs, [(0, 0, 1 << 13), (1, 0, 1 << 13)], [])
