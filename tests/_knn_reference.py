"""A float64 yardstick for the per-row top-k lists (graph.py:34-62), independent of every device route and of the fp32
oracle: plain NumPy, chunked over rows so that no N x N float64 matrix is ever held.

`lists_f64` gives the lists and, per row, the float64 distance between the k-th and the (k+1)-th similarity.  That gap is
what decides whether an fp32 computation MAY order the row's rank-k boundary differently: `check_lists` lets a row's member
set differ from the yardstick's only if the row's own gap AND the spread of the members in dispute are below `gap_tol`.
There is no free count of tolerated rows.

The rule is satisfiable by an fp32 computation.  Rows with gap < gap_tol (1e-6 on i.i.d. anchors, 4e-6 on clustered and
grouped ones, 2e-6 D / 1024 beyond 1024 columns) per shape (N, D, k), inputs from default_rng(N + D + k), and the rows
on which the oracle's fp32 sgemm lists (oracle.knn_topk, deterministic) differ from the float64 ones -- CPU figures; no
device list has been held to this yardstick yet:

    (6144, 512, 16) iid 6 / 0        (6144, 512, 33) iid 16 / 1       (6145, 600, 8) clustered 75 / 1
    (7168, 320, 16) iid 7 / 0        (7168, 384, 16) clustered 113 / 5  (7168, 385, 12) iid 4 / 0
    (6144, 769, 16) iid 8 / 0        (6144, 1536, 8) dups: every row / 0 (exact ties)
    (8192, 768, 44) iid 30 / 0       (8193, 20, 8) iid 0 / 0          (8193, 128, 16) grouped 60 / 1
    (12000, 64, 88) iid 22 / 1       (6143, 512, 16) iid 7 / 0        (6144, 511, 16) iid 5 / 0
    (6144, 512, 34) iid 11 / 0       (7167, 320, 16) iid 8 / 0        (8192, 128, 16) iid 10 / 0
    (8192, 768, 45) iid 29 / 0       (12000, 64, 89) iid 23 / 0       (10000, 64, 64) iid 11 / 0
    (8192, 64, 16) iid 3 / 1         (8192, 24, 1) iid 0 / 0          (8192, 24, 128) iid 19 / 0
    (8192, 600, 16) iid 10 / 0       D = 24, k = 16, iid: N = 4096 2 / 0, 5120 2 / 0, 5121 3 / 0, 6144 1 / 0, 6145 3 / 0,
    7168 3 / 0, 7169 1 / 1, 8191 3 / 0, 8192 1 / 0

(clustered: ~100 rows per cluster in cluster order, noise 0.35; grouped: 80 clusters of random sizes one after another;
dups: every row 40 times.)  One yardstick run takes 0.4-3.3 s."""
import numpy as np

from tests._fullsize import near_tie_gap


def _normalize_f64(Y):
    Y64 = np.asarray(Y, dtype=np.float64)
    with np.errstate(invalid="ignore"):  # inf / inf
        return Y64 / (np.linalg.norm(Y64, axis=1, keepdims=True) + 1e-12)  # graph.py:35


def lists_f64(Y, k, chunk=1024):
    """(idx int64 (N, k), val float64 (N, k), gap float64 (N,)): each row's k best columns in the order (similarity desc,
    index asc) (graph.py:46-49), diagonal excluded (graph.py:37), NaN similarities last (what a stable argsort of -S does),
    values clipped at 0 (graph.py:62); gap[r] = s_k - s_(k+1) of row r (inf where the row has no k + 1 comparable columns).
    A row without k comparable columns fills up with the non-comparable ones in index order at value 0."""
    N = Y.shape[0]
    k = int(max(1, min(k, N - 1)))  # graph.py:34
    Yn = _normalize_f64(Y)
    idx = np.empty((N, k), dtype=np.int64)
    val = np.empty((N, k), dtype=np.float64)
    gap = np.empty(N, dtype=np.float64)
    for r0 in range(0, N, chunk):
        r1 = min(N, r0 + chunk)
        n = r1 - r0
        with np.errstate(invalid="ignore"):
            S = Yn[r0:r1] @ Yn.T  # graph.py:36
        S[np.isnan(S)] = -np.inf  # ranks last ...
        S[np.arange(n), np.arange(r0, r1)] = -np.inf  # ... as does the diagonal (graph.py:37)
        np.negative(S, out=S)  # ascending from here on
        if k < N - 1:
            part = np.partition(S, k, axis=1)[:, :k + 1]
            kth, nxt = part[:, :k].max(axis=1), part[:, k]
        else:  # every off-diagonal column: the diagonal is the (k+1)-th
            kth, nxt = np.sort(S, axis=1)[:, k - 1], np.full(n, np.inf)
        with np.errstate(invalid="ignore"):  # inf - inf
            g = nxt - kth
        gap[r0:r1] = np.where(np.isnan(g), np.inf, g)
        # members: everything strictly better than the k-th value, then the columns equal to it by ascending index
        better = S < kth[:, None]
        need = k - better.sum(axis=1)
        equal = S == kth[:, None]
        equal[np.arange(n), np.arange(r0, r1)] = False  # (a row without k comparable columns: never the diagonal)
        better |= equal & (np.cumsum(equal, axis=1, dtype=np.int32) <= need[:, None])
        members = np.nonzero(better)[1].reshape(n, k)  # ascending index within a row
        ms = np.take_along_axis(S, members, axis=1)
        order = np.argsort(ms, axis=1, kind="stable")  # similarity desc; equal ones stay in index order
        idx[r0:r1] = np.take_along_axis(members, order, axis=1)
        val[r0:r1] = np.clip(-np.take_along_axis(ms, order, axis=1), 0.0, None)
    return idx, val, gap


def check_lists(Y, idx_dev, val_dev, k, gap_tol, rows=None, ref=None):
    """The device's lists against the yardstick's on every row (or on `rows`).  A list is k distinct columns of the lattice
    other than the row itself.  Same member set: the similarities agree member by member to atol = 2e-6 (the bound
    tests/_fullsize.py: check_knn_lists_on_sample holds the device to against sgemm).  Otherwise the row must be a rank-k
    near-tie by the yardstick's own measure: gap[row] < gap_tol, and the float64 similarities of the members in dispute lie
    within gap_tol of each other (near_tie_gap), as many on the one side as on the other.  `ref` = a lists_f64 result to
    share between calls.  Returns the number of rows whose member sets differed."""
    N = Y.shape[0]
    k = int(max(1, min(k, N - 1)))  # graph.py:34, as lists_f64
    idx_ref, val_ref, gap = lists_f64(Y, k) if ref is None else ref
    rows = np.arange(N) if rows is None else np.asarray(rows)
    dev = np.asarray(idx_dev)[rows].astype(np.int64)
    assert dev.shape[1] == idx_ref.shape[1] == k, f"lists of {dev.shape[1]} (device) / {idx_ref.shape[1]} (yardstick) members, k = {k}"
    od = np.argsort(dev, axis=1, kind="stable")
    oref = np.argsort(idx_ref[rows], axis=1, kind="stable")
    dev_s = np.take_along_axis(dev, od, axis=1)
    ref_s = np.take_along_axis(idx_ref[rows], oref, axis=1)
    bad = (dev_s < 0) | (dev_s >= N) | (dev_s == rows[:, None])
    assert not bad.any(), ("not a column of the lattice, or the row itself", rows[bad.any(axis=1)][:8].tolist())
    rep = dev_s[:, 1:] == dev_s[:, :-1]
    assert not rep.any(), ("repeated member", rows[rep.any(axis=1)][:8].tolist())
    differ = (dev_s != ref_s).any(axis=1)
    same = ~differ
    dv = np.take_along_axis(np.asarray(val_dev)[rows].astype(np.float64), od, axis=1)[same]
    rv = np.take_along_axis(val_ref[rows], oref, axis=1)[same]
    err = np.abs(dv - rv)
    assert not (err > 2e-6).any(), ("similarity", rows[same][(err > 2e-6).any(axis=1)][:8].tolist(), float(err.max()))
    for t in np.nonzero(differ)[0]:
        r = int(rows[t])
        d, f = set(dev_s[t].tolist()), set(ref_s[t].tolist())
        members = sorted(d ^ f)
        assert len(d - f) == len(f - d), (r, members)
        assert gap[r] < gap_tol, (r, members, float(gap[r]))
        spread = near_tie_gap(Y, r, members)
        assert spread < gap_tol, (r, members, spread)
    return int(differ.sum())
