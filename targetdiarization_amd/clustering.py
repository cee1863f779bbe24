"""HDBSCAN* on the host for the few-hundred speaker embeddings of the path.

The reference clusters per-clip target embeddings with `hdbscan.HDBSCAN(min_cluster_size=2, metric="euclidean")` and
drops the noise label (TargetASR.py:236-243); BASELINE's config 5 all-gathers the `[n*2,192]` embedding block "for
clustering".  The `hdbscan` package is third-party and absent, so the published algorithm is restated here (Campello,
Moulavi, Sander 2013; McInnes, Healy, Astels 2017 — the package's `generic`/`prims` path): core distances -> mutual
reachability -> minimum spanning tree -> single-linkage hierarchy -> condensed tree (min_cluster_size) -> excess-of-mass
selection (no single-cluster result) -> labels, noise = -1.  Dense O(n^2) arithmetic in float64: n is the number of
clips of one speaker or the utterances of a batch, not audio frames.  Parity unpinned against the `hdbscan` package
itself; tests compare with `sklearn.cluster.HDBSCAN` (the same algorithm) where scikit-learn is importable.
"""
from __future__ import annotations

import numpy as np


def _mst_prim(W: np.ndarray) -> np.ndarray:
    """minimum spanning tree of the dense symmetric weight matrix W: rows (a, b, weight), n-1 of them"""
    n = W.shape[0]
    in_tree = np.zeros(n, dtype=bool)
    best = np.full(n, np.inf)
    src = np.zeros(n, dtype=np.int64)
    edges = np.zeros((n - 1, 3))
    cur = 0
    in_tree[0] = True
    for i in range(n - 1):
        closer = ~in_tree & (W[cur] < best)
        best[closer] = W[cur][closer]
        src[closer] = cur
        cand = np.where(in_tree, np.inf, best)
        nxt = int(np.argmin(cand))
        edges[i] = (src[nxt], nxt, cand[nxt])
        in_tree[nxt] = True
        cur = nxt
    return edges


def _single_linkage(edges: np.ndarray, n: int):
    """sorted MST edges -> dendrogram rows (left, right, distance, size); node ids: points 0..n-1, merges n..2n-2"""
    order = np.argsort(edges[:, 2], kind="stable")
    parent = np.arange(2 * n - 1)
    size = np.ones(2 * n - 1, dtype=np.int64)

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root
    rows = []
    nxt = n
    for a, b, w in edges[order]:
        ra, rb = find(int(a)), find(int(b))
        rows.append((ra, rb, float(w), int(size[ra] + size[rb])))
        parent[ra] = parent[rb] = nxt
        size[nxt] = size[ra] + size[rb]
        nxt += 1
    return rows


def _bfs(rows, n, root):
    out, frontier = [], [root]
    while frontier:
        out.extend(frontier)
        nxt = []
        for x in frontier:
            if x >= n:
                nxt.extend(rows[x - n][:2])
        frontier = nxt
    return out


def hdbscan_labels(X, min_cluster_size: int = 2, min_samples: int | None = None) -> np.ndarray:
    """labels [n] int: 0..k-1 per cluster, -1 = noise (hdbscan.HDBSCAN(min_cluster_size, metric="euclidean").fit_predict)"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    if min_samples is None:
        min_samples = min_cluster_size
    if n <= max(min_cluster_size, 1):
        return np.full(n, -1, dtype=np.int64)
    sq = (X * X).sum(axis=1)
    D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (X @ X.T), 0.0))
    np.fill_diagonal(D, 0.0)
    k = min(n - 1, max(min_samples - 1, 0))           # min_samples neighbours INCLUDING the point itself
    core = np.sort(D, axis=1)[:, k]
    W = np.maximum(D, np.maximum(core[:, None], core[None, :]))
    rows = _single_linkage(_mst_prim(W), n)
    # ---- condensed tree: (parent cluster, child, lambda, child size); clusters are numbered from n in BFS order
    root = 2 * n - 2
    relabel = {root: n}
    next_label = n + 1
    ignore = set()
    ctree = []
    for node in _bfs(rows, n, root):
        if node < n or node in ignore:
            continue
        left, right, dist, _ = rows[node - n]
        lam = 1.0 / dist if dist > 0.0 else np.inf
        lc = rows[left - n][3] if left >= n else 1
        rc = rows[right - n][3] if right >= n else 1
        big_l, big_r = lc >= min_cluster_size, rc >= min_cluster_size
        if big_l and big_r:
            for child, cnt in ((left, lc), (right, rc)):
                relabel[child] = next_label
                ctree.append((relabel[node], next_label, lam, cnt))
                next_label += 1
            continue
        for child, big in ((left, big_l), (right, big_r)):
            if big:
                relabel[child] = relabel[node]          # the cluster lives on in its large side
            else:
                for sub in _bfs(rows, n, child):
                    if sub < n:
                        ctree.append((relabel[node], sub, lam, 1))
                    ignore.add(sub)
    # ---- stability and excess-of-mass selection
    birth = {n: 0.0}
    for p, c, lam, cnt in ctree:
        if c >= n:
            birth[c] = lam
    stability = {c: 0.0 for c in birth}
    for p, c, lam, cnt in ctree:
        stability[p] += (lam - birth[p]) * cnt
    children = {c: [] for c in birth}
    for p, c, lam, cnt in ctree:
        if c >= n:
            children[p].append(c)
    selected = {c: True for c in birth}
    for c in sorted(birth, reverse=True):
        if c == n:                                     # the root is never a cluster (allow_single_cluster=False)
            selected[c] = False
            continue
        sub = sum(stability[ch] for ch in children[c])
        if sub > stability[c]:
            selected[c] = False
            stability[c] = sub
        else:
            stack = list(children[c])
            while stack:
                d = stack.pop()
                selected[d] = False
                stack.extend(children[d])
    clusters = sorted(c for c, s in selected.items() if s)
    label_of = {c: i for i, c in enumerate(clusters)}
    # ---- labels: a point belongs to the selected cluster at or above the cluster it fell out of
    up = {c: p for p, c, lam, cnt in ctree if c >= n}
    labels = np.full(n, -1, dtype=np.int64)
    for p, c, lam, cnt in ctree:
        if c < n:
            q = p
            while q not in label_of and q in up:
                q = up[q]
            if q in label_of:
                labels[c] = label_of[q]
    return labels


# ---------------------------------------------------------------------------------------------------------------
# Spectral clustering of the CAM++ diarizer's window embeddings (modelscope speech_campplus_speaker-diarization_common:
# cluster_backend.SpectralCluster + merge-by-cosine) [upstream-recall; DESIGN §8.10 is the governing description].
# modelscope switches to UMAP + HDBSCAN from 2 048 embeddings on; UMAP is third-party and absent, so the spectral path
# serves every n.  k-means is an own deterministic one (k-means++ seeding from a fixed seed, Lloyd iterations).
# ---------------------------------------------------------------------------------------------------------------
def kmeans_labels(X: np.ndarray, k: int, seed: int = 0, n_init: int = 10, iters: int = 100) -> np.ndarray:
    """deterministic k-means: best inertia of n_init k-means++ starts drawn from default_rng(seed)"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    k = max(1, min(k, n))
    rng = np.random.default_rng(seed)
    best, best_inertia = np.zeros(n, dtype=np.int64), np.inf
    for _ in range(n_init):
        centres = [X[rng.integers(n)]]
        for _c in range(1, k):
            d2 = np.min(((X[:, None, :] - np.asarray(centres)[None]) ** 2).sum(-1), axis=1)
            tot = d2.sum()
            centres.append(X[rng.choice(n, p=d2 / tot)] if tot > 0 else X[rng.integers(n)])
        C = np.asarray(centres)
        lab = None
        for _it in range(iters):
            d2 = ((X[:, None, :] - C[None]) ** 2).sum(-1)
            new = d2.argmin(axis=1)
            if lab is not None and np.array_equal(new, lab):
                break
            lab = new
            for j in range(k):
                if np.any(lab == j):
                    C[j] = X[lab == j].mean(axis=0)
        inertia = ((X - C[lab]) ** 2).sum()
        if inertia < best_inertia - 1e-12:
            best, best_inertia = lab.copy(), inertia
    return best


def _unit(X):
    return X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-12)


def merge_by_cosine(labels: np.ndarray, X: np.ndarray, threshold: float = 0.78) -> np.ndarray:
    """merge the pair of clusters whose centres (mean embeddings) have the highest cosine while it exceeds threshold"""
    labels = np.asarray(labels).copy()
    while True:
        ids = np.unique(labels)
        if len(ids) <= 1:
            return labels
        C = _unit(np.stack([X[labels == i].mean(axis=0) for i in ids]))
        S = C @ C.T
        np.fill_diagonal(S, -np.inf)
        a, b = np.unravel_index(np.argmax(S), S.shape)
        if S[a, b] <= threshold:
            return labels
        labels[labels == ids[max(a, b)]] = ids[min(a, b)]


def spectral_drop(n: int, pval: float = 0.022, min_pnum: int = 6) -> int:
    """entries zeroed per row of the n x n affinity: all but the largest max(min_pnum, n - int((1 - pval) n))"""
    return max(0, min(int((1.0 - pval) * n), n - min_pnum))


def spectral_tail(w: np.ndarray, V: np.ndarray, X: np.ndarray, oracle_num: int | None = None, max_spks: int = 15,
                  merge_threshold: float = 0.78, seed: int = 0) -> np.ndarray:
    """lowest eigenvalues w [m] (ascending) and eigenvectors V [n,m] of the Laplacian, embeddings X [n,d] -> labels [n]: the speaker
    count from the largest eigengap (or oracle_num), k-means on the first k eigenvectors, then the merge by cosine"""
    n = V.shape[0]
    if oracle_num is not None:
        k = int(oracle_num)
    else:
        gaps = np.diff(w)[:max_spks]
        k = int(np.argmax(gaps)) + 1
    k = max(1, min(k, max_spks, n))
    labels = kmeans_labels(V[:, :k], k, seed=seed)
    if oracle_num is None:
        labels = merge_by_cosine(labels, X, merge_threshold)
    return labels


def spectral_labels(X: np.ndarray, oracle_num: int | None = None, min_num: int = 20, pval: float = 0.022, min_pnum: int = 6,
                    max_spks: int = 15, merge_threshold: float = 0.78, seed: int = 0) -> np.ndarray:
    """X [n,d] embeddings -> labels [n] (0-based, in no particular order).  n < min_num: all zeros."""
    from scipy.linalg import eigh
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    if n < min_num:
        return np.zeros(n, dtype=np.int64)
    U = _unit(X)
    A = U @ U.T
    drop = spectral_drop(n, pval, min_pnum)                          # per row: zero the `drop` smallest affinities
    if drop:
        idx = np.argsort(A, axis=1, kind="stable")[:, :drop]
        np.put_along_axis(A, idx, 0.0, axis=1)
    A = 0.5 * (A + A.T)
    np.fill_diagonal(A, 0.0)
    L = np.diag(A.sum(axis=1)) - A
    m = min(max_spks + 1, n)
    w, V = eigh(L, subset_by_index=[0, m - 1])
    return spectral_tail(w, V, X, oracle_num, max_spks, merge_threshold, seed)


SPECTRAL_DEVICE_MAX_N = 8192      # tdx_spectral_laplacian / tdx_symeig_lowest: element indices are int


def spectral_labels_device(X_dev, oracle_num: int | None = None, min_num: int = 20, pval: float = 0.022, min_pnum: int = 6,
                           max_spks: int = 15, merge_threshold: float = 0.78, seed: int = 0) -> np.ndarray:
    """spectral_labels for embeddings X_dev [n,d] that lie on the device (float32 torch tensor): affinity, pruning, Laplacian and
    its lowest eigenpairs on the device (ops.spectral_eig, csrc/spectral.hip); eigenvalues, the [n,16] eigenvectors and X come to the
    host for spectral_tail, the same function the host path ends with.  More than 8192 embeddings, more than 15 speakers or a
    device error: the reason is printed and the host function runs."""
    n = int(X_dev.shape[0])
    if n < min_num:
        return np.zeros(n, dtype=np.int64)
    kw = dict(oracle_num=oracle_num, max_spks=max_spks, merge_threshold=merge_threshold, seed=seed)
    m = min(max_spks + 1, n)
    why = None
    if n > SPECTRAL_DEVICE_MAX_N:
        why = f"{n} embeddings exceed the device limit of {SPECTRAL_DEVICE_MAX_N}"
    elif m > 16:
        why = f"max_spks = {max_spks} needs more than the 16 eigenpairs the device returns"
    else:
        from . import _lib, ops
        try:
            w, V = ops.spectral_eig(X_dev, spectral_drop(n, pval, min_pnum), m=m)
            w, V = w.cpu().numpy(), V.cpu().numpy()
        except _lib.TdxError as err:
            why = str(err)
    X = X_dev.detach().cpu().numpy().astype(np.float64)
    if why is not None:
        print(f"spectral_labels_device: {why}; clustering on the host")
        return spectral_labels(X, min_num=min_num, pval=pval, min_pnum=min_pnum, **kw)
    return spectral_tail(w, V, X, **kw)
