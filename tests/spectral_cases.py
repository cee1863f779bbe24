"""Inputs of the spectral-clustering tests (test_spectral_host.py on the CPU, test_gpu_spectral.py on the device): the blob
generator, the table of blob cases with the seeds chosen when the tests were written, the host Laplacian, and the table of
symmetric matrices the eigen-solver is tried on."""
import numpy as np

from targetdiarization_amd.clustering import _unit, spectral_drop

U53 = 2.0 ** -53


def blobs(n, k, noise, seed, balanced=True, d=192):
    """k Gaussian centres in d dimensions, n float32 embeddings around them -> (X [n,d], y [n])"""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((k, d))
    y = np.arange(n) % k if balanced else rng.integers(0, k, n)
    X = (C[y] + noise * rng.standard_normal((n, d))).astype(np.float32)
    return X, y


# (n, k, noise, seed, balanced): on each the host spectral_labels recovers y exactly, and the largest of the first 15 eigengaps of
# the host Laplacian is at least 4 times the second largest (asserted by the tests, not assumed)
BLOB_CASES = [
    (20, 2, 0.5, 242, True),
    (21, 3, 0.3, 17, True),
    (64, 3, 0.5, 2, False),
    (97, 4, 0.5, 3, True),
    (130, 2, 0.7, 4, False),
    (257, 5, 0.5, 5, True),
    (1200, 3, 0.9, 6, False),
    (2400, 4, 0.9, 7, True),
]
ONE_SPEAKER = (300, 1, 0.5, 8, True)
# (64, 3) for oracle_num = 2.  At noise <= 0.9 every row keeps its 6 neighbours inside its own blob, the pruned graph falls into 3
# components and the eigenvalue 0 is exactly 3-fold: V[:, :2] is then an arbitrary 2-dimensional cut of a 3-dimensional space and
# which two blobs k = 2 joins depends on the basis an eigen-solver happens to return (LAPACK's own choice included), so two
# correct solvers differ.  At noise 1.8 some neighbours lie across blobs, the graph is connected, the eigenvalues start
# 0 < 0.0062 < 0.037 << 0.43 and the first two eigenvectors are determined; the host still recovers y without oracle_num.
ORACLE_CASE = (64, 3, 1.8, 5, False)


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def host_prune_laplacian(A, drop):
    """the host rule on a given affinity: stable argsort, put_along_axis, symmetrise, zero diagonal, L = D - A"""
    A = np.array(A, dtype=np.float64)
    if drop:
        idx = np.argsort(A, axis=1, kind="stable")[:, :drop]
        np.put_along_axis(A, idx, 0.0, axis=1)
    A = 0.5 * (A + A.T)
    np.fill_diagonal(A, 0.0)
    return np.diag(A.sum(axis=1)) - A


def host_laplacian(X, drop=None):
    """float32 embeddings -> (unpruned affinity, Laplacian) as clustering.spectral_labels builds them"""
    U = _unit(np.asarray(X, dtype=np.float64))
    A = U @ U.T
    return A, host_prune_laplacian(A, spectral_drop(len(A)) if drop is None else drop)


def gap_ratio(w, max_spks=15):
    """largest / second largest of the first max_spks gaps of the ascending eigenvalues w"""
    g = np.sort(np.diff(w)[:max_spks])
    return g[-1] / g[-2]


def tied_rows(n=97, seed=11):
    """blobs whose rows 5 and 50 are copies of row 4: columns 4, 5 and 50 of every affinity row are equal to the bit"""
    X, y = blobs(n, 4, 0.5, seed)
    X[5] = X[4]
    X[50] = X[4]
    return X


def _sym(rng, n):
    A = rng.standard_normal((n, n))
    return 0.5 * (A + A.T)


def _block_diag(*blocks):
    n = sum(b.shape[0] for b in blocks)
    M = np.zeros((n, n))
    o = 0
    for b in blocks:
        M[o:o + len(b), o:o + len(b)] = b
        o += len(b)
    return M


def eig_cases():
    """name -> symmetric float64 matrix (symmetric to the bit)"""
    rng = np.random.default_rng(2024)
    clique = np.ones((12, 12)) - np.eye(12)
    cl = _block_diag(clique, clique)
    path = np.diag(np.r_[1.0, 2.0 * np.ones(38), 1.0]) - np.eye(40, k=1) - np.eye(40, k=-1)
    return {
        "diag23": np.diag(rng.standard_normal(23)),
        "zero17": np.zeros((17, 17)),
        "eye19": np.eye(19),
        "blocks_9_1_14": _block_diag(_sym(rng, 9), _sym(rng, 1), _sym(rng, 14)),
        "rand1": _sym(rng, 1),
        "rand2": _sym(rng, 2),
        "rand3": _sym(rng, 3),
        "cliques_2x12": np.diag(cl.sum(axis=1)) - cl,
        "rand65": _sym(rng, 65),
        "path40": path,
    }
