"""CPU tests of the spectral-clustering split (clustering.spectral_drop / spectral_tail), of the argument checks of the three
device entries (nothing is launched for a refused call) and of the `cluster` switch of the diarizer."""
import ctypes as C

import numpy as np
import pytest
from scipy.linalg import eigh

import spectral_cases as sc
from targetdiarization_amd import _lib
from targetdiarization_amd import diarization as dz
from targetdiarization_amd.clustering import spectral_drop, spectral_labels, spectral_labels_device, spectral_tail


@pytest.fixture(scope="module")
def lib():
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.lib()


@pytest.mark.parametrize("case", sc.BLOB_CASES + [sc.ONE_SPEAKER], ids=lambda c: f"n{c[0]}k{c[1]}")
def test_tail_on_the_host_eigenvectors_is_spectral_labels(case):
    X, y = sc.blobs(*case)
    n = len(X)
    _, L = sc.host_laplacian(X)
    w, V = eigh(L, subset_by_index=[0, min(16, n) - 1])
    want = spectral_labels(X)
    assert np.array_equal(spectral_tail(w, V, X.astype(np.float64)), want)
    assert sc.same_partition(want, y)
    if case[1] > 1:
        assert sc.gap_ratio(w) >= 4.0


def test_tail_with_oracle_num():
    X, y = sc.blobs(*sc.ORACLE_CASE)
    _, L = sc.host_laplacian(X)
    w, V = eigh(L, subset_by_index=[0, 15])
    assert sc.gap_ratio(w) >= 4.0 and w[1] > 1e-3 and w[2] > 2.0 * w[1] and sc.same_partition(spectral_labels(X), y)
    got = spectral_tail(w, V, X.astype(np.float64), oracle_num=2)
    assert np.array_equal(got, spectral_labels(X, oracle_num=2)) and len(set(got.tolist())) == 2


@pytest.mark.parametrize("n", [6, 20, 21, 273, 2400])
def test_spectral_drop_is_the_inline_formula(n):
    pval, min_pnum = 0.022, 6
    assert spectral_drop(n) == max(0, min(int((1.0 - pval) * n), n - min_pnum))
    assert spectral_drop(n, 0.1, 3) == max(0, min(int((1.0 - 0.1) * n), n - 3))
    assert 0 <= spectral_drop(n) < max(n, 1)


def test_argument_checks_without_a_device(lib):
    one = C.cast((C.c_char * 64)(), C.c_void_p)
    big = 1 << 40
    err = lib.tdx_last_error

    def lap(emb=one, n=32, d=192, drop=3, L=one, tap=None, ws=one, nb=big):
        return lib.tdx_spectral_laplacian(emb, n, d, drop, L, tap, ws, nb, None)

    def eig(M=one, n=32, m=16, w=one, V=one, ws=one, nb=big):
        return lib.tdx_symeig_lowest(M, n, m, w, V, ws, nb, None)

    assert lap(emb=None) == 1 and b"tdx_spectral_laplacian" in err()
    assert lap(L=None) == 1 and lap(ws=None) == 1
    assert lap(n=0) == 1 and lap(n=8193) == 1 and b"8192" in err()
    assert lap(d=0) == 1
    assert lap(drop=-1) == 1 and lap(drop=32) == 1 and b"drop" in err()
    need = lib.tdx_spectral_workspace_bytes(32, 192, 16)
    assert need > 0
    assert lap(nb=need - 1) == 4 and b"workspace too small" in err()
    assert eig(M=None) == 1 and b"tdx_symeig_lowest" in err()
    assert eig(w=None) == 1 and eig(V=None) == 1 and eig(ws=None) == 1
    assert eig(n=0) == 1 and eig(n=8193) == 1
    assert eig(m=0) == 1 and eig(m=17) == 1 and eig(n=5, m=6) == 1 and b"min(n, 16)" in err()
    assert eig(nb=lib.tdx_spectral_workspace_bytes(32, 1, 16) - 1) == 4
    for bad in [(0, 192, 1), (8193, 192, 16), (32, 0, 16), (32, 192, 0), (32, 192, 17), (5, 192, 6)]:
        assert lib.tdx_spectral_workspace_bytes(*bad) == 0
    # the scratch holds at least U [n,d] and the seven [n,16] planes of the inverse iteration, and grows with n
    assert lib.tdx_spectral_workspace_bytes(8192, 192, 16) >= 8192 * (192 + 7 * 16) * 8
    assert lib.tdx_spectral_workspace_bytes(1, 1, 1) > 0


def test_diarizer_rejects_an_unknown_cluster_value():
    with pytest.raises(ValueError):
        dz.CamppDiarizer({}, cluster="gpu?")


def test_diarize_calls_the_cluster_it_is_given():
    audio = np.zeros(16000 * 6, dtype=np.float32)
    seen = {}

    def embed(windows):
        return np.arange(len(windows) * 4, dtype=np.float32).reshape(len(windows), 4)

    def cluster(emb, oracle_num=None, **kw):
        seen.update(emb=emb, oracle_num=oracle_num, kw=kw)
        return np.arange(len(emb)) % 2

    res, windows, labels = dz.diarize(audio, embed, oracle_num=3, return_windows=True, cluster=cluster, seed=5)
    assert seen["oracle_num"] == 3 and seen["kw"] == {"seed": 5}
    assert seen["emb"].dtype == np.float64 and seen["emb"].shape == (len(windows), 4)
    assert np.array_equal(labels, np.arange(len(windows)) % 2)
    assert res == {"text": dz.postprocess(windows, labels)}


def test_device_labels_below_min_num_need_no_device():
    import torch
    assert not spectral_labels_device(torch.zeros(19, 192)).any()
    assert spectral_labels_device(torch.zeros(19, 192)).shape == (19,)
