"""-m gpu: spectral clustering on the device (csrc/spectral.hip) — the affinity against numpy in fp64, the pruning against the host
rule on the device's own affinity (exact), the eigen-solver against scipy.linalg.eigh at the n u scale of a backward-stable
tridiagonal method, the labels against clustering.spectral_labels as a partition, bitwise repeatability, and the diarizer with
cluster="device".  u = 2^-53 throughout."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from scipy.linalg import eigh

import campplus_oracle as orc
import spectral_cases as sc
from targetdiarization_amd import _lib, ops
from targetdiarization_amd.clustering import _unit, spectral_drop, spectral_labels, spectral_labels_device

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
U = sc.U53


def _stream():
    return torch.cuda.current_stream(dev).cuda_stream


def laplacian(X, drop, tap=True):
    """tdx_spectral_laplacian through the C entry -> (L, A_tap or None) as numpy"""
    l = _lib.lib()
    x = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
    n, d = x.shape
    nb = int(l.tdx_spectral_workspace_bytes(n, d, 1))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    L = torch.full((n, n), float("nan"), dtype=torch.float64, device=dev)
    A = torch.full((n, n), float("nan"), dtype=torch.float64, device=dev) if tap else None
    _lib.check(l.tdx_spectral_laplacian(x.data_ptr(), n, d, drop, L.data_ptr(), A.data_ptr() if tap else None, ws.data_ptr(), nb, _stream()))
    return L.cpu().numpy(), (A.cpu().numpy() if tap else None)


def symeig(M, m):
    """tdx_symeig_lowest through the C entry -> (w [m], V [n,m]) as numpy"""
    l = _lib.lib()
    n = M.shape[0]
    Md = torch.from_numpy(np.ascontiguousarray(M, dtype=np.float64)).to(dev)
    nb = int(l.tdx_spectral_workspace_bytes(n, 1, m))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    w = torch.full((m,), float("nan"), dtype=torch.float64, device=dev)
    V = torch.full((n, m), float("nan"), dtype=torch.float64, device=dev)
    _lib.check(l.tdx_symeig_lowest(Md.data_ptr(), n, m, w.data_ptr(), V.data_ptr(), ws.data_ptr(), nb, _stream()))
    return w.cpu().numpy(), V.cpu().numpy()


def check_eigenpairs(M, w, V, what):
    """the three bounds of the issue against scipy.linalg.eigh of the same matrix"""
    n, m = V.shape
    ref = eigh(M, eigvals_only=True)
    norm2 = float(np.abs(ref).max())
    e_val = float(np.abs(w - ref[:m]).max())
    e_res = float(np.abs(M @ V - V * w[None, :]).max())
    e_orth = float(np.abs(V.T @ V - np.eye(m)).max())
    print(f"{what}: n {n} m {m} |M|2 {norm2:.3e}  eigenvalues {e_val:.2e} (bound {8 * n * U * norm2:.2e})  residual {e_res:.2e} "
          f"(bound {64 * n * U * norm2:.2e})  orthogonality {e_orth:.2e} (bound {64 * n * U:.2e})")
    assert np.all(np.diff(w) >= 0)
    assert e_val <= 8 * n * U * norm2
    assert e_res <= 64 * n * U * norm2
    assert e_orth <= 64 * n * U


PRUNE_INPUTS = {
    "n20": lambda: sc.blobs(*sc.BLOB_CASES[0])[0],
    "n21": lambda: sc.blobs(*sc.BLOB_CASES[1])[0],
    "n130": lambda: sc.blobs(*sc.BLOB_CASES[4])[0],
    "n257": lambda: sc.blobs(*sc.BLOB_CASES[5])[0],
    "n97_ties": sc.tied_rows,
}


@functools.lru_cache(maxsize=None)
def device_laplacian(name):
    """(X, L, A_tap) with the default drop, computed once and shared (read-only)"""
    X = PRUNE_INPUTS[name]()
    L, A = laplacian(X, spectral_drop(len(X)))
    for a in (X, L, A):
        a.setflags(write=False)
    return X, L, A


# ------------------------------------------------------------------------------------------------ 1. affinity
@pytest.mark.parametrize("name", list(PRUNE_INPUTS))
def test_affinity_against_numpy_fp64(name):
    X, _, A = device_laplacian(name)
    d = X.shape[1]
    Un = _unit(X.astype(np.float64))
    err = float(np.abs(A - Un @ Un.T).max())
    print(f"{name}: max |A_tap - U U^T| {err:.2e} (bound {4 * (d + 4) * U:.2e})")
    assert err <= 4 * (d + 4) * U
    assert np.array_equal(A, A.T)


# ------------------------------------------------------------------------------------------------ 2. pruning
@pytest.mark.parametrize("name", list(PRUNE_INPUTS))
def test_pruning_is_the_host_rule_exactly(name):
    X = PRUNE_INPUTS[name]()
    n = len(X)
    if name == "n97_ties":
        A0 = device_laplacian(name)[2]
        assert np.array_equal(A0[:, 4], A0[:, 5]) and np.array_equal(A0[:, 4], A0[:, 50])      # the ties are there
    off = ~np.eye(n, dtype=bool)
    for drop in (0, spectral_drop(n), n - 1):
        L, A = (device_laplacian(name)[1:] if drop == spectral_drop(n) else laplacian(X, drop))
        want = sc.host_prune_laplacian(A, drop)
        assert np.array_equal(L[off].view(np.int64), want[off].view(np.int64)), (name, drop)
        dg = float(np.abs(np.diag(L) - np.diag(want)).max())
        bound = n * U * float(np.abs(np.diag(want)).max())
        print(f"{name} drop {drop}: diagonal differs by {dg:.2e} (bound {bound:.2e})")
        assert dg <= bound


def test_tap_is_optional():
    X = PRUNE_INPUTS["n21"]()
    L, _ = laplacian(X, spectral_drop(21), tap=False)
    assert np.array_equal(L, device_laplacian("n21")[1])


# ------------------------------------------------------------------------------------------------ 3. eigen-solver
EIG = sc.eig_cases()


@pytest.mark.parametrize("name", list(EIG))
def test_eigen_solver_on_the_case_table(name):
    M = EIG[name]
    n = M.shape[0]
    w, V = symeig(M, min(16, n))
    check_eigenpairs(M, w, V, name)
    w1, V1 = symeig(M, 1)
    check_eigenpairs(M, w1, V1, name + " (m = 1)")
    if name == "zero17":
        assert not w.any() and np.array_equal(V, np.eye(17)[:, :16])


@pytest.mark.parametrize("name", list(PRUNE_INPUTS))
def test_eigen_solver_on_the_laplacians(name):
    L = np.array(device_laplacian(name)[1])
    n = L.shape[0]
    w, V = symeig(L, min(16, n))
    check_eigenpairs(L, w, V, name)
    w1, V1 = symeig(L, 1)
    check_eigenpairs(L, w1, V1, name + " (m = 1)")


def test_the_cap_of_8192_rows():
    """n = 8192: the pruning and back-transformation kernels hold a row of 64 KB in LDS next to their scratch, element indices reach
    2^26 and L spans 512 MiB.  Everything is checked on the device: the Laplacian against the host rule restated with torch on the
    tap (stable argsort, exact), then the 16 lowest eigenpairs of a diagonal matrix (every Householder step is skipped)."""
    n, d = 8192, 16
    l = _lib.lib()
    X, _ = sc.blobs(n, 4, 0.9, 8192, d=d)
    x = torch.from_numpy(X).to(dev)
    drop = spectral_drop(n)
    nb = int(l.tdx_spectral_workspace_bytes(n, d, 16))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    L = torch.empty(n, n, dtype=torch.float64, device=dev)
    A = torch.empty(n, n, dtype=torch.float64, device=dev)
    _lib.check(l.tdx_spectral_laplacian(x.data_ptr(), n, d, drop, L.data_ptr(), A.data_ptr(), ws.data_ptr(), nb, _stream()))
    idx = torch.argsort(A, dim=1, stable=True)[:, :drop]
    A.scatter_(1, idx, 0.0)
    del idx
    A = 0.5 * (A + A.T)
    A.fill_diagonal_(0.0)
    rows = A.sum(dim=1)
    dg = float((torch.diagonal(L) - rows).abs().max())
    assert dg <= n * U * float(rows.abs().max())
    L.fill_diagonal_(0.0)
    want = 0.0 - A
    del A
    assert torch.equal(L.view(torch.int64), want.view(torch.int64))
    del want
    g = torch.Generator().manual_seed(8192)
    diag = torch.randn(n, generator=g, dtype=torch.float64)
    L.zero_()
    L.diagonal().copy_(diag.to(dev))
    M = L.clone()
    w = torch.empty(16, dtype=torch.float64, device=dev)
    V = torch.empty(n, 16, dtype=torch.float64, device=dev)
    _lib.check(l.tdx_symeig_lowest(L.data_ptr(), n, 16, w.data_ptr(), V.data_ptr(), ws.data_ptr(), nb, _stream()))
    order = torch.argsort(diag)[:16]
    norm2 = float(diag.abs().max())
    assert float((w.cpu() - diag[order]).abs().max()) <= 8 * n * U * norm2
    assert float((M @ V - V * w[None, :]).abs().max()) <= 64 * n * U * norm2
    assert float((V.T @ V - torch.eye(16, dtype=torch.float64, device=dev)).abs().max()) <= 64 * n * U
    assert torch.equal(V.abs().argmax(dim=0).cpu(), order)


# ------------------------------------------------------------------------------------------------ 4. labels
@functools.lru_cache(maxsize=None)
def host_side(case, oracle_num=None):
    """(X, y, host labels, host eigenvalues 0..15), computed once per case"""
    X, y = sc.blobs(*case)
    _, L = sc.host_laplacian(X)
    w = eigh(L, eigvals_only=True, subset_by_index=[0, min(16, len(X)) - 1])
    return X, y, spectral_labels(X, oracle_num=oracle_num), w


@pytest.mark.parametrize("case", sc.BLOB_CASES, ids=lambda c: f"n{c[0]}k{c[1]}")
def test_device_labels_are_the_host_partition(case):
    X, y, want, w_host = host_side(case)
    assert sc.gap_ratio(w_host) >= 4.0, sc.gap_ratio(w_host)
    got = spectral_labels_device(torch.from_numpy(X).to(dev))
    assert sc.same_partition(got, want) and sc.same_partition(got, y)
    if case[0] == 2400:                    # the benchmark-sized launch: its eigenpairs against LAPACK on the device's own Laplacian
        w, V, taps = ops.spectral_eig(torch.from_numpy(X).to(dev), spectral_drop(len(X)), return_taps=True)
        check_eigenpairs(taps["L"].cpu().numpy(), w.cpu().numpy(), V.cpu().numpy(), "n2400k4")


def test_device_labels_with_oracle_num_and_one_speaker():
    X, y, want, w_host = host_side(sc.ORACLE_CASE, 2)
    assert sc.gap_ratio(w_host) >= 4.0
    assert w_host[1] > 1e-3 and w_host[2] > 2.0 * w_host[1]            # the first two eigenvectors are determined (spectral_cases)
    assert sc.same_partition(spectral_labels(X), y)
    got = spectral_labels_device(torch.from_numpy(X).to(dev), oracle_num=2)
    assert sc.same_partition(got, want) and len(set(got.tolist())) == 2
    assert sc.same_partition(spectral_labels_device(torch.from_numpy(X).to(dev)), y)
    X1, _, want1, w1 = host_side(sc.ONE_SPEAKER)
    assert sc.gap_ratio(w1) >= 4.0
    got1 = spectral_labels_device(torch.from_numpy(X1).to(dev))
    assert not want1.any() and sc.same_partition(got1, want1)


# ------------------------------------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("case", [sc.BLOB_CASES[5], sc.BLOB_CASES[6]], ids=lambda c: f"n{c[0]}k{c[1]}")
def test_two_calls_return_the_same_bits(case):
    X, _ = sc.blobs(*case)
    x = torch.from_numpy(X).to(dev)
    drop = spectral_drop(len(X))
    w0, V0 = ops.spectral_eig(x, drop)
    w1, V1 = ops.spectral_eig(x, drop)
    assert torch.equal(w0.view(torch.int64), w1.view(torch.int64)) and torch.equal(V0.view(torch.int64), V1.view(torch.int64))
    L0, A0 = laplacian(X, drop)
    L1, A1 = laplacian(X, drop)
    assert np.array_equal(L0.view(np.int64), L1.view(np.int64)) and np.array_equal(A0.view(np.int64), A1.view(np.int64))


# ------------------------------------------------------------------------------------------------ 6. pipeline
@pytest.fixture(scope="module")
def sd():
    return orc.calibrated_state_dict()


@pytest.mark.parametrize("name", ["three", "two"])
def test_diarizer_with_device_clustering_matches_the_host_path(sd, name):
    from targetdiarization_amd import diarization as dz
    audio, _ = orc.conversation(name)
    res_h, win_h, lab_h = dz.CamppDiarizer(sd, cuda_device=0)(audio, return_windows=True)
    d = dz.CamppDiarizer(sd, cuda_device=0, cluster="device")
    res_d, win_d, lab_d = d(audio, return_windows=True)
    assert len(win_h) >= 20
    assert res_d == res_h and win_d == win_h and sc.same_partition(lab_d, lab_h)
    assert d(audio) == res_d


def test_target_diarization_passes_sd_cluster(sd, sd2):
    from targetdiarization_amd.diarization import CamppDiarizer
    from targetdiarization_amd.target_diarization import TargetDiarization
    from targetdiarization_amd.weights import recipe_eres2netv2_state_dict
    audio, _ = orc.conversation("three")
    td = TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=recipe_eres2netv2_state_dict(0), sd_state_dict=sd, sd_cluster="device")
    assert isinstance(td.sd_pipeline, CamppDiarizer) and td.sd_pipeline.cluster == "device"
    _, results, _ = td.infer(audio, None)
    assert len({r["speaker"] for r in results}) > 1
    with pytest.raises(ValueError):
        TargetDiarization(cuda_device=0, sep_state_dict=sd2, sd_state_dict=sd, sd_cluster="gpu?")


def test_few_windows_give_one_speaker_without_the_device_entries(sd, monkeypatch):
    from targetdiarization_amd import diarization as dz

    def refuse(*a, **k):
        raise AssertionError("the device entries were called for fewer than 20 windows")
    monkeypatch.setattr(ops, "spectral_eig", refuse)
    audio, _ = orc.conversation("two")
    res, windows, labels = dz.CamppDiarizer(sd, cuda_device=0, cluster="device")(audio[: 12 * 16000], return_windows=True)
    assert 0 < len(windows) < 20 and not np.asarray(labels).any()
    assert len({r[2] for r in res["text"]}) == 1
