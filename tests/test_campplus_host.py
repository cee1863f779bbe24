"""CPU tests of the CAM++ diarizer's host side: the shape table and the strict blob loader (tdx_campp_create rejects before
any device work), the fp64 oracle (tests/campplus_oracle.py), the window plan, the spectral clustering, the time
post-processing, and the whole host pipeline driven by the oracle embedder on two synthetic conversations."""
import ctypes as C

import numpy as np
import pytest
import torch

import campplus_oracle as orc
from targetdiarization_amd import _lib
from targetdiarization_amd import diarization as dz
from targetdiarization_amd.clustering import kmeans_labels, spectral_labels
from targetdiarization_amd.weights import (campplus_learnable, campplus_param_shapes, drop_num_batches_tracked, pack_blob,
                                           recipe_campplus_state_dict)


# ---------------------------------------------------------------- shapes and parsing
def test_shape_table_counts():
    s = campplus_param_shapes()
    assert len(s) == 815
    assert sum(int(np.prod(v)) for k, v in s.items() if campplus_learnable(k)) == 6848544
    wide = campplus_param_shapes(emb=512)          # the published 7.18 M model has a 512-d dense layer
    assert round(sum(int(np.prod(v)) for k, v in wide.items() if campplus_learnable(k)) / 1e6, 2) == 7.18
    sd = recipe_campplus_state_dict(0)
    assert list(sd) == list(s) and all(tuple(sd[k].shape) == tuple(v) for k, v in s.items())


@pytest.fixture(scope="module")
def lib():
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.lib()


def _create(lib, sd):
    blob = pack_blob(sd)
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    return lib.tdx_campp_create(buf, len(blob), 0, C.byref(C.c_void_p()))


def test_create_is_strict_both_ways(lib):
    sd = recipe_campplus_state_dict(0)
    for name in ("xvector.block2.tdnnd17.cam_layer.linear2.bias", "head.layer2.0.shortcut.1.running_var",
                 "xvector.dense.nonlinear.batchnorm.running_mean"):
        missing = dict(sd)
        del missing[name]
        assert _create(lib, missing) == 2
        assert name.encode() in lib.tdx_last_error()
    extra = dict(sd)
    extra["xvector.dense.nonlinear.batchnorm.weight"] = torch.ones(192)       # affine=False upstream: not a tensor of the model
    assert _create(lib, extra) == 2
    err = lib.tdx_last_error()
    assert b"unexpected" in err and b"xvector.dense.nonlinear.batchnorm.weight" in err
    tracked = dict(sd)
    tracked["head.bn1.num_batches_tracked"] = torch.zeros(())
    assert _create(lib, tracked) == 2 and b"head.bn1.num_batches_tracked" in lib.tdx_last_error()
    assert list(drop_num_batches_tracked(tracked)) == list(sd)               # the host drops them before packing
    wrong = dict(sd)
    wrong["xvector.tdnn.linear.weight"] = torch.zeros(128, 320, 3)
    assert _create(lib, wrong) == 2 and b"xvector.tdnn.linear.weight" in lib.tdx_last_error()
    blob = pack_blob(sd)[:-100]
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    assert lib.tdx_campp_create(buf, len(blob), 0, C.byref(C.c_void_p())) == 2


def test_null_handle_calls(lib):
    assert lib.tdx_campp_workspace_bytes(None, 1, 100) == 0
    assert lib.tdx_campp_flops(None, 1, 100) == 0.0
    assert lib.tdx_campp_forward(None, None, 1, 100, None, None, 0, None) == 1
    assert lib.tdx_campp_destroy(None) == 0


# ---------------------------------------------------------------- oracle
def test_segment_pooling_values():
    x = torch.arange(250, dtype=torch.float64).view(1, 1, 250)
    y = orc.seg_pooling(x)[0, 0]
    assert y[:100].eq(49.5).all() and y[100:200].eq(149.5).all() and y[200:].eq(224.5).all()
    ref = torch.nn.functional.avg_pool1d(x, 100, 100, ceil_mode=True)[0, 0]
    assert ref.tolist() == [49.5, 149.5, 224.5]


def test_oracle_fp32_agrees_with_fp64():
    sd = orc.calibrated_state_dict()
    feat = torch.randn(2, 215, 80, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2.0
    a = orc.forward(sd, feat, torch.float64)
    b = orc.forward(sd, feat, torch.float32).double()
    assert a.shape == (2, 192)
    rel = ((a - b).norm(dim=1) / a.norm(dim=1)).max().item()
    print("oracle fp32 vs fp64 rel-L2", rel)
    assert rel < 5e-5
    one = orc.forward(sd, feat[1:], torch.float64)
    assert torch.allclose(one[0], a[1], rtol=0, atol=1e-12)


# ---------------------------------------------------------------- window plan
def _sec(ws):
    return [[st / 16000, ed / 16000] for st, ed in ws]


def test_window_plan():
    assert _sec(dz.plan_windows([[0.0, 4.0]], 64000)) == [[0, 1.5], [0.75, 2.25], [1.5, 3.0], [2.25, 3.75], [2.5, 4.0]]
    w = dz.plan_windows([[0.5, 1.5]], 64000)                       # shorter than a window: one, zero-padded to 1.5 s
    assert _sec(w) == [[0.5, 1.5]]
    audio = np.arange(64000, dtype=np.float32)
    cut = dz.cut_windows(audio, w)
    assert len(cut) == 1 and cut[0].shape == (24000,) and cut[0][15999] == 23999 and not cut[0][16000:].any()
    assert _sec(dz.plan_windows([[0.0, 3.0]], 48000)) == [[0, 1.5], [0.75, 2.25], [1.5, 3.0]]     # an exact multiple of the shift
    two = dz.plan_windows([[1.0, 3.25], [10.0, 11.5]], 16000 * 12)
    assert _sec(two) == [[1.0, 2.5], [1.75, 3.25], [10.0, 11.5]]
    assert dz.plan_windows([[5.0, 9.0]], 16000 * 6) == [(80000, 96000)]                          # clipped to the audio
    assert dz.plan_windows([], 1000) == []


# ---------------------------------------------------------------- clustering
def _blobs(k, per, cos_between=None, seed=0, d=32, spread=0.05):
    rng = np.random.default_rng(seed)
    if cos_between is None:
        centres = np.linalg.qr(rng.standard_normal((d, d)))[0][:k]
    else:      # two centres at a given cosine
        a, b = np.linalg.qr(rng.standard_normal((d, d)))[0][:2]
        centres = np.stack([a, cos_between * a + np.sqrt(1 - cos_between ** 2) * b])
    X = np.concatenate([c + spread * rng.standard_normal((per, d)) / np.sqrt(d) for c in centres])
    y = np.repeat(np.arange(len(centres)), per)
    p = rng.permutation(len(y))
    return X[p], y[p]


def _same_partition(a, b):
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("k,per", [(2, 10), (3, 9), (4, 12)])
def test_spectral_recovers_blobs(k, per):
    X, y = _blobs(k, per, seed=k)
    lab = spectral_labels(X)
    assert _same_partition(lab, y)
    assert np.array_equal(lab, spectral_labels(X))                 # deterministic


def test_spectral_small_n_merge_and_oracle_num():
    X, y = _blobs(3, 9, seed=1)
    assert not spectral_labels(X[:19]).any()                       # fewer than 20 embeddings: one speaker
    X2, y2 = _blobs(2, 15, cos_between=0.9, seed=2, spread=0.02)
    assert len(set(spectral_labels(X2).tolist())) == 1             # centres closer than the merge threshold end as one label
    assert _same_partition(spectral_labels(X2, oracle_num=2), y2)  # ... unless the speaker count is given (no merging then)
    assert len(set(spectral_labels(X, oracle_num=2).tolist())) == 2
    assert _same_partition(kmeans_labels(X, 3), y)


# ---------------------------------------------------------------- post-processing
def _w(*secs):
    return [(int(a * 16000), int(b * 16000)) for a, b in secs]


def test_postprocess_cases():
    # relabel by first appearance + merge of adjacent windows + midpoint cut of the overlap
    win = _w((0, 1.5), (0.75, 2.25), (1.5, 3.0), (2.25, 3.75))
    assert dz.postprocess(win, [5, 5, 2, 2]) == [[0.0, 1.875, 0], [1.875, 3.75, 1]]
    # a 0.75 s island between two long segments goes to the nearer neighbour (ties: the earlier one)
    win = _w((0, 1.5), (0.75, 2.25), (1.5, 3.0), (2.25, 3.75), (3.0, 4.5), (3.75, 5.25))
    assert dz.postprocess(win, [0, 0, 1, 0, 0, 0]) == [[0.0, 5.25, 0]]
    # windows [0,2.25] | [1.5,3.0] | [2.25,5.25] -> cuts at 1.875 and 2.625: the middle segment lasts 0.75 s; both neighbours touch it
    assert dz.postprocess(win, [3, 3, 7, 4, 4, 4]) == [[0.0, 2.625, 0], [2.625, 5.25, 1]]
    # a gap between speech ranges is kept; a short segment next to a gap joins the neighbour it touches
    win = _w((0, 1.5), (0.75, 2.25), (1.5, 3.0), (10.0, 10.5), (10.0, 11.5), (10.75, 12.25))
    assert dz.postprocess(win, [0, 0, 0, 1, 0, 0]) == [[0.0, 3.0, 0], [10.0, 12.25, 0]]
    assert dz.postprocess(_w((0, 1.0)), [4]) == [[0.0, 1.0, 0]]
    assert dz.postprocess([], []) == []


# ---------------------------------------------------------------- end to end through the oracle embedder
@pytest.mark.parametrize("name,voices", [("three", 3), ("two", 2)])
def test_host_pipeline_on_a_conversation(name, voices):
    """every window that lies wholly inside one voice's turn gets that voice's label (up to permutation); windows that
    straddle a turn change may fall anywhere (at most 35 % of the windows)"""
    sd = orc.calibrated_state_dict()
    audio, turns = orc.conversation(name)
    res, windows, labels = dz.diarize(audio, orc.oracle_embedder(sd), return_windows=True)
    truth = orc.pure_window_truth(windows, turns)
    print(name, len(windows), "windows,", int((truth < 0).sum()), "straddle a turn change")
    assert (truth < 0).mean() <= 0.35
    assert orc.consistent_up_to_permutation(labels, truth)
    rows = res["text"]
    assert len({r[2] for r in rows}) == voices and rows[0][0] == 0.0 and rows[-1][1] == round(len(audio) / 16000, 3)
    assert all(a[1] == b[0] for a, b in zip(rows, rows[1:]))                # the conversation has no silence
    # the segment boundaries sit within one window shift of the true turn changes
    assert len(rows) == len(turns)
    assert all(abs(r[1] - t[1] / 16000) <= 0.75 for r, t in zip(rows, turns))
