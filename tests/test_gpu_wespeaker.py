"""-m gpu: WeSpeaker ResNet34 with masked pooling on the device (csrc/wespeaker.hip) against the fp64 oracle
(tests/wespeaker_oracle.py; third-party architecture restated from upstream, parity unpinned; recipe weights with the
calibrated BatchNorm statistics of tests/golden/wespeaker_calibration.json), and the embedder behind od_pipeline.
Embedding bar of the project: rel-L2 < 1e-4 and cosine distance < 1e-3 per row."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import pyannet_oracle as porc
import wespeaker_oracle as orc

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
SHAPES = [(1, 1), (1, 2), (2, 9), (3, 17), (2, 298), (1, 998)]
MASKED = [(2, 298, 3, 589), (1, 998, 3, 589), (3, 17, 2, 7), (1, 9, 1, 2)]


@pytest.fixture(scope="module")
def sd():
    return orc.calibrated_state_dict()


def _create(sd, mp, narrow):
    """a model created under TDX_WESPK_NARROW = narrow (the switch is read at create: one process holds both)"""
    from targetdiarization_amd.speaker import WeSpeakerResNet34
    mp.setenv("TDX_WESPK_NARROW", narrow)
    m = WeSpeakerResNet34(sd, dev)
    mp.delenv("TDX_WESPK_NARROW")
    return m


@pytest.fixture(scope="module")
def model(sd, monkeypatch_module):
    """the 13 narrow convolutions on conv3x3_narrow_kernel, whatever the default is"""
    return _create(sd, monkeypatch_module, "1")


@pytest.fixture(scope="module")
def shared(sd, monkeypatch_module):
    """the same weights with them on the shared core"""
    return _create(sd, monkeypatch_module, "0")


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def _ref(sd, B, F, masks=None):
    tr = orc.reference_trunk(orc.shape_feat(B, F), (B, F))
    return orc.head(sd, tr, None if masks is None else torch.from_numpy(masks), torch.float64).numpy()


def _check_rows(tag, out, ref):
    out, ref = np.asarray(out, dtype=np.float64).reshape(-1, 256), np.asarray(ref).reshape(-1, 256)
    for i, (o, r) in enumerate(zip(out, ref)):
        if np.isnan(r).all():
            print(f"{tag} row {i}: NaN row")
            assert np.isnan(o).all(), (tag, i)
            continue
        assert np.isfinite(r).all() and np.isfinite(o).all(), (tag, i)
        e, c = orc.rel_l2(o, r), orc.cos_dist(o, r)
        print(f"{tag} row {i}: rel-L2 {e:.3e} cosine distance {c:.3e}")
        assert e < orc.REL_BAR and c < orc.COS_BAR, (tag, i, e, c)


@pytest.mark.parametrize("which", ["narrow", "shared_core"])
@pytest.mark.parametrize("B,F", SHAPES)
def test_embed_features_vs_oracle(model, shared, sd, B, F, which):
    """(1,1): every stage one column wide; (1,2), (2,9): odd sizes through the three stride-2 stages; (3,17): the narrow
    kernel's tile edges inside a batch; (2,298): 47 680 rows cross 128-row tiles and batch boundaries; (1,998): the pipeline's"""
    out = (model if which == "narrow" else shared).embed_features(orc.shape_feat(B, F).to(dev))
    assert out.shape == (B, 256)
    _check_rows(f"{which} B={B} F={F}", out.cpu().numpy(), _ref(sd, B, F))


@pytest.mark.parametrize("B,F,S,Fw", MASKED)
def test_masked_pooling_vs_oracle(model, sd, B, F, S, Fw):
    """binary and fractional masks, an all-zero row and (Fw > T') a row that is non-zero on its own grid but vanishes at T';
    the S-mask call is bit-equal to S calls with one mask each and does not feel its NaN rows' neighbours"""
    feat = orc.shape_feat(B, F).to(dev)
    Tp = F
    for _ in range(3):
        Tp = (Tp - 1) // 2 + 1
    masks = orc.shape_masks(B, S, Fw, Tp)
    ref = _ref(sd, B, F, masks)
    nan_rows = np.isnan(ref).all(axis=-1)
    assert int(nan_rows.sum()) == (0 if S < 2 else (2 if S >= 3 and Fw > Tp else 1))
    assert masks[nan_rows].sum(axis=-1).tolist() == ([] if S < 2 else ([1.0, 0.0] if S >= 3 and Fw > Tp else [0.0]))
    w = torch.from_numpy(masks).to(dev)
    out = model.embed_features(feat, w)
    assert out.shape == (B, S, 256)
    _check_rows(f"B={B} F={F} S={S} Fw={Fw}", out.cpu().numpy(), ref)
    for s in range(S):
        one = model.embed_features(feat, w[:, s:s + 1].contiguous())
        assert torch.equal(one[:, 0].nan_to_num(nan=7.0), out[:, s].nan_to_num(nan=7.0)), s
    if nan_rows.any():
        w2 = w.clone()
        w2[torch.from_numpy(nan_rows).to(dev)] = 0.0                   # both NaN rows all-zero now: the finite rows must not move
        out2 = model.embed_features(feat, w2)
        assert torch.equal(out2.nan_to_num(nan=7.0), out.nan_to_num(nan=7.0))


def test_batch_independence(model, shared):
    feat = orc.shape_feat(3, 298).to(dev)
    for m in (model, shared):
        out = m.embed_features(feat)
        for b in range(3):
            assert torch.equal(m.embed_features(feat[b:b + 1])[0], out[b]), b


@pytest.mark.parametrize("B,F", [(2, 298), (1, 998)])
def test_narrow_against_shared_core(model, shared, sd, B, F):
    feat = orc.shape_feat(B, F).to(dev)
    a, b = model.embed_features(feat).cpu().numpy(), shared.embed_features(feat).cpu().numpy()
    ref = _ref(sd, B, F)
    _check_rows(f"narrow B={B} F={F}", a, ref)
    _check_rows(f"shared B={B} F={F}", b, ref)
    for i in range(B):
        d = orc.rel_l2(a[i], b[i])
        print(f"narrow vs shared core B={B} F={F} row {i}: rel-L2 {d:.3e}")
        assert d < 1e-5


def test_wave_to_embedding_vs_oracle(model, sd):
    waves = np.stack([porc.voice(24000, k, 31 + k) for k in range(3)]).astype(np.float32)
    feat = torch.stack([orc.features(torch.from_numpy(w).double()) for w in waves])
    ref = orc.forward(sd, feat).numpy()
    got_feat = model.fbank(torch.from_numpy(waves).to(dev))
    assert got_feat.shape == (3, 148, 80)
    print(f"Fbank('wespeaker') vs oracle features: max abs {float((got_feat.cpu().double() - feat).abs().max()):.3e}")
    _check_rows("wave", model(torch.from_numpy(waves).to(dev)).cpu().numpy(), ref)


def test_loader_and_arguments(sd, model):
    from targetdiarization_amd import _lib
    from targetdiarization_amd.speaker import WeSpeakerResNet34
    bad = dict(sd); bad.pop("resnet.layer3.0.shortcut.0.weight")
    with pytest.raises(_lib.TdxError, match="tensor missing or wrong shape: resnet.layer3.0.shortcut.0.weight"):
        WeSpeakerResNet34(bad, dev)
    bad = dict(sd); bad["resnet.not_a_parameter"] = torch.zeros(3)
    with pytest.raises(_lib.TdxError, match="unexpected tensor: resnet.not_a_parameter"):
        WeSpeakerResNet34(bad, dev)
    bad = dict(sd); bad["resnet.seg_1.weight"] = sd["resnet.seg_1.weight"].T.contiguous()
    with pytest.raises(_lib.TdxError, match="tensor missing or wrong shape: resnet.seg_1.weight"):
        WeSpeakerResNet34(bad, dev)
    withcount = dict(sd); withcount["resnet.bn1.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    WeSpeakerResNet34(withcount, dev).close()
    l = _lib.lib()
    assert model.workspace_bytes(1, 17, 1) > 0
    for B, F, S in ((0, 17, 1), (65, 17, 1), (1, 0, 1), (1, 17, 0), (1, 17, 9)):
        assert model.workspace_bytes(B, F, S) == 0, (B, F, S)
    assert model.flops(2, 998) == 2 * model.flops(1, 998) and 4.0e10 < model.flops(1, 998) < 5.5e10
    feat = torch.zeros(1, 17, 80, device=dev)
    w = torch.ones(1, 2, 7, device=dev)
    out = torch.full((1, 9, 256), 7.0, device=dev)
    buf = torch.empty(model.workspace_bytes(1, 17, 8), dtype=torch.uint8, device=dev)
    call = lambda B, F, wp, S, Fw, nbytes: l.tdx_wespk_forward(model._h, feat.data_ptr(), B, F, wp, S, Fw, out.data_ptr(), buf.data_ptr(), nbytes, None)
    for args in ((0, 17, w.data_ptr(), 2, 7), (65, 17, w.data_ptr(), 2, 7), (1, 0, w.data_ptr(), 2, 7), (1, 17, w.data_ptr(), 0, 7),
                 (1, 17, w.data_ptr(), 9, 7), (1, 17, w.data_ptr(), 2, 0), (1, 17, None, 2, 7)):
        assert call(*args, buf.numel()) == 1, args
        assert l.tdx_last_error()
    assert call(1, 17, w.data_ptr(), 2, 7, 15) == 4 and b"workspace too small" in l.tdx_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                       # nothing was launched
    m = WeSpeakerResNet34(sd, dev)
    m.close()
    with pytest.raises(_lib.TdxError):
        m.embed_features(feat)
    with pytest.raises(_lib.TdxError):
        WeSpeakerResNet34(sd, "cpu")


def test_end_to_end_tracks_equal_the_oracles(sd):
    from scipy.cluster.hierarchy import linkage
    from targetdiarization_amd import overlap
    from targetdiarization_amd.segmentation import PyanNet
    cal = orc.calibration()["e2e"]
    clip = porc.clip(12 * porc.SR, cal["seed"])
    seg_sd = porc.calibrated_state_dict()
    segment = lambda chunks: porc.forward(seg_sd, torch.from_numpy(chunks)).numpy()
    seen = {}
    embed_masked = lambda chunks, masks: seen.setdefault("E", orc.embed_masked(sd, chunks, masks))
    want = overlap.diarize(clip, segment, None, embed_masked=embed_masked)
    # the margin first: no merge of the oracle's centroid linkage lies within 1e-2 of the threshold
    starts, _ = overlap.chunk_plan(clip.shape[0])
    chunks = overlap.cut_chunks(clip, starts)
    seg = overlap.powerset_to_speakers(segment(chunks))
    emb, owner = overlap.masked_embeddings(chunks, seg, lambda c, m: seen["E"])
    train = np.array([seg[k, :, j].mean() >= 0.2 for k, j in owner], dtype=bool)
    heights = linkage(overlap._unit(emb[train]), method="centroid", metric="euclidean")[:, 2]
    gap = float(np.abs(heights - overlap.DEFAULT_THRESHOLD).min())
    print(f"merge heights {np.round(heights, 4).tolist()}, nearest to the threshold by {gap:.4f}")
    assert gap > cal["margin"] == 1e-2
    from targetdiarization_amd.speaker import WeSpeakerResNet34
    d = overlap.PyannoteDiarizer(PyanNet(seg_sd, dev), None, embedder=WeSpeakerResNet34(sd, dev))      # the default setting
    got = d(clip)
    d.close()
    print(f"12 s: {got}")
    assert got == want and len(got) >= 2


def test_wiring(sd, sd2):
    from targetdiarization_amd import overlap
    from targetdiarization_amd.speaker import WeSpeakerResNet34
    from targetdiarization_amd.target_diarization import TargetDiarization
    from targetdiarization_amd.weights import recipe_eres2netv2_state_dict
    spk = recipe_eres2netv2_state_dict(0)
    seg_sd = porc.calibrated_state_dict()
    td = TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk, od_state_dict=seg_sd, od_embed_state_dict=sd)
    assert isinstance(td.od_pipeline, overlap.PyannoteDiarizer) and isinstance(td.od_pipeline.embedder, WeSpeakerResNet34)
    td.od_pipeline.close()
    old = TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk, od_state_dict=seg_sd)
    assert old.od_pipeline.embedder is None and old.od_pipeline.embed == old.hp.spk.get_speaker_embeddings
    old.od_pipeline.close()
    alone = TargetDiarization(cuda_device=0, sep_state_dict=sd2, od_state_dict=seg_sd, od_embed_state_dict=sd)   # no `embed` needed any more
    assert isinstance(alone.od_pipeline.embedder, WeSpeakerResNet34) and alone.od_pipeline.embed is None
    alone.od_pipeline.close()
    mine = lambda audio: []
    assert TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk, od_state_dict=seg_sd, od_embed_state_dict=sd,
                             od_pipeline=mine).od_pipeline is mine


def test_two_threads_on_one_model(model):
    feat = [orc.shape_feat(3, 17).to(dev), orc.shape_feat(2, 298).to(dev)]
    w = [torch.from_numpy(orc.shape_masks(3, 2, 7, 3)).to(dev), torch.from_numpy(orc.shape_masks(2, 3, 589, 38)).to(dev)]
    want = [model.embed_features(f, m).cpu().numpy() for f, m in zip(feat, w)]
    got, errs = [[], []], []

    def worker(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream(dev)):
                for _ in range(4):
                    got[i].append(model.embed_features(feat[i], w[i]).cpu().numpy())
        except Exception as e:                           # noqa: BLE001
            errs.append(repr(e))
    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs, errs
    for i in range(2):
        assert len(got[i]) == 4 and all(np.array_equal(g, want[i], equal_nan=True) for g in got[i])


def test_graph_capture_replays_bit_equal(model):
    from targetdiarization_amd import _lib
    B, F, S, Fw = 1, 298, 3, 589
    feat = orc.shape_feat(B, F).to(dev)
    w = torch.from_numpy(orc.shape_masks(2, S, Fw, 38)[1:]).to(dev).contiguous()      # chunk 1's masks: no NaN row
    eager = model.embed_features(feat, w)
    l = _lib.lib()
    ws = torch.empty(model.workspace_bytes(B, F, S), dtype=torch.uint8, device=dev)
    out = torch.zeros(B, S, 256, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with model._guard.lock:
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            _lib.check(l.tdx_wespk_forward(model._h, feat.data_ptr(), B, F, w.data_ptr(), S, Fw, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                           C.c_void_p(side.cuda_stream)))
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                                 # a capture records, it does not run
    g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(eager).all() and torch.equal(out, eager)
