"""-m gpu: PyanNet on the device (csrc/pyannet.hip, targetdiarization_amd/segmentation.py) and the overlap detector built on it
(overlap.PyannoteDiarizer) against the fp64 oracle (tests/pyannet_oracle.py; third-party architecture restated from upstream,
parity unpinned; recipe weights with the calibrated classifier).  Bars: the project's rel-L2 < 1e-4 on the log-probabilities
and on each tap, per shape; |logp - oracle| below the bound stored in tests/golden/pyannet_calibration.json (10x the oracle's
own fp32-vs-fp64 difference on the same clips); the argmax EQUAL to the oracle's wherever the oracle's top-2 margin is at
least 20x that bound; tracks EQUAL to overlap.diarize run on the oracle's log-probabilities
(tests/test_pyannet_host.py keeps every frame of the end-to-end clips clear of that margin)."""
import threading

import numpy as np
import pytest
import torch

import pyannet_oracle as orc

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


def rel_l2(a, b):
    a = torch.as_tensor(np.asarray(a)).double().reshape(-1); b = torch.as_tensor(np.asarray(b)).double().reshape(-1)
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def sd():
    return orc.calibrated_state_dict()


@pytest.fixture(scope="module")
def model(sd):
    from targetdiarization_amd.segmentation import PyanNet
    m = PyanNet(sd, dev)
    assert m.chunk_tile == orc.REC_TILE            # what the built kernel reports: SHAPES holds a full tile plus one chunk
    yield m
    m.close()


@pytest.fixture(scope="module")
def got(model):
    """the device on every posterior clip: [(logp, tap_sincnet, tap_lstm), ...] as numpy"""
    return [tuple(t.cpu().numpy() for t in model.log_probs(torch.from_numpy(c).to(dev), taps=True)) for c in orc.posterior_clips()]


def test_log_probs_and_taps_vs_oracle(model, got):
    bound = orc.calibration()["logp_device_bound"]
    for (B, T), c, (logp, ts, tl), (rlogp, rts, rtl) in zip(orc.SHAPES, orc.posterior_clips(), got, orc.reference()):
        F = orc.frames(T)
        assert model.frames(T) == F and logp.shape == (B, F, 7) and ts.shape == (B, F, 60) and tl.shape == (B, F, 256)
        assert np.isfinite(logp).all()
        r, d = rel_l2(logp, rlogp), float(np.abs(logp.astype(np.float64) - rlogp).max())
        lse = float(np.abs(np.log(np.exp(logp.astype(np.float64)).sum(axis=-1))).max())
        rs, rl = rel_l2(ts, rts), rel_l2(tl, rtl)
        print(f"B={B} T={T}: logp rel-L2 {r:.3e}, max abs {d:.3e} (bound {bound:.3e}), |logsumexp| {lse:.3e}, sincnet rel-L2 {rs:.3e}, lstm rel-L2 {rl:.3e}")
        assert r < 1e-4 and d <= bound and lse < 1e-5, (B, T, r, d, lse)
        assert rs < 1e-4 and rl < 1e-4, (B, T, rs, rl)
        plain = model.log_probs(torch.from_numpy(c).to(dev)).cpu().numpy()          # NULL taps
        assert np.array_equal(plain, logp)


def test_argmax_equals_the_oracle_where_the_margin_is_clear(got):
    floor = orc.MARGIN_FACTOR * orc.calibration()["logp_device_bound"]
    for (B, T), (logp, _, _), (rlogp, _, _) in zip(orc.SHAPES, got, orc.reference()):
        for b in range(B):
            clear = orc.margins(rlogp[b]) >= floor
            left_out = 1.0 - clear.mean()
            print(f"B={B} T={T} clip {b}: {int((~clear).sum())} of {clear.size} frames left out")
            assert left_out <= 0.05
            assert np.array_equal(logp[b].argmax(axis=-1)[clear], rlogp[b].argmax(axis=-1)[clear])


def test_batch_independence(sd, model, got):
    clips = [(i, b) for i, (B, T) in enumerate(orc.SHAPES) if T == 16000 for b in range(B)]          # four clips of T = 16000
    lone = [model.log_probs(torch.from_numpy(orc.posterior_clips()[i][b:b + 1]).to(dev)).cpu().numpy()[0] for i, b in clips]
    from targetdiarization_amd.segmentation import PyanNet
    small = PyanNet(sd, dev, max_chunks_per_launch=2)
    try:
        for m, order in ((model, [2, 0, 3, 1, 2]), (small, [3, 1, 0, 2, 1, 0, 3])):
            batch = np.stack([orc.posterior_clips()[clips[k][0]][clips[k][1]] for k in order])
            out = m.log_probs(torch.from_numpy(batch).to(dev)).cpu().numpy()
            for pos, k in enumerate(order):
                r = rel_l2(out[pos], lone[k])
                print(f"max_chunks_per_launch {m.max_chunks_per_launch}: clip {k} at position {pos}: rel-L2 {r:.3e}, bit-equal {bool(np.array_equal(out[pos], lone[k]))}")
                assert r < 1e-5
    finally:
        small.close()
    silent = np.zeros(16000, np.float32)
    loud = (30.0 * orc.posterior_clips()[1][0]).astype(np.float32)
    alone = model.log_probs(torch.from_numpy(silent[None]).to(dev)).cpu().numpy()[0]
    pair = model.log_probs(torch.from_numpy(np.stack([loud, silent, loud])).to(dev)).cpu().numpy()
    assert np.isfinite(alone).all() and np.array_equal(pair[1], alone)       # unchanged: no sum or over-read reaches a neighbour


def test_loader_and_arguments(sd, model):
    from targetdiarization_amd import _lib
    from targetdiarization_amd.segmentation import PyanNet
    bad = dict(sd); bad.pop("lstm.weight_hh_l2_reverse")
    with pytest.raises(_lib.TdxError, match="tensor missing or wrong shape: lstm.weight_hh_l2_reverse"):
        PyanNet(bad, dev)
    bad = dict(sd); bad["sincnet.not_a_parameter"] = torch.zeros(3)
    with pytest.raises(_lib.TdxError, match="unexpected tensor: sincnet.not_a_parameter"):
        PyanNet(bad, dev)
    bad = dict(sd); bad["sincnet.conv1d.1.weight"] = sd["sincnet.conv1d.1.weight"].transpose(0, 1).contiguous()
    with pytest.raises(_lib.TdxError, match="tensor missing or wrong shape: sincnet.conv1d.1.weight"):
        PyanNet(bad, dev)
    withbuf = dict(sd); withbuf["sincnet.conv1d.0.filterbank.n_"] = torch.zeros(1, 125); withbuf["sincnet.conv1d.0.filterbank.window_"] = torch.zeros(125)
    PyanNet(withbuf, dev).close()                                                  # the derived buffers are dropped before packing
    l = _lib.lib()
    assert [l.tdx_pyannet_frames(t) for t in (1260, 1261, 160000, 160001)] == [0, 2, 589, 0]
    assert model.workspace_bytes(1, 1260) == 0 and model.workspace_bytes(0, 16000) == 0 and model.workspace_bytes(1, 160001) == 0
    ws = [model.workspace_bytes(b, 16000) for b in (1, 2, 3, 8, 64)]
    wt = [model.workspace_bytes(2, t) for t in (1261, 8000, 16000, 48000, 160000)]
    assert ws[0] > 0 and all(a <= b for a, b in zip(ws, ws[1:])) and wt[0] > 0 and all(a <= b for a, b in zip(wt, wt[1:]))
    for b, t in ((1, 1261), (3, 16000), (5, 160000)):
        assert model.flops(2 * b, t) == 2 * model.flops(b, t) > 0
    # bad shapes and a short workspace are status codes, and nothing is launched: the poisoned output stays as it is
    x = torch.zeros(1, 16000, device=dev)
    out = torch.full((1, orc.frames(16000), 7), 7.0, device=dev)
    buf = torch.empty(model.workspace_bytes(1, 16000), dtype=torch.uint8, device=dev)
    call = lambda T, nbytes: l.tdx_pyannet_forward(model._h, x.data_ptr(), 1, T, out.data_ptr(), None, None, buf.data_ptr(), nbytes, None)
    assert call(1260, buf.numel()) == 1 and b"T must be in" in l.tdx_last_error()
    assert call(160001, buf.numel()) == 1
    assert call(16000, buf.numel() - 1) == 4 and b"workspace too small" in l.tdx_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(_lib.TdxError):
        model.log_probs(torch.zeros(1, 1000, device=dev))
    with pytest.raises(_lib.TdxError):
        PyanNet(sd, "cpu")


def test_end_to_end_tracks_equal_the_oracle(sd, model):
    from targetdiarization_amd import overlap
    d = overlap.PyannoteDiarizer(model, orc.band_energy_embed)
    for clip in orc.e2e_clips():
        want = overlap.diarize(clip, lambda chunks: orc.forward(sd, chunks).numpy(), orc.band_energy_embed)
        got = d(clip)
        print(f"{len(clip) / 16000:.0f} s: {got}")
        assert got == want and len(got) >= 2


def test_wiring(sd, model, sd2, monkeypatch):
    from targetdiarization_amd import overlap
    from targetdiarization_amd.target_diarization import TargetDiarization
    from targetdiarization_amd.target_diarization_stream import TargetDiarizationStream
    from targetdiarization_amd.weights import recipe_eres2netv2_state_dict
    spk = recipe_eres2netv2_state_dict(0)
    td = TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk, od_state_dict=sd)
    od = td.od_pipeline
    assert isinstance(od, overlap.PyannoteDiarizer) and od.embed == td.hp.spk.get_speaker_embeddings
    assert od.threshold == overlap.DEFAULT_THRESHOLD
    mine = lambda audio: []
    assert TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk, od_state_dict=sd, od_pipeline=mine).od_pipeline is mine
    assert TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk).od_pipeline is None
    stub = TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk, od_state_dict=sd, od_embed=orc.band_energy_embed,
                             pyannote_clustering_threshold=0.5)
    assert stub.od_pipeline.embed is orc.band_energy_embed and stub.od_pipeline.threshold == 0.5
    seen = []
    real = overlap.cluster_embeddings
    monkeypatch.setattr(overlap, "cluster_embeddings", lambda X, threshold, msz: (seen.append(threshold), real(X, threshold, msz))[1])
    clip = orc.e2e_clips()[0]
    tracks = stub.od_pipeline(clip)
    monkeypatch.undo()
    assert seen == [0.5] and tracks == overlap.diarize(clip, od.segment, orc.band_energy_embed, 0.5)
    target_spk, result, audio = td.infer(clip)                                     # 12 s, two voices at a time in places
    assert isinstance(target_spk, str) and isinstance(result, list) and result
    for r in result:
        assert set(r) >= {"speaker", "timerange", "text", "type", "score"} and r["type"] in ("single", "overlap")
    s = TargetDiarizationStream(cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk, od_state_dict=sd, od_embed=orc.band_energy_embed)
    assert isinstance(s.od_pipeline, overlap.PyannoteDiarizer)
    calls = []
    seg = s.od_pipeline.segment
    s.od_pipeline.segment = lambda chunks: (calls.append(chunks.shape), seg(chunks))[1]
    sess = s.session()
    for n in (1, 2):                                                               # the first buffer defines the target, the second may be an overlap
        out = list(sess.process_single_chunk(orc.e2e_clips()[1], is_single=False))
        assert calls == [(1, 160000)] * n and len(out) <= 1
        for r in out:
            assert r["type"] in ("single", "overlap")


def test_two_threads_on_one_model(model):
    jobs = [torch.from_numpy(orc.posterior_clips()[2]).to(dev), torch.from_numpy(orc.posterior_clips()[4]).to(dev)]
    want = [model.log_probs(j).cpu().numpy() for j in jobs]
    got, errs = [[], []], []

    def worker(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream(dev)):
                for _ in range(4):
                    got[i].append(model.log_probs(jobs[i]).cpu().numpy())
        except Exception as e:                           # noqa: BLE001
            errs.append(repr(e))
    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs, errs
    for i in range(2):
        assert len(got[i]) == 4 and all(np.array_equal(g, want[i]) for g in got[i])


def test_graph_capture_replays_bit_equal(model):
    x = torch.from_numpy(orc.posterior_clips()[2]).to(dev)                          # B = 3: a full tile and a one-chunk tile
    B, T = x.shape
    ws = torch.empty(model.workspace_bytes(B, T), dtype=torch.uint8, device=dev)
    eager, out = torch.empty(B, orc.frames(T), 7, device=dev), torch.zeros(B, orc.frames(T), 7, device=dev)
    with model._guard.call():
        model.forward_into(x, eager, None, None, ws)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with model._guard.lock:
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            model.forward_into(x, out, None, None, ws)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                                 # a capture records, it does not run
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
