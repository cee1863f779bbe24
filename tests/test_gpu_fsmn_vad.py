"""-m gpu: FSMN-VAD on the device (csrc/fsmn_vad.hip, targetdiarization_amd/vad.py) against the fp64 oracle
(tests/fsmn_vad_oracle.py; third-party architecture restated from upstream, parity unpinned; recipe weights with the
calibrated CMVN and silence row).  Bars: the project's rel-L2 < 1e-4 on the posterior per clip; |p0 - oracle| below the bound
stored in tests/golden/fsmn_vad_calibration.json (10x the oracle's own fp32-vs-fp64 difference on the same clips); speech
ranges EQUAL to the segmenter run on the oracle's p0 (tests/test_fsmn_vad_host.py keeps every frame clear of the threshold)."""
import threading

import numpy as np
import pytest
import torch

import fsmn_vad_oracle as orc

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


def rel_l2(a, b):
    a = torch.as_tensor(np.asarray(a)).double().reshape(-1); b = torch.as_tensor(np.asarray(b)).double().reshape(-1)
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def cal():
    return orc.calibrated_state_dict()


@pytest.fixture(scope="module")
def model(cal):
    from targetdiarization_amd.vad import FsmnVad
    return FsmnVad(cal[0], cal[1], dev)


@pytest.fixture(scope="module")
def clips():
    return orc.posterior_clips()


@pytest.fixture(scope="module")
def lone(model, clips):
    """every posterior clip run alone: [(p0, post), ...]"""
    return [model.posteriors([c], with_post=True)[0] for c in clips]


@pytest.fixture(scope="module")
def ref(cal, clips):
    """fp64 oracle per clip: [(p0, post), ...] as numpy"""
    return [tuple(t.numpy() for t in orc.forward(cal[0], cal[1], c)) for c in clips]


def test_posteriors_vs_oracle(lone, ref):
    bound = orc.calibration()["p0_device_bound"]
    for T, (p0, post), (rp0, rpost) in zip(orc.POSTERIOR_FRAMES, lone, ref):
        assert p0.shape == (T,) and post.shape == (T, 248) and np.isfinite(post).all()
        assert (post >= 0).all() and np.abs(post.astype(np.float64).sum(axis=1) - 1.0).max() < 1e-5      # a softmax
        assert np.array_equal(post[:, 0], p0)
        r = rel_l2(post, rpost)
        rl = rel_l2(np.log(post.astype(np.float64)), np.log(rpost))                                     # logits up to the row's constant
        d = float(np.abs(p0.astype(np.float64) - rp0).max())
        print(f"T={T}: posterior rel-L2 {r:.3e}, log-posterior rel-L2 {rl:.3e}, max |p0 - oracle| {d:.3e} (bound {bound:.3e})")
        assert r < 1e-4 and rl < 1e-4, (T, r, rl)
        assert d <= bound, (T, d, bound)


def test_no_leak_across_clips(model, clips, lone):
    order = [5, 0, 7, 2, 4, 1, 6, 3]
    got = model.posteriors([clips[i] for i in order])
    for k, i in enumerate(order):
        r = rel_l2(got[k], lone[i][0])
        print(f"clip T={orc.POSTERIOR_FRAMES[i]} at position {k}: packed vs alone rel-L2 {r:.3e}, bit-equal {bool(np.array_equal(got[k], lone[i][0]))}")
        assert got[k].shape == lone[i][0].shape and r < 1e-5
    loud, silent = orc.leak_pair()
    alone = model.posteriors([silent])[0]
    pair = model.posteriors([loud, silent])
    r = rel_l2(pair[1][:19], alone[:19])
    print(f"silence behind a loud clip, first 19 frames: rel-L2 {r:.3e}")
    assert r < 1e-5 and rel_l2(pair[1], alone) < 1e-5
    assert rel_l2(pair[0], model.posteriors([loud])[0]) < 1e-5          # and LFR's right edge does not read the next clip


def test_edges(model, clips, lone, monkeypatch):
    p0_only = model.posteriors([clips[6]])[0]                            # post_dev = NULL
    assert np.array_equal(p0_only, lone[6][0])
    calls = []
    real = model.forward_into
    monkeypatch.setattr(model, "forward_into", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    short = np.zeros(399, np.float32)
    assert model(short) == [] and model.detect_batch([short, short[:0]]) == [[], []] and calls == []       # no frames: no launch
    mixed = model.posteriors([short, clips[4], short])                   # empty clips inside a batch
    assert calls == [1] and mixed[0].shape == (0,) and mixed[2].shape == (0,) and rel_l2(mixed[1], lone[4][0]) < 1e-5
    ws = [model.workspace_bytes(r) for r in (1, 2, 63, 64, 65, 128, 129, 1000, 180000)]
    assert ws[0] > 0 and all(a <= b for a, b in zip(ws, ws[1:])) and model.workspace_bytes(0) == 0
    for r in (1, 77, 300):
        assert model.flops(2 * r) == 2 * model.flops(r) > 0


def test_end_to_end_ranges_equal_the_oracle(model, cal):
    from targetdiarization_amd.vad import segments
    for clip in orc.e2e_clips():
        p0 = orc.forward(cal[0], cal[1], clip)[0].numpy()
        for sil in (0.0, 0.5, 0.8):
            want = [[round(p / 1000, 3) for p in seg] for seg in segments(p0, len(clip), int(sil * 1000))]
            got = model(clip, sil)
            print(f"min_silence_sec {sil}: {got}")
            assert got == want and len(got) >= 1
    both = model.detect_batch(orc.e2e_clips(), 0.5)
    assert both == [model(c, 0.5) for c in orc.e2e_clips()]


def test_wiring(model, cal, sd2):
    from targetdiarization_amd.asr_processor import ASRProcessor
    from targetdiarization_amd.diarization import CamppDiarizer
    from targetdiarization_amd.target_asr import TargetASR
    from targetdiarization_amd.target_diarization import TargetDiarization, _whole_clip_vad
    from targetdiarization_amd.vad import FsmnVad
    from targetdiarization_amd.weights import recipe_campplus_state_dict
    sd, cmvn = cal
    clip = orc.e2e_clips()[0]
    a = ASRProcessor(is_vad=True, vad_state_dict=sd, vad_cmvn=cmvn, verbose_log=False)
    assert a.is_vad and a.vad_detection(clip) == model(clip, 0.5)
    assert a.vad_detection(clip, min_silence_sec=0.0) == model(clip, 0.0)
    assert a.vad_detection(clip, format_to_sec=False) == model.detect_batch_ms([clip], 500)[0]
    td = TargetDiarization(cuda_device=0, sep_state_dict=sd2, vad_state_dict=sd, vad_cmvn=cmvn, sd_state_dict=recipe_campplus_state_dict(0))
    assert isinstance(td.vad, FsmnVad) and isinstance(td.sd_pipeline, CamppDiarizer) and td.sd_pipeline.vad is td.vad
    assert td.vad(clip) == model(clip, 0.5)
    assert TargetDiarization(cuda_device=0, sep_state_dict=sd2).vad is _whole_clip_vad
    mine = lambda audio: [[0.0, 1.0]]
    assert TargetDiarization(cuda_device=0, sep_state_dict=sd2, vad=mine, vad_state_dict=sd, vad_cmvn=cmvn).vad is mine
    t = TargetASR(cuda_device=0, vad_state_dict=sd, vad_cmvn=cmvn)
    assert isinstance(t.vad, FsmnVad) and t.vad(clip) == model(clip, 0.5)
    assert not isinstance(TargetASR(cuda_device=0).vad, FsmnVad)


def test_two_threads_on_one_model(model):
    jobs = [orc.e2e_clips()[0], orc.posterior_clips()[7]]
    want = [model.posteriors([c])[0] for c in jobs]
    got, errs = [[], []], []

    def worker(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream(dev)):
                for _ in range(4):
                    got[i].append(model.posteriors([jobs[i]])[0])
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


def test_graph_capture_replays_bit_equal(model, clips):
    feat, frames = model.features([clips[5], clips[2], clips[6]])
    rows = int(feat.shape[0])
    starts = torch.tensor([0] + list(np.cumsum(frames)), dtype=torch.int32, device=dev)
    ws = torch.empty(model.workspace_bytes(rows), dtype=torch.uint8, device=dev)
    eager, out = torch.empty(rows, device=dev), torch.zeros(rows, device=dev)
    with model._guard.call():
        model.forward_into(feat, starts, eager, None, ws)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with model._guard.lock:
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            model.forward_into(feat, starts, out, None, ws)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                                 # a capture records, it does not run
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
