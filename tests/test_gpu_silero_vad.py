"""-m gpu: silero-VAD on the device (csrc/silero_vad.hip, targetdiarization_amd/silero.py) against the fp64 oracle
(tests/silero_vad_oracle.py; third-party architecture restated from upstream, parity unpinned; recipe weights with the
calibrated head).  Bars: the project's rel-L2 < 1e-4 per clip on p, on the logit recovered from p, on the encoder output and
on the LSTM h; |p - oracle| below the bound stored in tests/golden/silero_vad_calibration.json (10x the oracle's own
fp32-vs-fp64 difference on the same clips); timestamps EQUAL to the state machine run on the oracle's p
(tests/test_silero_vad_host.py keeps every chunk clear of both thresholds)."""
import threading

import numpy as np
import pytest
import torch

import silero_vad_oracle as orc

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
W = 512


def rel_l2(a, b):
    a = torch.as_tensor(np.asarray(a)).double().reshape(-1); b = torch.as_tensor(np.asarray(b)).double().reshape(-1)
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def sd():
    return orc.calibrated_state_dict()


@pytest.fixture(scope="module")
def model(sd):
    from targetdiarization_amd.silero import SileroVad
    return SileroVad(sd, dev)


@pytest.fixture(scope="module")
def clips():
    return orc.prob_clips()


@pytest.fixture(scope="module")
def lone(model, clips):
    """every probability clip run alone: [(p, feat, h), ...]"""
    return [model.probabilities([c], taps=True)[0] for c in clips]


@pytest.fixture(scope="module")
def ref(sd, clips):
    """fp64 oracle per clip: [(p, feat, h), ...] as numpy"""
    return [tuple(t.numpy() for t in orc.forward(sd, c)) for c in clips]


def test_probabilities_vs_oracle(lone, ref):
    bound = orc.calibration()["p_device_bound"]
    logit = lambda p: np.log(p / (1.0 - p))
    for n, N, (p, feat, h), (rp, rfeat, rh) in zip(orc.PROB_SAMPLES, (1, 1, 1, 2, 2, 4, 33, 313), lone, ref):
        assert p.shape == (N,) and feat.shape == (N, 128) and h.shape == (N, 128)
        assert np.isfinite(p).all() and np.isfinite(feat).all() and np.isfinite(h).all() and (feat >= 0).all()
        r = rel_l2(p, rp)
        rl = rel_l2(logit(p.astype(np.float64)), logit(rp))
        rf, rh_ = rel_l2(feat, rfeat), rel_l2(h, rh)
        d = float(np.abs(p.astype(np.float64) - rp).max())
        print(f"n={n} ({N} chunks): p rel-L2 {r:.3e}, logit rel-L2 {rl:.3e}, encoder rel-L2 {rf:.3e}, h rel-L2 {rh_:.3e}, "
              f"max |p - oracle| {d:.3e} (bound {bound:.3e})")
        assert r < 1e-4 and rl < 1e-4 and rf < 1e-4 and rh_ < 1e-4, (n, r, rl, rf, rh_)
        assert d <= bound, (n, d, bound)


@pytest.mark.parametrize("order", [[6], [7, 3], [5, 0, 6], [5, 0, 7, 2, 4, 1, 6, 3, 5]], ids=["1", "2", "3", "9"])
def test_packed_batch_equals_lone_runs(model, clips, lone, order):
    got = model.probabilities([clips[i] for i in order])
    for k, i in enumerate(order):
        r = rel_l2(got[k], lone[i][0])
        print(f"clip n={orc.PROB_SAMPLES[i]} at position {k} of {len(order)}: packed vs alone rel-L2 {r:.3e}, bit-equal {bool(np.array_equal(got[k], lone[i][0]))}")
        assert got[k].shape == lone[i][0].shape and r < 1e-5


def test_no_leak_across_clips(model):
    loud, silent = orc.leak_pair()
    alone = model.probabilities([silent])[0]
    pair = model.probabilities([loud, silent])
    print(f"silence behind a loud clip: max |packed - alone| {float(np.abs(pair[1] - alone).max()):.3e}")
    assert np.array_equal(pair[1], alone)                      # neither the 64 samples of context nor (h, c) cross the boundary
    assert np.array_equal(pair[0], model.probabilities([loud])[0])


@pytest.mark.parametrize("k", [0, 1, 5])
def test_causal_and_reflect_pad_reads_no_later_chunk(model, k):
    a, b = orc.causal_pair(k)
    pa, pb = model.probabilities([a])[0], model.probabilities([b])[0]
    assert np.array_equal(pa[:k + 1], pb[:k + 1])              # bit-equal: chunk k's right pad is its own mirrored tail
    assert not np.array_equal(pa[k + 1:], pb[k + 1:])


def test_edges(model, clips, lone, monkeypatch):
    p_only = model.probabilities([clips[6]])[0]                # taps NULL
    assert np.array_equal(p_only, lone[6][0])
    calls = []
    real = model.forward_into
    monkeypatch.setattr(model, "forward_into", lambda *a, **k: (calls.append(int(a[1].shape[0]) - 1), real(*a, **k))[1])
    none = np.zeros(0, np.float32)
    assert model(none) == [] and model.frames(none) == [] and model.timestamps_batch([none, none]) == [[], []] and calls == []
    taps = model.probabilities([none], taps=True)[0]
    assert taps[0].shape == (0,) and taps[1].shape == (0, 128) and taps[2].shape == (0, 128) and calls == []
    mixed = model.probabilities([none, clips[5], none, clips[3]])
    assert calls == [2] and mixed[0].shape == (0,) and mixed[2].shape == (0,)          # ONE forward, over the two live clips
    assert np.array_equal(mixed[1], lone[5][0]) and np.array_equal(mixed[3], lone[3][0])
    ws = [model.workspace_bytes(1, n) for n in (1, 2, 63, 64, 65, 313, 938, 1 << 20)]
    assert ws[0] > 0 and all(a <= b for a, b in zip(ws, ws[1:]))
    assert model.workspace_bytes(9, 9) > 0 and model.workspace_bytes(1024, 1024) > 0
    for nclips, total in ((0, 10), (1, 0), (3, 2), (1025, 2000), (1, (1 << 20) + 1), (-1, 5)):
        assert model.workspace_bytes(nclips, total) == 0, (nclips, total)
    for n in (1, 33, 313):
        assert model.flops(2 * n) == 2 * model.flops(n) > 0
    from targetdiarization_amd import _lib
    x = torch.zeros(2 * W, device=dev); st = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev); p = torch.empty(2, device=dev)
    small = torch.empty(64, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.TdxError):
        real(x, st, p, None, None, small)                      # workspace too small: refused before any launch


def test_end_to_end_timestamps_equal_the_oracle(model, sd):
    from targetdiarization_amd.silero import speech_timestamps
    for clip in orc.e2e_clips():
        rp = orc.forward(sd, clip)[0].numpy()
        assert model(clip) == speech_timestamps(rp, len(clip), min_silence_duration_ms=100, return_seconds=True)
        assert model.frames(clip) == speech_timestamps(rp, len(clip), min_silence_duration_ms=100)
        for sil in (0, 100, 500):
            want = speech_timestamps(rp, len(clip), min_silence_duration_ms=sil)
            got = model.timestamps_batch([clip], min_silence_duration_ms=sil)[0]
            print(f"min_silence_duration_ms {sil}: {got}")
            assert got == want and len(got) >= 1
    both = model.timestamps_batch(orc.e2e_clips(), return_seconds=True)
    assert both == [model(c) for c in orc.e2e_clips()] and both[1][-1][1] == round(len(orc.e2e_clips()[1]) / 16000, 1)


def test_wiring(model, sd, sd2, tmp_path, capsys):
    from safetensors.torch import save_file
    from targetdiarization_amd.audio_processor import AudioProcessor
    from targetdiarization_amd.silero import SileroVad
    from targetdiarization_amd.target_diarization import _whole_clip_vad
    from targetdiarization_amd.target_diarization_stream import TargetDiarizationStream
    clip = orc.e2e_clips()[0]
    frames = model.frames(clip)
    assert len(frames) == 2
    ap = AudioProcessor(is_separate_audio=True, separater_state_dict=sd2, cuda_device=0, verbose_log=False, silero_state_dict=sd)
    plug = AudioProcessor(is_separate_audio=True, separater_state_dict=sd2, cuda_device=0, verbose_log=False, silero_vad=model.frames)
    assert ap.silero_vad(clip) == frames
    got, want = ap.separate_speaker(clip, 16000, low_gpu_ram=True), plug.separate_speaker(clip, 16000, low_gpu_ram=True)
    assert len(got[0]) > 0 and all(np.array_equal(g, w) for g, w in zip(got, want))
    mine = lambda a: [[0, 100]]
    assert AudioProcessor(verbose_log=False, silero_vad=mine, silero_state_dict=sd).silero_vad is mine
    assert AudioProcessor(verbose_log=False).silero_vad is None
    path = str(tmp_path / "silero_vad.safetensors")
    save_file({"_model." + k: v for k, v in sd.items()}, path)
    assert AudioProcessor(verbose_log=False, silero_model_file=path).silero_vad(clip) == frames
    capsys.readouterr()
    assert AudioProcessor(verbose_log=False, silero_model_file=str(tmp_path / "absent.jit")).silero_vad is None
    assert "Failed to load silero VAD model" in capsys.readouterr().out
    td = TargetDiarizationStream(cuda_device=0, sep_state_dict=sd2, silero_state_dict=sd)
    assert isinstance(td.stream_vad, SileroVad) and td.session().stream_vad is td.stream_vad
    assert td.stream_vad(clip) == model(clip)
    mine_s = lambda a: [[0.0, 1.0]]
    assert TargetDiarizationStream(cuda_device=0, sep_state_dict=sd2, stream_vad=mine_s, silero_state_dict=sd).stream_vad is mine_s
    assert TargetDiarizationStream(cuda_device=0, sep_state_dict=sd2).stream_vad is _whole_clip_vad
    bad = dict(sd); bad.pop("decoder.rnn.bias_hh")
    capsys.readouterr()
    assert TargetDiarizationStream(cuda_device=0, sep_state_dict=sd2, silero_state_dict=bad).stream_vad is _whole_clip_vad
    assert "Failed to load silero VAD model" in capsys.readouterr().out


def test_two_threads_on_one_model(model):
    jobs = [orc.e2e_clips()[0], orc.prob_clips()[7]]
    want = [model.probabilities([c])[0] for c in jobs]
    got, errs = [[], []], []

    def worker(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream(dev)):
                for _ in range(4):
                    got[i].append(model.probabilities([jobs[i]])[0])
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
    parts = [clips[5], clips[2], clips[6]]
    chunks = [(len(c) + W - 1) // W for c in parts]
    total = sum(chunks)
    packed = np.zeros(total * W, np.float32)
    starts = np.concatenate([[0], np.cumsum(chunks)]).astype(np.int32)
    for c, a in zip(parts, starts):
        packed[a * W:a * W + len(c)] = c
    wav, st = torch.from_numpy(packed).to(dev), torch.from_numpy(starts).to(dev)
    ws = torch.empty(model.workspace_bytes(len(parts), total), dtype=torch.uint8, device=dev)
    eager, out = torch.empty(total, device=dev), torch.zeros(total, device=dev)
    with model._guard.call():
        model.forward_into(wav, st, eager, None, None, ws)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with model._guard.lock:
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            model.forward_into(wav, st, out, None, None, ws)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                                 # a capture records, it does not run
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
