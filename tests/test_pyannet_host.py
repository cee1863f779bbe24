"""CPU tests of the PyanNet stage: the frame arithmetic, the sinc filters, the calibration of the recipe weights
(tests/golden/pyannet_calibration.json, tools/make_goldens_pyannet.py) and the host pipeline of overlap.py — its pure
functions on hand-worked cases, and end to end on a synthetic truth with a stub segmenter and a stub embedder."""
import os
import sys

import numpy as np
import pytest
import torch

import pyannet_oracle as orc
from targetdiarization_amd import overlap
from targetdiarization_amd.weights import pack_pyannet_blob, pyannet_param_shapes, recipe_pyannet_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_table():
    table = {160000: 589, 48000: 175, 16000: 56, 8000: 26, 1261: 2}
    for T, F in table.items():
        assert orc.frames(T) == F
    sd = recipe_pyannet_state_dict(0)
    assert orc.frames(1260) == 0 and orc.frames(160001) == 0
    assert orc.forward(sd, np.zeros(1261, np.float32)).shape == (1, 2, 7) and orc.forward(sd, np.zeros(8000, np.float32)).shape == (1, 26, 7)
    assert overlap.FRAMES == orc.frames(overlap.CHUNK) and overlap.FRAME_STEP == 10 * 3 * 3 * 3


def test_shapes_follow_the_built_kernels_chunk_tile():
    """the device test's "full tile plus one chunk" shape is derived from the tile the library was compiled with"""
    from targetdiarization_amd import _lib
    tile = _lib.lib().tdx_pyannet_chunk_tile()
    assert tile == orc.REC_TILE and (tile + 1, 8000) in orc.SHAPES


def test_sinc_filters():
    sd = recipe_pyannet_state_dict(0)
    f = orc.sinc_filters(sd["sincnet.conv1d.0.filterbank.low_hz_"], sd["sincnet.conv1d.0.filterbank.band_hz_"]).numpy()
    assert f.shape == (80, 251) and f.dtype == np.float64
    cos, sin = f[:40], f[40:]
    assert np.array_equal(cos, cos[:, ::-1]) and np.allclose(cos[:, 125], 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(sin, -sin[:, ::-1]) and np.array_equal(sin[:, 125], np.zeros(40))
    # a cosine filter passes its band's centre frequency and its sine partner is the same band in quadrature
    low = 50.0 + np.abs(sd["sincnet.conv1d.0.filterbank.low_hz_"].numpy().reshape(-1))
    band = 50.0 + np.abs(sd["sincnet.conv1d.0.filterbank.band_hz_"].numpy().reshape(-1))
    t = np.arange(-125, 126) / 16000.0
    for k in (0, 13, 39):
        fc = low[k] + band[k] / 2
        inside, outside = abs(cos[k] @ np.cos(2 * np.pi * fc * t)), abs(cos[k] @ np.cos(2 * np.pi * (fc + 3 * band[k] + 400) * t))
        assert inside > 10 * outside
        assert abs(sin[k] @ np.sin(2 * np.pi * fc * t)) == pytest.approx(inside, rel=0.05) and abs(sin[k] @ np.cos(2 * np.pi * fc * t)) < 1e-9
    assert (np.diff(low) > 0).all()


def test_recipe_and_packer():
    sd = recipe_pyannet_state_dict(0)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(pyannet_param_shapes())
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), recipe_pyannet_state_dict(0).values()))
    extra = dict(sd); extra["sincnet.conv1d.0.filterbank.n_"] = torch.zeros(1, 125); extra["sincnet.conv1d.0.filterbank.window_"] = torch.zeros(125)
    assert pack_pyannet_blob(extra) == pack_pyannet_blob(sd)


@pytest.fixture(scope="module")
def cal():
    return orc.calibration()


def test_calibration_is_reproducible_and_spreads_the_classes(cal):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_goldens_pyannet as tool
    finally:
        sys.path.pop(0)
    again = tool.calibrate(cal["seed"])
    for k, v in again.items():
        if "fp32_vs_fp64" in k or k == "logp_device_bound":       # rounding residue: it depends on the host's fp32 kernels and threads;
            tol = cal["fp32_residue_tolerance_factor"]            # the golden file itself says how far a rerun may be off
            assert tol == tool.FP32_RESIDUE_TOLERANCE and v / tol < cal[k] < tol * v, k
        else:
            assert cal[k] == pytest.approx(v, rel=1e-6), k
    assert cal["logp_device_bound"] == pytest.approx(10.0 * cal["logp_fp32_vs_fp64_max_abs"], rel=1e-12)
    assert cal["pre_gain_logit_std"] >= 0.05
    floor = orc.MARGIN_FACTOR * cal["logp_device_bound"]
    seen = np.zeros(7, dtype=np.int64)
    for (B, T), (logp, _, _) in zip(orc.SHAPES, orc.reference()):
        seen += np.bincount(logp.argmax(axis=-1).reshape(-1), minlength=7)
        for b in range(B):
            below = float((orc.margins(logp[b]) < floor).mean())
            print(f"B={B} T={T} clip {b}: {below:.4f} of the frames below the margin {floor:.3e}")
            assert below <= 0.05
    assert (seen > 0).all(), seen


def test_end_to_end_clips_are_clear_of_the_margin(cal):
    sd = orc.calibrated_state_dict()
    floor = orc.MARGIN_FACTOR * cal["logp_device_bound"]
    for clip, n in zip(orc.e2e_clips(), (12 * 16000, 4 * 16000)):
        assert clip.shape == (n,)
        starts, _ = overlap.chunk_plan(n)
        m = orc.margins(orc.forward(sd, overlap.cut_chunks(clip, starts)).numpy())
        print(f"{n // 16000} s: {m.shape[0]} chunks, smallest top-2 margin {m.min():.3e} (floor {floor:.3e})")
        assert m.min() >= floor


# ---- host pipeline: pure functions ---------------------------------------------------------------------------------------
def test_chunk_plan():
    want = {1: [0], 159999: [0], 160000: [0], 160001: [0, 16000], 176000: [0, 16000], 176001: [0, 16000, 32000],
            480000: list(range(0, 320001, 16000))}
    for n, starts in want.items():
        got, total = overlap.chunk_plan(n)
        assert got == starts and total == int(round(starts[-1] / 270)) + 589
        assert starts[-1] + overlap.CHUNK >= n                                       # every sample is inside a chunk
    x = overlap.cut_chunks(np.arange(160001, dtype=np.float32), [0, 16000])
    assert x.shape == (2, 160000) and x[1, 0] == 16000 and x[1, 144000] == 160000 and not x[1, 144001:].any()


def test_powerset_map():
    logp = np.full((1, 7, 7), -5.0)
    logp[0, np.arange(7), np.arange(7)] = -0.1
    assert overlap.powerset_to_speakers(logp)[0].tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1]]


def test_speaker_count_by_hand():
    """three chunks of 4 frames at global offsets 0, 2, 4 (starts 0, 540, 1080 samples)"""
    seg = np.zeros((3, 4, 3), dtype=np.int8)
    seg[0, :, 0] = 1                      # chunk 0: one speaker on all 4 frames
    seg[1, :, 0] = 1; seg[1, 2:, 1] = 1   # chunk 1: two speakers on its last 2 frames
    seg[2, 0, :2] = 1                     # chunk 2: two speakers on its first frame, then nobody
    count = overlap.speaker_count(seg, [0, 540, 1080], 9)
    #  frame      0  1  2          3          4              5              6  7  8
    #  mean       1  1  (1+1)/2    (1+1)/2    (2+2)/2        (2+0)/2        0  0  -
    assert count.tolist() == [1, 1, 1, 1, 2, 1, 0, 0, 0]
    assert overlap.speaker_count(np.ones((1, 4, 3), np.int8)[:, :, :2] * 1, [0], 4).tolist() == [2, 2, 2, 2]
    # rint rounds a half to even: one chunk hears 1, the other 2 -> 1.5 -> 2; 0 and 1 -> 0.5 -> 0
    seg = np.zeros((2, 2, 3), dtype=np.int8); seg[0, :, 0] = 1; seg[1, 0, :2] = 1; seg[1, 1, :] = 0; seg[0, 1, 0] = 0; seg[1, 1, 0] = 1
    assert overlap.speaker_count(seg, [0, 0], 2).tolist() == [2, 0]


def _blob(centre, n, rng, noise=0.02):
    return overlap._unit(centre + noise * rng.standard_normal((n, len(centre))))


def test_clustering_rules():
    rng = np.random.default_rng(5)
    e = np.eye(8)
    # the adaptive minimum: 30 embeddings -> min(12, round(3)) = 3; a pair far from both blobs rejoins the nearest large cluster
    X = np.concatenate([_blob(e[0], 15, rng), _blob(e[1], 13, rng), _blob(overlap._unit(0.8 * e[1] + 0.6 * e[2]), 2, rng)])
    labels, cen = overlap.cluster_embeddings(X, threshold=0.5)
    assert cen.shape == (2, 8) and len(set(labels[:15])) == 1 and len(set(labels[15:])) == 1 and labels[0] != labels[15]
    # with 10 embeddings the minimum is 1: the far pair stays a cluster of its own
    X = np.concatenate([_blob(e[0], 4, rng), _blob(e[1], 4, rng), _blob(e[2], 2, rng)])
    labels, cen = overlap.cluster_embeddings(X, threshold=0.5)
    assert cen.shape == (3, 8) and labels[8] == labels[9] and len({labels[0], labels[4], labels[8]}) == 3
    # 200 embeddings: the minimum is capped at 12; a blob of 11 is dissolved, one of 12 stays
    X = np.concatenate([_blob(e[0], 177, rng), _blob(e[1], 12, rng), _blob(overlap._unit(0.9 * e[0] + 0.44 * e[3]), 11, rng)])
    labels, cen = overlap.cluster_embeddings(X, threshold=0.3)
    assert cen.shape == (2, 8) and len(set(labels[177:189])) == 1 and labels[177] != labels[0] and (labels[189:] == labels[0]).all()
    # no large cluster: one cluster (threshold so small that every point is alone, minimum 2)
    labels, cen = overlap.cluster_embeddings(_blob(e[0], 20, rng, noise=0.2), threshold=1e-6)
    assert cen.shape == (1, 8) and not labels.any()
    # a single embedding is one cluster
    labels, cen = overlap.cluster_embeddings(e[3:4] * 7.0, threshold=0.5)
    assert labels.tolist() == [0] and np.allclose(cen, e[3:4])


def test_assignment_of_missing_and_inactive_speakers():
    """2 chunks of 589 frames at 0 and 1 s; speakers A (slot 0 / slot 1) and B (slot 1 / slot 0) have embeddings; in chunk 1
    slot 2 is a short burst (0.3 s: no embedding) on frames where chunk 0 hears B alone; slot 2 of chunk 0 is never active"""
    seg = np.zeros((2, 589, 3), dtype=np.int8)
    off = overlap.frame_offset(16000)
    seg[0, 0:200, 0] = 1; seg[0, 300:500, 1] = 1
    seg[1, 0:200 - off, 1] = 1; seg[1, 300 - off:330 - off, 0] = 1; seg[1, 350 - off:500 - off, 0] = 1
    seg[1, 332 - off:348 - off, 2] = 1                                                 # 16 frames = 0.27 s: missing
    seg[0, 332:348, 1] = 1
    chunks = np.zeros((2, 160000), np.float32)
    clips, owner = overlap.gather_clips(chunks, seg)
    assert owner == [(0, 0), (0, 1), (1, 0), (1, 1)]
    a, b = np.eye(4)[0], np.eye(4)[1]
    emb = np.stack([a, b, b, a])
    out = overlap.assign_speakers(seg, [0, 16000], off + 589, emb, owner, threshold=0.5)
    assert out[0, 2] == -1                                                             # never active: no cluster
    assert out[0, 0] == out[1, 1] and out[0, 1] == out[1, 0] and out[0, 0] != out[0, 1]
    assert out[1, 2] == out[0, 1]                                                      # the missing one joins what the other chunk hears there
    # nothing has an embedding: every active speaker is cluster 0
    out = overlap.assign_speakers(seg, [0, 16000], off + 589, np.zeros((0, 4)), [], threshold=0.5)
    assert out.tolist() == [[0, 0, -1], [0, 0, 0]]
    # embeddings, but no speaker reaches 20 % of its chunk: nothing to train on, one cluster
    short = np.zeros((1, 589, 3), dtype=np.int8); short[0, 0:60, 0] = 1; short[0, 100:160, 1] = 1
    assert overlap.assign_speakers(short, [0], 589, np.stack([a, b]), [(0, 0), (0, 1)], threshold=0.5).tolist() == [[0, 0, -1]]


def test_model_dir_sources(tmp_path, capsys):
    """od_model_dir: pytorch_model.bin bare or under "state_dict"; whatever goes wrong with a directory prints and leaves None"""
    sd = recipe_pyannet_state_dict(0)
    assert overlap.load_model_dir("pyannote/speaker-diarization-3.1") is None and overlap.load_model_dir(str(tmp_path)) is None
    assert overlap.build_od_pipeline(None, "pyannote/speaker-diarization-3.1", embed=len) is None
    assert overlap.build_od_pipeline(None, str(tmp_path), embed=len) is None and capsys.readouterr().out == ""
    for name, obj in (("bare", sd), ("wrapped", {"state_dict": sd, "epoch": 3})):
        d = tmp_path / name
        d.mkdir()
        torch.save(obj, str(d / "pytorch_model.bin"))
        got = overlap.load_model_dir(str(d))
        assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    # an unreadable file; a checkpoint whose names the loader rejects; no embedder to share
    junk = tmp_path / "junk"; junk.mkdir(); (junk / "pytorch_model.bin").write_bytes(b"not a checkpoint")
    wrong = tmp_path / "wrong"; wrong.mkdir(); torch.save({"lstm.weight_ih_l0": torch.zeros(512, 60)}, str(wrong / "pytorch_model.bin"))
    for d, embed in ((junk, len), (wrong, len), (tmp_path / "bare", None)):
        assert overlap.build_od_pipeline(None, str(d), embed=embed) is None
        assert f"Failed to load the overlap detector from {d}" in capsys.readouterr().out
    with pytest.raises(ValueError):                                                    # weights handed in directly fail loudly
        overlap.build_od_pipeline(sd, None, embed=None)


# ---- host pipeline end to end on a synthetic truth -----------------------------------------------------------------------
TRUTH_40S = {0: [(1.0, 9.0), (20.0, 27.0)], 1: [(7.5, 15.0), (25.0, 33.0)], 2: [(16.0, 19.0), (34.5, 39.0)]}     # 0 and 1 overlap twice


def _stubs(truth, n, seed=3, dim=16):
    """segment: the truth rasterised at the frame centres, the local slots permuted differently in every chunk; embed: a fixed
    unit vector per true speaker plus small seeded noise (the clip's speaker is read back from a watermark in the samples)"""
    starts, _ = overlap.chunk_plan(n)
    wave = np.zeros(n, np.float32)
    for spk, ranges in truth.items():                       # the samples name their speakers: bit `spk` of the value
        for a, b in ranges:
            wave[int(a * 16000):int(b * 16000)] += 2.0 ** spk
    centres = (np.arange(589) * 270 + 991 / 2.0)

    def segment(chunks):
        assert chunks.shape == (len(starts), 160000)
        out = np.full((len(starts), 589, 7), -10.0)
        for k, s in enumerate(starts):
            perm = np.random.default_rng([seed, k]).permutation(3)
            t = (overlap.frame_offset(s) * 270 + centres) / 16000.0          # frame centres on the global grid
            act = np.zeros((589, 3), dtype=np.int8)
            for spk, ranges in truth.items():
                for a, b in ranges:
                    act[(t >= a) & (t < b) & (t < n / 16000.0), perm[spk]] = 1
            cls = [overlap.POWERSET.tolist().index(r) for r in act.tolist()]
            out[k, np.arange(589), cls] = -0.01
        return out

    base = overlap._unit(np.random.default_rng(seed).standard_normal((3, dim)))

    def embed(clips):
        rng = np.random.default_rng([seed, len(clips)])
        out = []
        for c in clips:
            vals, counts = np.unique(np.round(c).astype(int), return_counts=True)
            v = int(vals[np.argmax(counts)])                # the commonest sample value: the speaker(s) of most of the clip
            spk = [s for s in range(3) if v >> s & 1]
            out.append(overlap._unit(base[spk].sum(axis=0)) + 0.02 * rng.standard_normal(dim))
        return np.stack(out)
    return wave, segment, embed


def _check_against_truth(tracks, truth, n):
    step = 270 / 16000.0
    by_label = {}
    for s, e, lab in tracks:
        by_label.setdefault(lab, []).append((s, e))
    truth = {k: [(a, min(b, n / 16000.0)) for a, b in v if a < n / 16000.0] for k, v in truth.items()}
    truth = {k: v for k, v in truth.items() if v}
    assert len(by_label) == len(truth)
    ov = lambda x, y: sum(max(0.0, min(a[1], b[1]) - max(a[0], b[0])) for a in x for b in y)
    for spk, ranges in truth.items():
        lab = max(by_label, key=lambda l: ov(by_label[l], ranges))
        got = sorted(by_label.pop(lab))
        assert len(got) == len(ranges), (spk, got, ranges)
        for (s, e), (a, b) in zip(got, ranges):
            assert abs(s - a) <= step + 1e-3 and abs(e - b) <= step + 1e-3, (spk, (s, e), (a, b))


def _true_overlaps(truth, n):
    out = []
    keys = sorted(truth)
    for i, p in enumerate(keys):
        for q in keys[i + 1:]:
            for a in truth[p]:
                for b in truth[q]:
                    s, e = max(a[0], b[0]), min(a[1], b[1], n / 16000.0)
                    if e > s:
                        out.append((s, e))
    return sorted(out)


class _Parser:
    verbose_log = False


def _parse_overlaps(tracks):
    from targetdiarization_amd.target_diarization import TargetDiarization
    return TargetDiarization.od_result_parser(_Parser(), tracks, output_overlap=True)


@pytest.mark.parametrize("seconds", [40, 6])
def test_diarize_recovers_the_truth(seconds):
    n = seconds * 16000
    wave, segment, embed = _stubs(TRUTH_40S, n)
    tracks = overlap.diarize(wave, segment, embed, threshold=0.5)
    assert all(0.0 <= s < e <= n / 16000.0 for s, e, _ in tracks)
    assert [t[2] for t in tracks][0] == "SPEAKER_00"                                  # numbered by first appearance
    _check_against_truth(tracks, TRUTH_40S, n)
    od = _parse_overlaps(tracks)
    want = _true_overlaps(TRUTH_40S, n)
    got = sorted({tuple(r) for rs in od.values() for r in rs})
    assert len(got) == len(want), (got, want)
    for (s, e), (a, b) in zip(got, want):
        assert abs(s - a) <= 270 / 16000.0 + 1e-3 and abs(e - b) <= 270 / 16000.0 + 1e-3


def test_diarize_silence_and_a_speaker_without_clean_speech():
    n = 12 * 16000
    wave, segment, embed = _stubs({}, n)
    assert overlap.diarize(wave, segment, embed) == [] and overlap.diarize(np.zeros(0, np.float32), segment, embed) == []
    # speaker 1 speaks only while speaker 0 does (never 0.4 s alone): its embedding comes from all its active frames
    truth = {0: [(1.0, 8.0)], 1: [(3.0, 5.0)]}
    wave, segment, embed = _stubs(truth, n)
    clips, owner = overlap.gather_clips(overlap.cut_chunks(wave, overlap.chunk_plan(n)[0]),
                                        overlap.powerset_to_speakers(segment(overlap.cut_chunks(wave, overlap.chunk_plan(n)[0]))))
    assert len(clips) == 2 * len(overlap.chunk_plan(n)[0])
    _check_against_truth(overlap.diarize(wave, segment, embed, threshold=0.5), truth, n)
