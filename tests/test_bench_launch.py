"""CPU test of bench.py's launcher contract: `python bench.py --gpus 2` with no external launcher starts two
child ranks itself (torch.distributed.run, gloo in --dry-run: kernels skipped, embeddings fabricated as in
test_distributed_cpu.py), the printed line says "n_gpus": 2, and a WORLD_SIZE / --gpus mismatch exits non-zero."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(argv, env=None, timeout=300):
    e = dict(os.environ)
    e.pop("RANK", None); e.pop("WORLD_SIZE", None); e.pop("LOCAL_RANK", None)
    if env:
        e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, env=e, timeout=timeout, cwd=ROOT)


def _json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


def test_gpus2_self_launch_dry_run():
    r = _run(["--gpus", "2", "--dry-run", "--steps", "2", "--warmup", "1", "--utterances-per-step", "7"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout               # rank 0 only
    line = lines[0]
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["warmup"] == 1
    assert line["dry_run"] is True and line["gather_ok"] is True
    assert line["scaling"] == "strong" and line["metric"].startswith("real-time factor")


def test_gpus1_dry_run_single_process():
    r = _run(["--gpus", "1", "--dry-run", "--steps", "1", "--warmup", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert _json_lines(r.stdout)[0]["n_gpus"] == 1


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "4", "--dry-run"], env={"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_dump_outputs_dry_run_is_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's results as float32/float64 .npy files; two runs with the same
    arguments write the same arrays, and --steps sets the number of timed steps"""
    import numpy as np
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = _run(["--gpus", "1", "--dry-run", "--steps", "3", "--warmup", "1", "--utterances-per-step", "9", "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-2000:]
        line = _json_lines(r.stdout)[0]
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        dumps.append(np.load(d / "embeddings.npy"))
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (18, 192)
    assert np.array_equal(dumps[0], dumps[1])


def test_hotpath_outputs_sample_and_types(tmp_path):
    """the default workload's results (1800 s: two 28.8 M-sample streams) dump as a fixed seeded sample within 64 MB in all;
    token ids, timestamps and text become float64 arrays"""
    import numpy as np
    import bench
    n = 1800 * 16000
    streams = [(np.arange(n, dtype=np.float32), -np.arange(n, dtype=np.float32))]
    seg = {"token_ids": [7, 8], "scores": [0.5, 0.25], "timestamp": [[0, 40], [40, 80]], "text": "七八。"}
    out = {"streams": streams, "embeddings": np.ones((360, 192), np.float32), "scores": np.zeros(360, np.float32),
           "asr": [[seg] * 60, [seg] * 60], "d2h_bytes": 1}
    arr = bench.hotpath_outputs(out)
    bench.dump_outputs(str(tmp_path), arr)
    files = {p.stem: np.load(p) for p in tmp_path.iterdir()}
    assert set(files) == {"streams", "embeddings", "scores", "asr_tokens_per_segment", "asr_token_ids", "asr_token_scores",
                          "asr_timestamps_ms", "punc_text_lengths", "punc_text_codepoints"}
    assert sum(a.nbytes for a in files.values()) <= 64 * 2 ** 20
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    s = files["streams"]
    assert s.dtype == np.float32 and 0 < s.size <= bench.DUMP_MAX_SAMPLES
    assert np.array_equal(s, bench.hotpath_outputs(out)["streams"])          # fixed positions
    assert files["asr_timestamps_ms"].shape == (240, 2) and files["asr_token_ids"].sum() == 120 * 15
    assert "".join(map(chr, files["punc_text_codepoints"][:3].astype(int))) == "七八。"
