"""Mint tests/golden/whisper_decode_ts_golden.npz: what tdx_whisper_decode_ts gives, bit for bit, on the cases of
tests/whisper_longform_cases.decode_ts_golden_run (decode_case S / 3, S / 9, M / 3 with the no-speech probability, S / 3 also with a
two-head capture; branch_case M with max_initial_timestamp_index 5): ids, scores, counts, nospeech per case, xattn for S / 3, and
the commit that computed them.  tests/test_gpu_whisper_longform.py::test_decode_ts_is_unchanged compares the tree's build with it.

Run it on a build of the commit whose results are to be kept (--package DIR imports targetdiarization_amd from that checkout, as
tools/whisper_longform_bench.py does), never on the build under test.  Needs a HIP device.

    python tools/make_goldens_whisper_decode_ts.py --package ../parent --commit $(git -C ../parent rev-parse HEAD)
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "whisper_decode_ts_golden.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=ROOT, help="the checkout whose targetdiarization_amd computes the fixture")
    ap.add_argument("--commit", default=None, help="its commit hash (default: git rev-parse HEAD in --package)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    pkg = os.path.abspath(a.package)
    commit = a.commit or subprocess.check_output(["git", "-C", pkg, "rev-parse", "HEAD"], text=True).strip()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, pkg)

    import torch
    import targetdiarization_amd
    import whisper_longform_cases as lc
    from targetdiarization_amd import whisper as W

    assert torch.cuda.is_available(), "the fixture is computed on a HIP device"
    assert os.path.dirname(os.path.dirname(os.path.abspath(targetdiarization_amd.__file__))) == pkg, targetdiarization_amd.__file__
    models = {}

    def model_of(name):
        if name not in models:
            cfg, sd = lc.weights(name, 1, lc.SCALE)
            models[name] = W.WhisperASR(sd, cfg, device="cuda:0", generation_config=lc.gen_config(name))
        return models[name]
    out = lc.decode_ts_golden_run(model_of)
    for k, v in out.items():
        print(f"  {k}: {v.dtype} {list(v.shape)}" + (f" {v.tolist()}" if k.startswith(("counts", "nospeech")) else ""))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, commit=np.array(commit), **out)
    print(a.out, os.path.getsize(a.out), "bytes, commit", commit)


if __name__ == "__main__":
    main()
