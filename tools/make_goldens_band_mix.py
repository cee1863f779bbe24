"""Mint tests/golden/band_mix.npz by EXECUTING the reference's own mix_audio_by_freq, mix_audio, audio_normalize, audio_gain and
generate_noise (AudioProcessor.py:386-414, 786-882).  Needs the reference tree at /root/reference.  Test infrastructure: only the data
is committed, and no test reads the reference.

AudioProcessor.py imports third-party packages that are absent here (audioread, librosa, pyloudnorm, soundfile, audiostretchy, dotenv,
omegaconf, pydub); none of them is touched by the methods exercised below, so empty placeholder modules are put in sys.modules for
the import to succeed, the optional packages are switched off through the module's own environment variable, and the class is
instantiated WITHOUT running __init__.  Inputs are float64, so the reference computes in double under any numpy."""
import contextlib
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference/AudioProcessor.py"

# (name, n_main, n_aux, sampling_rate, main_freq_range, aux_freq_range, force_align)
MIX_CASES = [
    ("n6_default", 6, 6, 16000, [0, 4000], [0, 8000], False),
    ("n7_default", 7, 7, 16000, [0, 4000], [0, 8000], False),
    ("n257_default", 257, 257, 16000, [0, 4000], [0, 8000], False),
    ("n1000_default", 1000, 1000, 16000, [0, 4000], [0, 8000], False),
    ("n1009_default", 1009, 1009, 16000, [0, 4000], [0, 8000], False),
    ("n257_none", 257, 257, 16000, None, None, False),
    ("n7_none", 7, 7, 44100, None, [], False),
    ("n257_disjoint", 257, 257, 16000, [0, 1000], [3000, 5000], False),
    ("n257_disjoint2", 257, 257, 16000, [5000, 7000], [100, 2000], False),
    ("n1000_onebin", 1000, 1000, 16000, [0, 2000], [2000, 6000], False),       # 2000 Hz is bin 125 exactly: an overlap of one bin
    ("n257_partial", 257, 257, 16000, [100, 3000], [2000, 7000], False),
    ("n257_reversed", 257, 257, 16000, [3000, 100], [0, 8000], False),
    ("n257_cover", 257, 257, 16000, [0, 9000], [1000, 3000], False),
    ("n257_beyond", 257, 257, 8000, [0, 4000], [-5, 99999], False),
    ("n257_truncate", 257, 300, 16000, [0, 4000], [0, 8000], True),
    ("n257_mismatch", 257, 200, 16000, [0, 4000], [0, 8000], False),
]


def load_reference_class():
    os.environ["AUDIOPROCESSOR_DISABLED_PACKAGES"] = "mdx,noisereduce,enhancer,separater,restorer"      # (torch: a class body names it)
    for name in ("audioread", "librosa", "pyloudnorm", "soundfile", "audiostretchy", "audiostretchy.stretch", "dotenv", "omegaconf", "pydub",
                 "pydub.silence"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["audiostretchy.stretch"].AudioStretch = object
    sys.modules["dotenv"].load_dotenv = lambda *a, **k: None
    sys.modules["omegaconf"].OmegaConf = object
    sys.modules["pydub"].AudioSegment = object
    sys.modules["pydub.silence"].split_on_silence = None
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_audio_processor", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ref = object.__new__(mod.AudioProcessor)
    ref.verbose_log = False
    return ref


def main():
    ref = load_reference_class()
    out = {}
    quiet = contextlib.redirect_stdout(io.StringIO())
    for i, (name, n, n_aux, sr, mr, ar, align) in enumerate(MIX_CASES):
        rng = np.random.default_rng(100 + i)
        # (values that float32 holds exactly: stored as float32, fed as float64)
        a, b = [(rng.standard_normal(k) * 0.3).astype(np.float32).astype(np.float64) for k in (n, n_aux)]
        with quiet:
            y = ref.mix_audio_by_freq(a, b, sr, None if mr is None else list(mr), None if ar is None else list(ar), align)
        out[f"mixf_{name}_main"], out[f"mixf_{name}_aux"] = a.astype(np.float32), b.astype(np.float32)
        out[f"mixf_{name}_same"] = np.array(y is a)
        if y is not a:
            out[f"mixf_{name}_out"] = np.asarray(y)
    try:                                                    # n = 1: irfft is asked for 0 points
        with quiet:
            ref.mix_audio_by_freq(np.array([0.5]), np.array([0.25]), 16000)
        out["mixf_n1_raises"] = np.array(False)
    except Exception:
        out["mixf_n1_raises"] = np.array(True)

    rng = np.random.default_rng(7)
    x = (rng.standard_normal(300) * 0.2).astype(np.float32)
    out["host_x"] = x
    with quiet:
        for tag, db, clip in (("p6", 6.0, False), ("p20clip", 20.0, True), ("m3", -3.0, False), ("zero", 0.0, True)):
            out[f"gain_{tag}"] = np.asarray(ref.audio_gain(x, db, clip))
        out["gain_zero_same"] = np.array(ref.audio_gain(x, 0.0) is x)
        out["norm_default"] = np.asarray(ref.audio_normalize(x))
        out["norm_m6"] = np.asarray(ref.audio_normalize(x, -6.0))
        z = np.zeros(16, dtype=np.float32)
        out["norm_zero_same"] = np.array(ref.audio_normalize(z) is z)
        clips = [x, (rng.standard_normal(200) * 0.2).astype(np.float32), (rng.standard_normal(300) * 0.2).astype(np.float32)]
        for k, c in enumerate(clips):
            out[f"mix_clip{k}"] = c
        out["mix_sum_norm"] = np.asarray(ref.mix_audio(list(clips)))
        out["mix_sum_raw"] = np.asarray(ref.mix_audio(list(clips), normalize=False))
        out["mix_stack_norm"] = np.asarray(ref.mix_audio(list(clips), combine_channels=False))
        out["mix_single_same"] = np.array(ref.mix_audio([x]) is x)
        for k, (kind, db) in enumerate((("brown", 0.0), ("pink", 0.0), ("pink", -6.0), ("silence", 0.0), ("white", 3.0))):
            np.random.seed(k)
            out[f"noise_{k}_{kind}"] = np.asarray(ref.generate_noise(8000, 0.05, db, kind))
    path = os.path.join(ROOT, "tests", "golden", "band_mix.npz")
    out["mixf_cases"] = np.array([repr(c) for c in MIX_CASES])
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
