"""Mint the Apollo restorer fixtures under tests/golden/ by executing the reference's own apollo.py (build machine only:
the reference tree is not on the GPU machines, and no GPU test reads it).

    python tools/make_goldens_apollo.py [REFERENCE_MODELS_DIR]

* imports look2hear/models/base_model.py and apollo.py BY PATH into a synthetic package (the package __init__ imports absent
  third-party modules); nothing of the reference is copied;
* strict-loads weights.recipe_apollo_state_dict(seed=0) into Apollo(sr=44100, win=20, feature_dim=256, layer=6): the key
  catalogue of weights.apollo_param_shapes is checked by the load itself;
* pins tests/apollo_oracle.py against the reference: < 1e-11 rel-L2 in float64, < 3e-5 in float32 (asserted);
* writes apollo_catalogue.json, apollo_ref_6l.npz (outputs of two recipe clips), apollo_taps_6l.npz (a subset of frames and
  bands of four intermediate tensors of the short clip) and apollo_pin_report.json.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import apollo_oracle as orc                                           # noqa: E402
from targetdiarization_amd.weights import apollo_param_shapes, recipe_apollo_state_dict, recipe_wave   # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
catalogue = []                                                        # the reference module's own state-dict names and shapes
LENS = (44137, 1324)
TAP_BANDS = [0, 1, 39, 78, 79]


def load_reference(models_dir):
    pkg = types.ModuleType("l2h_apollo")
    pkg.__path__ = [models_dir]
    sys.modules["l2h_apollo"] = pkg
    for name in ("base_model", "apollo"):
        spec = importlib.util.spec_from_file_location(f"l2h_apollo.{name}", os.path.join(models_dir, f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"l2h_apollo.{name}"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["l2h_apollo.apollo"].Apollo


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def run_reference(Apollo, sd, x, dtype, taps=None):
    """reference forward on [1, 1, n]; hann_window follows the default dtype, so it is switched with the model's.  The
    reference's RMSNorm casts its input to float32 (`input.float()`); in the float64 run that cast is made an identity for the
    duration of the call, so that the float64 pin compares arithmetic (the float32 run keeps it, and is pinned as is)."""
    prev, to_float = torch.get_default_dtype(), torch.Tensor.float
    torch.set_default_dtype(dtype)
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else to_float(self, *a, **k)
    try:
        m = Apollo(sr=44100, win=20, feature_dim=256, layer=6)
        m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
        m = m.to(dtype).eval()
        catalogue[:] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        hooks = []
        if taps is not None:
            hooks.append(m.net[0].register_forward_pre_hook(lambda mod, inp: taps.__setitem__("features", inp[0].detach().clone())))
            hooks.append(m.net[0].register_forward_hook(lambda mod, inp, out: taps.__setitem__("net.0", out.detach().clone())))
            hooks.append(m.net[5].register_forward_hook(lambda mod, inp, out: taps.__setitem__("net.5", out.detach().clone())))
            for i in range(80):
                hooks.append(m.output[i].register_forward_hook(
                    lambda mod, inp, out, i=i: taps.__setitem__(f"head.{i}", out.detach().clone())))
        with torch.no_grad():
            y = m(x.to(dtype).reshape(1, 1, -1)).reshape(-1)
        for h in hooks:
            h.remove()
        return y
    finally:
        torch.set_default_dtype(prev)
        torch.Tensor.float = to_float


def main():
    from oracle._load_reference import REF_MODELS
    models_dir = sys.argv[1] if len(sys.argv) > 1 else REF_MODELS
    Apollo = load_reference(models_dir)
    sd = recipe_apollo_state_dict(seed=0)
    shapes = apollo_param_shapes()
    report, outs = {}, {}
    sd64 = orc.cast_state_dict(sd, torch.float64)
    ref_taps = {}
    for n in LENS:
        x = torch.from_numpy(recipe_wave("apollo", 1, n)[0])
        taps = ref_taps if n == LENS[1] else None
        y64 = run_reference(Apollo, sd, x.double(), torch.float64, taps)
        y32 = run_reference(Apollo, sd, x, torch.float32)
        o64 = orc.apollo_forward(x.double().unsqueeze(0), sd64)[0]
        o32 = orc.apollo_forward(x.unsqueeze(0), sd)[0]
        report[f"n{n}"] = {"oracle64_vs_ref64": rel(o64, y64), "oracle32_vs_ref32": rel(o32, y32), "ref32_vs_ref64": rel(y32, y64)}
        print(n, report[f"n{n}"], flush=True)
        assert report[f"n{n}"]["oracle64_vs_ref64"] < 1e-11, report
        assert report[f"n{n}"]["oracle32_vs_ref32"] < 3e-5, report
        outs[f"x{n}"] = x.numpy()
        outs[f"y{n}"] = y64.numpy()
    # taps of the short clip: reference layout [1, nband, 256, T] -> [T, nband, 256] on a band subset; the head spectra -> [T, 442]
    T = orc.frames_of(LENS[1])
    tap = {"bands": np.array(TAP_BANDS)}
    for k in ("features", "net.0", "net.5"):
        tap[k] = ref_taps[k][0].permute(2, 0, 1)[:, TAP_BANDS].numpy()
    re, im = [], []
    for i, bw in enumerate(orc.BANDS):
        h = ref_taps[f"head.{i}"][0]                                   # [2bw, T]
        re.append(h[:bw]); im.append(h[bw:])
    tap["spec_re"] = torch.cat(re, 0).t().numpy()
    tap["spec_im"] = torch.cat(im, 0).t().numpy()
    assert tap["spec_re"].shape == (T, 442)
    otaps = {}
    orc.apollo_forward(torch.from_numpy(outs[f"x{LENS[1]}"]).double().unsqueeze(0), sd64, taps=otaps)
    report["taps"] = {k: rel(otaps[k][0][:, TAP_BANDS], tap[k]) for k in ("features", "net.0", "net.5")}
    report["taps"]["spec"] = max(rel(otaps["spec"][0].real, tap["spec_re"]), rel(otaps["spec"][0].imag, tap["spec_im"]))
    print(report["taps"])
    assert max(report["taps"].values()) < 1e-11, report
    assert catalogue == [[k, list(v)] for k, v in shapes.items()]
    report["params"] = int(sum(int(np.prod(s)) for s in shapes.values()))
    report["tensors"] = len(shapes)
    os.makedirs(GOLD, exist_ok=True)
    with open(os.path.join(GOLD, "apollo_catalogue.json"), "w") as fh:
        json.dump(catalogue, fh)
    np.savez_compressed(os.path.join(GOLD, "apollo_ref_6l.npz"), **outs)
    np.savez_compressed(os.path.join(GOLD, "apollo_taps_6l.npz"), **tap)
    with open(os.path.join(GOLD, "apollo_pin_report.json"), "w") as fh:
        json.dump(report, fh, indent=1)
    for f in ("apollo_catalogue.json", "apollo_ref_6l.npz", "apollo_taps_6l.npz", "apollo_pin_report.json"):
        sz = os.path.getsize(os.path.join(GOLD, f))
        print(f, sz)
        assert sz <= 1 << 20, f


if __name__ == "__main__":
    main()
