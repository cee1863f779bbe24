"""CPU tests of the Apollo restorer: the recipe catalogue against the reference's own state-dict names, the restatement
(tests/apollo_oracle.py) against the reference's outputs and intermediate taps (tests/golden/apollo_*, minted by
tools/make_goldens_apollo.py), and the strict weight loading of tdx_apollo_create (no device work before the blob is accepted)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import apollo_oracle as orc
from targetdiarization_amd import _lib
from targetdiarization_amd.weights import apollo_param_shapes, pack_blob, recipe_apollo_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def sd64():
    return orc.cast_state_dict(recipe_apollo_state_dict(seed=0), torch.float64)


def test_catalogue_matches_reference():
    ref = json.load(open(os.path.join(GOLD, "apollo_catalogue.json")))
    ours = [[k, list(v)] for k, v in apollo_param_shapes().items()]
    assert len(ref) == 654
    assert ours == ref
    assert sum(int(np.prod(s)) for _, s in ref) == json.load(open(os.path.join(GOLD, "apollo_pin_report.json")))["params"]
    sd = recipe_apollo_state_dict(seed=0)
    assert [[k, list(v.shape)] for k, v in sd.items()] == ref
    cos, sin = sd["net.0.band_net.cos_freq"], sd["net.0.band_net.sin_freq"]
    assert torch.equal(cos[:, 0::2], cos[:, 1::2]) and float(cos[0].min()) == 1.0 and float(sin[0].abs().max()) == 0.0


@pytest.mark.parametrize("n", [44137, 1324])
def test_restatement_matches_reference_outputs(sd64, n):
    g = np.load(os.path.join(GOLD, "apollo_ref_6l.npz"))
    x = torch.from_numpy(g[f"x{n}"]).double().unsqueeze(0)
    y = orc.apollo_forward(x, sd64)[0]
    assert y.shape == (n,)
    assert rel(y, g[f"y{n}"]) <= 1e-6


def test_restatement_matches_reference_taps(sd64):
    g = np.load(os.path.join(GOLD, "apollo_taps_6l.npz"))
    x = torch.from_numpy(np.load(os.path.join(GOLD, "apollo_ref_6l.npz"))["x1324"]).double().unsqueeze(0)
    taps = {}
    orc.apollo_forward(x, sd64, taps=taps)
    bands = list(g["bands"])
    for k in ("features", "net.0", "net.5"):
        assert rel(taps[k][0][:, bands], g[k]) <= 1e-6, k
    assert rel(taps["spec"][0].real, g["spec_re"]) <= 1e-6
    assert rel(taps["spec"][0].imag, g["spec_im"]) <= 1e-6


def test_istft_ignores_imaginary_dc_and_nyquist():
    spec = torch.randn(1, 5, 442, dtype=torch.complex128)
    y0 = orc.istft(spec, 1800)
    spec[..., 0] = spec[..., 0].real + 0j
    spec[..., 441] = spec[..., 441].real + 0j
    assert torch.equal(y0, orc.istft(spec, 1800))


@pytest.fixture(scope="module")
def lib():
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.lib()


def _create(lib, sd, num_layers=2):
    blob = pack_blob(sd)
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    h = C.c_void_p()
    return lib.tdx_apollo_create(num_layers, buf, len(blob), 0, C.byref(h))


def test_create_rejects_bad_blobs(lib):
    """strict both ways, like load_state_dict(strict=True): a missing, an extra or a mis-shaped tensor (same element count
    included) is TDX_E_BLOB before any device work"""
    sd = recipe_apollo_state_dict(seed=3, num_layers=2)
    missing = dict(sd)
    del missing["net.1.seq_net.blocks.2.conv.4.bias"]
    assert _create(lib, missing) == 2
    assert b"net.1.seq_net.blocks.2.conv.4.bias" in lib.tdx_last_error()
    no_rope = dict(sd)
    del no_rope["net.0.band_net.sin_freq"]
    assert _create(lib, no_rope) == 2
    extra = dict(sd)
    extra["net.2.band_net.cos_freq"] = sd["net.0.band_net.cos_freq"]
    assert _create(lib, extra) == 2
    assert b"unexpected" in lib.tdx_last_error()
    assert _create(lib, sd, num_layers=3) == 2                      # a 2-layer blob is not a 3-layer model
    reshaped = dict(sd)
    reshaped["BN.7.1.weight"] = sd["BN.7.1.weight"].reshape(256, 1, 11)
    assert _create(lib, reshaped) == 2
    assert b"BN.7.1.weight" in lib.tdx_last_error()
    wrong = dict(sd)
    wrong["output.79.1.bias"] = torch.zeros(20)
    assert _create(lib, wrong) == 2
    assert _create(lib, sd, num_layers=0) == 1
    blob = pack_blob(sd)[:-100]                                       # truncated data section
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    assert lib.tdx_apollo_create(2, buf, len(blob), 0, C.byref(C.c_void_p())) == 2


def test_workspace_and_flops_without_a_handle(lib):
    assert lib.tdx_apollo_workspace_bytes(None, 10) == 0
    assert lib.tdx_apollo_flops(None, 10) == 0.0
    assert lib.tdx_apollo_forward(None, None, None, 0, None, 0, None, None, 0, None) == 1


def test_restore_audio_skips_without_restorer(capsys):
    """no restorer (the folder does not exist, or cuda_device=-1): the input comes back unchanged with the reference's print"""
    from targetdiarization_amd.audio_processor import AudioProcessor
    ap = AudioProcessor(is_restore_audio=True, restorer_weights_folder="/nonexistent/apollo", cuda_device=-1, verbose_log=False)
    assert ap.is_restore_audio is False
    x = np.linspace(-0.1, 0.1, 3000, dtype=np.float32)
    assert ap.restore_audio(x, 16000, keep_sampling_rate=True) is x
    assert "Skip module: restore_audio" in capsys.readouterr().out
    ap = AudioProcessor(is_restore_audio=True, cuda_device=-1, verbose_log=False, restorer_state_dict=recipe_apollo_state_dict(num_layers=1))
    assert ap.is_restore_audio is False
    out = capsys.readouterr().out
    assert "Failed to init restorer model" in out and "no CPU restorer" in out
    assert ap.restore_audio(x, 16000, output_audio_only=True) is x


def test_restore_plan_covers_every_sample():
    """the launch plan of ApolloRestorer: windows with the 54-frame halo, owned sample ranges tiling each clip exactly once"""
    from targetdiarization_amd.apollo import HALO, HOP, ApolloRestorer, frames_of
    r = ApolloRestorer.__new__(ApolloRestorer)
    r.max_frames = 300
    lens = [442, 44137, 300 * 441 + 5, 1000 * 441 + 17, 3 * 44100 + 200]
    launches = r.plan(lens)
    cover = {c: [] for c in range(len(lens))}
    for launch in launches:
        assert sum(it[2] - it[1] for it in launch) <= r.max_frames and len(launch) <= 64
        for c, lo, hi, slo, shi in launch:
            T = frames_of(lens[c])
            cover[c].append((slo, shi))
            if lo > 0:
                assert slo // HOP >= lo + HALO
            if hi < T:
                assert (shi - 1 + HOP) // HOP <= hi - 1 - HALO
    for c, n in enumerate(lens):
        spans = sorted(cover[c])
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
