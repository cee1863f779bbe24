"""CPU tests of the weight loading every tdx_*_create shares: a missing tensor, a tensor of the wrong size, an unexpected tensor
(the strict loaders) and a transposed one (the loaders that check shapes) are all TDX_E_BLOB with the tensor's name in
tdx_last_error(), before any device work — so none of this needs a GPU."""
import ctypes as C
from functools import lru_cache

import pytest
import torch

from targetdiarization_amd import _lib
from targetdiarization_amd import weights as W

MF2 = "mask_net.mdl.intra_mdl.mossformerM."
MDX_CFG = dict(L=1, l=1, g=32, bn=8, dim_f=32)       # the smallest geometry tdx_mdx_create accepts (dim_t = 1)

# model -> (state dict, create(lib, buf, nbytes, out), strict, a tensor every checkpoint has, a 2-D tensor if shapes are checked)
MODELS = {
    "mf2": (lambda: W.recipe_state_dict(num_blocks=2),
            lambda l, b, n, h: l.tdx_mf2_create(C.byref(_lib.Mf2Config(num_blocks=2, channels=512, kernel_size=16, num_spks=2, group_size=256)), b, n, 0, h),
            True, MF2 + "fsmn.1.gated_fsmn.fsmn.conv.conv2.weight", None),
    "pfenc": (lambda: W.recipe_paraformer_state_dict(num_blocks=2),
              lambda l, b, n, h: l.tdx_pfenc_create(2, b, n, 0, h), False, "encoder.encoders.0.self_attn.fsmn_block.weight", None),
    "pfdec": (lambda: W.recipe_paraformer_decoder_state_dict(num_blocks=2, vocab=64),
              lambda l, b, n, h: l.tdx_pfdec_create(2, 64, b, n, 0, h), False, "decoder.decoders.1.src_attn.linear_k_v.weight", None),
    "eres2net": (lambda: W.recipe_eres2netv2_state_dict(),
                 lambda l, b, n, h: l.tdx_eres2net_create(b, n, 0, h), False, "layer3.2.fuse_models.1.local_att.1.running_var", None),
    "mdx": (lambda: W.recipe_mdx_state_dict(**MDX_CFG),
            lambda l, b, n, h: l.tdx_mdx_create(C.byref(_lib.MdxConfig(num_blocks=1, l=1, g=32, k=3, bn=8, dim_f=32, dim_t=1)), b, n, 0, h),
            True, "bottleneck_block.tdf.3.weight", None),
    "punc": (lambda: W.recipe_punc_state_dict(num_blocks=1, vocab=64),
             lambda l, b, n, h: l.tdx_punc_create(1, 64, 6, b, n, 0, h), True, "encoder.encoders0.0.self_attn.fsmn_block.weight", None),
    "apollo": (lambda: W.recipe_apollo_state_dict(num_layers=1),
               lambda l, b, n, h: l.tdx_apollo_create(1, b, n, 0, h), True, "net.0.seq_net.blocks.2.conv.2.weight", "net.0.band_net.cos_freq"),
    "campplus": (lambda: W.recipe_campplus_state_dict(),
                 lambda l, b, n, h: l.tdx_campp_create(b, n, 0, h), True, "xvector.block2.tdnnd17.cam_layer.linear2.bias", None),
    "fsmn_vad": (lambda: _fsmn_vad_tensors(),
                 lambda l, b, n, h: l.tdx_fsmnvad_create(b, n, 0, h), True, "encoder.fsmn.2.affine.linear.weight", "encoder.in_linear1.linear.weight"),
    "pyannet": (lambda: W.recipe_pyannet_state_dict(),
                lambda l, b, n, h: l.tdx_pyannet_create(b, n, 0, h), True, "lstm.bias_hh_l3_reverse", "lstm.weight_ih_l0"),
    "silero": (lambda: W.recipe_silero_vad_state_dict(),
               lambda l, b, n, h: l.tdx_silero_create(b, n, 0, h), True, "decoder.rnn.bias_hh", "decoder.rnn.weight_ih"),
    "wespeaker": (lambda: W.recipe_wespeaker_state_dict(),
                  lambda l, b, n, h: l.tdx_wespk_create(b, n, 0, h), True, "resnet.layer3.5.bn2.running_var", "resnet.seg_1.weight"),
    "sensevoice": (lambda: W.recipe_sensevoice_state_dict(num_blocks=1, tp_blocks=0, vocab=64),
                   lambda l, b, n, h: l.tdx_sv_create(1, 0, 64, b, n, 0, h), False, "encoder.tp_norm.bias", "ctc.ctc_lo.weight"),
    "pfdec_ts": (lambda: _pfdec_ts_tensors(),
                 lambda l, b, n, h: l.tdx_pfdec_create(2, 64, b, n, 0, h), False, "predictor.blstm.bias_hh_l0_reverse", "predictor.blstm.weight_ih_l0"),
}
# the models' own packers, where they have one
PACK = {"pyannet": W.pack_pyannet_blob, "silero": W.pack_silero_vad_blob}
STRICT = [m for m, v in MODELS.items() if v[2]]
SHAPED = [m for m, v in MODELS.items() if v[4]]


def _fsmn_vad_tensors():
    """the recipe plus the CMVN vectors pack_fsmn_vad_blob adds to it: the tensors tdx_fsmnvad_create reads"""
    sd = dict(W.recipe_fsmn_vad_state_dict())
    sd["cmvn.shift"] = torch.zeros(400); sd["cmvn.scale"] = torch.ones(400)
    return sd


def _pfdec_ts_tensors():
    """the Paraformer decoder with the timestamp head's 12 tensors present"""
    sd = dict(W.recipe_paraformer_decoder_state_dict(num_blocks=2, vocab=64))
    sd.update(W.recipe_paraformer_timestamp_state_dict())
    return sd


@pytest.fixture(scope="module")
def lib():
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.lib()


@lru_cache(maxsize=None)
def _tensors(model):
    return dict(MODELS[model][0]())


def _create(lib, model, sd):
    blob = PACK.get(model, W.pack_blob)(sd)
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    h = C.c_void_p()
    rc = MODELS[model][1](lib, buf, len(blob), C.byref(h))
    assert not h.value                                          # nothing is handed out on failure
    return rc, lib.tdx_last_error()


@pytest.mark.parametrize("model", list(MODELS))
def test_missing_tensor(lib, model):
    name = MODELS[model][3]
    sd = dict(_tensors(model))
    del sd[name]
    rc, err = _create(lib, model, sd)
    assert rc == 2 and name.encode() in err


@pytest.mark.parametrize("model", list(MODELS))
def test_tensor_one_element_short(lib, model):
    name = MODELS[model][3]
    sd = dict(_tensors(model))
    sd[name] = sd[name].reshape(-1)[:-1].clone()
    rc, err = _create(lib, model, sd)
    assert rc == 2 and name.encode() in err


@pytest.mark.parametrize("model", STRICT)
def test_unexpected_tensor(lib, model):
    sd = dict(_tensors(model))
    sd["zz.not_a_tensor_of_the_model"] = torch.zeros(3)
    rc, err = _create(lib, model, sd)
    assert rc == 2 and b"unexpected" in err and b"zz.not_a_tensor_of_the_model" in err


@pytest.mark.parametrize("model", SHAPED)
def test_transposed_tensor(lib, model):
    name = MODELS[model][4]
    sd = dict(_tensors(model))
    assert sd[name].dim() == 2 and sd[name].shape[0] != sd[name].shape[1]
    sd[name] = sd[name].t().contiguous()                        # same numel, other shape
    rc, err = _create(lib, model, sd)
    assert rc == 2 and name.encode() in err


# ---- the Loader's pointer binding (Loader::bind / resolve), through the host-only hook tdx_diag_loader_bind ----
BIND = dict(n=70, npad=130, L=2, C=5, k=3, N=6, K=10, Npad=8, Kp=16)


@pytest.fixture(scope="module")
def diag():
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.diag()


@lru_cache(maxsize=None)
def _bind_tensors():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    b = BIND
    sd = {"plain": r(b["n"]), "padded": r(b["n"]), "twice": r(b["n"]), "lin.weight": r(b["N"], b["K"]), "lin.bias": r(b["N"])}
    for l in range(b["L"]):
        sd[f"layers.{l}.tap"] = r(b["C"], b["k"])
        sd[f"layers.{l}.rows"] = r(b["N"], b["K"])
    return sd


def _bind(diag, sd):
    """-> (status, error text, bound fields that are not null, the tensors read back through their bound pointers)"""
    b = BIND
    sizes = [b["n"], b["npad"], b["n"], b["Npad"] * b["Kp"], b["Npad"]] + [b["k"] * b["C"], b["N"] * b["Kp"]] * b["L"]
    blob = W.pack_blob(sd)
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    out = torch.full((sum(sizes),), float("nan"))
    nonnull = C.c_int(-1)
    rc = diag.tdx_diag_loader_bind(buf, len(blob), *[b[k] for k in ("n", "npad", "L", "C", "k", "N", "K", "Npad", "Kp")],
                                   out.data_ptr(), out.numel(), C.byref(nonnull))
    return rc, diag.tdx_diag_last_error(), nonnull.value, out.split(sizes)


def test_bound_pointers_read_back_what_was_staged(diag):
    b, sd = BIND, _bind_tensors()
    rc, err, nonnull, got = _bind(diag, sd)
    assert rc == 0, err
    assert nonnull == 5 + 2 * b["L"]
    pad = torch.nn.functional.pad
    want = [sd["plain"], pad(sd["padded"], (0, b["npad"] - b["n"])), 2.0 * sd["twice"],
            pad(sd["lin.weight"], (0, b["Kp"] - b["K"], 0, b["Npad"] - b["N"])), pad(sd["lin.bias"], (0, b["Npad"] - b["N"]))]
    for l in range(b["L"]):
        want += [sd[f"layers.{l}.tap"].t(), pad(sd[f"layers.{l}.rows"], (0, b["Kp"] - b["K"]))]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert torch.equal(g, w.contiguous().reshape(-1))        # bit for bit, the padding exactly zero


@pytest.mark.parametrize("name", ["twice", "lin.bias", "layers.1.tap"])
def test_bound_pointers_stay_null_when_a_tensor_is_missing(diag, name):
    sd = dict(_bind_tensors())
    del sd[name]
    rc, err, nonnull, got = _bind(diag, sd)
    assert rc == 2 and name.encode() in err
    assert nonnull == 0
    assert all(torch.isnan(g).all() for g in got)               # nothing was copied out
