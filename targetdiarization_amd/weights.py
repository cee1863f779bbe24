"""Weight catalogue, deterministic recipe weights and the TDXW blob format.

* `mossformer2_param_shapes` restates the state_dict layout of the reference's
  MossFormer2 (reference: look2hear/models/mossformer2.py:532-561 and the sub-modules it
  builds; key list verified against the imported reference by oracle/make_goldens.py).
* `recipe_state_dict` fills that layout from a counter-based PRNG (Philox keyed by the
  tensor *name*), so the 223 MB of fp32 weights never have to be committed or shipped:
  the oracle, the tests and bench.py all regenerate bit-identical weights.
  No trained checkpoint ships with the reference (checkpoints/ holds only .gitkeep).
* `pack_blob` serialises {name: tensor} into the flat "TDXW" container that the C-ABI
  (`tdx_mf2_create`, include/tdx.h) parses by tensor name.  A real checkpoint
  (base_model.py:52-64 format: {"model_name", "state_dict"}) goes through the same packer.
"""
from __future__ import annotations

import struct
import zlib
from collections import OrderedDict

import numpy as np
import torch

_PFX = "mask_net.mdl.intra_mdl.mossformerM."


def mossformer2_param_shapes(num_blocks: int = 24, d: int = 512, kernel_size: int = 16,
                             num_spks: int = 2, qk_dim: int = 128, expansion: int = 4,
                             inner: int = 256, rot_dim: int = 32) -> "OrderedDict[str, tuple]":
    """Ordered {state_dict key: shape}; same key order as the reference's nn.Module."""
    hid = d * expansion
    s = OrderedDict()
    s["enc.conv1d.weight"] = (d, 1, kernel_size)
    s["mask_net.norm.weight"] = (d,)
    s["mask_net.norm.bias"] = (d,)
    s["mask_net.conv1d_encoder.weight"] = (d, d, 1)
    s["mask_net.pos_enc.scale"] = (1,)
    s["mask_net.pos_enc.inv_freq"] = (d // 2,)
    for l in range(num_blocks):
        p = f"{_PFX}fsmn.{l}."
        s[p + "conv1.0.weight"] = (inner, d, 1)
        s[p + "conv1.0.bias"] = (inner,)
        s[p + "conv1.1.weight"] = (1,)
        s[p + "norm1.weight"] = (inner,)
        s[p + "norm1.bias"] = (inner,)
        for br in ("to_u", "to_v"):
            q = p + f"gated_fsmn.{br}.mdl."
            s[q + "0.weight"] = (inner,)
            s[q + "0.bias"] = (inner,)
            s[q + "1.weight"] = (inner, inner)
            s[q + "1.bias"] = (inner,)
            s[q + "3.sequential.1.conv.weight"] = (inner, 1, 17)
        q = p + "gated_fsmn.fsmn."
        s[q + "linear.weight"] = (inner, inner)
        s[q + "linear.bias"] = (inner,)
        s[q + "project.weight"] = (inner, inner)
        s[q + "conv.conv1.weight"] = (inner, 1, 39, 1)
        s[q + "conv.norm1.weight"] = (inner,)
        s[q + "conv.norm1.bias"] = (inner,)
        s[q + "conv.prelu1.weight"] = (inner,)
        s[q + "conv.conv2.weight"] = (inner, 2, 39, 1)
        s[q + "conv.norm2.weight"] = (inner,)
        s[q + "conv.norm2.bias"] = (inner,)
        s[q + "conv.prelu2.weight"] = (inner,)
        s[p + "norm2.weight"] = (inner,)
        s[p + "norm2.bias"] = (inner,)
        s[p + "conv2.weight"] = (d, inner, 1)
        s[p + "conv2.bias"] = (d,)
    for l in range(num_blocks):
        p = f"{_PFX}layers.{l}."
        s[p + "rotary_pos_emb.freqs"] = (rot_dim // 2,)
        for nm, (i, o) in (("to_hidden", (d, hid)), ("to_qk", (d, qk_dim))):
            s[p + nm + ".mdl.0.g"] = (1,)
            s[p + nm + ".mdl.1.weight"] = (o, i)
            s[p + nm + ".mdl.1.bias"] = (o,)
            s[p + nm + ".mdl.3.sequential.1.conv.weight"] = (o, 1, 17)
        s[p + "qk_offset_scale.gamma"] = (4, qk_dim)
        s[p + "qk_offset_scale.beta"] = (4, qk_dim)
        s[p + "to_out.mdl.0.g"] = (1,)
        s[p + "to_out.mdl.1.weight"] = (d, 2 * d)
        s[p + "to_out.mdl.1.bias"] = (d,)
        s[p + "to_out.mdl.3.sequential.1.conv.weight"] = (d, 1, 17)
    s["mask_net.mdl.intra_mdl.norm.weight"] = (d,)
    s["mask_net.mdl.intra_mdl.norm.bias"] = (d,)
    s["mask_net.mdl.intra_norm.weight"] = (d,)
    s["mask_net.mdl.intra_norm.bias"] = (d,)
    s["mask_net.conv1d_out.weight"] = (d * num_spks, d, 1)
    s["mask_net.conv1d_out.bias"] = (d * num_spks,)
    s["mask_net.conv1_decoder.weight"] = (d, d, 1)
    s["mask_net.prelu.weight"] = (1,)
    s["mask_net.output.0.weight"] = (d, d, 1)
    s["mask_net.output.0.bias"] = (d,)
    s["mask_net.output_gate.0.weight"] = (d, d, 1)
    s["mask_net.output_gate.0.bias"] = (d,)
    s["dec.weight"] = (d, 1, kernel_size)
    return s


def philox_uniform(name: str, n: int, seed: int = 0) -> np.ndarray:
    """n float32 values in [-1, 1): top 24 bits of Philox4x64 raw words, keyed by
    (seed, crc32(name)).  `random_raw` is the documented stable bit stream."""
    key = np.array([seed & 0xFFFFFFFFFFFFFFFF, zlib.crc32(name.encode())], dtype=np.uint64)
    raw = np.random.Philox(key=key).random_raw(n)
    f = (raw >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / (1 << 24))
    return (f * np.float32(2.0) - np.float32(1.0)).astype(np.float32)


def _recipe_tensor(name: str, shape: tuple, seed: int) -> torch.Tensor:
    n = int(np.prod(shape))
    if name.endswith("pos_enc.inv_freq"):
        dim = shape[0] * 2
        return 1.0 / (10000 ** (torch.arange(0, dim, 2).float() / dim))
    if name.endswith("rotary_pos_emb.freqs"):
        dim = shape[0] * 2
        return 1.0 / (10000 ** (torch.arange(0, dim, 2).float() / dim))
    u = torch.from_numpy(philox_uniform(name, n, seed)).reshape(shape)
    leaf = name.rsplit(".", 1)[-1]
    is_norm = any(t in name for t in (".norm.", ".norm1.", ".norm2.", "intra_norm.", ".mdl.0.weight", ".mdl.0.bias"))
    if name.endswith(".g") or name.endswith("pos_enc.scale"):
        return 1.0 + 0.2 * u
    if "prelu" in name or name.endswith("conv1.1.weight"):
        return 0.25 + 0.1 * u
    if name.endswith("qk_offset_scale.gamma"):
        return 2.5 + 1.0 * u      # large enough that the relu^2 quadratic branch matters
    if name.endswith("qk_offset_scale.beta"):
        return 0.3 * u
    if is_norm:
        return (1.0 + 0.2 * u) if leaf == "weight" else (0.1 * u)
    if leaf == "bias":
        return 0.1 * u
    fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
    return u * float(1.0 / np.sqrt(fan_in))


def recipe_state_dict(seed: int = 0, num_blocks: int = 24, **kw) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic fp32 weights for the MossFormer2 layout (see module docstring)."""
    out = OrderedDict()
    for name, shape in mossformer2_param_shapes(num_blocks=num_blocks, **kw).items():
        # the reference shares ONE RotaryEmbedding across layers -> identical tensors
        out[name] = _recipe_tensor(name, shape, seed).to(torch.float32).contiguous()
    return out


def paraformer_encoder_param_shapes(num_blocks: int = 50, d: int = 512, d_in: int = 560, ffn: int = 2048,
                                    ksize: int = 11) -> "OrderedDict[str, tuple]":
    """funasr SANMEncoder state_dict layout [upstream-recall, SURVEY Appendix B.4]: one
    `encoders0` layer (560 -> 512) + num_blocks-1 `encoders` layers + after_norm."""
    s = OrderedDict()

    def layer(p, din):
        s[p + "self_attn.linear_out.weight"] = (d, d)
        s[p + "self_attn.linear_out.bias"] = (d,)
        s[p + "self_attn.linear_q_k_v.weight"] = (3 * d, din)
        s[p + "self_attn.linear_q_k_v.bias"] = (3 * d,)
        s[p + "self_attn.fsmn_block.weight"] = (d, 1, ksize)
        s[p + "feed_forward.w_1.weight"] = (ffn, d)
        s[p + "feed_forward.w_1.bias"] = (ffn,)
        s[p + "feed_forward.w_2.weight"] = (d, ffn)
        s[p + "feed_forward.w_2.bias"] = (d,)
        s[p + "norm1.weight"] = (din,)
        s[p + "norm1.bias"] = (din,)
        s[p + "norm2.weight"] = (d,)
        s[p + "norm2.bias"] = (d,)

    layer("encoder.encoders0.0.", d_in)
    for i in range(num_blocks - 1):
        layer(f"encoder.encoders.{i}.", d)
    s["encoder.after_norm.weight"] = (d,)
    s["encoder.after_norm.bias"] = (d,)
    return s


def recipe_paraformer_state_dict(seed: int = 0, num_blocks: int = 50) -> "OrderedDict[str, torch.Tensor]":
    out = OrderedDict()
    for name, shape in paraformer_encoder_param_shapes(num_blocks).items():
        n = int(np.prod(shape))
        u = torch.from_numpy(philox_uniform("pf:" + name, n, seed)).reshape(shape)
        leaf = name.rsplit(".", 1)[-1]
        if ".norm" in name or "after_norm" in name:
            t = (1.0 + 0.2 * u) if leaf == "weight" else 0.1 * u
        elif leaf == "bias":
            t = 0.1 * u
        else:
            fan_in = int(np.prod(shape[1:]))
            t = u * float(1.0 / np.sqrt(fan_in))
        out[name] = t.to(torch.float32).contiguous()
    return out


def sensevoice_param_shapes(num_blocks: int = 50, tp_blocks: int = 20, vocab: int = 25055) -> "OrderedDict[str, tuple]":
    """funasr SenseVoiceSmall state_dict layout [upstream-recall]: the 16-row prompt embedding, SenseVoiceEncoderSmall (the SANM
    encoder's layers plus `tp_encoders` and `tp_norm`) and the CTC projection."""
    s = OrderedDict()
    s["embed.weight"] = (16, 560)
    enc = paraformer_encoder_param_shapes(num_blocks)
    for k, v in enc.items():
        s[k] = v
    for i in range(tp_blocks):
        for k, v in enc.items():
            if k.startswith("encoder.encoders0.0."):
                s[f"encoder.tp_encoders.{i}." + k[len("encoder.encoders0.0."):]] = tuple(512 if d == 560 else d for d in v)
    s["encoder.tp_norm.weight"] = (512,)
    s["encoder.tp_norm.bias"] = (512,)
    s["ctc.ctc_lo.weight"] = (vocab, 512)
    s["ctc.ctc_lo.bias"] = (vocab,)
    return s


def recipe_sensevoice_state_dict(seed: int = 0, num_blocks: int = 50, tp_blocks: int = 20, vocab: int = 25055,
                                 blank_bias: float = 0.0) -> "OrderedDict[str, torch.Tensor]":
    """blank_bias is added to the CTC bias of id 0: with random weights it sets the share of blank frames of the greedy decode"""
    out = OrderedDict()
    for name, shape in sensevoice_param_shapes(num_blocks, tp_blocks, vocab).items():
        n = int(np.prod(shape))
        u = torch.from_numpy(philox_uniform("sv:" + name, n, seed)).reshape(shape)
        leaf = name.rsplit(".", 1)[-1]
        if ".norm" in name or "_norm" in name:
            t = (1.0 + 0.2 * u) if leaf == "weight" else 0.1 * u
        elif leaf == "bias":
            t = 0.1 * u
        elif name == "embed.weight":
            t = u
        else:
            fan_in = int(np.prod(shape[1:]))
            t = u * float(1.0 / np.sqrt(fan_in))
        out[name] = t.to(torch.float32).contiguous()
    out["ctc.ctc_lo.bias"][0] += blank_bias
    return out


def paraformer_decoder_param_shapes(num_blocks: int = 16, d: int = 512, ffn: int = 2048, ksize: int = 11,
                                    vocab: int = 8404) -> "OrderedDict[str, tuple]":
    """funasr Paraformer (CifPredictorV2 + ParaformerSANMDecoder) state_dict layout [upstream-recall, SURVEY Appendix B.4]:
    predictor conv/linear, `decoders.{i}` (FFN -> FSMN memory -> cross attention), one FFN-only `decoders3.0`, after_norm,
    output_layer.  (`decoder.embed` is unused by the non-autoregressive forward and not part of the recipe.)"""
    s = OrderedDict()
    s["predictor.cif_conv1d.weight"] = (d, d, 3)
    s["predictor.cif_conv1d.bias"] = (d,)
    s["predictor.cif_output.weight"] = (1, d)
    s["predictor.cif_output.bias"] = (1,)

    def ff(p):
        s[p + "feed_forward.w_1.weight"] = (ffn, d)
        s[p + "feed_forward.w_1.bias"] = (ffn,)
        s[p + "feed_forward.w_2.weight"] = (d, ffn)
        s[p + "feed_forward.norm.weight"] = (ffn,)
        s[p + "feed_forward.norm.bias"] = (ffn,)
        s[p + "norm1.weight"] = (d,)
        s[p + "norm1.bias"] = (d,)

    for i in range(num_blocks):
        p = f"decoder.decoders.{i}."
        ff(p)
        s[p + "self_attn.fsmn_block.weight"] = (d, 1, ksize)
        s[p + "norm2.weight"] = (d,); s[p + "norm2.bias"] = (d,)
        s[p + "src_attn.linear_q.weight"] = (d, d); s[p + "src_attn.linear_q.bias"] = (d,)
        s[p + "src_attn.linear_k_v.weight"] = (2 * d, d); s[p + "src_attn.linear_k_v.bias"] = (2 * d,)
        s[p + "src_attn.linear_out.weight"] = (d, d); s[p + "src_attn.linear_out.bias"] = (d,)
        s[p + "norm3.weight"] = (d,); s[p + "norm3.bias"] = (d,)
    ff("decoder.decoders3.0.")
    s["decoder.after_norm.weight"] = (d,)
    s["decoder.after_norm.bias"] = (d,)
    s["decoder.output_layer.weight"] = (vocab, d)
    s["decoder.output_layer.bias"] = (vocab,)
    return s


def recipe_paraformer_decoder_state_dict(seed: int = 0, num_blocks: int = 16, vocab: int = 8404) -> "OrderedDict[str, torch.Tensor]":
    out = OrderedDict()
    for name, shape in paraformer_decoder_param_shapes(num_blocks, vocab=vocab).items():
        n = int(np.prod(shape))
        u = torch.from_numpy(philox_uniform("pfd:" + name, n, seed)).reshape(shape)
        leaf = name.rsplit(".", 1)[-1]
        if "norm" in name:
            t = (1.0 + 0.2 * u) if leaf == "weight" else 0.1 * u
        elif name == "predictor.cif_output.bias":
            t = torch.full(shape, -1.0)                      # sigmoid around 0.27: one token per ~4 encoder frames
        elif leaf == "bias":
            t = 0.1 * u
        else:
            fan_in = int(np.prod(shape[1:]))
            t = u * float(np.sqrt(3.0 / fan_in))
        out[name] = t.to(torch.float32).contiguous()
    return out


def paraformer_timestamp_param_shapes(d: int = 512, hidden: int = 512) -> "OrderedDict[str, tuple]":
    """the second head of funasr's CifPredictorV3 (BiCifParaformer) [upstream-recall]: ConvTranspose1d(d, d, 3, stride 3),
    nn.LSTM(d, hidden, 1, bidirectional) and Linear(2 * hidden, 1) — 12 tensors"""
    s = OrderedDict()
    s["predictor.upsample_cnn.weight"] = (d, d, 3)
    s["predictor.upsample_cnn.bias"] = (d,)
    for sfx in ("", "_reverse"):
        s["predictor.blstm.weight_ih_l0" + sfx] = (4 * hidden, d)
        s["predictor.blstm.weight_hh_l0" + sfx] = (4 * hidden, hidden)
        s["predictor.blstm.bias_ih_l0" + sfx] = (4 * hidden,)
        s["predictor.blstm.bias_hh_l0" + sfx] = (4 * hidden,)
    s["predictor.cif_output2.weight"] = (1, 2 * hidden)
    s["predictor.cif_output2.bias"] = (1,)
    return s


def recipe_paraformer_timestamp_state_dict(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Weights of unit gain (variance 1 / fan_in; the transposed convolution's fan-in is its 512 input channels: kernel = stride,
    one tap per output frame), so that the LSTM's gate pre-activations have a spread of about 1 and do not saturate.  The output
    bias puts 0.25 * sigmoid - 0.01 near 0.09: three upsampled frames then carry what one encoder frame of the main predictor
    does (sigmoid(-1) = 0.27), and the sum of the upsampled alphas lands near the token count before it is re-normalised."""
    out = OrderedDict()
    for name, shape in paraformer_timestamp_param_shapes().items():
        n = int(np.prod(shape))
        u = torch.from_numpy(philox_uniform("pfts:" + name, n, seed)).reshape(shape)
        leaf = name.rsplit(".", 1)[-1]
        if name == "predictor.cif_output2.bias":
            t = torch.full(shape, -0.4)
        elif leaf.startswith("bias"):
            t = 0.1 * u
        else:
            fan_in = shape[0] if name == "predictor.upsample_cnn.weight" else int(np.prod(shape[1:]))
            t = u * float(np.sqrt(3.0 / fan_in))
        out[name] = t.to(torch.float32).contiguous()
    return out


def eres2netv2_param_shapes(m: int = 64, feat_dim: int = 80, emb: int = 192, base_width: int = 24, scale: int = 4,
                            expansion: int = 4, num_blocks=(3, 4, 6, 3)) -> "OrderedDict[str, tuple]":
    """3D-Speaker ERes2NetV2 state_dict layout [upstream-recall, SURVEY Appendix B.3]."""
    s = OrderedDict()

    def bn(p, c):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            s[p + leaf] = (c,)

    def aff(p, c, r=4):
        inter = c // r
        s[p + "local_att.0.weight"] = (inter, 2 * c, 1, 1); s[p + "local_att.0.bias"] = (inter,)
        bn(p + "local_att.1.", inter)
        s[p + "local_att.3.weight"] = (c, inter, 1, 1); s[p + "local_att.3.bias"] = (c,)
        bn(p + "local_att.4.", c)

    s["conv1.weight"] = (m, 1, 3, 3); bn("bn1.", m)
    in_planes = m
    for li, (nb, stride) in enumerate(zip(num_blocks, (1, 2, 2, 2)), start=1):
        planes = m * (2 ** (li - 1))
        width = int(np.floor(planes * (base_width / 64.0)))
        for i in range(nb):
            p = f"layer{li}.{i}."
            st = stride if i == 0 else 1
            s[p + "conv1.weight"] = (width * scale, in_planes, 1, 1); bn(p + "bn1.", width * scale)
            for j in range(scale):
                s[p + f"convs.{j}.weight"] = (width, width, 3, 3); bn(p + f"bns.{j}.", width)
            s[p + "conv3.weight"] = (planes * expansion, width * scale, 1, 1); bn(p + "bn3.", planes * expansion)
            if st != 1 or in_planes != planes * expansion:
                s[p + "shortcut.0.weight"] = (planes * expansion, in_planes, 1, 1); bn(p + "shortcut.1.", planes * expansion)
            if li >= 3:
                for j in range(scale - 1):
                    aff(p + f"fuse_models.{j}.", width)
            in_planes = planes * expansion
    s["layer3_ds.weight"] = (m * 8 * expansion, m * 4 * expansion, 3, 3)
    aff("fuse34.", m * 8 * expansion)
    s["seg_1.weight"] = (emb, (feat_dim // 8) * m * 8 * expansion * 2)
    s["seg_1.bias"] = (emb,)
    return s


def recipe_eres2netv2_state_dict(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    out = OrderedDict()
    for name, shape in eres2netv2_param_shapes().items():
        n = int(np.prod(shape))
        u = torch.from_numpy(philox_uniform("sv:" + name, n, seed)).reshape(shape)
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "running_var":
            t = 1.0 + 0.3 * u
        elif leaf == "running_mean":
            t = 0.1 * u
        elif len(shape) == 1 and leaf == "weight":
            t = 1.0 + 0.2 * u                      # BatchNorm gamma
        elif leaf == "bias":
            t = 0.1 * u
        else:
            fan_in = int(np.prod(shape[1:]))
            t = u * float(np.sqrt(3.0 / fan_in))    # variance-preserving so 16 bottlenecks stay O(1)
        out[name] = t.to(torch.float32).contiguous()
    return out


def recipe_wave(name: str, batch: int, n: int, seed: int = 0, amp: float = 0.1) -> np.ndarray:
    """Deterministic synthetic input waveforms [batch, n] float32 in [-amp, amp)."""
    return (philox_uniform(f"wave:{name}", batch * n, seed) * np.float32(amp)).reshape(batch, n)


# ---------------------------------------------------------------------------------------
# TDXW blob: magic(8) | u32 n | n x { u16 name_len | name | u8 ndim | u32 dims[ndim] |
#            u64 data_offset (bytes from start of data section) } | pad to 64 | data (f32 LE)
# ---------------------------------------------------------------------------------------
TDXW_MAGIC = b"TDXW0001"


def pack_blob(state_dict) -> bytes:
    head = bytearray()
    head += TDXW_MAGIC
    items = [(k, v) for k, v in state_dict.items()]
    head += struct.pack("<I", len(items))
    datas = []
    off = 0
    for k, v in items:
        a = np.ascontiguousarray(v.detach().cpu().to(torch.float32).numpy() if isinstance(v, torch.Tensor)
                                 else np.asarray(v, dtype=np.float32))
        kb = k.encode()
        head += struct.pack("<H", len(kb)) + kb
        head += struct.pack("<B", a.ndim)
        for dim in a.shape:
            head += struct.pack("<I", dim)
        head += struct.pack("<Q", off)
        datas.append(a.tobytes())
        off += (a.nbytes + 63) // 64 * 64
    pad = (-len(head)) % 64
    head += b"\0" * pad
    body = bytearray()
    for dbytes in datas:
        body += dbytes
        body += b"\0" * ((-len(dbytes)) % 64)
    return bytes(head) + bytes(body)


# ---------------------------------------------------------------------------------------
# MDX-Net denoiser body (KUIELab ConvTDFNet / TFC-TDF v2; the network inside the UVR-MDX-NET *.onnx files that
# AudioProcessor.init_mdx_model hands to onnxruntime, AudioProcessor.py:224-241).  [upstream-recall]: module tree of
# kuielab/mdx-net `ConvTDFNet` (first_conv, encoding_blocks.{i}.{tfc.H.{j}, tdf}, ds.{i}, bottleneck_block, us.{i},
# decoding_blocks.{i}, final_conv), BatchNorm2d norms (the rmsprop-trained public models), no checkpoint in the reference tree.
# ---------------------------------------------------------------------------------------
def mdx_param_shapes(L: int = 11, l: int = 3, g: int = 32, k: int = 3, bn: int = 8, bias: bool = False, dim_c: int = 4,
                     dim_f: int = 3072) -> "OrderedDict[str, tuple]":
    s = OrderedDict()
    n = L // 2

    def norm(p, c):
        s[p + "weight"] = (c,); s[p + "bias"] = (c,); s[p + "running_mean"] = (c,); s[p + "running_var"] = (c,)

    def tfc_tdf(p, c, f):
        for j in range(l):
            s[f"{p}tfc.H.{j}.0.weight"] = (c, c, k, k); s[f"{p}tfc.H.{j}.0.bias"] = (c,)
            norm(f"{p}tfc.H.{j}.1.", c)
        s[p + "tdf.0.weight"] = (f // bn, f)
        if bias:
            s[p + "tdf.0.bias"] = (f // bn,)
        norm(p + "tdf.1.", c)
        s[p + "tdf.3.weight"] = (f, f // bn)
        if bias:
            s[p + "tdf.3.bias"] = (f,)
        norm(p + "tdf.4.", c)
    s["first_conv.0.weight"] = (g, dim_c, 1, 1); s["first_conv.0.bias"] = (g,)
    norm("first_conv.1.", g)
    f, c = dim_f, g
    for i in range(n):
        tfc_tdf(f"encoding_blocks.{i}.", c, f)
        s[f"ds.{i}.0.weight"] = (c + g, c, 2, 2); s[f"ds.{i}.0.bias"] = (c + g,)
        norm(f"ds.{i}.1.", c + g)
        f //= 2; c += g
    tfc_tdf("bottleneck_block.", c, f)
    for i in range(n):
        s[f"us.{i}.0.weight"] = (c, c - g, 2, 2); s[f"us.{i}.0.bias"] = (c - g,)      # ConvTranspose2d: [in, out, kh, kw]
        norm(f"us.{i}.1.", c - g)
        f *= 2; c -= g
        tfc_tdf(f"decoding_blocks.{i}.", c, f)
    s["final_conv.0.weight"] = (dim_c, c, 1, 1); s["final_conv.0.bias"] = (dim_c,)
    return s


def recipe_mdx_state_dict(seed: int = 0, **kw) -> "OrderedDict[str, torch.Tensor]":
    out = OrderedDict()
    for name, shape in mdx_param_shapes(**kw).items():
        u = torch.from_numpy(philox_uniform("mdx:" + name, int(np.prod(shape)), seed)).reshape(shape)
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "running_var":
            t = 1.0 + 0.3 * u
        elif leaf == "running_mean":
            t = 0.1 * u
        elif len(shape) == 1 and leaf == "weight":
            t = 1.0 + 0.2 * u                      # BatchNorm gamma
        elif leaf == "bias":
            t = 0.1 * u
        elif name.startswith("us."):               # ConvTranspose2d [in, out, 2, 2]: every output pixel sees `in` inputs
            t = u * float(np.sqrt(3.0 / shape[0]))
        else:
            fan_in = int(np.prod(shape[1:]))
            t = u * float(np.sqrt(3.0 / fan_in))    # keeps the activations O(1) through the ~35 layers (x + tdf(x), x * skip included)
        out[name] = t.to(torch.float32).contiguous()
    return out


# ---------------------------------------------------------------------------------------
# CT-Transformer punctuation model (funasr CTTransformer: Embedding -> SANM encoder -> Linear) [upstream-recall]
# ---------------------------------------------------------------------------------------
def punc_param_shapes(num_blocks: int = 4, vocab: int = 272727, npunc: int = 6, d: int = 256, ffn: int = 1024, ksize: int = 11) -> "OrderedDict[str, tuple]":
    s = OrderedDict()
    s["embed.weight"] = (vocab, d)

    def layer(p):
        s[p + "self_attn.linear_q_k_v.weight"] = (3 * d, d); s[p + "self_attn.linear_q_k_v.bias"] = (3 * d,)
        s[p + "self_attn.fsmn_block.weight"] = (d, 1, ksize)
        s[p + "self_attn.linear_out.weight"] = (d, d); s[p + "self_attn.linear_out.bias"] = (d,)
        s[p + "feed_forward.w_1.weight"] = (ffn, d); s[p + "feed_forward.w_1.bias"] = (ffn,)
        s[p + "feed_forward.w_2.weight"] = (d, ffn); s[p + "feed_forward.w_2.bias"] = (d,)
        s[p + "norm1.weight"] = (d,); s[p + "norm1.bias"] = (d,); s[p + "norm2.weight"] = (d,); s[p + "norm2.bias"] = (d,)
    layer("encoder.encoders0.0.")
    for i in range(num_blocks - 1):
        layer(f"encoder.encoders.{i}.")
    s["encoder.after_norm.weight"] = (d,); s["encoder.after_norm.bias"] = (d,)
    s["decoder.weight"] = (npunc, d); s["decoder.bias"] = (npunc,)
    return s


def recipe_punc_state_dict(seed: int = 0, num_blocks: int = 4, vocab: int = 4096, npunc: int = 6) -> "OrderedDict[str, torch.Tensor]":
    """(a small vocabulary by default: the real table is 272 727 x 256 = 279 MB)"""
    out = OrderedDict()
    for name, shape in punc_param_shapes(num_blocks, vocab, npunc).items():
        u = torch.from_numpy(philox_uniform("punc:" + name, int(np.prod(shape)), seed)).reshape(shape)
        leaf = name.rsplit(".", 1)[-1]
        if name == "embed.weight":
            t = 0.5 * u
        elif name.startswith("decoder."):
            t = u * (2.0 if leaf == "weight" else 0.5)          # spread logits: every class gets chosen somewhere ...
            if leaf == "bias":
                t = t.clone(); t[0] = -30.0                     # ... except <unk> (a trained model does not emit it; funasr would print it literally)
        elif ".norm" in name or "after_norm" in name:
            t = (1.0 + 0.2 * u) if leaf == "weight" else 0.1 * u
        elif leaf == "bias":
            t = 0.1 * u
        else:
            t = u * float(1.0 / np.sqrt(int(np.prod(shape[1:]))))
        out[name] = t.to(torch.float32).contiguous()
    return out


# ---------------------------------------------------------------------------------------
# Apollo band-split RoFormer restorer (look2hear/models/apollo.py, built by AudioProcessor.init_restorer_model with
# sr=44100, win=20, feature_dim=256, layer=6): 80 bands (79 x 5 bins + 47), 6 BSNet layers.  Key list verified against the
# imported reference by tools/make_goldens_apollo.py (tests/golden/apollo_catalogue.json).
# ---------------------------------------------------------------------------------------
APOLLO_BANDS = [5] * 79 + [47]


def apollo_param_shapes(num_layers: int = 6, d: int = 256) -> "OrderedDict[str, tuple]":
    """Ordered {state_dict key: shape}, module order of the reference (rotary tables are registered buffers: they are in the
    state dict and a strict load checks them)."""
    s = OrderedDict()
    for i, bw in enumerate(APOLLO_BANDS):
        s[f"BN.{i}.0.weight"] = (2 * bw + 1,)
        s[f"BN.{i}.1.weight"] = (d, 2 * bw + 1, 1)
        s[f"BN.{i}.1.bias"] = (d,)
    for l in range(num_layers):
        p = f"net.{l}.band_net."
        s[p + "cos_freq"] = (100, 32)
        s[p + "sin_freq"] = (100, 32)
        s[p + "input_norm.weight"] = (d,)
        s[p + "weight.weight"] = (3 * d, d, 1)
        s[p + "output.weight"] = (d, d, 1)
        s[p + "MLP.0.weight"] = (d,)
        s[p + "MLP.1.weight"] = (8 * d, d, 1)
        s[p + "MLP_output.weight"] = (d, 4 * d, 1)
        for b in range(3):
            q = f"net.{l}.seq_net.blocks.{b}.conv."
            s[q + "0.weight"] = (d, 1, 7)
            s[q + "0.bias"] = (d,)
            s[q + "1.weight"] = (d,)
            s[q + "2.weight"] = (4 * d, d, 1)
            s[q + "2.bias"] = (4 * d,)
            s[q + "4.weight"] = (d, 4 * d, 1)
            s[q + "4.bias"] = (d,)
    for i, bw in enumerate(APOLLO_BANDS):
        s[f"output.{i}.0.weight"] = (d,)
        s[f"output.{i}.1.weight"] = (4 * bw, d, 1)
        s[f"output.{i}.1.bias"] = (4 * bw,)
    return s


def apollo_rotary_tables(window: int = 100, dim: int = 32, theta: float = 10000.0):
    """cos / sin tables [window, dim] in float32, computed the way Roformer._calc_rotary_emb does (pair-duplicated angles)."""
    freq = 1.0 / (theta ** (torch.arange(0, dim, 2)[: dim // 2] / dim))
    ang = torch.arange(0, window).reshape(-1, 1) * freq.reshape(1, -1)
    cos = torch.stack([torch.cos(ang)] * 2, -1).reshape(window, dim)
    sin = torch.stack([torch.sin(ang)] * 2, -1).reshape(window, dim)
    return cos.to(torch.float32), sin.to(torch.float32)


def recipe_apollo_state_dict(seed: int = 0, num_layers: int = 6) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic fp32 weights for the Apollo layout: conv weights and biases U(+-1/sqrt(fan_in)) (PyTorch's Conv1d init range),
    RMSNorm weights 1 + 0.1 u, the rotary buffers as the reference computes them."""
    cos, sin = apollo_rotary_tables()
    shapes = apollo_param_shapes(num_layers)
    out = OrderedDict()
    for name, shape in shapes.items():
        if name.endswith("cos_freq") or name.endswith("sin_freq"):
            out[name] = (cos if name.endswith("cos_freq") else sin).clone()
            continue
        u = torch.from_numpy(philox_uniform("apollo:" + name, int(np.prod(shape)), seed)).reshape(shape)
        if len(shape) == 1 and name.endswith(".weight"):         # every 1-D weight is an RMSNorm gain (conv weights are 3-D)
            t = 1.0 + 0.1 * u
        else:
            wshape = shapes[name[:-len("bias")] + "weight"] if name.endswith(".bias") else shape
            t = u * float(1.0 / np.sqrt(int(np.prod(wshape[1:]))))
        out[name] = t.to(torch.float32).contiguous()
    return out


# ---------------------------------------------------------------------------------------
# CAM++ (3D-Speaker speakerlab/models/campplus/{DTDNN,layers}.py: FCM head + D-TDNN with context-aware masking)
# [upstream-recall]: the source is not vendored; tests/campplus_oracle.py restates the forward and csrc/campplus.hip
# loads exactly these names (strict both ways).  BatchNorm entries: weight, bias, running_mean, running_var
# (num_batches_tracked is dropped before packing); dense.nonlinear.batchnorm is affine=False.
# ---------------------------------------------------------------------------------------
def campplus_param_shapes(feat_dim: int = 80, emb: int = 192, growth: int = 32, bn_size: int = 4, init: int = 128,
                          layers=(12, 24, 16), m: int = 32) -> "OrderedDict[str, tuple]":
    s = OrderedDict()

    def bn(p, c, affine=True):
        for leaf in (("weight", "bias") if affine else ()) + ("running_mean", "running_var"):
            s[p + leaf] = (c,)

    s["head.conv1.weight"] = (m, 1, 3, 3); bn("head.bn1.", m)
    for li in (1, 2):
        for i in (0, 1):
            p = f"head.layer{li}.{i}."
            s[p + "conv1.weight"] = (m, m, 3, 3); bn(p + "bn1.", m)
            s[p + "conv2.weight"] = (m, m, 3, 3); bn(p + "bn2.", m)
            if i == 0:
                s[p + "shortcut.0.weight"] = (m, m, 1, 1); bn(p + "shortcut.1.", m)
    s["head.conv2.weight"] = (m, m, 3, 3); bn("head.bn2.", m)
    c = m * (feat_dim // 8)
    s["xvector.tdnn.linear.weight"] = (init, c, 5); bn("xvector.tdnn.nonlinear.batchnorm.", init)
    c = init
    bnc = bn_size * growth
    for bi, nl in enumerate(layers, start=1):
        for i in range(nl):
            p = f"xvector.block{bi}.tdnnd{i + 1}."
            bn(p + "nonlinear1.batchnorm.", c + growth * i)
            s[p + "linear1.weight"] = (bnc, c + growth * i, 1)
            bn(p + "nonlinear2.batchnorm.", bnc)
            s[p + "cam_layer.linear_local.weight"] = (growth, bnc, 3)
            s[p + "cam_layer.linear1.weight"] = (bnc // 2, bnc, 1); s[p + "cam_layer.linear1.bias"] = (bnc // 2,)
            s[p + "cam_layer.linear2.weight"] = (growth, bnc // 2, 1); s[p + "cam_layer.linear2.bias"] = (growth,)
        c += growth * nl
        bn(f"xvector.transit{bi}.nonlinear.batchnorm.", c)
        s[f"xvector.transit{bi}.linear.weight"] = (c // 2, c, 1)
        c //= 2
    bn("xvector.out_nonlinear.batchnorm.", c)
    s["xvector.dense.linear.weight"] = (emb, 2 * c, 1)
    bn("xvector.dense.nonlinear.batchnorm.", emb, affine=False)
    return s


def campplus_learnable(name: str) -> bool:
    return not name.endswith(("running_mean", "running_var"))


def recipe_campplus_state_dict(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic fp32 weights for the CAM++ layout, in the manner of recipe_eres2netv2_state_dict.  With these
    plain weights the embedding hardly depends on the input (the final BatchNorm's statistics do not match the
    activations); tests calibrate `xvector.dense.nonlinear.batchnorm.*` from tests/golden/campplus_calibration.json."""
    out = OrderedDict()
    for name, shape in campplus_param_shapes().items():
        n = int(np.prod(shape))
        u = torch.from_numpy(philox_uniform("campp:" + name, n, seed)).reshape(shape)
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "running_var":
            t = 1.0 + 0.3 * u
        elif leaf == "running_mean":
            t = 0.1 * u
        elif len(shape) == 1 and leaf == "weight":
            t = 1.0 + 0.2 * u                      # BatchNorm gamma
        elif leaf == "bias":
            t = 0.1 * u
        else:
            fan_in = int(np.prod(shape[1:]))
            t = u * float(np.sqrt(3.0 / fan_in))
        out[name] = t.to(torch.float32).contiguous()
    return out


def drop_num_batches_tracked(state_dict):
    """PyTorch checkpoints carry one int64 `num_batches_tracked` per BatchNorm; the device loaders are strict, so they go."""
    return OrderedDict((k, v) for k, v in state_dict.items() if not k.endswith("num_batches_tracked"))


# ---------------------------------------------------------------------------------------
# FSMN-VAD (funasr/models/fsmn_vad_streaming/encoder.py, speech_fsmn_vad_zh-cn-16k-common-pytorch config)
# [upstream-recall]: the source is not vendored and no checkpoint is at hand, parity is unpinned; tests/fsmn_vad_oracle.py
# restates the forward and csrc/fsmn_vad.hip loads exactly these names plus cmvn.shift / cmvn.scale (strict both ways).
# ---------------------------------------------------------------------------------------
def fsmn_vad_param_shapes(d_in: int = 400, h1: int = 140, d: int = 250, proj: int = 128, taps: int = 20, layers: int = 4,
                          classes: int = 248) -> "OrderedDict[str, tuple]":
    s = OrderedDict()
    s["encoder.in_linear1.linear.weight"] = (h1, d_in); s["encoder.in_linear1.linear.bias"] = (h1,)
    s["encoder.in_linear2.linear.weight"] = (d, h1); s["encoder.in_linear2.linear.bias"] = (d,)
    for i in range(layers):
        p = f"encoder.fsmn.{i}."
        s[p + "linear.linear.weight"] = (proj, d)
        s[p + "fsmn_block.conv_left.weight"] = (proj, 1, taps, 1)
        s[p + "affine.linear.weight"] = (d, proj); s[p + "affine.linear.bias"] = (d,)
    s["encoder.out_linear1.linear.weight"] = (h1, d); s["encoder.out_linear1.linear.bias"] = (h1,)
    s["encoder.out_linear2.linear.weight"] = (classes, h1); s["encoder.out_linear2.linear.bias"] = (classes,)
    return s


def recipe_fsmn_vad_state_dict(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic fp32 weights for the FSMN-VAD layout (Philox keyed by the tensor name, fan-in scaled, like
    recipe_campplus_state_dict).  With these plain weights every posterior sits near 1/248; the tests fit row 0 of
    out_linear2 and the CMVN from tests/golden/fsmn_vad_calibration.json."""
    out = OrderedDict()
    for name, shape in fsmn_vad_param_shapes().items():
        n = int(np.prod(shape))
        u = torch.from_numpy(philox_uniform("fsmnvad:" + name, n, seed)).reshape(shape)
        if name.endswith("bias"):
            t = 0.1 * u
        else:
            # fan-in scaled so the activations keep their level through the stack: gain 2 where a ReLU follows (in_linear2,
            # affine), 1 otherwise; the memory taps add a quarter of the identity path's variance
            fan_in = int(np.prod(shape[1:]))
            gain = 2.0 if "in_linear2" in name or "affine" in name else (0.25 if "conv_left" in name else 1.0)
            t = u * float(np.sqrt(3.0 * gain / fan_in))
        out[name] = t.to(torch.float32).contiguous()
    return out


def pack_fsmn_vad_blob(state_dict, cmvn=None) -> bytes:
    """The TDXW blob tdx_fsmnvad_create reads: the state dict under funasr's names (a checkpoint's bare `in_linear1...` keys
    get the `encoder.` prefix) plus cmvn.shift / cmvn.scale [400]; cmvn = (shift, scale) or None = (0, 1)."""
    sd = OrderedDict()
    for k, v in state_dict.items():
        sd[k if k.startswith(("encoder.", "cmvn.")) else "encoder." + k] = v
    if cmvn is not None:
        sd["cmvn.shift"], sd["cmvn.scale"] = (np.asarray(torch.as_tensor(c).detach().cpu(), dtype=np.float32).reshape(-1) for c in cmvn)
    elif "cmvn.shift" not in sd:
        sd["cmvn.shift"], sd["cmvn.scale"] = np.zeros(400, np.float32), np.ones(400, np.float32)
    return pack_blob(sd)


def parse_kaldi_cmvn(path: str):
    """am.mvn (Kaldi nnet text): the vectors after <AddShift> and <Rescale>, each `<LearnRateCoef> 0 [ v ... ]` -> (shift, scale)"""
    import re
    text = open(path).read()
    out = []
    for tag in ("<AddShift>", "<Rescale>"):
        m = re.search(re.escape(tag) + r".*?\[(.*?)\]", text, flags=re.S)
        if not m:
            raise ValueError(f"{path}: no {tag} vector")
        out.append(np.array(m.group(1).split(), dtype=np.float64).astype(np.float32))
    if out[0].shape != out[1].shape:
        raise ValueError(f"{path}: <AddShift> and <Rescale> differ in length")
    return out[0], out[1]


# ---------------------------------------------------------------------------------------
# PyanNet (pyannote.audio models/segmentation/PyanNet.py, the segmentation-3.0 configuration: SincNet stride 10, a 4-layer
# bidirectional LSTM of 128 units, linears 128/128, 7 powerset classes)
# [upstream-recall]: the source is not vendored and no checkpoint is at hand, parity is unpinned; tests/pyannet_oracle.py
# restates the forward and csrc/pyannet.hip loads exactly these names (strict both ways).
# ---------------------------------------------------------------------------------------
def pyannet_param_shapes(hidden: int = 128, layers: int = 4, classes: int = 7) -> "OrderedDict[str, tuple]":
    s = OrderedDict()
    s["sincnet.wav_norm1d.weight"] = (1,); s["sincnet.wav_norm1d.bias"] = (1,)
    s["sincnet.conv1d.0.filterbank.low_hz_"] = (40, 1); s["sincnet.conv1d.0.filterbank.band_hz_"] = (40, 1)
    s["sincnet.conv1d.1.weight"] = (60, 80, 5); s["sincnet.conv1d.1.bias"] = (60,)
    s["sincnet.conv1d.2.weight"] = (60, 60, 5); s["sincnet.conv1d.2.bias"] = (60,)
    for i, c in enumerate((80, 60, 60)):
        s[f"sincnet.norm1d.{i}.weight"] = (c,); s[f"sincnet.norm1d.{i}.bias"] = (c,)
    for l in range(layers):
        for sfx in ("", "_reverse"):
            s[f"lstm.weight_ih_l{l}{sfx}"] = (4 * hidden, 60 if l == 0 else 2 * hidden)
            s[f"lstm.weight_hh_l{l}{sfx}"] = (4 * hidden, hidden)
            s[f"lstm.bias_ih_l{l}{sfx}"] = (4 * hidden,); s[f"lstm.bias_hh_l{l}{sfx}"] = (4 * hidden,)
    s["linear.0.weight"] = (hidden, 2 * hidden); s["linear.0.bias"] = (hidden,)
    s["linear.1.weight"] = (hidden, hidden); s["linear.1.bias"] = (hidden,)
    s["classifier.weight"] = (classes, hidden); s["classifier.bias"] = (classes,)
    return s


def recipe_pyannet_state_dict(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic fp32 weights for the PyanNet layout (Philox keyed by the tensor name).  The sinc band edges are
    asteroid's mel-spaced initialisation (30 Hz .. 7900 Hz).  torch's default 1/sqrt(hidden) scale makes this network almost
    ignore its input (logit standard deviation ~1e-3 over a clip), so the matrices are fan-in scaled with gains that keep the
    signal alive through the stack: 3 on the LSTM's input matrices, 1.5 on the recurrent ones, 2 before a leaky_relu, 4 on
    the classifier.  tests/golden/pyannet_calibration.json holds the classifier gain and bias that do the rest."""
    out = OrderedDict()
    mel = np.linspace(2595.0 * np.log10(1.0 + 30.0 / 700.0), 2595.0 * np.log10(1.0 + 7900.0 / 700.0), 41)
    hz = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    for name, shape in pyannet_param_shapes().items():
        n = int(np.prod(shape))
        u = torch.from_numpy(philox_uniform("pyannet:" + name, n, seed)).reshape(shape)
        if name.endswith("low_hz_"):
            t = torch.from_numpy(hz[:-1]).reshape(shape)
        elif name.endswith("band_hz_"):
            t = torch.from_numpy(np.diff(hz)).reshape(shape)
        elif "norm1d" in name:
            t = (1.0 + 0.2 * u) if name.endswith("weight") else 0.1 * u
        elif "bias" in name:
            t = 0.1 * u
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = 3.0 if "weight_ih" in name else 1.5 if "weight_hh" in name else 4.0 if name.startswith("classifier") else 2.0
            t = u * float(np.sqrt(3.0 * gain / fan_in))
        out[name] = t.to(torch.float32).contiguous()
    return out


def pack_pyannet_blob(state_dict) -> bytes:
    """The TDXW blob tdx_pyannet_create reads: pyannote's names; the filterbank's derived buffers (n_, window_), which a
    checkpoint carries next to low_hz_ / band_hz_, are dropped (the device rebuilds the filters in fp64)"""
    return pack_blob(OrderedDict((k, v) for k, v in state_dict.items() if not k.endswith(("filterbank.n_", "filterbank.window_"))))


# ---------------------------------------------------------------------------------------
# silero-VAD v5, 16 kHz branch (the `silero_vad` package's model: STFT magnitude, four Conv1d(k=3) + ReLU, LSTMCell(128,128),
# a 128 -> 1 sigmoid head)
# [upstream-recall]: the source is not vendored and no checkpoint is at hand, parity is unpinned; tests/silero_vad_oracle.py
# restates the forward and csrc/silero_vad.hip loads exactly these names (strict both ways).
# ---------------------------------------------------------------------------------------
def silero_vad_param_shapes() -> "OrderedDict[str, tuple]":
    s = OrderedDict()
    s["stft.forward_basis_buffer"] = (258, 1, 256)
    for i, (co, ci) in enumerate(((128, 129), (64, 128), (64, 64), (128, 64))):
        s[f"encoder.{i}.reparam_conv.weight"] = (co, ci, 3); s[f"encoder.{i}.reparam_conv.bias"] = (co,)
    s["decoder.rnn.weight_ih"] = (512, 128); s["decoder.rnn.weight_hh"] = (512, 128)
    s["decoder.rnn.bias_ih"] = (512,); s["decoder.rnn.bias_hh"] = (512,)
    s["decoder.decoder.2.weight"] = (1, 128, 1); s["decoder.decoder.2.bias"] = (1,)
    return s


def recipe_silero_vad_state_dict(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic fp32 weights for the silero-VAD layout (Philox keyed by the tensor name).  The basis is what upstream
    stores: cos / -sin of the 256-point DFT, rows 0..128, times a periodic Hann window.  The matrices are fan-in scaled with
    gains that keep the signal alive through the stack — 2 before a ReLU, 8 on the first convolution (magnitudes of quiet audio
    are small), 3 on the LSTM's input matrix, 1.5 on the recurrent one — so that the network does not ignore its input;
    tests/golden/silero_vad_calibration.json holds the head that does the rest."""
    out = OrderedDict()
    n = np.arange(256, dtype=np.float64)
    k = np.arange(129, dtype=np.float64)[:, None]
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / 256.0)
    ang = 2.0 * np.pi * k * n[None, :] / 256.0
    basis = np.concatenate([np.cos(ang) * hann, -np.sin(ang) * hann])[:, None, :]
    for name, shape in silero_vad_param_shapes().items():
        if name == "stft.forward_basis_buffer":
            out[name] = torch.from_numpy(basis).to(torch.float32).contiguous()
            continue
        u = torch.from_numpy(philox_uniform("silero:" + name, int(np.prod(shape)), seed)).reshape(shape)
        if "bias" in name:
            t = 0.1 * u
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = 8.0 if name.startswith("encoder.0.") else 3.0 if "weight_ih" in name else 1.5 if "weight_hh" in name else 2.0
            t = u * float(np.sqrt(3.0 * gain / fan_in))
        out[name] = t.to(torch.float32).contiguous()
    return out


def pack_silero_vad_blob(state_dict) -> bytes:
    """The TDXW blob tdx_silero_create reads: the 16 kHz branch under its bare names (a `_model.` prefix is stripped, the
    8 kHz branch `_model_8k.*` dropped)"""
    sd = OrderedDict()
    for k, v in state_dict.items():
        if k.startswith("_model_8k."):
            continue
        sd[k[len("_model."):] if k.startswith("_model.") else k] = v
    return pack_blob(sd)


# ---------------------------------------------------------------------------------------
# WeSpeaker ResNet34 (wespeaker/models/resnet.py ResNet34: m_channels 32, feat_dim 80, embed_dim 256, TSTP,
# two_emb_layer False; pyannote.audio WeSpeakerResNet34 keeps it under `resnet.`) [upstream-recall]: the source is not
# vendored and no checkpoint is at hand, parity is unpinned; tests/wespeaker_oracle.py restates the forward and
# csrc/wespeaker.hip loads exactly these names (strict both ways; num_batches_tracked is dropped before packing).
# ---------------------------------------------------------------------------------------
def wespeaker_param_shapes(m: int = 32, feat_dim: int = 80, emb: int = 256, blocks=(3, 4, 6, 3)) -> "OrderedDict[str, tuple]":
    s = OrderedDict()

    def bn(p, c):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            s[p + leaf] = (c,)

    s["resnet.conv1.weight"] = (m, 1, 3, 3); bn("resnet.bn1.", m)
    cin = m
    for li, nb in enumerate(blocks):
        cout = m << li
        for i in range(nb):
            p = f"resnet.layer{li + 1}.{i}."
            stride = 2 if (i == 0 and li > 0) else 1
            s[p + "conv1.weight"] = (cout, cin, 3, 3); bn(p + "bn1.", cout)
            s[p + "conv2.weight"] = (cout, cout, 3, 3); bn(p + "bn2.", cout)
            if stride != 1 or cin != cout:
                s[p + "shortcut.0.weight"] = (cout, cin, 1, 1); bn(p + "shortcut.1.", cout)
            cin = cout
    s["resnet.seg_1.weight"] = (emb, 2 * cin * (feat_dim // 8))
    s["resnet.seg_1.bias"] = (emb,)
    return s


def recipe_wespeaker_state_dict(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic fp32 weights for the WeSpeaker ResNet34 layout: fan-in scaled convolutions, BatchNorm gamma near 1.
    The running statistics written here do not match the activations; the tests replace them with the ones of
    tests/golden/wespeaker_calibration.json (one fp64 pass of the oracle over seeded synthetic voices), which keeps all
    33 convolutions alive."""
    out = OrderedDict()
    for name, shape in wespeaker_param_shapes().items():
        n = int(np.prod(shape))
        u = torch.from_numpy(philox_uniform("wespk:" + name, n, seed)).reshape(shape)
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "running_var":
            t = 1.0 + 0.3 * u
        elif leaf == "running_mean":
            t = 0.1 * u
        elif len(shape) == 1 and leaf == "weight":
            t = 1.0 + 0.2 * u                      # BatchNorm gamma
        elif leaf == "bias":
            t = 0.1 * u
        else:
            fan_in = int(np.prod(shape[1:]))
            t = u * float(np.sqrt(3.0 / fan_in))
        out[name] = t.to(torch.float32).contiguous()
    return out


WHISPER_CONFIG_KEYS = ("n_mels", "n_audio_ctx", "d_model", "enc_heads", "enc_layers", "enc_ffn", "n_text_ctx", "dec_heads", "dec_layers",
                       "dec_ffn", "vocab", "activation")


def whisper_config(cfg=None, **kw) -> dict:
    """The Whisper sizes as one dict (WHISPER_CONFIG_KEYS).  Accepts that dict, keyword arguments, transformers' config.json
    dict or a WhisperConfig object (num_mel_bins, max_source_positions, encoder_attention_heads, ...); the FFN widths default
    to 4 d_model, the context sizes to 1500 / 448, the activation to "gelu"."""
    if cfg is not None and not isinstance(cfg, dict):
        cfg = cfg.to_dict()
    c = dict(cfg or {})
    c.update(kw)
    if "num_mel_bins" in c or "vocab_size" in c:
        c = {"n_mels": c.get("num_mel_bins", 80), "n_audio_ctx": c.get("max_source_positions", 1500), "d_model": c["d_model"],
             "enc_heads": c["encoder_attention_heads"], "enc_layers": c["encoder_layers"], "enc_ffn": c.get("encoder_ffn_dim", 4 * c["d_model"]),
             "n_text_ctx": c.get("max_target_positions", 448), "dec_heads": c["decoder_attention_heads"], "dec_layers": c["decoder_layers"],
             "dec_ffn": c.get("decoder_ffn_dim", 4 * c["d_model"]), "vocab": c["vocab_size"], "activation": c.get("activation_function", "gelu")}
    d = int(c["d_model"])
    heads = int(c.get("enc_heads", c.get("heads", d // 64)))
    out = {"n_mels": int(c.get("n_mels", 80)), "n_audio_ctx": int(c.get("n_audio_ctx", 1500)), "d_model": d, "enc_heads": heads,
           "enc_layers": int(c["enc_layers"]), "enc_ffn": int(c.get("enc_ffn", 4 * d)), "n_text_ctx": int(c.get("n_text_ctx", 448)),
           "dec_heads": int(c.get("dec_heads", heads)), "dec_layers": int(c["dec_layers"]), "dec_ffn": int(c.get("dec_ffn", 4 * d)),
           "vocab": int(c["vocab"]), "activation": str(c.get("activation", "gelu"))}
    return out


def whisper_param_shapes(cfg) -> "OrderedDict[str, tuple]":
    """transformers' WhisperForConditionalGeneration.state_dict() layout (tests/test_whisper_host.py compares it with upstream):
    k_proj has no bias; proj_out.weight is tied to model.decoder.embed_tokens.weight."""
    c = whisper_config(cfg)
    d = c["d_model"]
    s = OrderedDict()

    def attn(p):
        s[p + ".k_proj.weight"] = (d, d)
        s[p + ".v_proj.weight"] = (d, d)
        s[p + ".v_proj.bias"] = (d,)
        s[p + ".q_proj.weight"] = (d, d)
        s[p + ".q_proj.bias"] = (d,)
        s[p + ".out_proj.weight"] = (d, d)
        s[p + ".out_proj.bias"] = (d,)

    def norm(p):
        s[p + ".weight"] = (d,)
        s[p + ".bias"] = (d,)

    def ffn(p, f):
        s[p + "fc1.weight"] = (f, d)
        s[p + "fc1.bias"] = (f,)
        s[p + "fc2.weight"] = (d, f)
        s[p + "fc2.bias"] = (d,)
        norm(p + "final_layer_norm")

    s["model.encoder.conv1.weight"] = (d, c["n_mels"], 3)
    s["model.encoder.conv1.bias"] = (d,)
    s["model.encoder.conv2.weight"] = (d, d, 3)
    s["model.encoder.conv2.bias"] = (d,)
    s["model.encoder.embed_positions.weight"] = (c["n_audio_ctx"], d)
    for l in range(c["enc_layers"]):
        p = f"model.encoder.layers.{l}."
        attn(p + "self_attn")
        norm(p + "self_attn_layer_norm")
        ffn(p, c["enc_ffn"])
    norm("model.encoder.layer_norm")
    s["model.decoder.embed_tokens.weight"] = (c["vocab"], d)
    s["model.decoder.embed_positions.weight"] = (c["n_text_ctx"], d)
    for l in range(c["dec_layers"]):
        p = f"model.decoder.layers.{l}."
        attn(p + "self_attn")
        norm(p + "self_attn_layer_norm")
        attn(p + "encoder_attn")
        norm(p + "encoder_attn_layer_norm")
        ffn(p, c["dec_ffn"])
    norm("model.decoder.layer_norm")
    s["proj_out.weight"] = (c["vocab"], d)
    return s


def recipe_whisper_state_dict(seed: int, cfg) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic fp32 weights in the Whisper layout.  Matrices and convolution kernels are N(0, 0.02) as transformers
    initialises them, times 4 (without the factor a random model repeats one token and its top two logits nearly tie: no
    test of a decoder); biases N(0, 0.1); LayerNorm gains 1 + N(0, 0.1); decoder positions N(0, 0.5); encoder positions the
    sinusoids transformers stores.  Every tensor has its own generator, keyed by (seed, crc32(name))."""
    c = whisper_config(cfg)
    out = OrderedDict()
    for name, shape in whisper_param_shapes(c).items():
        if name == "proj_out.weight":
            out[name] = out["model.decoder.embed_tokens.weight"]
            continue
        g = torch.Generator()
        g.manual_seed(((int(seed) & 0x7FFFFFFF) << 32) | zlib.crc32(name.encode()))
        n = torch.randn(shape, generator=g, dtype=torch.float32)
        if name == "model.encoder.embed_positions.weight":
            length, ch = shape
            inc = np.log(10000.0) / (ch // 2 - 1)
            t = torch.arange(length).float()[:, None] * torch.exp(-inc * torch.arange(ch // 2).float())[None, :]
            v = torch.cat([t.sin(), t.cos()], dim=1)
        elif name == "model.decoder.embed_positions.weight":
            v = 0.5 * n
        elif name.endswith("layer_norm.weight"):
            v = 1.0 + 0.1 * n
        elif name.endswith(".bias"):
            v = 0.1 * n
        else:
            v = 0.08 * n
        out[name] = v.to(torch.float32).contiguous()
    return out


# ---------------------------------------------------------------------------------------
# emotion2vec (funasr `Emotion2vec`: a data2vec 2.0 audio encoder + a linear head; iic/emotion2vec_plus_large behind the
# reference's emotion_detection, ASRProcessor.py:277-283).  [upstream-recall]: no checkpoint and no funasr here, the parameter
# names below are restated from fairseq's data2vec 2.0 / funasr and are unpinned.  EMOTION2VEC_NAMES is the ONE table that
# says where a tensor lives upstream: (name in the TDXW blob, upstream name, what is added to the blob's index to get the
# upstream one).  {n} is a layer / block index.
# ---------------------------------------------------------------------------------------
_E2V_AUDIO = "modality_encoders.AUDIO."
EMOTION2VEC_NAMES = (
    ("conv.{n}.weight", _E2V_AUDIO + "local_encoder.conv_layers.{n}.0.weight", 0),
    ("conv.{n}.ln.weight", _E2V_AUDIO + "local_encoder.conv_layers.{n}.2.1.weight", 0),
    ("conv.{n}.ln.bias", _E2V_AUDIO + "local_encoder.conv_layers.{n}.2.1.bias", 0),
    ("proj.ln.weight", _E2V_AUDIO + "project_features.1.weight", 0),
    ("proj.ln.bias", _E2V_AUDIO + "project_features.1.bias", 0),
    ("proj.weight", _E2V_AUDIO + "project_features.2.weight", 0),
    ("proj.bias", _E2V_AUDIO + "project_features.2.bias", 0),
    ("pos.{n}.weight", _E2V_AUDIO + "relative_positional_encoder.{n}.0.weight", 1),
    ("pos.{n}.bias", _E2V_AUDIO + "relative_positional_encoder.{n}.0.bias", 1),
    ("extra_tokens", _E2V_AUDIO + "extra_tokens", 0),
    ("alibi_scale", _E2V_AUDIO + "alibi_scale", 0),
    ("prenet.norm.weight", _E2V_AUDIO + "context_encoder.norm.weight", 0),
    ("prenet.norm.bias", _E2V_AUDIO + "context_encoder.norm.bias", 0),
    ("prenet.blocks.{n}.", _E2V_AUDIO + "context_encoder.blocks.{n}.", 0),      # + a leaf of EMOTION2VEC_BLOCK_LEAVES
    ("blocks.{n}.", "blocks.{n}.", 0),
    ("head.weight", "proj.weight", 0),
    ("head.bias", "proj.bias", 0),
)
EMOTION2VEC_BLOCK_LEAVES = ("attn.qkv", "attn.proj", "norm1", "mlp.fc1", "mlp.fc2", "norm2")
EMOTION2VEC_IGNORED = (_E2V_AUDIO + "decoder.", "_ema.")       # and any key that contains "mask_emb"
EMOTION2VEC_STRIDES = (5, 2, 2, 2, 2, 2, 2)
EMOTION2VEC_CONFIG_KEYS = ("C", "D", "H", "E", "prenet_depth", "depth", "conv_kernels", "conv_strides", "pos_layers", "pos_k", "pos_groups",
                           "n_classes")


def emotion2vec_upstream_name(blob_pattern: str, n: int = 0, leaf: str = "") -> str:
    """the upstream name of the tensor the blob calls `blob_pattern` (an entry of EMOTION2VEC_NAMES) at index n"""
    for pat, up, off in EMOTION2VEC_NAMES:
        if pat == blob_pattern:
            return up.replace("{n}", str(n + off)) + leaf
    raise KeyError(blob_pattern)


def emotion2vec_config(cfg=None, **kw) -> dict:
    """The emotion2vec sizes as one dict (EMOTION2VEC_CONFIG_KEYS); the defaults are iic/emotion2vec_plus_large (C 512, D 1024,
    16 heads, 10 extra tokens, 4 + 24 blocks, kernels (10, 3, 3, 3, 3, 2, 2), strides (5, 2, 2, 2, 2, 2, 2), 5 positional layers
    of 19 taps in 16 groups, 9 classes)."""
    c = dict(cfg or {})
    c.update(kw)
    D = int(c.get("D", 1024))
    kernels = tuple(int(k) for k in c.get("conv_kernels", (10, 3, 3, 3, 3, 2, 2)))
    strides = c.get("conv_strides")
    strides = tuple(int(s) for s in strides) if strides is not None else EMOTION2VEC_STRIDES[:len(kernels)]
    if len(strides) != len(kernels):
        raise ValueError(f"emotion2vec_config: {len(kernels)} conv kernels but {len(strides)} strides")
    return {"C": int(c.get("C", 512)), "D": D, "H": int(c.get("H", D // 64)), "E": int(c.get("E", 10)),
            "prenet_depth": int(c.get("prenet_depth", 4)), "depth": int(c.get("depth", 24)), "conv_kernels": kernels, "conv_strides": strides,
            "pos_layers": int(c.get("pos_layers", 5)), "pos_k": int(c.get("pos_k", 19)), "pos_groups": int(c.get("pos_groups", 16)),
            "n_classes": int(c.get("n_classes", 9))}


def emotion2vec_frames(n: int, cfg=None) -> int:
    """frames of a clip of n samples: L' = floor((L - k) / s) + 1 per conv layer (0 when the clip is too short)"""
    c = emotion2vec_config(cfg)
    L = int(n)
    for k, s in zip(c["conv_kernels"], c["conv_strides"]):
        if L < k:
            return 0
        L = (L - k) // s + 1
    return L


def emotion2vec_param_shapes(cfg=None) -> "OrderedDict[str, tuple]":
    """the state dict of funasr's Emotion2vec in upstream names (without the pre-training decoder, the EMA copy and mask_emb)"""
    c = emotion2vec_config(cfg)
    C, D = c["C"], c["D"]
    s = OrderedDict()
    up = emotion2vec_upstream_name
    for i, k in enumerate(c["conv_kernels"]):
        s[up("conv.{n}.weight", i)] = (C, 1 if i == 0 else C, k)
        s[up("conv.{n}.ln.weight", i)] = (C,)
        s[up("conv.{n}.ln.bias", i)] = (C,)
    s[up("proj.ln.weight")] = (C,)
    s[up("proj.ln.bias")] = (C,)
    s[up("proj.weight")] = (D, C)
    s[up("proj.bias")] = (D,)
    for l in range(c["pos_layers"]):
        s[up("pos.{n}.weight", l)] = (D, D // c["pos_groups"], c["pos_k"])
        s[up("pos.{n}.bias", l)] = (D,)
    s[up("extra_tokens")] = (1, c["E"], D)
    s[up("alibi_scale")] = (1, 1, c["H"], 1, 1)
    s[up("prenet.norm.weight")] = (D,)
    s[up("prenet.norm.bias")] = (D,)
    for pat, nb in (("prenet.blocks.{n}.", c["prenet_depth"]), ("blocks.{n}.", c["depth"])):
        for b in range(nb):
            for leaf, shp in (("attn.qkv", (3 * D, D)), ("attn.proj", (D, D)), ("norm1", (D,)), ("mlp.fc1", (4 * D, D)), ("mlp.fc2", (D, 4 * D)),
                              ("norm2", (D,))):
                s[up(pat, b, leaf + ".weight")] = shp
                s[up(pat, b, leaf + ".bias")] = (shp[0],)
    s[up("head.weight")] = (c["n_classes"], D)
    s[up("head.bias")] = (c["n_classes"],)
    return s


def recipe_emotion2vec_state_dict(seed: int = 0, cfg=None, head_gain: float = 4.0) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic fp32 weights in the upstream layout, from the Philox recipe: matrices and kernels u / sqrt(fan_in) (the
    head times head_gain: a flat head would make the top-1 test say nothing), biases 0.1 u, LayerNorm gains 1 + 0.2 u.  Upstream
    initialises alibi_scale to 1 and extra_tokens to 0; here alibi_scale lies in [0.5, 2] with head 1 NEGATIVE (the clamp at 0
    is exercised) and extra_tokens are 0.5 u (a zero prefix would hide indexing errors)."""
    c = emotion2vec_config(cfg)
    out = OrderedDict()
    for name, shape in emotion2vec_param_shapes(c).items():
        n = int(np.prod(shape))
        u = torch.from_numpy(philox_uniform("emotion2vec:" + name, n, seed)).reshape(shape)
        leaf = name.rsplit(".", 1)[-1]
        is_norm = any(t in name for t in (".norm.", ".norm1.", ".norm2.", ".2.1.", "project_features.1."))
        if name.endswith("alibi_scale"):
            v = 1.25 + 0.75 * u
            if c["H"] > 1:
                v.reshape(-1)[1] = -0.5
        elif name.endswith("extra_tokens"):
            v = 0.5 * u
        elif is_norm:
            v = (1.0 + 0.2 * u) if leaf == "weight" else 0.1 * u
        elif leaf == "bias":
            v = 0.1 * u
        else:
            fan_in = int(np.prod(shape[1:]))
            v = u * float((head_gain if name == "proj.weight" else 1.0) / np.sqrt(fan_in))
        out[name] = v.to(torch.float32).contiguous()
    return out
