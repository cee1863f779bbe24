"""The tiny Whisper models of the long-form tests (tests/test_whisper_longform_host.py, tests/test_gpu_whisper_longform.py): a
window of 128 feature frames (n_audio_ctx 64), timestamp ids that span exactly one window (65 of them), and a first timestamp id
that is no multiple of the head's 64-column slices.
  S: d 64, 1 head, n_text_ctx 32, 40 text ids + 9 specials + 65 timestamps = 114 ids (2 slices, tb = 49 inside the first)
  M: d 128, 2 heads, n_text_ctx 64, 70 text ids + 9 specials + 65 timestamps = 144 ids (3 slices, the last partial; tb = 79 inside the second)"""
import functools

import torch

from targetdiarization_amd.weights import recipe_whisper_state_dict, whisper_config

CFGS = {"S": dict(d_model=64, enc_heads=1, enc_layers=1, dec_layers=2, n_mels=80, n_audio_ctx=64, n_text_ctx=32, vocab=114),
        "M": dict(d_model=128, enc_heads=2, enc_layers=1, dec_layers=2, n_mels=80, n_audio_ctx=64, n_text_ctx=64, vocab=144)}
NTEXT = {"S": 40, "M": 70}


def gen_config(name):
    """the generation config as WhisperASR reads it (a dict with transformers' field names)"""
    n, T = NTEXT[name], CFGS[name]["n_text_ctx"]
    return {"eos_token_id": n, "decoder_start_token_id": n + 1, "lang_to_id": {"<|en|>": n + 2, "<|zh|>": n + 3},
            "task_to_id": {"translate": n + 4, "transcribe": n + 5}, "prev_sot_token_id": n + 6, "no_timestamps_token_id": n + 8,
            "suppress_tokens": [1, 2, n + 1, n + 2, n + 3, n + 4, n + 5, n + 6, n + 7], "begin_suppress_tokens": [3, n],
            "max_length": T, "is_multilingual": True, "pad_token_id": n, "bos_token_id": n, "alignment_heads": [[1, 0]]}


def ids_of(name):
    g = gen_config(name)
    return {"eos": g["eos_token_id"], "sot": g["decoder_start_token_id"], "en": g["lang_to_id"]["<|en|>"], "transcribe": g["task_to_id"]["transcribe"],
            "prev": g["prev_sot_token_id"], "nospeech": g["no_timestamps_token_id"] - 1, "tb": g["no_timestamps_token_id"] + 1}


@functools.lru_cache(maxsize=None)
def weights(name, seed=1, scale=1.0, nospeech_boost=0.0):
    """recipe weights; scale multiplies the token embedding (sharper or flatter logits); nospeech_boost raises the no-speech
    logit by that much at every step: the decoder's final LayerNorm bias moves along the no-speech id's embedding"""
    cfg = whisper_config(CFGS[name])
    sd = recipe_whisper_state_dict(seed, cfg)
    if scale != 1.0 or nospeech_boost != 0.0:
        sd = {k: v.clone() for k, v in sd.items()}
        E = sd["model.decoder.embed_tokens.weight"]
        E *= scale
        if nospeech_boost:
            e = E[ids_of(name)["nospeech"]]
            sd["model.decoder.layer_norm.bias"] += nospeech_boost * e / float(e @ e)
        sd["proj_out.weight"] = E
    return cfg, sd


def hf_model(name, sd):
    """transformers' WhisperForConditionalGeneration in fp32 with the tiny generation config"""
    from transformers import GenerationConfig, WhisperConfig, WhisperForConditionalGeneration
    c, g = whisper_config(CFGS[name]), gen_config(name)
    hc = WhisperConfig(vocab_size=c["vocab"], num_mel_bins=c["n_mels"], d_model=c["d_model"], encoder_layers=c["enc_layers"],
                       decoder_layers=c["dec_layers"], encoder_attention_heads=c["enc_heads"], decoder_attention_heads=c["dec_heads"],
                       encoder_ffn_dim=c["enc_ffn"], decoder_ffn_dim=c["dec_ffn"], max_source_positions=c["n_audio_ctx"],
                       max_target_positions=c["n_text_ctx"], activation_function=c["activation"], eos_token_id=g["eos_token_id"],
                       pad_token_id=g["pad_token_id"], bos_token_id=g["bos_token_id"], decoder_start_token_id=g["decoder_start_token_id"],
                       suppress_tokens=None, begin_suppress_tokens=None)
    m = WhisperForConditionalGeneration(hc).eval()
    m.load_state_dict(sd, strict=True)
    m.generation_config = GenerationConfig(**{k: v for k, v in g.items()}, return_timestamps=True)
    return m


def noise(n, seed, amp=0.1):
    return amp * torch.randn(n, generator=torch.Generator().manual_seed(seed))


# ---- the decode cases of tests/test_gpu_whisper_longform.py.  The seeds were searched on the CPU so that every decision of the fp64
# oracle (an argmax, or the mass-versus-best-text test) keeps a margin above the test's bound; the test recomputes the margins.
def histories(name):
    """every branch of the rules: empty (the first step); text only (one id, two ids: no timestamp anywhere); one timestamp;
    timestamp text; text then a timestamp (with and without a timestamp before the text); two timestamps; text after a timestamp;
    text after a pair; <|0.00|> then text; the last timestamp id after text; a text id next to eos"""
    I = ids_of(name)
    tb = I["tb"]
    return [[], [5], [5, 6], [tb + 4], [tb + 2, 5], [5, tb + 7], [tb + 2, 5, tb + 7], [tb + 2, 5, tb + 7, tb + 7], [tb + 2, 5, 6],
            [tb + 2, 5, tb + 7, tb + 7, 9, 4], [tb, 5], [tb, 5, tb + 64], [tb + 1, 7, I["eos"] - 1]]


DECODE_SEEDS = {("S", 1): 1, ("S", 3): 1, ("S", 9): 1, ("M", 3): 1}
BRANCH_SEEDS = {"S": 1, "M": 1}
SCALE = 3.0                                             # of the token embedding: decisions with clear margins


def decode_case(name, B, seed=None):
    """B rows with prefixes of different lengths (3 = no history, 7, 14, and one that leaves room for 2 ids), one row with a
    budget of 4 ids -> (features [B, n_mels, 128], rows [{"prefix", "max_new", "sot_pos"}])"""
    seed = DECODE_SEEDS[(name, B)] if seed is None else seed
    I, T, n = ids_of(name), CFGS[name]["n_text_ctx"], NTEXT[name]
    g = torch.Generator().manual_seed(1000 + seed)
    feats = 0.5 * torch.randn(B, CFGS[name]["n_mels"], 2 * CFGS[name]["n_audio_ctx"], generator=g)
    plens = {1: [14], 3: [3, 7, T - 2], 9: [3, 7, 14, T - 2, 3, 7, 14, 5, 9]}[B]
    budgets = {1: [T], 3: [T, 4, T], 9: [T, 4, T, T, T, T, 6, T, T]}[B]
    rows = []
    for pl, mn in zip(plens, budgets):
        text = torch.randint(3, n, (max(0, pl - 4),), generator=g).tolist()
        prefix = ([I["prev"]] + text if pl > 3 else []) + [I["sot"], I["en"], I["transcribe"]]
        rows.append({"prefix": prefix, "max_new": mn, "sot_pos": len(prefix) - 3})
    return feats, rows


def branch_case(name, seed=None):
    """one row per history of histories(): the prefix ends in the history and `begin` = 3 marks where it starts"""
    seed = BRANCH_SEEDS[name] if seed is None else seed
    I = ids_of(name)
    g = torch.Generator().manual_seed(2000 + seed)
    hs = histories(name)
    feats = 0.5 * torch.randn(len(hs), CFGS[name]["n_mels"], 2 * CFGS[name]["n_audio_ctx"], generator=g)
    return feats, [{"prefix": [I["sot"], I["en"], I["transcribe"]] + h, "max_new": 2, "sot_pos": 0, "begin": 3} for h in hs]


GOLDEN_CFG = dict(d_model=128, enc_heads=2, enc_layers=2, dec_layers=2, n_mels=80, vocab=51865, n_audio_ctx=100)     # test_gpu_whisper.py's C


def old_decode_run(W, nb):
    """tdx_whisper_decode on configuration C of tests/test_gpu_whisper.py (recipe weights of seed 1, that file's features of seed 11),
    the Chinese transcription prefix, the default suppress lists, 24 new ids, nb clips -> (ids, scores, counts) on the CPU.
    tests/golden/whisper_decode_golden.npz holds what the commit before tdx_whisper_decode_ts gave."""
    cfg = whisper_config(GOLDEN_CFG)
    m = W.WhisperASR(recipe_whisper_state_dict(1, cfg), cfg, device="cuda:0")
    g = torch.Generator().manual_seed(11)
    feats = 0.5 * torch.randn(32, cfg["n_mels"], 2 * cfg["n_audio_ctx"], generator=g)[:nb]
    gen = W.default_generation_config(cfg["vocab"])
    prefix = W.decode_prefix("chinese", "transcribe", None, gen, cfg["n_text_ctx"])
    _, state = m.encode(feats, with_state=True)
    ids, sc, cnt = m.decode(state, prefix, 24, gen["suppress_tokens"], gen["begin_suppress_tokens"])
    out = ids.cpu()[:, :32].clone(), sc.cpu()[:, :32].clone(), cnt.cpu().clone()
    m.close()
    return out


GOLDEN_TS_CAPTURE = [[1, 0], [0, 0]]


def decode_ts_golden_run(model_of):
    """tdx_whisper_decode_ts on decode_case S / 3, S / 9, M / 3 (sot_pos given; S / 3 with the capture of GOLDEN_TS_CAPTURE) and on
    branch_case M with max_initial_timestamp_index 5 -> {key: numpy array}.  model_of(name): the WhisperASR of weights(name, 1, SCALE)
    under gen_config(name).  tests/golden/whisper_decode_ts_golden.npz holds what the commit before the three decode entry points
    shared one loop gave (tools/make_goldens_whisper_decode_ts.py)."""
    out = {}
    cases = [(f"{n}{B}", n, decode_case(n, B), -1, GOLDEN_TS_CAPTURE if (n, B) == ("S", 3) else None) for n, B in (("S", 3), ("S", 9), ("M", 3))]
    cases.append(("branchM", "M", branch_case("M"), 5, None))
    for tag, name, (feats, rows), max_initial, heads in cases:
        m, g = model_of(name), gen_config(name)
        _, state = m.encode(feats, with_state=True)
        ids, sc, cnt, nosp, xattn = m.decode_ts(state, [r["prefix"] for r in rows], [r["max_new"] for r in rows], suppress=g["suppress_tokens"],
                                                begin_suppress=g["begin_suppress_tokens"], max_initial_timestamp_index=max_initial,
                                                begin=[r.get("begin", len(r["prefix"])) for r in rows], sot_pos=[r["sot_pos"] for r in rows], heads=heads)
        out.update({f"ids_{tag}": ids.cpu().numpy(), f"scores_{tag}": sc.cpu().numpy(), f"counts_{tag}": cnt.cpu().numpy(), f"nospeech_{tag}": nosp.cpu().numpy()})
        if heads is not None:
            out[f"xattn_{tag}"] = xattn.cpu().numpy()
    return out


def oracle_rows(name, sd64, cfg, enc, rows, max_initial=None, eos=None):
    """the fp64 oracle's greedy_ts for every row, enc [B, S, d] in fp64"""
    import whisper_longform_oracle as lo
    I, g = ids_of(name), gen_config(name)
    out = []
    with torch.no_grad():
        for b, r in enumerate(rows):
            out.append(lo.greedy_ts(sd64, cfg, enc[b:b + 1], r["prefix"], r["max_new"], I["tb"], I["eos"] if eos is None else eos, g["suppress_tokens"], g["begin_suppress_tokens"],
                                    max_initial, r.get("begin"), I["nospeech"], r["sot_pos"]))
    return out
