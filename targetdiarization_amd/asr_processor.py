"""ASRProcessor — the paraformer branch of the reference's `asr_detection` (ASRProcessor.py:373-442)
around the MI355X encoder.  The swap point is `self.asr['paraformer'].generate(input=wav, hotword=…)`
(:424): the neural forward runs through `tdx_pfenc_*` (SANM encoder) and, when the state dict carries the
`predictor.*` / `decoder.*` tensors, `tdx_pfdec_*` (CIF predictor + NAR SANM decoder): tokens are the argmax
ids, mapped to text through `token_list` (funasr's tokens.json, absent here: "<id>" placeholders by default).
A custom `decoder(encoder_out[T',512]) -> {"text": str, "timestamp": [[start_ms, end_ms], ...]}` plug-in overrides it.
The post-processing of the result dicts (:427-437: ms -> s, token/timestamp pairing) and the
print-and-degrade behaviour for missing engines (:375-389) are the reference's."""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np


class ASRProcessor:
    whisper_long_form = False                        # (an instance made without __init__ keeps the one-window path)
    whisper_fallback = False                         # (... and greedy decoding)

    def __init__(self, is_asr: bool = False, fast_asr: bool = False, asr_model_dir=None, is_vad: bool = False, vad_model_dir: str = "",
                 is_punc: bool = False, punc_model_dir: str = "", is_timestamp: bool = False, timestamp_model_dir: str = "",
                 is_emotion: bool = False, emotion_model_dir: str = "", is_diarization: bool = False, diarization_model_dir: str = "",
                 is_asr_api: bool = False, api_config_path: str = "", verbose_log: bool = True, cuda_device: int = 0, ap=None,
                 *, asr_state_dict=None, decoder: Optional[Callable] = None, punctuation: Optional[Callable] = None, token_list=None,
                 punc_state_dict=None, punc_vocab=None, vad_state_dict=None, vad_cmvn=None,
                 sensevoice_state_dict=None, sensevoice_token_list=None, sensevoice_cmvn=None,
                 whisper_state_dict=None, whisper_config=None, whisper_token_list=None, whisper_tokenizer=None, whisper_generation_config=None,
                 whisper_engine: str = "whisper_finetune", whisper_alignment_heads=None,
                 emotion_state_dict=None, emotion_config=None, emotion_labels=None, whisper_long_form: bool = False,
                 whisper_fallback: bool = False):
        self.is_asr = is_asr
        self.whisper_long_form = bool(whisper_long_form)  # whisper_v2 / whisper_v3: clips over 30 s go through WhisperASR.transcribe
        self.whisper_fallback = bool(whisper_fallback)    # ... and transcribe runs whisper.transcribe's temperature fallback (its defaults)
        self.verbose_log = verbose_log
        self.ap = ap
        self.cuda_device = cuda_device
        self.pitch = None                                # pitch.Pyin, created by the first f0_compute
        self.is_vad = is_vad
        self.vad = None
        if is_vad:                                       # ASRProcessor.py:253-260: load, or print and switch the feature off
            try:
                from .vad import build_vad
                self.vad = build_vad(vad_state_dict, vad_cmvn, vad_model_dir, cuda_device)
                if self.vad is None:
                    raise FileNotFoundError(f"no vad_state_dict, and {vad_model_dir!r} is not a directory holding model.pt and am.mvn")
            except Exception as e:
                self.is_vad = False
                print(f"Failed to load FunASR VAD model: {e}")
        self.is_emotion = is_emotion
        self.emotion = None
        if is_emotion:                                   # ASRProcessor.py:277-283: load, or print and switch the feature off
            try:
                from .emotion import build_emotion
                self.emotion = build_emotion(emotion_state_dict, emotion_config, emotion_labels, emotion_model_dir, cuda_device)
                if self.emotion is None:
                    raise FileNotFoundError(f"no emotion_state_dict, and {emotion_model_dir!r} is not a directory holding model.pt")
            except Exception as e:
                self.is_emotion = False
                print(f"Failed to load Modelscope emotion detection model: {e}")
        self.decoder = decoder
        self.punctuation = punctuation
        if punctuation is None and punc_state_dict is not None:      # ASRProcessor.py:261-268: load, or print and switch the feature off
            try:
                from .punctuation import CTTransformer
                self.punctuation = CTTransformer(punc_state_dict, device=f"cuda:{cuda_device}", vocab=punc_vocab)
            except Exception as e:
                print(f"Failed to load punctuation restorer model: {e}")
        self.is_punc = self.punctuation is not None
        self.token_list = token_list
        self.asr = {}
        self.nar_decoder = None
        if is_asr and asr_state_dict is not None:
            try:
                from .paraformer import ParaformerDecoder, ParaformerEncoder
                enc_sd = {k: v for k, v in asr_state_dict.items() if k.startswith("encoder.")}
                self.asr["paraformer"] = ParaformerEncoder(enc_sd, device=f"cuda:{cuda_device}")
                if decoder is None and any(k.startswith("decoder.decoders.") for k in asr_state_dict):
                    self.nar_decoder = ParaformerDecoder(asr_state_dict, device=f"cuda:{cuda_device}")
                    self.decoder = self._nar_decode
            except Exception as e:                       # ASRProcessor.py:215-264: print, feature off
                print(f"Load ASR model failed: {e}")
                self.is_asr = False
        if is_asr and sensevoice_state_dict is not None:         # ASRProcessor.py:215-264: a second engine next to the first; print, leave it out
            try:
                from .sensevoice import build_sensevoice
                self.asr["sensevoice"] = build_sensevoice(sensevoice_state_dict, sensevoice_token_list, sensevoice_cmvn, cuda_device=cuda_device)
                self.is_asr = True
            except Exception as e:
                print(f"Load ASR model failed: {e}")
        # ASRProcessor.py:244-251: the Whisper engine, from weights or from a directory whose name says "whisper" and "finetune"
        import os
        wdir = asr_model_dir if isinstance(asr_model_dir, str) and "whisper" in asr_model_dir.lower() and "finetune" in asr_model_dir.lower() \
            and os.path.isdir(asr_model_dir) else None
        # ASRProcessor.py:232-243: the engines with word timestamps, from one OpenAI-format file whose name says "whisper" and "v2" / "v3"
        # (a vocab.json next to it is read when present), or from weights with whisper_engine="whisper_v2" | "whisper_v3"
        wfile, engine = None, str(whisper_engine).lower()
        if isinstance(asr_model_dir, str) and "whisper" in asr_model_dir.lower() and os.path.isfile(asr_model_dir):
            for tag in ("v2", "v3"):
                if wfile is None and tag in asr_model_dir.lower():
                    wfile, engine = asr_model_dir, "whisper_" + tag
        if engine not in ("whisper_finetune", "whisper_v2", "whisper_v3"):
            print(f"Failed to load Whisper model: whisper_engine {whisper_engine!r} is none of whisper_finetune, whisper_v2, whisper_v3")
        elif is_asr and (whisper_state_dict is not None or wdir is not None or wfile is not None):
            label = {"whisper_finetune": "finetune", "whisper_v2": "V2", "whisper_v3": "V3"}[engine]
            try:
                from .whisper import build_whisper
                m = build_whisper(whisper_state_dict, whisper_config, wfile if wfile is not None else wdir, whisper_token_list, whisper_tokenizer,
                                  whisper_generation_config, cuda_device, alignment_heads=whisper_alignment_heads)
                if m is None:
                    raise FileNotFoundError(f"{wdir!r} holds no config.json with model.safetensors or pytorch_model.bin")
                self.asr[engine] = m
                self.is_asr = True
            except Exception as e:
                print(f"Failed to load Whisper {label} model: {e}")

    def _nar_decode(self, enc_out):
        """encoder output [T',512] -> {"text", "timestamp"} through the device CIF predictor + NAR decoder"""
        r = self.nar_decoder.decode(enc_out[None])[0]
        toks = [self.token_list[i] if self.token_list is not None and i < len(self.token_list) else f"<{i}>" for i in r["token_ids"]]
        return {"text": " ".join(toks), "timestamp": r["timestamp"], "token_ids": r["token_ids"]}

    def punctuation_restore(self, text):
        """ASRProcessor.punctuation_restore (:880-897): str or list of str; no model / empty text / a failing model -> the text unchanged"""
        if self.punctuation is None:
            if self.verbose_log:
                print("Modelscope punctuation restorer model hasn't been loaded. Return original result.")
            return text
        if not text:
            return text
        try:
            if isinstance(text, str):
                return self.punctuation(text)
            return [self.punctuation(t) if t else t for t in text]
        except Exception as e:
            print(f"Failed in punctuation_restore: {e}")
            return text

    @staticmethod
    def detect_language(text: str) -> str:
        """ASRProcessor.py:1013-1031: "en" only if Latin letters outnumber CJK ideographs, else "zh" """
        chinese_count = sum(1 for ch in text if "\u4e00" <= ch <= "\u9fff")
        english_count = sum(1 for ch in text if "a" <= ch.lower() <= "z")
        return "en" if english_count > chinese_count else "zh"

    @staticmethod
    def paraformer_postprocess(result_list: list, no_punc: bool, punctuation_restore, detect_language) -> list:
        """ASRProcessor.py:427-440 verbatim in meaning: timestamps ms -> s (3 decimals), paired with the
        space-separated tokens (padded with "" when there are fewer tokens than stamps)."""
        for i, result in enumerate(result_list):
            if "timestamp" in result:
                texts = result["text"].split(" ")
                value = [[round(point / 1000, 3) for point in clip] for clip in result["timestamp"]]
                if len(texts) < len(value):
                    texts.extend([""] * (len(value) - len(texts)))
                result_list[i]["timestamp"] = [(texts[j], value[j]) for j in range(len(value))]
                if not no_punc:
                    result_list[i]["text"] = punctuation_restore(result_list[i]["text"])
            if "language" not in result:
                result_list[i]["language"] = detect_language(result["text"])
        return result_list

    # ASRProcessor.py:742-817
    def vad_detection(self, wav_file, min_silence_sec: float = 0.5, min_clip_sec: float = 0.0, max_clip_sec: float = 0.0,
                      format_to_sec: bool = True, output_folder: str = "", output_name: str = "", output_format: str = "wav"):
        """16 kHz float32 audio -> [[start, end], ...] in seconds (format_to_sec=False: the detector's own milliseconds, before the
        min_clip_sec merge and the max_clip_sec split, as the reference returns them).  `self.vad.generate(...)` (:765) is the device
        FSMN-VAD (vad.FsmnVad); an empty detection with min_clip_sec > 0 returns [] where the reference raises IndexError."""
        if self.verbose_log:
            print("\nRunning module: vad_detection")
        if not self.is_vad or self.vad is None:
            print("FunASR VAD model hasn't been loaded. Return empty result.")
            return []
        sampling_rate = 16000
        orig_audio_data = None
        if isinstance(wav_file, str):
            if not hasattr(self.ap, "read_audio"):
                raise ValueError("vad_detection: pass 16 kHz float32 numpy audio (file decoding is outside the MI355X hot path)")
            audio_data, sampling_rate = self.ap.read_audio(wav_file)
            if sampling_rate != 16000:                   # :752-755: clips are then cut from the audio at its own rate
                orig_audio_data = audio_data.copy()
                audio_data, _ = self.ap.audio_resample(audio_data=audio_data, orig_sr=sampling_rate, target_sr=16000)
            audio_data = self.ap.audio_to_mono(audio_data)
        elif isinstance(wav_file, bytes):
            if not hasattr(self.ap, "raw_bytes_to_ndarray"):
                raise ValueError("vad_detection: pass 16 kHz float32 numpy audio (byte decoding is outside the MI355X hot path)")
            audio_data = self.ap.raw_bytes_to_ndarray(audio_bytes=wav_file)
        else:
            audio_data = wav_file
        from .vad import clip_ranges
        value = self.vad.detect_batch_ms([np.asarray(audio_data, dtype=np.float32).reshape(-1)], int(min_silence_sec * 1000))[0]
        value_sec = [[round(point / 1000, 3) for point in clip] for clip in value]
        value_sec = clip_ranges(value_sec, min_clip_sec, max_clip_sec)
        if output_folder:
            if not (hasattr(self.ap, "write_to_file") and hasattr(self.ap, "split_audio_by_time")):
                print("vad_detection: output_folder needs an `ap` with split_audio_by_time and write_to_file; nothing written")
            else:
                import os
                os.makedirs(output_folder, exist_ok=True)
                for i, clip in enumerate(value_sec):
                    audio_clip = self.ap.split_audio_by_time(audio_data=audio_data if orig_audio_data is None else orig_audio_data, sampling_rate=sampling_rate, start_time=clip[0], end_time=clip[1])
                    if output_name:
                        base_name = output_name
                    elif isinstance(wav_file, str):
                        base_name = os.path.basename(wav_file).split(".")[0]
                    else:
                        base_name = os.path.abspath(output_folder).replace("\\", "/").split("/")[-1]
                    self.ap.write_to_file(output_path=f"{output_folder}/{base_name}_{i}.{output_format}", audio_data=audio_clip, sampling_rate=sampling_rate)
        return value_sec if format_to_sec else value

    # ASRProcessor.py:935-973
    def emotion_detection(self, wav_file, output_emotion_only: bool = False):
        """16 kHz float32 audio, or a list of clips -> [{"key", "cls", "emotion", "label_score"}, ...]; with output_emotion_only
        the emotion of the single clip, or the list of emotions.  `self.emotion(...)` (:945) is the device emotion2vec
        (emotion.Emotion2vec); a list goes through one call, bucketed by length."""
        if self.verbose_log:
            print("\nRunning module: emotion_detection")
        result_list = []
        if not self.is_emotion or self.emotion is None:
            print("Modelscope emotion detection model hasn't been loaded. Return empty result.")
            return "" if output_emotion_only else result_list
        clips = []
        for w in (wav_file if isinstance(wav_file, list) else [wav_file]):
            if isinstance(w, str):
                if not hasattr(self.ap, "read_audio"):
                    raise ValueError("emotion_detection: pass 16 kHz float32 numpy audio (file decoding is outside the MI355X hot path)")
                audio_data, sampling_rate = self.ap.read_audio(w)
                if sampling_rate != 16000:
                    audio_data, _ = self.ap.audio_resample(audio_data=audio_data, orig_sr=sampling_rate, target_sr=16000)
                w = self.ap.audio_to_mono(audio_data)
            elif isinstance(w, bytes):
                if not hasattr(self.ap, "raw_bytes_to_ndarray"):
                    raise ValueError("emotion_detection: pass 16 kHz float32 numpy audio (byte decoding is outside the MI355X hot path)")
                w = self.ap.raw_bytes_to_ndarray(audio_bytes=w)
            clips.append(np.asarray(w, dtype=np.float32).reshape(-1))
        res = self.emotion(clips, granularity="utterance", extract_embedding=False)
        for r in res:
            key = r["key"]
            labels = r["labels"]
            scores = [round(score, 6) for score in r["scores"]]
            top_results = sorted(zip(labels, scores), key=lambda x: x[1], reverse=True)
            emotion = top_results[0][0].split("/")[-1].strip()
            score = top_results[0][1]
            if score >= 0.95 and emotion not in ["excited"]:
                if emotion in ["fearful", "disgusted", "sad", "angry"]:
                    emotion_cls = "negative"
                else:
                    emotion_cls = "positive"
            else:
                emotion_cls = "neutral"
            result_list.append({"key": key, "cls": emotion_cls, "emotion": emotion, "label_score": top_results})
        if output_emotion_only:
            if len(result_list) == 1:
                return result_list[0]["emotion"]
            return [result["emotion"] for result in result_list]
        return result_list

    # ASRProcessor.py:1003-1010
    def f0_compute(self, wav_file, sampling_rate: int = 16000, fmin: float = 50.0, fmax: float = 300.0):
        """audio (any rate, float) -> f0 in Hz, one value per 512-sample hop, NaN where the frame is unvoiced:
        `librosa.pyin(audio_data, fmin=fmin, fmax=fmax, sr=sampling_rate)[0]` (:1009) on the device (pitch.Pyin).  No device,
        a failed init or parameters pyin rejects: the reason is printed and an empty float64 array returned."""
        if isinstance(wav_file, str):
            if not (hasattr(self.ap, "read_audio") and hasattr(self.ap, "audio_to_mono")):
                raise ValueError("f0_compute: pass float numpy audio (file decoding is outside the MI355X hot path)")
            audio_data, sampling_rate = self.ap.read_audio(wav_file)
            audio_data = self.ap.audio_to_mono(audio_data)
        else:
            audio_data = wav_file
        try:
            if self.pitch is None:
                if self.cuda_device is None or int(self.cuda_device) < 0:
                    raise RuntimeError("no device (cuda_device < 0); there is no CPU path")
                from .pitch import Pyin
                self.pitch = Pyin(f"cuda:{int(self.cuda_device)}")
            return self.pitch.pyin(np.asarray(audio_data), fmin=fmin, fmax=fmax, sr=sampling_rate)[0]
        except Exception as e:
            print(f"Failed in f0_compute: {e}")
            return np.zeros(0, dtype=np.float64)

    def asr_detection(self, wav_file, language: str = "auto", prompt: str = "", asr_engine: str = "paraformer", no_punc: bool = False,
                      output_text_only: bool = False, output_raw_result: bool = False):
        result_list = []
        if not self.is_asr or not self.asr:
            print("ASR models haven't been loaded. Return empty result.")
            return "" if output_text_only else result_list
        asr_engine = asr_engine.lower()
        if asr_engine not in self.asr:                   # :390-391 (an engine that is not loaded falls back too, where the reference raises KeyError)
            asr_engine = list(self.asr.keys())[0]
        if asr_engine == "paraformer" and self.decoder is None:
            print("ASR models haven't been loaded. Return empty result.")
            return "" if output_text_only else result_list
        if isinstance(wav_file, (str, bytes)):
            raise ValueError("asr_detection: pass 16 kHz float32 numpy audio (file decoding is outside the MI355X hot path)")
        import torch
        wavs = wav_file if isinstance(wav_file, list) else [wav_file]
        if asr_engine == "sensevoice":                   # :398-421
            from .sensevoice import join_text_only, parse_tagged_text
            res = self.asr["sensevoice"].generate(wavs, language=language, use_itn=True)
            if output_raw_result:
                return res
            for clip in res:
                lang, emo, text = parse_tagged_text(clip["text"], no_punc)
                result_list.append({"key": clip["key"], "language": lang, "text": text, "emotion": emo})
            return join_text_only(result_list) if output_text_only else result_list
        if asr_engine == "whisper_finetune":             # :489-526
            from .sensevoice import join_text_only
            m = self.asr["whisper_finetune"]
            prompt_ids = None
            if m.tokenizer is not None:                  # :505 encodes the prompt whatever it is, the empty one included
                prompt_ids = m.tokenizer.get_prompt_ids(prompt)
            elif prompt:
                print("Whisper: no tokenizer loaded, the prompt is ignored.")
            clips = [np.asarray(w, dtype=np.float32).reshape(-1)[:480000] for w in wavs]     # the feature extractor keeps 30 s
            res = m.generate(clips, language="chinese", task="transcribe", prompt_ids=prompt_ids, keys=[str(k) for k in range(len(clips))])
            if output_raw_result:
                return res
            result_list = [{"key": r["key"], "language": self.detect_language(r["text"]), "text": r["text"].strip()} for r in res]
            return join_text_only(result_list) if output_text_only else result_list
        if asr_engine in ("whisper_v2", "whisper_v3"):   # :443-488
            from .sensevoice import join_text_only
            m = self.asr[asr_engine]
            prompt_ids = None
            if m.tokenizer is not None:                  # the prompt goes through the tokenizer as for whisper_finetune
                prompt_ids = m.tokenizer.get_prompt_ids(prompt)
            elif prompt:
                print("Whisper: no tokenizer loaded, the prompt is ignored.")
            auto = language is None or str(language).lower() == "auto"
            from .whisper import fallback_options, language_code
            full = [np.asarray(w, dtype=np.float32).reshape(-1) for w in wavs]
            if self.whisper_long_form and any(w.shape[0] > 480000 for w in full):
                # whisper.transcribe's long-form loop (WhisperASR.transcribe): nothing is cut; the whole text and all words are reported
                res = m.transcribe(full, language=None if auto else str(language).lower(), task="transcribe", prompt_ids=prompt_ids,
                                   keys=[str(k) for k in range(len(full))], **fallback_options(self.whisper_fallback))
                if output_raw_result:
                    return res
                for r in res:
                    result_list.append({"key": r["key"], "language": r["language"], "text": r["text"],
                                        "timestamp": [(str(w), [float(a), float(b)]) for s in r["segments"] for w, (a, b) in s["words"]]})
                return join_text_only(result_list) if output_text_only else result_list
            clips = [w[:480000] for w in full]             # one 30 s segment per clip (the long-form loop is behind whisper_long_form)
            res = m.generate(clips, language=None if auto else str(language).lower(), task="transcribe", prompt_ids=prompt_ids,
                             keys=[str(k) for k in range(len(clips))], return_timestamps=True)
            if output_raw_result:
                return res
            for r in res:
                result_list.append({"key": r["key"], "language": r["language"] if auto else language_code(language), "text": r["text"],
                                    "timestamp": [(str(w), [float(a), float(b)]) for w, (a, b) in r["words"]]})
            return join_text_only(result_list) if output_text_only else result_list
        enc = self.asr["paraformer"]
        for k, w in enumerate(wavs):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(1, -1)))
            out = enc(x.to(enc.device))[0]
            res = dict(self.decoder(out))
            res.setdefault("key", f"clip_{k}")
            result_list.append(res)
        if output_raw_result:
            return result_list
        result_list = self.paraformer_postprocess(result_list, no_punc, self.punctuation_restore, self.detect_language)
        if output_text_only:
            return "".join(r["text"] for r in result_list)
        return result_list
