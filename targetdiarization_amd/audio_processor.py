"""AudioProcessor — drop-in for the hot-path slice of the reference's AudioProcessor
(/root/reference/AudioProcessor.py): same constructor signature (:125-130), same device
convention (:205-221), same never-raise/degrade error convention (:171-202, :886-888) and
the same `separate_speaker` contract (:885-956).  What differs is *how* it runs: all windows
of equal length are batched into ONE device launch sequence (the reference loops with
batch = 1), on the MI355X-native MossFormer2 (libtdx.so).

`denoise_vocal` (:601-713) keeps the reference's outer 15 s / 1 s-margin chunker and the block plan of
`process_audio_chunk` (:605-643) around the device STFT / iSTFT (`frontend.BlockSTFT` = ConvTDFNet.stft/.istft
:82-120); the MDX net BODY (a third-party ONNX model in the reference: no weights, no onnxruntime here) is either the device
implementation of its architecture (`mdx_state_dict` -> `mdx.ConvTDFNetBody`, csrc/mdx.hip; parity unpinned) or any plug-in
`mdx_model(spec[n,4,dim_f,dim_t]) -> spec` on device tensors.  Resampling runs on the device polyphase resampler
(`ops.resample_poly`; the reference calls librosa: parity unpinned).

`restore_audio` (:959-980) runs the Apollo restorer on the device (`apollo.ApolloRestorer`, csrc/apollo.hip) from
`<restorer_weights_folder>/pytorch_model.bin` like `init_restorer_model` (:277-281), or from an in-memory `restorer_state_dict`.

`denoise_vocal`'s other body (:654-656, `fast_mode=True` or no MDX model: `nr.reduce_noise(y=audio_data, sr=sampling_rate)`) is
noisereduce's non-stationary spectral gate on the device (`noise_gate.SpectralGate`, csrc/noise_gate.hip) behind the constructor
flag `noise_reduce=True`; with the default False the audio is returned unchanged, as before.  The third-party algorithm is
restated from upstream (package parity unpinned); where the smoothed magnitude is exactly 0 the mask is 0 (upstream: NaN).

`audio_stretch` (:468-499), `audio_pitch` (:452-465) and `eq_match` (:502-546) run librosa's phase-vocoder time stretch, its pitch
shift and the reference's spectral-mean equaliser on the device (`effects.PhaseVocoder`, csrc/pvoc.hip), created by the first
call; the audiostretchy branch of `audio_stretch` is not taken, the resampler behind the pitch shift is the project's own, and
a file name as the EQ target is refused.  They never raise: the reason is printed and the input returned.

Out of scope here: enhancer, file I/O — those flags are accepted and degrade to "module skipped" exactly like
the reference does when a package is disabled.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from .loudness import integrated_loudness
from .separator import MossFormer2Separator


class AudioProcessor:
    def __init__(self,
                 is_denoise_vocal: bool = False, mdx_weights_file: str = "mdx/weights/UVR-MDX-NET-Inst_HQ_3.onnx",
                 is_enhance_vocal: bool = False, enhancer_weights_folder: str = "resemble_enhance/model_repo/enhancer_stage2",
                 is_separate_audio: bool = False, separater_weights_folder: str = "look2hear/checkpoints/TFGNet-Noise",
                 is_restore_audio: bool = False, restorer_weights_folder: str = "JusperLee/Apollo",
                 verbose_log: bool = True, cuda_device: int = 0, quality: int = 2,
                 separater_state_dict=None, mdx_model=None, mdx_dim_f: int = 3072, mdx_n_fft: int = 6144, silero_vad=None,
                 mdx_state_dict=None, mdx_args=None, restorer_state_dict=None, silero_state_dict=None, silero_model_file=None,
                 noise_reduce: bool = False):
        """`separater_state_dict` (extension): an in-memory state_dict instead of
        `<separater_weights_folder>/best_model.pth` — no checkpoint ships with the reference.
        `mdx_model` (extension): the MDX net body as a callable on device tensors, spec[n,4,dim_f,256] -> spec (the
        reference runs the ONNX file through onnxruntime, AudioProcessor.py:231-233,630); without it the denoiser is off,
        like a failed `init_mdx_model` (:171-176).  `mdx_dim_f` / `mdx_n_fft`: the ONNX metadata the reference reads (:234-237).
        `restorer_state_dict` (extension): the Apollo weights in memory instead of `<restorer_weights_folder>/pytorch_model.bin`
        (the reference's 6 layers, or as many as the dict holds).
        `silero_state_dict` / `silero_model_file` (extension): silero-VAD's weights in memory or as a file; without a `silero_vad`
        plug-in they put the device detector (silero.SileroVad.frames) behind `separate_speaker(low_gpu_ram=True)`.
        `noise_reduce` (extension): run noisereduce's spectral gate on the device (noise_gate.SpectralGate) where the reference
        calls `nr.reduce_noise` (:655): `denoise_vocal(fast_mode=True)` and the denoiser-off case.  False: audio returned unchanged."""
        if is_denoise_vocal and mdx_model is None and mdx_state_dict is not None:
            # the ConvTDFNet body on the device (mdx.ConvTDFNetBody, csrc/mdx.hip) from a state dict with the PyTorch module names;
            # `mdx_args`: its geometry (L, l, g, k, bn, dim_f, dim_t, max_blocks_per_launch).  A failure prints and leaves the denoiser
            # off, like a failed `init_mdx_model` (AudioProcessor.py:171-176)
            try:
                from .mdx import ConvTDFNetBody
                mdx_model = ConvTDFNetBody(mdx_state_dict, f"cuda:{0 if cuda_device is None else cuda_device}", **(mdx_args or {}))
            except Exception as e:
                print(f"Failed to init MDX model: {e}")
        self.is_denoise_vocal = bool(is_denoise_vocal and mdx_model is not None)
        self.mdx_model = mdx_model
        self.silero_vad = silero_vad            # low_gpu_ram plug-in: silero_vad(audio[n] f32 @16 kHz) -> [[start, end], ...] in samples (:903-905)
        if silero_vad is None and (silero_state_dict is not None or silero_model_file is not None):
            try:                                # the device silero-VAD (silero.py, tdx_silero_*); a source that fails prints and leaves None
                from .silero import build_silero
                model = build_silero(silero_state_dict, silero_model_file, 0 if cuda_device is None else cuda_device)
                self.silero_vad = model.frames if model is not None else None
            except Exception as e:
                print(f"Failed to load silero VAD model: {e}")
        self.mdx_net = None
        self._mdx_geom = (mdx_n_fft, {1: 256, 2: 1024, 3: 2048}.get(quality, 1024), mdx_dim_f)        # :225-240
        if is_denoise_vocal and mdx_model is None:
            print("Failed to init MDX model: the MDX net body is a third-party ONNX model; pass mdx_model=callable(spec)->spec")
        self.is_enhance_vocal = False
        self.is_separate_audio = is_separate_audio
        self.mdx_weights_file = mdx_weights_file.replace("\\", "/")
        self.enhancer_weights_folder = enhancer_weights_folder.replace("\\", "/")
        self.separater_weights_folder = separater_weights_folder.replace("\\", "/").rstrip("/")
        self.restorer_weights_folder = restorer_weights_folder.replace("\\", "/")
        self.verbose_log = verbose_log
        self.cuda_device = cuda_device
        self.quality = quality
        self.separater = None
        self.get_device()
        if self.is_separate_audio and (separater_state_dict is not None or os.path.isdir(self.separater_weights_folder)):
            try:
                self.init_separater_model(separater_state_dict)
            except Exception as e:                       # AudioProcessor.py:189-193
                print(f"Failed to init separater model: {e}")
                self.is_separate_audio = False
        else:
            self.is_separate_audio = False
        self.noise_gate = None
        self.noise_reduce = bool(noise_reduce) and str(self.device) != "cpu"
        if self.noise_reduce:
            try:
                from .noise_gate import SpectralGate
                self.noise_gate = SpectralGate("cuda:0" if self.device == "cuda" else self.device)
            except Exception as e:
                print(f"Failed to init noise gate: {e}")
                self.noise_reduce = False
        self.effects = None                              # effects.PhaseVocoder, created by the first audio_stretch / audio_pitch / eq_match
        self.fft = None                                  # fft.DeviceFFT, created by the first mix_audio_by_freq
        self.restorer = None
        self.is_restore_audio = is_restore_audio
        if self.is_restore_audio and (restorer_state_dict is not None or os.path.isdir(self.restorer_weights_folder)):
            try:
                self.init_restorer_model(restorer_state_dict)
            except Exception as e:                       # AudioProcessor.py:195-200
                print(f"Failed to init restorer model: {e}")
                self.is_restore_audio = False
        else:
            self.is_restore_audio = False

    # AudioProcessor.py:205-221 — None -> auto, -1 -> cpu, n -> cuda:n
    def get_device(self):
        if self.cuda_device is None:
            self.device = "cuda" if torch.cuda.is_available() else "cpu"
        elif self.cuda_device == -1:
            self.device = "cpu"
        else:
            self.device = f"cuda:{self.cuda_device}"
            try:
                torch.cuda.set_device(self.device)
            except Exception as e:
                print(f"Failed to set CUDA device: {e}")

    # AudioProcessor.py:268-274 (config.yaml's model: block only carries constructor kwargs;
    # the MI355X build supports the constructor defaults + num_blocks)
    def init_separater_model(self, state_dict=None):
        if str(self.device) == "cpu":
            raise _lib.TdxError("the MI355X build has no CPU separator (cuda_device=-1 is not supported)")
        dev = "cuda:0" if self.device == "cuda" else self.device
        if state_dict is not None:
            self.separater = MossFormer2Separator(state_dict, device=dev)
        else:
            # config.yaml's `model:` block minus `_target_` = constructor kwargs (AudioProcessor.py:269-271)
            model_args = {}
            cfg_path = f"{self.separater_weights_folder}/config.yaml"
            if os.path.exists(cfg_path):
                import yaml
                with open(cfg_path) as fh:
                    model_args = dict((yaml.safe_load(fh) or {}).get("model", {}) or {})
                model_args.pop("_target_", None)
            self.separater = MossFormer2Separator.from_pretrain(f"{self.separater_weights_folder}/best_model.pth", device=dev, **model_args)
        self.separater.eval()

    # AudioProcessor.py:277-281 (sr=44100, win=20, feature_dim=256, layer=6; BaseModel.from_pretrain loads strictly)
    def init_restorer_model(self, state_dict=None):
        from .apollo import ApolloRestorer, load_state_dict
        if str(self.device) == "cpu":
            raise _lib.TdxError("the MI355X build has no CPU restorer (cuda_device=-1 is not supported)")
        num_layers = 6
        if state_dict is None:
            state_dict = load_state_dict(self.restorer_weights_folder)
        else:                                            # in-memory weights: as many BSNet layers as they hold
            num_layers = sum(1 for k in state_dict if k.endswith("band_net.cos_freq"))
        self.restorer = ApolloRestorer(state_dict, device=self._dev(), num_layers=num_layers).eval()

    # AudioProcessor.py:959-980
    def restore_audio(self, audio_data, sampling_rate: int, keep_sampling_rate: bool = False, output_audio_only: bool = False):
        """Resample to 44.1 kHz, restore, and optionally resample back.  Mono [n] -> [n]; [n, C] is restored as C independent clips
        and returned as [C, n] (the reference's squeezed model output).  numpy in -> numpy out, device tensor in -> device tensor
        out.  Returns (audio, rate) — rate 44100 unless keep_sampling_rate — or the audio alone with output_audio_only.
        Unlike the reference, keep_sampling_rate resamples a [C, n] result along time: the reference hands the [C, n] array to a
        resampler that expects [n, C], i.e. it resamples across channels."""
        if not self.is_restore_audio:
            print("\nSkip module: restore_audio")
            return audio_data
        if self.verbose_log:
            print("\nRunning module: restore_audio")
        orig_sr = sampling_rate
        is_np = isinstance(audio_data, np.ndarray)
        x = torch.from_numpy(np.ascontiguousarray(audio_data, dtype=np.float32)) if is_np else audio_data
        x = x.to(self._dev(), torch.float32)
        x, sampling_rate = self.audio_resample(x, orig_sr, 44100)
        outs = self.restorer([x] if x.ndim == 1 else list(x.t()))
        out = outs[0] if x.ndim == 1 or x.shape[1] == 1 else torch.stack(outs)
        if keep_sampling_rate:
            out, sampling_rate = self.audio_resample(out if out.ndim == 1 else out.t(), 44100, orig_sr)
            out = out if out.ndim == 1 else out.t().contiguous()
        if is_np:
            out = out.cpu().numpy().astype(np.float32)
        if output_audio_only:
            return out
        return out, sampling_rate

    def restore_streams_device(self, streams, sampling_rate: int = 16000):
        """restore_audio(keep_sampling_rate=True, output_audio_only=True) for a list of 1-D device streams: resampled to 44.1 kHz
        (equal lengths share a launch), ONE restorer call for all of them, resampled back"""
        if not streams:
            return []
        return self._resample_many(self.restorer(self._resample_many(streams, sampling_rate, 44100)), 44100, sampling_rate)

    @staticmethod
    def _resample_many(xs, orig_sr: int, target_sr: int):
        from . import ops
        if orig_sr == target_sr:
            return list(xs)
        out, by_len = [None] * len(xs), {}
        for i, x in enumerate(xs):
            by_len.setdefault(int(x.shape[0]), []).append(i)
        for idxs in by_len.values():
            y = ops.resample_poly(torch.stack([xs[i] for i in idxs]), orig_sr, target_sr)
            for j, i in enumerate(idxs):
                out[i] = y[j]
        return out

    # AudioProcessor.py:1123-1127
    def meter_loudness(self, audio_data: np.ndarray, sampling_rate: int):
        return round(integrated_loudness(audio_data, sampling_rate), 1)

    @staticmethod
    def window_plan(n: int, window_size: int = 160000, start: int = 0):
        """[start,end) windows for one VAD frame — AudioProcessor.py:920-935."""
        starts, ends = [], []
        k = n // window_size
        if k == 0:
            starts.append(start); ends.append(start + n)
        else:
            for j in range(k):
                starts.append(start + j * window_size); ends.append(start + (j + 1) * window_size)
            if n % window_size > 0:
                if n % window_size > window_size / 2:
                    starts.append(ends[-1]); ends.append(start + n)
                else:
                    ends[-1] = start + n
        return list(zip(starts, ends))

    def separate_windows_device(self, windows, max_batch: int = 32):
        """Run the separator on a list of 1-D float32 windows (host arrays or device tensors); windows of
        equal length share one batched forward (bit-compatible with B=1: the model has no cross-sample op and
        the reference never pads a batch, mossformer_block.py:485).  Returns a list of [2,T] DEVICE tensors."""
        out = [None] * len(windows)
        by_len = {}
        for i, w in enumerate(windows):
            by_len.setdefault(int(w.shape[0]), []).append(i)
        dev = self.separater.device
        for T, idxs in by_len.items():
            for c in range(0, len(idxs), max_batch):         # bound the workspace: <= max_batch windows / launch
                chunk = idxs[c:c + max_batch]
                if isinstance(windows[chunk[0]], torch.Tensor):
                    x = torch.stack([windows[i] for i in chunk]).to(dev, torch.float32)
                else:
                    x = torch.from_numpy(np.stack([windows[i] for i in chunk]).astype(np.float32, copy=False)).to(dev)
                y = self.separater(x)
                for j, i in enumerate(chunk):
                    out[i] = y[j]
        return out

    def separate_windows(self, windows):
        """as above, host arrays"""
        return [t.cpu().numpy() for t in self.separate_windows_device(windows)]

    def louder_first_device(self, pairs):
        """The reference's LUFS compare & swap (AudioProcessor.py:949-952) for a list of device stream pairs
        [2,n]: one BS.1770 launch per distinct length (tdx_loudness), values rounded to 0.1 like meter_loudness
        (:1123-1127).  Only the [k,2] loudness values cross to the host (the rounding rule is Python's); the
        streams stay on the device.  Returns the list of [2,n] device tensors, louder stream first."""
        from . import ops
        swap = [False] * len(pairs)
        by_len = {}
        for i, p in enumerate(pairs):
            by_len.setdefault(int(p.shape[1]), []).append(i)
        for n, idxs in by_len.items():
            if n < 6400:
                continue                                      # shorter than one 400 ms gating block: the reference's ValueError path
            l = ops.loudness(torch.cat([pairs[i] for i in idxs], 0), 16000).cpu().numpy().reshape(len(idxs), 2)
            for k, i in enumerate(idxs):
                swap[i] = round(float(l[k, 0]), 1) < round(float(l[k, 1]), 1)
        return [p.flip(0) if swap[i] else p for i, p in enumerate(pairs)]

    def louder_first(self, pairs):
        """host form: list of (spk1, spk2) numpy arrays"""
        res = []
        for p in self.louder_first_device(pairs):
            h = p.cpu().numpy()
            res.append((h[0], h[1]))
        return res

    # ---- AudioProcessor.py:350-383 (pure numpy in the reference; torch here, same arithmetic) ----
    @staticmethod
    def mono_to_stereo(audio):
        return audio.reshape(-1, 1).repeat(1, 2) if audio.ndim == 1 else audio

    @staticmethod
    def audio_to_mono(audio):
        return audio if audio.ndim == 1 else audio.double().mean(dim=1).float()      # np.average with unit weights, float64 accumulate

    def audio_resample(self, audio_data, orig_sr: int, target_sr: int, output_audio_only: bool = False):
        """:549-569 on the device (`ops.resample_poly`); numpy in -> numpy out, device tensor in -> device tensor out"""
        from . import ops
        if target_sr == orig_sr:
            return audio_data if output_audio_only else (audio_data, target_sr)
        is_np = isinstance(audio_data, np.ndarray)
        x = torch.from_numpy(np.ascontiguousarray(audio_data, dtype=np.float32)).to(self._dev()) if is_np else audio_data
        y = ops.resample_poly(x if x.ndim == 1 else x.t().contiguous(), orig_sr, target_sr)
        y = y if y.ndim == 1 else y.t().contiguous()
        if is_np:
            y = y.cpu().numpy().astype(np.float32)
        return y if output_audio_only else (y, target_sr)

    def _dev(self):
        return torch.device("cuda:0" if self.device == "cuda" else self.device)

    def _effects(self):
        if self.effects is None:
            if str(self.device) == "cpu":
                raise _lib.TdxError("no device (cuda_device=-1); there is no CPU path")
            from .effects import PhaseVocoder
            self.effects = PhaseVocoder(self._dev())
        return self.effects

    @staticmethod
    def _channels_first(audio_data, who):
        a = np.asarray(audio_data)
        if a.ndim not in (1, 2) or a.size == 0:
            raise ValueError(f"{who}: the audio must be [n] or [n, C] and not empty, got shape {a.shape}")
        return np.ascontiguousarray(a.T, dtype=np.float32)

    # AudioProcessor.py:452-465
    def audio_pitch(self, audio_data: np.ndarray, sampling_rate: int, pitch_semitone: float):
        """`librosa.effects.pitch_shift(audio_data, sr=sampling_rate, n_steps=pitch_semitone)` per channel on the device:
        [n] -> [n], [n, C] -> [n, C] float32.  A failure prints its reason and returns the input."""
        if self.verbose_log:
            print("\nRunning module: audio_pitch")
            print(f"Pitch semitone: {pitch_semitone}")
        if pitch_semitone == 0.0:
            if self.verbose_log:
                print("Pitch semitone is zero. Skip.")
            return audio_data
        try:
            out = self._effects().pitch_shift(self._channels_first(audio_data, "audio_pitch"), sampling_rate, float(pitch_semitone))
            return np.ascontiguousarray(out.T)
        except Exception as e:
            print(f"Failed in audio_pitch: {e}")
            return audio_data

    # AudioProcessor.py:468-499 (the librosa branch; the int16 round trip of the audiostretchy branch is not taken)
    def audio_stretch(self, audio_data: np.ndarray, sampling_rate: int, speed_factor: float):
        """`librosa.effects.time_stretch(audio_data, rate=speed_factor)` per channel on the device: [n] -> [round(n / speed_factor)],
        [n, C] -> [n', C] float32.  A negative factor or a failure prints its reason and returns the input."""
        if self.verbose_log:
            print("\nRunning module: audio_stretch")
            print(f"Speed factor: {speed_factor}")
        if speed_factor == 0.0:
            if self.verbose_log:
                print("Speed factor is zero. Skip.")
            return audio_data
        if not speed_factor > 0:
            print(f"Speed factor {speed_factor} is not positive. Skip.")
            return audio_data
        try:
            out = self._effects().time_stretch(self._channels_first(audio_data, "audio_stretch"), float(speed_factor))
            return np.ascontiguousarray(out.T)
        except Exception as e:
            print(f"Failed in audio_stretch: {e}")
            return audio_data

    # AudioProcessor.py:502-546
    def eq_match(self, source_audio: np.ndarray, target_audio, source_sampling_rate: int = 16000, target_sampling_rate: int = 16000,
                 n_fft: int = 2048, hop_length: int = 512):
        """The reference's EQ match of a mono source to a target given as an ndarray or as a dict with `array` / `stft` /
        `sampling_rate` / `n_fft` / `hop_length` (:511-518).  A file name as the target (audio or .pkl: there is no file decoding
        here, and this library does not unpickle files), a 2-D source or a failure prints its reason and returns the source."""
        target_stft = None
        if isinstance(target_audio, str):
            print("eq_match: a file name as the target is not supported (pass the array, or the dict of a target pickle); source returned unchanged")
            return source_audio
        if isinstance(target_audio, dict):
            target_dict = target_audio.copy()
            target_audio = target_dict.get("array", None)
            target_stft = target_dict.get("stft", None)
            target_sampling_rate = target_dict.get("sampling_rate", 16000)
            n_fft = target_dict.get("n_fft", 2048)
            hop_length = target_dict.get("hop_length", 512)
        if hop_length > n_fft:
            hop_length = int(n_fft / 4)
        if self.verbose_log:
            print("\nRunning module: eq_match")
            print(f"FFT window size: {n_fft}")
            print(f"Hop length: {hop_length}")
        if np.asarray(source_audio).ndim != 1:
            print(f"eq_match: the source must be mono [n], got shape {np.asarray(source_audio).shape}; source returned unchanged")
            return source_audio
        try:
            fx = self._effects()
            source = np.asarray(source_audio, dtype=np.float32)
            if source_sampling_rate < target_sampling_rate:
                source, _ = self.audio_resample(source, source_sampling_rate, target_sampling_rate)
            elif source_sampling_rate > target_sampling_rate:
                if target_audio is None and target_stft is not None:
                    target_audio = fx.istft(target_stft, hop_length=hop_length)          # :529 (n_fft from the bins, as upstream)
                    target_stft = None
                target_audio, _ = self.audio_resample(np.asarray(target_audio, dtype=np.float32), target_sampling_rate, source_sampling_rate)
            if target_stft is None:
                out = fx.eq_match(source, target=target_audio, n_fft=n_fft, hop_length=hop_length)
            else:
                out = fx.eq_match(source, target_stft=target_stft, n_fft=n_fft, hop_length=hop_length)
            if source_sampling_rate < target_sampling_rate:
                out, _ = self.audio_resample(out, target_sampling_rate, source_sampling_rate)
            return out
        except Exception as e:
            print(f"Failed in eq_match: {e}")
            return source_audio

    # ---- AudioProcessor.py:386-414, 786-842: one elementwise pass over data that lives on the host (and numpy's global random
    # stream, which np.random.seed must keep reproducing) — host-only on purpose, plain numpy with the reference's arithmetic
    def audio_gain(self, audio_data: np.ndarray, gain_db: float, clip_limit: bool = False):
        if self.verbose_log:
            print("\nRunning module: audio_gain")
            print(f"Gain dB: {gain_db}")
            print(f"Apply clip limit: {clip_limit}")
        if gain_db == 0.0:
            if self.verbose_log:
                print("gain_db is zero. Skip.")
            return audio_data
        output_audio = audio_data * 10 ** (gain_db / 20.0)
        if clip_limit:
            output_audio = np.clip(output_audio, -1, 1)
        return output_audio

    def audio_normalize(self, audio_data: np.ndarray, target_peak_db: float = -0.1):
        if self.verbose_log:
            print("\nRunning module: audio_normalize")
            print(f"Target peak dB: {target_peak_db}")
        current_peak = np.max(np.abs(audio_data))
        if current_peak == 0.0:
            return audio_data
        gain_db = target_peak_db - 20 * np.log10(current_peak)
        return np.clip(audio_data * 10 ** (gain_db / 20), -1.0, 1.0)

    def generate_noise(self, sampling_rate: int = 16000, duration_sec: float = 1.0, gain_db: float = 0.0, noise_type: str = "brown"):
        """white / pink / brown noise or silence, float32 [int(duration_sec * sampling_rate)]; the pink filter runs in float64"""
        n = int(duration_sec * sampling_rate)
        white = np.random.normal(0, 1, n)             # drawn for every type, silence included: the global stream advances alike
        if noise_type == "silence":
            shaped = np.zeros(n)
        elif noise_type == "pink":                    # 1 / sqrt(f) on the spectrum (bin 0 kept), peak-normalised
            f = np.fft.rfftfreq(n, d=1.0 / sampling_rate)
            shaped = np.fft.irfft(np.fft.rfft(white) * np.concatenate(([1], 1 / np.sqrt(f[1:]))), n=n)
            shaped = shaped / np.max(np.abs(shaped))
        elif noise_type == "brown":                   # a random walk, peak-normalised
            shaped = np.cumsum(white)
            shaped = shaped / np.max(np.abs(shaped))
        else:                                         # any other name: the white noise as drawn
            shaped = white
        out = shaped.astype(np.float32)
        return out if gain_db == 0.0 else self.audio_gain(out, gain_db)

    @staticmethod
    def _to_mono_host(audio_data: np.ndarray):
        """int16_to_float32 + audio_to_mono of the reference (:350-368, :1043-1048) for one [n, C] host array"""
        if np.issubdtype(audio_data.dtype, np.floating):
            audio_data = audio_data.astype(np.float32)
        else:
            audio_data = np.clip(audio_data / 32768.0, -1.0, 1.0).astype(np.float32)
        channels = audio_data.shape[1]
        weights = {6: np.array([1, 1, 1, 0.5, 0.7, 0.7]), 8: np.array([1, 1, 1, 0.5, 0.7, 0.7, 0.5, 0.5])}.get(channels, np.ones(channels))
        return np.average(audio_data.reshape((-1, channels)), axis=1, weights=weights).astype(np.float32)

    def mix_audio(self, audio_data_list: list, combine_channels: bool = True, normalize: bool = True):
        """Sum (or stack as channels) a list of clips, the shorter ones padded with silence; like the reference, multi-channel
        entries of the caller's list are replaced by their mono mix."""
        if self.verbose_log:
            print("\nRunning module: mix_audio")
        if isinstance(audio_data_list, np.ndarray):
            print("Input should be a np.ndarray audio list.")
            return audio_data_list
        if len(audio_data_list) == 1:
            print("Length of audio_data_list should be greater than 2.")
            return audio_data_list[0]
        for i, clip in enumerate(audio_data_list):
            if clip.ndim > 1:
                audio_data_list[i] = self._to_mono_host(clip)
        length = max((c.shape[0] for c in audio_data_list), default=0)
        rows = [c if c.shape[0] == length else np.concatenate((c, np.zeros(length - c.shape[0], dtype=np.float32))) for c in audio_data_list]
        if combine_channels:
            mixed = np.zeros(length, dtype=np.float32)
            for r in rows:                           # in list order, one at a time: the sum's rounding is the reference's
                mixed = mixed + r
        else:
            mixed = np.stack(rows, axis=1)
        mixed = mixed.astype(np.float32)
        return self.audio_normalize(mixed) if normalize else mixed

    def _fft(self):
        if self.fft is None:
            if str(self.device) == "cpu":
                raise _lib.TdxError("no device (cuda_device=-1); there is no CPU path")
            from .fft import DeviceFFT
            self.fft = DeviceFFT(self._dev())
        return self.fft

    # AudioProcessor.py:845-882
    def mix_audio_by_freq(self, audio_main: np.ndarray, audio_aux: np.ndarray, sampling_rate: int = 16000, main_freq_range=[0, 4000],
                          aux_freq_range=[0, 8000], force_align: bool = False):
        """The spectrum of `audio_main` in main_freq_range, that of `audio_aux` in aux_freq_range and a linear cross-fade where the two
        overlap, transformed back: float32 [2 * (n // 2)] (the reference calls irfft without a length, so an odd clip comes back one
        sample shorter; it returns float64).  One whole-clip FFT on the device (fft.DeviceFFT.band_mix, csrc/fft.hpp).  With force_align
        a shorter aux is padded with silence (the reference pads main instead and then fails).  Clips of different lengths without
        force_align, input that is not 1-D, fewer than 2 samples or a failure print their reason and return audio_main."""
        if self.verbose_log:
            print("\nRunning module: mix_audio_by_freq")
        try:
            main, aux = np.asarray(audio_main), np.asarray(audio_aux)
            if main.ndim != 1 or aux.ndim != 1:
                print(f"mix_audio_by_freq: the clips must be 1-D, got shapes {main.shape} and {aux.shape}; audio_main returned unchanged")
                return audio_main
            if main.shape[0] != aux.shape[0]:
                if not force_align:
                    print("audio_main and audio_aux should have same lengths with same sampling rates.")
                    return audio_main
                if main.shape[0] < aux.shape[0]:
                    aux = aux[:main.shape[0]]
                else:
                    aux = np.concatenate((aux, np.zeros(main.shape[0] - aux.shape[0], dtype=aux.dtype)))
            if main.shape[0] < 2:
                print("mix_audio_by_freq: the clips need at least 2 samples; audio_main returned unchanged")
                return audio_main
            from .fft import band_mix_plan
            plan = band_mix_plan(main.shape[0], sampling_rate, list(main_freq_range) if main_freq_range else None,
                                 list(aux_freq_range) if aux_freq_range else None)
            if self.verbose_log:
                print(f"Frequency selected from audio_main: {plan['main_freq_range']}")
                print(f"Frequency selected from audio_aux: {plan['aux_freq_range']}")
            return self._fft().band_mix(main, aux, plan)
        except Exception as e:
            print(f"Failed in mix_audio_by_freq: {e}")
            return audio_main

    def init_mdx_model(self):
        """:224-241: the block STFT geometry (hop by `quality`, dim_t = 2**8 frames)"""
        from .frontend import BlockSTFT
        n_fft, hop, dim_f = self._mdx_geom
        self.mdx_net = BlockSTFT(n_fft=n_fft, hop=hop, dim_f=dim_f, dim_t=256, device=self._dev())

    @staticmethod
    def mdx_segments(total_samples: int, chunk_size: int, margin_size: int):
        """The outer chunker of denoise_vocal (:666-706) as index arithmetic: [(start, end, start_trim, end_trim)] — segment
        [start, end) of the audio is processed and [start_trim, len - end_trim) of the result is kept (end_trim None = to the end);
        the trims are clamped to half the PROCESSED segment's length, which equals the segment's length (:693-699)."""
        if total_samples <= chunk_size:
            return [(0, total_samples, 0, None)]
        margin_size = min(margin_size, chunk_size)
        segs, cursor, k = [], 0, 0
        while cursor < total_samples:
            start = max(0, cursor - (0 if k == 0 else margin_size))
            chunk_end = cursor + chunk_size
            last = chunk_end >= total_samples
            end = total_samples if last else min(chunk_end + margin_size, total_samples)
            segs.append([start, end])
            k += 1
            cursor += chunk_size
            if last:
                break
        out = []
        for i, (a, b) in enumerate(segs):
            n = b - a
            out.append((a, b, 0 if i == 0 else min(margin_size, n // 2), None if i == len(segs) - 1 else min(margin_size, n // 2)))
        return out

    # AudioProcessor.py:601-713
    def denoise_vocal(self, audio_data: np.ndarray, sampling_rate: int = 16000, fast_mode: bool = False):
        if not self.is_denoise_vocal:
            fast_mode = True
        if self.verbose_log:
            print("\nRunning module: denoise_vocal")
            print("Using method: noisereduce" if fast_mode else f"Using method: MDX-Net\nUsing model: {self.mdx_weights_file}")
        if fast_mode and self.noise_reduce:
            return self.noise_gate.reduce_noise(audio_data, sampling_rate)                 # :655
        if fast_mode:
            print("denoise_vocal: noisereduce (fast_mode) runs on the device only with noise_reduce=True; audio returned unchanged")
            return audio_data
        if self.mdx_net is None:
            self.init_mdx_model()
        net = self.mdx_net
        dev = self._dev()
        x = torch.from_numpy(np.ascontiguousarray(audio_data, dtype=np.float32)).to(dev)
        new_sr = sampling_rate
        if sampling_rate != 44100:
            x, new_sr = self.audio_resample(x, sampling_rate, 44100)
        is_mono = x.ndim == 1
        if is_mono:
            x = self.mono_to_stereo(x)
        total = x.shape[0]
        segs = self.mdx_segments(total, int(15.0 * new_sr), int(1.0 * new_sr))
        # ---- process_audio_chunk (:605-643) for ALL segments in one batched STFT -> net -> iSTFT
        trim = net.n_fft // 2
        gen = net.chunk_size - 2 * trim
        blocks, plan = [], []
        for (a, b, _, _) in segs:
            n = b - a
            pad = (gen - (n % gen)) % gen
            mix = torch.cat((torch.zeros(2, trim, device=dev), x[a:b].t(), torch.zeros(2, pad + trim, device=dev)), dim=1)
            blk = mix.unfold(1, net.chunk_size, gen).permute(1, 0, 2)            # [nb, 2, chunk], stride gen (:613-617)
            plan.append((n, pad, blk.shape[0]))
            blocks.append(blk)
        waves = torch.cat(blocks, 0).contiguous()
        spec = net.stft(waves)
        pred = self.mdx_model(spec)
        wav = net.istft(pred)                                                   # [nb_total, 2, chunk]
        inst = "inst" in os.path.basename(self.mdx_weights_file).lower()
        outs, k = [], 0
        for (a, b, t0, t1), (n, pad, nb) in zip(segs, plan):
            o = wav[k:k + nb, :, trim:net.chunk_size - trim].transpose(0, 1).reshape(2, -1)
            k += nb
            o = o[:, :o.shape[1] - pad] if pad > 0 else o[:, :0]                   # `[:, :-pad]` is EMPTY when pad == 0 (:637)
            o = o.t()
            if inst:
                if o.shape[0] != n:                                             # numpy: (n,2) - (0,2) cannot broadcast
                    raise ValueError(f"operands could not be broadcast together with shapes ({n},2) ({o.shape[0]},2) ")
                o = torch.clamp(x[a:b] - o, -1.0, 1.0)
            else:
                o = torch.clamp(o, -1.0, 1.0)
            outs.append(o[t0:(o.shape[0] - t1) if t1 is not None else None] if len(segs) > 1 else o)
        out = torch.cat(outs, 0) if len(outs) > 1 else outs[0]
        if is_mono:
            out = self.audio_to_mono(out)
        if new_sr != sampling_rate:
            out, _ = self.audio_resample(out, new_sr, sampling_rate)
        return out.cpu().numpy().astype(np.float32)

    # AudioProcessor.py:885-956
    def separate_speaker(self, audio_data: np.ndarray, sampling_rate: int = 16000, low_gpu_ram: bool = False):
        if not self.is_separate_audio:
            print("\nSkip module: separate_speaker")
            return audio_data, audio_data
        orig_sr = sampling_rate
        if sampling_rate != 16000:                                   # :889-891
            audio_data, sampling_rate = self.audio_resample(np.asarray(audio_data, dtype=np.float32), sampling_rate, 16000)
        window_size, is_vad = (16000, True) if low_gpu_ram else (160000, False)      # :892-897
        if self.verbose_log:
            print("\nRunning module: separate_speaker")
            print(f"Window size: {window_size}")
            print(f"Use VAD: {is_vad}")
        if is_vad:
            # :903-905 — silero VAD: the device detector (silero_state_dict / silero_model_file) or a plug-in,
            # silero_vad(audio[n] f32) -> [[start, end], ...] in samples
            if self.silero_vad is None:
                print("separate_speaker: low_gpu_ram needs silero-VAD weights or a silero_vad plug-in; treating the whole clip as one speech frame")
                vad_frames = [[0, audio_data.shape[0]]]
            else:
                vad_frames = [[int(a), int(b)] for a, b in self.silero_vad(audio_data)]
        else:
            vad_frames = [[0, audio_data.shape[0]]]
        # :908-948 as a plan: the output is [zeros up to the first frame][frame 0][zeros between frames][frame 1]... (nothing
        # after the last frame: the reference's output is shorter than its input when the VAD cuts the tail); every window of
        # every frame goes through the separator, equal lengths batched
        pieces, wins, filled = [], [], 0
        for i, (f0, f1) in enumerate(vad_frames):
            if f0 > filled:
                gap = f0 if i == 0 else f0 - vad_frames[i - 1][1]
                pieces.append(("zeros", gap)); filled += gap
            for (a, b) in self.window_plan(f1 - f0, window_size, f0):
                if b - a < 16:
                    # MossFormer2's encoder needs >= kernel_size samples (the reference would raise inside conv1d)
                    pieces.append(("zeros", b - a))
                else:
                    pieces.append(("win", len(wins))); wins.append(audio_data[a:b].astype(np.float32, copy=True))
                filled += b - a
        if not wins:
            return audio_data, audio_data
        max_batch = max(1, min(512, (32 * 160000) // max(len(w) for w in wins)))
        outs = self.separate_windows_device(wins, max_batch)
        dev = outs[0].device
        cat = torch.cat([outs[k] if kind == "win" else torch.zeros(2, k, device=dev) for kind, k in pieces], dim=1)
        spk1, spk2 = self.louder_first([cat])[0]                     # louder stream first, :949-952 (metered on the device)
        if orig_sr != sampling_rate:                                 # :953-955
            spk1 = self.audio_resample(spk1, sampling_rate, orig_sr, output_audio_only=True)
            spk2 = self.audio_resample(spk2, sampling_rate, orig_sr, output_audio_only=True)
        return spk1, spk2
