"""ctypes binding of libtdx.so (include/tdx.h).  Fails loudly when the library is missing:
there is no CPU / PyTorch fallback anywhere in the product path."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libtdx.so")


class TdxError(RuntimeError):
    pass


class Mf2Config(C.Structure):
    _fields_ = [("num_blocks", C.c_int32), ("channels", C.c_int32), ("kernel_size", C.c_int32),
                ("num_spks", C.c_int32), ("group_size", C.c_int32), ("reserved", C.c_int32 * 3)]


class MdxConfig(C.Structure):
    _fields_ = [("num_blocks", C.c_int32), ("l", C.c_int32), ("g", C.c_int32), ("k", C.c_int32), ("bn", C.c_int32),
                ("dim_f", C.c_int32), ("dim_t", C.c_int32), ("reserved", C.c_int32)]


class WhisperConfig(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("n_audio_ctx", C.c_int32), ("d_model", C.c_int32), ("enc_heads", C.c_int32),
                ("enc_layers", C.c_int32), ("enc_ffn", C.c_int32), ("n_text_ctx", C.c_int32), ("dec_heads", C.c_int32),
                ("dec_layers", C.c_int32), ("dec_ffn", C.c_int32), ("vocab", C.c_int32), ("gelu", C.c_int32), ("reserved", C.c_int32 * 4)]


class Emo2vConfig(C.Structure):
    _fields_ = [("C", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("E", C.c_int32), ("prenet_depth", C.c_int32), ("depth", C.c_int32),
                ("n_conv", C.c_int32), ("conv_k", C.c_int32 * 8), ("conv_s", C.c_int32 * 8), ("pos_layers", C.c_int32), ("pos_k", C.c_int32),
                ("pos_groups", C.c_int32), ("n_classes", C.c_int32), ("reserved", C.c_int32 * 4)]


class PyinParams(C.Structure):
    _fields_ = [("frame_length", C.c_int32), ("win_length", C.c_int32), ("hop_length", C.c_int32), ("center", C.c_int32),
                ("min_period", C.c_int32), ("max_period", C.c_int32), ("n_pitch_bins", C.c_int32), ("n_thresholds", C.c_int32),
                ("width", C.c_int32), ("reserved", C.c_int32 * 3), ("sr", C.c_double), ("fmin", C.c_double), ("bins_per_octave", C.c_double),
                ("no_trough_prob", C.c_double), ("log_stay", C.c_double), ("log_switch", C.c_double), ("log_init_unvoiced", C.c_double)]


_lib = None

# every symbol include/tdx.h declares: (restype, argtypes)
_vp, _sz, _i, _fp = C.c_void_p, C.c_size_t, C.c_int, C.c_void_p
SIGNATURES = {
    "tdx_version": (C.c_char_p, []),
    "tdx_last_error": (C.c_char_p, []),
    "tdx_mf2_create": (_i, [C.POINTER(Mf2Config), _vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_mf2_destroy": (_i, [_vp]),
    "tdx_mf2_enable_taps": (_i, [_vp, _i]),
    "tdx_mf2_profile_enable": (_i, [_vp, _i]),
    "tdx_mf2_profile_collect": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    "tdx_mf2_workspace_bytes": (_sz, [_vp, _i, _i]),
    "tdx_mf2_forward": (_i, [_vp, _fp, _i, _i, _fp, _vp, _sz, _vp]),
    "tdx_mf2_flops": (C.c_double, [_vp, _i, _i]),
    "tdx_mf2_tap": (_i, [_vp, C.c_char_p, _i, _i, _vp, _fp, _sz, C.POINTER(_sz), _vp]),
    "tdx_cal_attention": (_i, [_fp] * 7 + [_i, _i, _i, _fp, _fp, _vp, _sz, _vp]),
    "tdx_cal_attention_workspace_bytes": (_sz, [_i, _i, _i]),
    "tdx_dilated_dense_net": (_i, [_fp, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "tdx_dilated_dense_net_workspace_bytes": (_sz, [_i, _i]),
    "tdx_linear": (_i, [_fp, _fp, _fp, _i, _i, _i, _fp, _vp]),
    "tdx_fbank_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "tdx_fbank_destroy": (_i, [_vp]),
    "tdx_fbank_frames": (_i, [_i]),
    "tdx_fbank_workspace_bytes": (_sz, [_i, _i]),
    "tdx_fbank_forward": (_i, [_vp, _fp, _i, _i, _fp, _vp, _sz, _vp]),
    "tdx_lfr_cmvn": (_i, [_fp, _i, _i, _fp, _fp, _fp, _vp]),
    "tdx_stft_create": (_i, [_i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "tdx_stft_destroy": (_i, [_vp]),
    "tdx_stft_chunk_size": (_i, [_vp]),
    "tdx_stft_workspace_bytes": (_sz, [_vp, _i]),
    "tdx_stft_forward": (_i, [_vp, _fp, _i, _fp, _vp, _sz, _vp]),
    "tdx_stft_inverse": (_i, [_vp, _fp, _i, _fp, _vp, _sz, _vp]),
    "tdx_mdx_create": (_i, [C.POINTER(MdxConfig), _vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_mdx_destroy": (_i, [_vp]),
    "tdx_mdx_workspace_bytes": (_sz, [_vp, _i]),
    "tdx_mdx_flops": (C.c_double, [_vp, _i]),
    "tdx_mdx_forward": (_i, [_vp, _fp, _i, _fp, _vp, _sz, _vp]),
    "tdx_punc_create": (_i, [_i, _i, _i, _vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_punc_destroy": (_i, [_vp]),
    "tdx_punc_workspace_bytes": (_sz, [_vp, _i, _i]),
    "tdx_punc_forward": (_i, [_vp, _vp, _vp, _i, _i, _fp, _vp, _sz, _vp]),
    "tdx_pfenc_create": (_i, [_i, _vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_pfenc_destroy": (_i, [_vp]),
    "tdx_pfenc_workspace_bytes": (_sz, [_vp, _i, _i]),
    "tdx_pfenc_flops": (C.c_double, [_vp, _i, _i]),
    "tdx_pfenc_forward": (_i, [_vp, _fp, _vp, _i, _i, _fp, _vp, _sz, _vp]),
    "tdx_pfdec_create": (_i, [_i, _i, _vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_pfdec_destroy": (_i, [_vp]),
    "tdx_pfdec_predict_workspace_bytes": (_sz, [_vp, _i, _i]),
    "tdx_pfdec_predict": (_i, [_vp, _fp, _i, _i, _fp, _fp, _vp, _vp, _vp, _sz, _vp]),
    "tdx_pfdec_decode_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "tdx_pfdec_decode": (_i, [_vp, _fp, _i, _vp, _fp, _i, _i, _i, _vp, _fp, _vp, _sz, _vp]),
    "tdx_pfdec_has_timestamps": (_i, [_vp]),
    "tdx_pfdec_set_cif_residual": (_i, [_vp, _i]),
    "tdx_pfdec_set_alpha2": (_i, [_vp, C.c_float, C.c_float]),
    "tdx_pfdec_timestamps_workspace_bytes": (_sz, [_vp, _i, _i]),
    "tdx_pfdec_timestamps": (_i, [_vp, _fp, _i, _i, _vp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "tdx_eres2net_create": (_i, [_vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_eres2net_destroy": (_i, [_vp]),
    "tdx_eres2net_workspace_bytes": (_sz, [_vp, _i, _i]),
    "tdx_eres2net_flops": (C.c_double, [_vp, _i, _i]),
    "tdx_eres2net_forward": (_i, [_vp, _fp, _i, _i, _fp, _vp, _sz, _vp]),
    "tdx_cosine_scores": (_i, [_fp, _fp, _i, _i, _fp, _vp]),
    "tdx_loudness_workspace_bytes": (_sz, [_i, C.c_long, _i]),
    "tdx_loudness": (_i, [_fp, _i, C.c_long, _i, _vp, _vp, _sz, _vp]),
    "tdx_resample_poly": (_i, [_fp, C.c_long, _i, _i, _i, _fp, _i, _fp, C.c_long, _vp]),
    "tdx_apollo_create": (_i, [_i, _vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_apollo_destroy": (_i, [_vp]),
    "tdx_apollo_workspace_bytes": (_sz, [_vp, _i]),
    "tdx_apollo_flops": (C.c_double, [_vp, _i]),
    "tdx_apollo_forward": (_i, [_vp, _fp, _vp, _i, _vp, _i, _fp, _vp, _sz, _vp]),
    "tdx_campp_create": (_i, [_vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_campp_destroy": (_i, [_vp]),
    "tdx_campp_workspace_bytes": (_sz, [_vp, _i, _i]),
    "tdx_campp_flops": (C.c_double, [_vp, _i, _i]),
    "tdx_campp_forward": (_i, [_vp, _fp, _i, _i, _fp, _vp, _sz, _vp]),
    "tdx_fsmnvad_create": (_i, [_vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_fsmnvad_destroy": (_i, [_vp]),
    "tdx_fsmnvad_workspace_bytes": (_sz, [_vp, _i]),
    "tdx_fsmnvad_flops": (C.c_double, [_vp, _i]),
    "tdx_fsmnvad_forward": (_i, [_vp, _fp, _vp, _i, _i, _fp, _fp, _vp, _sz, _vp]),
    "tdx_pyannet_create": (_i, [_vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_pyannet_destroy": (_i, [_vp]),
    "tdx_pyannet_frames": (_i, [_i]),
    "tdx_pyannet_chunk_tile": (_i, []),
    "tdx_pyannet_workspace_bytes": (_sz, [_vp, _i, _i]),
    "tdx_pyannet_flops": (C.c_double, [_vp, _i, _i]),
    "tdx_pyannet_forward": (_i, [_vp, _fp, _i, _i, _fp, _fp, _fp, _vp, _sz, _vp]),
    "tdx_silero_create": (_i, [_vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_silero_destroy": (_i, [_vp]),
    "tdx_silero_workspace_bytes": (_sz, [_vp, _i, _i]),
    "tdx_silero_flops": (C.c_double, [_vp, _i]),
    "tdx_silero_forward": (_i, [_vp, _fp, _vp, _i, _i, _fp, _fp, _fp, _vp, _sz, _vp]),
    "tdx_wespk_create": (_i, [_vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_wespk_destroy": (_i, [_vp]),
    "tdx_wespk_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "tdx_wespk_forward": (_i, [_vp, _fp, _i, _i, _fp, _i, _i, _fp, _vp, _sz, _vp]),
    "tdx_sv_create": (_i, [_i, _i, _i, _vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_sv_destroy": (_i, [_vp]),
    "tdx_sv_workspace_bytes": (_sz, [_vp, _i, _i]),
    "tdx_sv_flops": (C.c_double, [_vp, _i, _i]),
    "tdx_sv_forward": (_i, [_vp, _fp, _i, _i, C.POINTER(C.c_int), _fp, _vp, _fp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "tdx_ctc_collapse": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "tdx_whisper_create": (_i, [C.POINTER(WhisperConfig), _vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_whisper_destroy": (_i, [_vp]),
    "tdx_whisper_workspace_bytes": (_sz, [_vp, _i]),
    "tdx_whisper_flops": (C.c_double, [_vp, _i, _i]),
    "tdx_whisper_logmel": (_i, [_vp, _fp, _vp, _i, C.c_long, _fp, _vp, _sz, _vp]),
    "tdx_whisper_encode": (_i, [_vp, _fp, _i, _fp, _fp, _vp, _sz, _vp]),
    "tdx_whisper_decode": (_i, [_vp, _fp, _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int), _i, _i, _i, _vp, _fp, _vp, _vp, _sz, _vp]),
    "tdx_whisper_decode_xattn": (_i, [_vp, _fp, _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int), _i, _i, _i,
                                      C.POINTER(C.c_int), _i, _i, _i, _fp, _vp, _fp, _vp, _vp, _sz, _vp]),
    "tdx_whisper_logmel_long_workspace_bytes": (_sz, [_vp, C.c_long]),
    "tdx_whisper_logmel_long": (_i, [_vp, _fp, C.c_long, _fp, _vp, _sz, _vp]),
    "tdx_whisper_decode_ts": (_i, [_vp, _fp, _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _i,
                                   C.POINTER(C.c_int), _i, _i, _i, _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int), _fp, C.POINTER(C.c_int), _i,
                                   C.POINTER(C.c_int), _i, _fp, _vp, _fp, _vp, _vp, _sz, _vp]),
    "tdx_whisper_decode_sample_workspace_bytes": (_sz, [_vp, _i]),
    "tdx_whisper_decode_ts_sample": (_i, [_vp, _fp, _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _i,
                                          C.POINTER(C.c_int), _i, _i, _i, _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int), _fp, C.POINTER(C.c_int), _i,
                                          C.POINTER(C.c_int), _i, _fp, _vp, _fp, _vp, C.POINTER(C.c_float), C.POINTER(C.c_ulonglong), C.c_ulonglong,
                                          _vp, _sz, _vp]),
    "tdx_token_align_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "tdx_token_align": (_i, [_fp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _fp, _vp, _sz, _vp]),
    "tdx_ngate_create": (_i, [_i, C.POINTER(_vp)]),
    "tdx_ngate_destroy": (_i, [_vp]),
    "tdx_ngate_rows": (C.c_long, [C.c_long]),
    "tdx_ngate_workspace_bytes": (_sz, [_vp, C.c_long]),
    "tdx_ngate_forward": (_i, [_vp, _fp, C.c_long, _vp, _vp, _i, C.c_long, C.c_double, _i, _i, C.c_float, C.c_float, C.c_float, _fp,
                               _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "tdx_emo2v_create": (_i, [C.POINTER(Emo2vConfig), _vp, _sz, _i, C.POINTER(_vp)]),
    "tdx_emo2v_destroy": (_i, [_vp]),
    "tdx_emo2v_frames": (C.c_long, [_vp, C.c_long]),
    "tdx_emo2v_workspace_bytes": (_sz, [_vp, _i, C.c_long]),
    "tdx_emo2v_forward": (_i, [_vp, _fp, _i, C.c_long, _fp, _fp, _fp, _vp, _sz, _vp]),
    "tdx_emo2v_forward_taps": (_i, [_vp, _fp, _i, C.c_long, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "tdx_pyin_create": (_i, [_i, C.POINTER(_vp)]),
    "tdx_pyin_destroy": (_i, [_vp]),
    "tdx_pyin_workspace_bytes": (_sz, [_vp, C.POINTER(PyinParams), C.c_long]),
    "tdx_pyin_forward": (_i, [_vp, _fp, C.c_long, _vp, _vp, _i, C.POINTER(PyinParams), _vp, _sz, _vp, _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "tdx_pyin_viterbi": (_i, [_vp, _fp, C.c_long, C.POINTER(PyinParams), _vp, _sz, _vp, _vp, _sz, _vp]),
    "tdx_pvoc_create": (_i, [_i, C.POINTER(_vp)]),
    "tdx_pvoc_destroy": (_i, [_vp]),
    "tdx_pvoc_prepare": (_i, [_vp, _i]),
    "tdx_pvoc_workspace_bytes": (_sz, [_vp, _i, _i, _i, C.c_long, C.c_long]),
    "tdx_pvoc_stretch": (_i, [_vp, _fp, _i, C.c_long, _vp, _vp, _vp, _i, C.c_long, _fp, _fp, _fp, _vp, _sz, _vp]),
    "tdx_pvoc_vocode": (_i, [_vp, _fp, _i, _i, _i, _vp, _vp, _vp, _i, _fp, _vp]),
    "tdx_pvoc_istft": (_i, [_vp, _fp, _i, _i, _i, C.c_long, _fp, _vp, _sz, _vp]),
    "tdx_pvoc_eq_match": (_i, [_vp, _fp, C.c_long, _fp, C.c_long, _fp, _i, _i, _i, _fp, _fp, _vp, _vp, _fp, _vp, _sz, _vp]),
    "tdx_resample_sinc_length": (C.c_long, [C.c_long, C.c_double]),
    "tdx_resample_sinc": (_i, [_fp, _i, C.c_long, C.c_double, _fp, C.c_long, _vp]),
    "tdx_spectral_workspace_bytes": (_sz, [_i, _i, _i]),
    "tdx_spectral_laplacian": (_i, [_fp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "tdx_symeig_lowest": (_i, [_vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "tdx_fft_workspace_bytes": (_sz, [C.c_long, _i]),
    "tdx_fft_c2c": (_i, [_fp, C.c_long, _i, _i, _fp, _vp, _sz, _vp]),
    "tdx_fft_r2c": (_i, [_fp, C.c_long, _i, _fp, _vp, _sz, _vp]),
    "tdx_fft_c2r": (_i, [_fp, C.c_long, _i, _fp, _vp, _sz, _vp]),
    "tdx_fft_band_mix_workspace_bytes": (_sz, [C.c_long]),
    "tdx_fft_band_mix": (_i, [_fp, _fp, C.c_long, C.POINTER(C.c_long), _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
}


def lib():
    """Load libtdx.so once; raise TdxError if it is absent (never fall back)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TdxError(f"{LIB_PATH} not found: build it with `python -m targetdiarization_amd.build` "
                           "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        # One HIP runtime per process: libtdx.so NEEDs libamdhip64.so.7 by SONAME.  PyTorch-ROCm
        # ships its own copy with that SONAME; device pointers and streams handed across the
        # C-ABI belong to torch's runtime, so it must be the one libtdx binds to.  Importing
        # torch first guarantees that (loading libtdx first would pull in /opt/rocm's copy and
        # leave the process with two runtimes -> "no ROCm-capable device").
        import torch  # noqa: F401
        tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(tl):
            C.CDLL(tl, mode=C.RTLD_GLOBAL)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


# every symbol include/tdx_test.h declares (libtdx_diag.so: test hooks, never used by the product path)
_l = C.c_long


class GemmSeg(C.Structure):
    """tdx_gemm_seg of include/tdx_test.h: one K segment of a tdx_gemm_f32 launch."""
    _fields_ = [("A", _vp), ("B", _vp), ("lda", _l), ("ldb", _l), ("strideA", _l), ("strideB", _l), ("strideA2", _l), ("strideB2", _l),
                ("K", _i), ("zdiv", _i), ("kchunk", _i), ("ktotal", _i)]


class H3Seg(C.Structure):
    """tdx_h3_seg of include/tdx_test.h: one K segment of a tdx_h3_gemm_ex launch (the H3Seg of csrc/gemm_h3.hpp)."""
    _fields_ = [("A", _vp), ("B", _vp), ("sa", _vp), ("sb", _vp), ("lda", _l), ("ldb", _l),
                ("strideA", _l), ("strideB", _l), ("strideA2", _l), ("strideB2", _l),
                ("strideSA", _l), ("strideSB", _l), ("strideSA2", _l), ("strideSB2", _l),
                ("sa_mul", _i), ("sb_mul", _i), ("K", _i), ("zdiv", _i), ("kchunk", _i), ("ktotal", _i), ("segk", _i),
                ("strideSeg", _l), ("a_shift", _i), ("a_period", _i), ("a_zero", _vp)]


DIAG_SIGNATURES = {
    "tdx_diag_last_error": (C.c_char_p, []),
    "tdx_h3_gemm_ex": (_i, [_i] * 4 + [C.POINTER(H3Seg)] * 2 + [_i] * 12 + [_vp, _vp, _l, _l, _i, C.POINTER(_i), _vp]),
    "tdx_h3_gemm_f32a": (_i, [_vp, _l, C.c_float, _vp, _vp, _vp] + [_i] * 8 + [_vp, _l, _i, _vp]),
    "tdx_h3_plan": (_i, [_i] * 5 + [C.POINTER(_i)] * 2),
    "tdx_h3_tile_of_block": (_i, [C.POINTER(_i), _i, _i, _i] + [C.POINTER(_i)] * 3),
    "tdx_h3_split_rows_static": (_i, [_vp, _l, _vp, _l, _i, C.c_float, _vp]),
    "tdx_h3_split_rows_long": (_i, [_vp, _l, _vp, _vp, _l, _i, _vp]),
    "tdx_h3_split_kmajor_ex": (_i, [_vp, _l, _vp, _l, _i, C.c_float, _i, _vp, _vp, _i, _i, _vp]),
    "tdx_h3_split_rows": (_i, [_vp, _l, _vp, _vp, _l, _i, _vp]),
    "tdx_h3_split_kmajor": (_i, [_vp, _l, _vp, _l, _i, C.c_float, _vp]),
    "tdx_h3_gemm_x": (_i, [_i] + [_vp] * 5 + [_i] * 3 + [_vp]),
    "tdx_h3_gemm": (_i, [_vp] * 6 + [_i] * 3 + [_vp]),
    "tdx_h3_gemm_variant": (_i, [_vp] * 6 + [_i] * 4 + [_vp]),
    "tdx_linear_variant": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp]),
    "tdx_linear_epi": (_i, [_vp] * 5 + [_i] * 5 + [_vp]),
    "tdx_gemm_f32": (_i, [_i] * 3 + [C.POINTER(GemmSeg)] * 2 + [_i] * 5 + [_vp, _l, _l, _i, C.POINTER(_i), _vp]),
    "tdx_gemm_f32_conv": (_i, [_vp, _l, _vp] + [_i] * 11 + [_vp, _l, _i, C.POINTER(_i), _vp]),
    "tdx_attn_gate_planes_workspace_bytes": (_sz, [_i, _i, _i]),
    "tdx_attn_gate_planes": (_i, [_vp] * 7 + [_i] * 5 + [_vp] * 5 + [_sz, _vp]),
    "tdx_diag_dft_analysis": (_i, [_i, _i, _l, _l, _l, _i, _vp]),
    "tdx_diag_dft_synthesis": (_i, [_i, _i, _l, _l, _i, _vp]),
    "tdx_diag_loader_bind": (_i, [_vp, _sz] + [_i] * 9 + [_vp, _sz, C.POINTER(_i)]),
    "tdx_test_whisper_noise": (_i, [C.c_ulonglong, C.c_ulonglong, _i, _i, _i, _vp, _vp, _vp]),
    "tdx_test_fft_workspace_bytes": (_sz, [_l, _i, _i]),
    "tdx_test_fft_passes": (_i, [_i, _i]),
    "tdx_test_fft_c2c": (_i, [_vp, _l, _i, _i, _vp, _vp, _sz, _vp, _i]),
    "tdx_fill_bench": (_i, [_i, _vp, _l, _i, _i, _vp, _vp]),
    "tdx_fill_bench2": (_i, [_i, _vp, _i, _i, _i, _vp, _vp]),
    "tdx_fill_bench3": (_i, [_vp, _l, _i, _l, _i, _i, _i, _vp, _vp]),
}
DIAG_PATH = os.path.join(HERE, "libtdx_diag.so")
_diag = None


def diag():
    """Load libtdx_diag.so (tests / tools only)."""
    global _diag
    if _diag is None:
        if not os.path.exists(DIAG_PATH):
            raise TdxError(f"{DIAG_PATH} not found: build it with `python -m targetdiarization_amd.build`")
        lib()                                   # torch's HIP runtime first (see lib())
        l = C.CDLL(DIAG_PATH)
        for name, (res, args) in DIAG_SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _diag = l
    return _diag


def check(status: int):
    if status != 0:
        raise TdxError(f"libtdx status {status}: {lib().tdx_last_error().decode()}")


class HandleGuard:
    """Serialises the calls on ONE model object (one tdx handle, its grow-only workspace and its graph-replay buffers) — the
    threading contract of include/tdx.h seen from the host side.  The C handles are re-entrant per (workspace, stream) pair; the
    Python wrappers share one workspace per object, so they serialise instead:
      * host side: a re-entrant lock held while a forward is enqueued (two threads on one model: one after the other);
      * device side: an event chain — every call makes ITS stream wait for the event recorded behind the previous call,
        whatever stream that one ran on, so the shared workspace / static graph buffers never serve two forwards at a time
        (the reference serves one shared model from a REST handler and a WebSocket worker thread, main.py:42,366-367).
    Calls on DIFFERENT model objects (separator || target-clip embedding, embeddings || Paraformer) still overlap.
    Inside a stream capture nothing is waited for or recorded (an event from outside a capture cannot be waited on there);
    the capturing caller holds the lock for the whole capture."""

    def __init__(self, device):
        import threading
        self.device = device
        self.lock = threading.RLock()
        self._event = None
        self._ws = None

    def call(self):
        return _GuardedCall(self)

    def workspace(self, nbytes: int):
        """the grow-only workspace (use inside `with guard.call():`).  Before a smaller buffer is dropped the host waits for its
        last user: the caching allocator would hand the block back to the stream that allocated it, which has not waited."""
        import torch
        nbytes = max(int(nbytes), 16)
        if self._ws is None or self._ws.numel() < nbytes:
            if self._ws is not None and self._event is not None:
                self._event.synchronize()
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws


class _GuardedCall:
    def __init__(self, g):
        self.g = g

    def __enter__(self):
        import torch
        g = self.g
        g.lock.acquire()
        try:
            self.stream = torch.cuda.current_stream(g.device)
            self.capturing = torch.cuda.is_current_stream_capturing()
            if g._event is not None and not self.capturing:
                self.stream.wait_event(g._event)
        except BaseException:
            g.lock.release()
            raise
        return g

    def __exit__(self, *exc):
        import torch
        g = self.g
        try:
            if not self.capturing:
                if g._event is None:
                    g._event = torch.cuda.Event()
                g._event.record(self.stream)      # (re-recording is safe: a wait binds to the record that preceded it)
        finally:
            g.lock.release()
        return False


class Handle:
    """Owner of one tdx_*_create'd handle: checks the device, copies the weight blob into a ctypes buffer, creates the handle
    with its device current and destroys it once — on close(), or when the last reference goes.

        Handle(device, who, create_fn, destroy_fn, *create_args, blob=None)

    calls create_fn(*create_args, [blob, len(blob),] device_index, &handle).  `.ptr` is the c_void_p to pass to the C-ABI
    (NULL after close(): a late call is then TDX_E_INVALID, not a use after free), `.device` the torch.device with its index
    resolved, `.guard` the HandleGuard that serialises the calls on the handle."""

    def __init__(self, device, who, create_fn, destroy_fn, *create_args, blob=None):
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise TdxError(f"{who} needs a HIP device (cuda:N); there is no CPU path")
        idx = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.ptr = C.c_void_p()
        self._destroy = destroy_fn
        if blob is not None:
            create_args += ((C.c_char * len(blob)).from_buffer_copy(blob), len(blob))
        with torch.cuda.device(idx):
            check(create_fn(*create_args, idx, C.byref(self.ptr)))
        self.guard = HandleGuard(self.device)

    def close(self):
        if self.ptr:
            self._destroy(self.ptr)
            self.ptr.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GraphRunner:
    """HIP-graph replay of a C-ABI forward for SMALL problems (the reference's own call pattern is one clip per call: a
    forward is then hundreds of 10-100 us kernels and the launch gaps are a sizeable part of the latency).  The forwards
    allocate nothing, never synchronise and issue only kernel launches on the caller's stream (include/tdx.h), so a launch
    sequence is captured once per key (shape) with its own static input / output / workspace and replayed.
    (A hipMemsetAsync inside a captured sequence broke the node order on ROCm 7.2: the forwards contain none.)

    A key is captured when it is seen the SECOND time (`capture_after`): a capture costs a warm-up forward + the capture + the
    first replay, which a shape that never comes back (streaming buffers: a new T on almost every call) would pay for nothing —
    `__call__` returns None for such a call and the caller runs the plain eager forward.  Entries are evicted least recently
    used first; before an entry's static buffers are dropped the host waits for its last replay (they were allocated on one
    stream and replayed on others).  Callers serialise their use of one runner (HandleGuard)."""

    def __init__(self, device, max_entries: int = 8, capture_after: int = 2):
        from collections import OrderedDict
        self.device = device
        self.max_entries = max_entries
        self.capture_after = capture_after
        self._g = OrderedDict()
        self._seen = OrderedDict()
        self.captures = 0

    def _evict_one(self):
        _, (g, si, so, ws, last) = self._g.popitem(last=False)
        last.synchronize()

    def __call__(self, key, x, out_shape, ws_bytes: int, launch):
        """launch(in_tensor, out_tensor, workspace_tensor, stream_handle) issues the forward.  Returns a fresh output tensor, or
        None when the key has not been seen `capture_after` times yet (run eager)."""
        import torch
        ent = self._g.get(key)
        if ent is None:
            n = self._seen.pop(key, 0) + 1
            if n < self.capture_after:
                self._seen[key] = n
                while len(self._seen) > 256:
                    self._seen.popitem(last=False)
                return None
            while len(self._g) >= self.max_entries:
                self._evict_one()
            si = torch.empty_like(x)
            so = torch.empty(out_shape, dtype=torch.float32, device=self.device)
            ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=self.device)
            si.copy_(x)
            main = torch.cuda.current_stream(self.device)
            side = torch.cuda.Stream(self.device)

            def run():
                launch(si, so, ws, torch.cuda.current_stream(self.device).cuda_stream)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                run()                                  # warm-up outside the capture, ON THE CAPTURE STREAM (function attributes, first-use
                                                       # state, the separator's per-stream fork/join context: csrc/mf2.hip side_for)
            g = torch.cuda.CUDAGraph()
            # thread_local: another thread's GPU work (a second session on another model object) must not fail this capture
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                run()
            main.wait_stream(side)
            ent = self._g[key] = [g, si, so, ws, torch.cuda.Event()]
            self.captures += 1
        else:
            self._g.move_to_end(key)
        g, si, so, ws, last = ent
        si.copy_(x)
        g.replay()
        out = so.clone()
        last.record(torch.cuda.current_stream(self.device))
        return out
