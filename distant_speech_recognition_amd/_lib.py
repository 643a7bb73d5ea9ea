"""Loader of the C-ABI shared library (csrc/libbtkhip.so, declared in include/btkhip.h).

The HIP extension is the product: there is NO CPU fallback.  If the library is missing the
import of anything that needs it fails loudly (build it with `python -c "import
__graft_entry__ as g; g.build()"` or `make -C distant_speech_recognition_amd/csrc`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (BTK_LIB_PATH: a measurement build of the same library -- e.g. one compiled with -DBTK_EXP=...; never a fallback)
LIB_PATH = os.environ.get("BTK_LIB_PATH") or os.path.join(_HERE, "csrc", "libbtkhip.so")

_lib = None


class BtkError(RuntimeError):
    """Raised for a non-zero status of a C-ABI call; .code holds the BTK_ERR_* value."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


BTK_OK = 0
BTK_ERR_DIMENSION = -1
BTK_ERR_CONSISTENCY = -2
BTK_ERR_ALLOCATION = -3
BTK_ERR_PARAMETER = -4
BTK_ERR_HIP = -5
BTK_ERR_NUMERIC = -6
BTK_AEC_FRAME_CONTINUE = -(1 << 30)  # frame_no0 of btk_aec_process: count up from the state's frames done
BTK_TDOA_NO_PEAK = -(1 << 31)        # lag of btk_tdoa_gcc_peaks where a frame has no peak (include/btkhip.h)
BTK_PF_MCCOWAN_RULES = 0x10      # type bit of btk_zelinski_process (include/btkhip.h)
BTK_SS_TRAIN, BTK_SS_SUBTRACT = 1, 2     # frame flags / mode bits of btk_ss_process
BTK_WIENER_UPDATE_NOISE = 1              # frame flag / mode bit of btk_wiener_process
BTK_SS_FORM_AUTO, BTK_SS_FORM_ROWS = 0, 1
BTK_BINAURAL_KIM, BTK_BINAURAL_IID, BTK_BINAURAL_FDIID = 0, 1, 2     # kind of the btk_binaural_* entry points
BTK_VAD_POWER, BTK_VAD_NORMALIZED, BTK_VAD_TSPS = 0, 1, 2             # kind of btk_vad_band_power
BTK_VAD_RULE_SINGLE, BTK_VAD_RULE_MI, BTK_VAD_RULE_MULTISTAGE = 0, 1, 2     # rule of btk_vad_hangover

_vp, _i, _l, _f, _d = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double

# name -> (restype, argtypes); mirrors include/btkhip.h one to one
SIGNATURES = {
    "btk_last_error": (C.c_char_p, []),
    "btk_version": (_i, []),
    "btk_device_count": (_i, []),
    "btk_set_device": (_i, [_i]),
    "btk_synchronize": (_i, [_vp]),
    "btk_fb_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _vp]),
    "btk_fb_destroy": (None, [_vp]),
    "btk_fb_processing_delay": (_i, [_vp]),
    "btk_fb_lookahead": (_i, [_vp]),
    "btk_fb_analysis_num_frames": (_l, [_vp, _l]),
    "btk_fb_synthesis_num_blocks": (_l, [_vp, _l]),
    "btk_fb_analysis": (_i, [_vp, _vp, _l, _l, _i, _i, _vp, _l, _l, _l, _vp]),
    "btk_fb_analysis_bins": (_i, [_vp, _vp, _l, _l, _i, _i, _vp, _l, _l, _l, _i, _i, _vp]),
    "btk_fb_analysis_polyphase": (_i, [_vp, _vp, _l, _l, _i, _i, _vp, _l, _l, _vp]),
    "btk_fb_synthesis": (_i, [_vp, _vp, _l, _l, _i, _vp, _l, _l, _l, _vp]),
    "btk_fb_synthesis_aligned_form": (_i, [_vp]),
    "btk_bf_apply": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _l, _l, _vp]),
    "btk_fb_analysis_bf_scratch_bytes": (_l, [_vp, _i, _i, _i, _l]),
    "btk_fb_analysis_bf_fused": (_i, [_vp]),
    "btk_fb_analysis_bf": (_i, [_vp, _vp, _l, _l, _i, _i, _vp, _i, _vp, _l, _l, _l, _vp, _l, _vp]),
    "btk_fb_analysis_bf_i16_fused": (_i, [_vp]),
    "btk_fb_analysis_i16_direct": (_i, [_vp]),
    "btk_fb_analysis_i16": (_i, [_vp, _vp, _l, _l, _i, _i, _vp, _l, _l, _l, _vp]),
    "btk_fb_analysis_bf_i16": (_i, [_vp, _vp, _l, _l, _i, _i, _vp, _i, _vp, _l, _l, _l, _vp, _l, _vp]),
    "btk_nlms_workspace_bytes": (_l, [_i, _l]),
    "btk_nlms_process": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _l, _l, _vp, _vp, _vp, _vp, _vp]),
    "btk_nlms_process_nc": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _l, _l, _vp, _vp, _vp, _vp, _vp]),
    "btk_nlms_constraint_vectors": (_i, [_vp, _vp, _i, _i, _vp]),
    "btk_nlms_u_to_wa_nc": (_i, [_vp, _vp, _i, _i, _vp]),
    "btk_nlms_wa_to_u": (_i, [_vp, _vp, _i, _vp]),
    "btk_nlms_u_to_wa": (_i, [_vp, _vp, _i, _vp]),
    "btk_rls_workspace_bytes": (_l, [_i, _l]),
    "btk_rls_init": (_i, [_i, _vp, _i, _d, _i, _i, _i, _vp, _vp, _vp]),
    "btk_rls_process": (_i, [_i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _l, _l, _vp, _vp, _vp, _vp, _vp]),
    "btk_rls_init_nc": (_i, [_i, _vp, _i, _vp, _i, _d, _i, _i, _i, _vp, _vp, _vp]),
    "btk_rls_process_nc": (_i, [_i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _l, _l, _vp, _vp, _vp, _vp, _vp]),
    "btk_aec_max_filter_length": (_i, []),
    "btk_aec_dtd_state_in_lds": (_i, [_i, _i]),
    "btk_aec_init": (_i, [_i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "btk_aec_process": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _l, _l, _l, _vp, _vp, _vp, _vp, _vp, _vp]),
    "btk_bf_apply_stats": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _l, _l, _vp]),
    "btk_zelinski_process": (_i, [_vp, _vp, _vp, _i, _i, _i, _l, _l, _d, _i, _i, _l, _vp, _vp, _vp, _vp]),
    "btk_pf_coherence_coeffs": (_i, [_vp, _f, _i, _i, _vp, _vp, _vp]),
    "btk_bf_apply_stats2": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _l, _l, _vp]),
    "btk_lefkimmiatis_process": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _l, _l, _d, _i, _i, _l, _vp, _vp, _vp, _vp]),
    "btk_mvdr_lambda": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp]),
    "btk_frame_energy": (_i, [_vp, _i, _i, _i, _l, _l, _vp, _l, _vp]),
    "btk_pcm_i16_to_f32": (_i, [_vp, _vp, _l, _vp]),
    "btk_pcm_f32_to_i16": (_i, [_vp, _vp, _l, _vp]),
    "btk_pcm_i16_deinterleave": (_i, [_vp, _vp, _l, _i, _l, _vp]),
    "btk_gather_rows": (_i, [_vp, _vp, _i, _l, _vp]),
    "btk_cov_frame_gate": (_i, [_vp, _vp, _i, _l, _l, _f, _vp, _vp, _vp]),
    "btk_cov_accumulate": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _l, _l, _i, _vp]),
    "btk_cov_scale": (_i, [_vp, _d, _i, _i, _i, _vp]),
    "btk_cov_finalize": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "btk_cov_mask_count": (_i, [_vp, _vp, _i, _i, _l, _l, _vp, _vp]),
    "btk_cov_trace_normalize": (_i, [_vp, _i, _i, _vp]),
    "btk_sos_scratch_bytes": (_l, [_i, _i]),
    "btk_bmvdr_weights": (_i, [_vp, _vp, _i, _i, _i, _d, _vp, _vp, _vp, _vp]),
    "btk_gev_weights": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "btk_mvdr_scratch_bytes": (_l, [_i, _i]),
    "btk_csvdc_scratch_bytes": (_l, [_i, _i, _i]),
    "btk_csvdc_values": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "btk_mvdr_linpack_rule_scratch_bytes": (_l, [_i, _i]),
    "btk_mvdr_linpack_rule": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "btk_csvdc_full_scratch_bytes": (_l, [_i, _i, _i]),
    "btk_csvdc_full": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "btk_pinv_linpack_scratch_bytes": (_l, [_i, _i, _i]),
    "btk_pinv_linpack": (_i, [_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "btk_mvdr_linpack_full_scratch_bytes": (_l, [_i, _i]),
    "btk_mvdr_linpack_full": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    "btk_mvdr_diffuse_model": (_i, [_vp, _i, _i, _f, _f, _vp, _vp]),
    "btk_mvdr_diagonal_loading": (_i, [_vp, _i, _i, _f, _vp]),
    "btk_mvdr_weights": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp]),
    "btk_mvdr_weights_shard": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "btk_mvdr_divide_nondiagonal": (_i, [_vp, _i, _i, _f, _vp]),
    "btk_mvdr_weights_flags": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "btk_mvdr_weights_streams": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "btk_mvdr_pinv_fallback": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, C.POINTER(_i), _vp]),
    "btk_mvdr_pinv_scratch_bytes": (_l, [_i, _i]),
    "btk_mvdr_pinv_fallback_async": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "btk_mvdr_pinv_not_converged": (_i, []),
    "btk_mvdr_pinv_fallback_host": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, C.POINTER(_i), _vp]),
    "btk_pinv": (_i, [_vp, _i, _i, _f, _vp, C.POINTER(_i)]),
    "btk_wpe_workspace_bytes": (_l, [_i, _i, _i, _i, _i, _l]),
    "btk_wpe_estimate": (_i, [_vp, _i, _i, _i, _l, _l, _i, _i, _i, _d, _d, _i, _i, _vp, _vp, _vp, _vp]),
    "btk_wpe_apply": (_i, [_vp, _vp, _vp, _i, _i, _i, _l, _l, _i, _i, _i, _i, _vp]),
    "btk_bin_range": (None, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "btk_allgather_bins": (_i, [_vp, _vp, _vp, _i, _i, _l, _i, _i, _vp]),
    "btk_bin_rows_padded": (_i, [_i, _i]),
    "btk_allgather_bins_inplace": (_i, [_vp, _vp, _i, _i, _l, _i, _i, _vp]),
    "btk_weights_mainlobe": (_i, [_i, _i, _f, _vp, _vp]),
    "btk_weights_mainlobe_halfband": (_i, [_i, _i, _f, _vp, _vp]),
    "btk_weights_mainlobe_2": (_i, [_i, _i, _f, _vp, _vp, _vp]),
    "btk_weights_mainlobe_n": (_i, [_i, _i, _f, _vp, _vp, _i, _vp]),
    "btk_weights_blocking_matrix": (_i, [_vp, _i, _i, _vp]),
    "btk_weights_sidelobe": (_i, [_vp, _vp, _i, _i, _vp]),
    "btk_weights_gsc_effective": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "btk_srp_grid": (_i, [_f, _f, _f, C.POINTER(_i), _vp]),
    "btk_srp_delays": (_i, [_i, _vp, _d, _vp]),
    "btk_srp_table": (_i, [_i, _i, _f, _vp, _i, _vp, _i, _i, _vp]),
    "btk_srp_packed_elems": (_l, [_i, _i, _i]),
    "btk_srp_pack_table": (_i, [_vp, _i, _i, _i, _vp]),
    "btk_srp_power": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _l, _l, _i, _i, _i, _vp]),
    "btk_srp_select": (_i, [_vp, _vp, _f, _i, _vp, _vp, _vp, _vp, _i, _i, _l, _vp]),
    "btk_hos_max_channels": (_i, []),
    "btk_hos_workspace_bytes": (_l, [_i, _i, _i, _i, _l]),
    "btk_hos_eval": (_i, [_vp, _vp, _vp, _vp, _vp, _d, _d, _d, _i, _vp, _vp, _vp, _i, _i, _i, _i, _l, _l, _vp, _vp, _vp, _vp]),
    "btk_hos_minimize": (_i, [_vp, _vp, _vp, _vp, _vp, _d, _d, _d, _i, _vp, _vp, _vp, _i, _i, _i, _i, _l, _l, _i, _d, _d, _i, _d,
                              _vp, _vp, _vp, _vp, _vp, _vp]),
    # GCC-PHAT TDOA: HammingFeature + FFTFeature (feature/feature.cc:1177-1258), PHATFeature.next + TDOAFeature.next (lib/pytdoa.py:32-114)
    "btk_tdoa_frames": (_l, [_l, _i]),
    "btk_tdoa_spectra": (_i, [_vp, _l, _l, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "btk_tdoa_gcc_peaks": (_i, [_vp, _vp, _vp, _i, _f, _i, _i, _l, _i, _vp, _vp, _vp, _vp]),
    # EKF / IEKF tracking over the TDOA peaks: ExtendedKalmanFilter.next, KalmanFilter.update, IteratedExtendedKalmanFilter.update
    # (lib/pykalman.py:84-162, :199-266); the first argument points to an EkfParams
    "btk_ekf_track": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _l, _vp, _vp, _vp, _vp, _vp]),
    # ASR front end: PreemphasisFeature ... CepstralFeature (feature/feature.cc:1128-1144, :1177-1314, :1672-1792, :1892-2122,
    # :2326-2415; matrix/gslmatrix.cc:107-131); the first argument of btk_fe_process points to an FeParams
    "btk_fe_frames": (_l, [_l, _i, _i, _i]),
    "btk_fe_process": (_i, [_vp, _vp, _vp]),
    "btk_fe_mel_table": (_i, [_i, _f, _f, _f, _i, _i, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    "btk_fe_vtln_table": (_i, [_i, _i, _d, _d, _i, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    "btk_fe_dct_table": (_i, [_i, _i, _i, _vp]),
    # FFT block convolution: OverlapAdd::next / OverlapSave::next (convolution/convolution.cc:83-131, :196-230)
    "btk_conv_plan": (_i, [_i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "btk_conv_filter_spectra": (_i, [_vp, _l, _i, _i, _i, _i, _i, _vp, _vp]),
    "btk_conv_apply": (_i, [_vp, _l, _l, _l, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _l, _l, _vp]),
    "btk_conv_blocks": (_i, [_vp, _l, _l, _i, _l, _l, _vp, _i, _i, _i, _i, _vp, _vp]),
    # single-channel enhancement: SpectralSubtractor / AveragePSDEstimator / WienerFilter (postfilter/spectralsubtraction.cc:57-129,
    # :216-285, :314-362) and HighPassFilter (postfilter/postfilter.cc:1215-1239)
    "btk_ss_max_channels": (_i, []),
    "btk_ss_process": (_i, [_vp, _vp, _i, _i, _i, _l, _l, _vp, _i, _d, _d, _vp, _l, _vp, _vp, _vp, _vp, _i, _vp]),
    "btk_ss_finish_training": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "btk_ss_clear": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "btk_wiener_process": (_i, [_vp, _vp, _vp, _i, _i, _l, _l, _vp, _i, _d, _d, _d, _l, _vp, _vp, _vp]),
    "btk_spec_highpass": (_i, [_vp, _vp, _i, _i, _i, _l, _l, _vp]),
    # PR banks and the windowed FFT bank: PerfectReconstructionFFTAnalysisBank / ...SynthesisBank / NormalFFTAnalysisBank
    # (modulated/modulated.cc:683-718, :861-898, :203-227) and get_window (:47-72)
    "btk_get_window": (_i, [_i, _i, _vp]),
    "btk_prfb_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _vp, _l]),
    "btk_prfb_destroy": (None, [_vp]),
    "btk_prfb_processing_delay": (_i, [_vp]),
    "btk_prfb_num_frames": (_l, [_vp, _l]),
    "btk_prfb_num_blocks": (_l, [_vp, _l]),
    "btk_prfb_analysis": (_i, [_vp, _vp, _l, _l, _i, _i, _vp, _l, _l, _l, _vp]),
    "btk_prfb_synthesis": (_i, [_vp, _vp, _l, _l, _i, _vp, _l, _l, _l, _vp]),
    "btk_stft_create": (_i, [C.POINTER(_vp), _i, _i, _i]),
    "btk_stft_destroy": (None, [_vp]),
    "btk_stft_num_frames": (_l, [_vp, _l]),
    "btk_stft_analysis": (_i, [_vp, _vp, _l, _l, _i, _i, _vp, _l, _l, _l, _vp]),
    # binaural binary-mask filters and threshold estimators (postfilter/binauralprocessing.cc)
    "btk_binaural_max_candidates": (_i, []),
    "btk_binaural_mask": (_i, [_vp, _vp, _vp, _i, _i, _l, _l, _i, _i, _d, _vp, _d, _d, _l, _vp, _vp]),
    "btk_binaural_stats_scratch_bytes": (_l, [_i, _i, _l, _i]),
    "btk_binaural_stats": (_i, [_vp, _vp, _i, _i, _l, _l, _i, _vp, _i, _i, _d, _d, _i, _i, _vp, _vp, _vp, _vp, _l, _vp]),
    "btk_binaural_candidates": (_i, [_d, _d, _d, _vp, _i, C.POINTER(_i), C.POINTER(_i)]),
    "btk_binaural_threshold": (_i, [_i, _i, _i, _i, _vp, _vp, C.c_longlong, _d, C.POINTER(_d), _vp, _vp]),
    # voice activity detection, the energy family of sad/sad.cc (:126-180, :472-836, :996-1063, :1712-1951)
    "btk_vad_frame_energy": (_i, [_vp, _i, _i, _i, _l, _l, _l, _l, _vp, _l, _vp]),
    "btk_vad_band_limits": (_i, [_i, _d, _d, _d, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "btk_vad_band_power": (_i, [_vp, _i, _i, _i, _i, _l, _l, _l, _l, _l, _i, _i, _d, _vp, _vp, _vp, _l, _vp]),
    "btk_vad_energy_metric_state_bytes": (_l, [_i]),
    "btk_vad_energy_metric": (_i, [_vp, _l, _i, _l, _i, _i, C.c_uint, C.c_uint, _vp, _vp, _l, _vp]),
    "btk_vad_simple_energy": (_i, [_vp, _l, _i, _l, _d, _d, _vp, _vp, _vp, _l, _vp]),
    "btk_vad_hangover": (_i, [_vp, _vp, _i, _i, _i, _l, _l, C.c_uint, C.c_uint, _i, _vp, _vp, _l, _vp, _i, _vp, _vp]),
    "btk_vad_gather": (_i, [_vp, _i, _l, _i, _l, _vp, _vp, _l, _vp, _vp]),
    # objective measures (objective_measure/objective_measure.cc:42-185, :284-331)
    "btk_obj_snr_workspace_bytes": (_l, [_i, _l]),
    "btk_obj_snr": (_i, [_vp, _l, _vp, _l, _i, _vp, _vp, _i, _vp, _l, _vp, _l, _vp, _vp]),
    "btk_obj_snr_db": (_f, [_d, _d]),
    "btk_obj_is_tile_frames": (_i, [_vp]),
    "btk_obj_is_distance": (_i, [_vp, _vp, _l, _vp, _l, _i, _vp, _vp, _l, _l, _vp, _vp, _vp, _l, _vp]),
    # multichannel cross-correlation localisation (localization/mcc_localizer.cc:54-161, :322-451; localization.cc:107-118)
    "btk_mcc_max_sample_delay": (_l, [C.c_uint, _f]),
    "btk_mcc_sample_delays": (_i, [C.c_uint, _i, _vp, _vp]),
    "btk_mcc_linear_grid": (_i, [C.c_uint, _i, _vp, _f, _i, C.POINTER(_i), C.POINTER(_f), C.POINTER(_f), _vp, _vp, _vp]),
    "btk_mcc_cost": (_i, [_vp, _l, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "btk_mcc_select": (_i, [_vp, _l, _i, _i, _vp, _vp, _vp]),
    "btk_mcc_matrices": (_i, [_vp, _l, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
}


class EkfParams(C.Structure):
    """btk_ekf_params of include/btkhip.h, field by field."""
    _fields_ = [("n", _i), ("model", _i), ("type", _i), ("F", _d * 9), ("U", _d * 9), ("sigmaV2", _d), ("time_delta", _d),
                ("gate_prob", _d), ("num_iterations", _i), ("iteration_threshold", _d), ("threshold", _d), ("minimum_pairs", _i),
                ("Ts", _d), ("c", _d)]


class FeParams(C.Structure):
    """btk_fe_params of include/btkhip.h, field by field."""
    _fields_ = [("S", _i), ("C", _i), ("T", _l), ("in_stage", _i), ("in_dim", _i), ("len", _l), ("pcm_stride", _l), ("D", _i),
                ("shift", _i), ("L", _i), ("window", _i), ("preemph", _i), ("mu", _d), ("prior0", _vp), ("powN", _i),
                ("vtlnN", _i), ("vtln_nw", _i), ("vtln_rows", _vp), ("vtln_w", _vp), ("melN", _i), ("mel_nw", _i),
                ("mel_rows", _vp), ("mel_w", _vp), ("log_m", _d), ("log_a", _d), ("log_floor", _i), ("cepN", _i), ("dct", _vp),
                ("out", _vp * 7)]


def lib():
    """Return the loaded library; raise if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "distant_speech_recognition_amd: HIP extension %s is missing -- build it with "
                "`make -C distant_speech_recognition_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)           # AttributeError here == header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code):
    if code != BTK_OK:
        msg = lib().btk_last_error()
        raise BtkError(code, msg.decode() if msg else "btkhip error %d" % code)
    return code
