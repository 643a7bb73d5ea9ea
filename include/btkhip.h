/*
 * btkhip.h -- thin C-ABI of the MI355X (gfx950) subband-beamforming engine.
 *
 * This is the drop-in boundary: plain C, opaque handles, explicit sizes, int status codes.
 * Bulk data pointers marked [dev] are DEVICE pointers (HBM) owned by the caller; pointers
 * marked [host] are host memory read during the call only.  `stream` is a hipStream_t passed
 * as void* (NULL = default stream).  Nothing here needs PyTorch.
 *
 * Each entry point cites the reference interface it replaces (paths relative to
 * btk20_src/ of kkumatani/distant_speech_recognition).  The reference has no FFI of its own for
 * this path (it is a single-process C++/SWIG library); INTEGRATION.md shows the binding a
 * maintainer adds on the reference side.
 *
 * Data layout in HBM (K = M/2+1 computed bins):
 *   pcm   float32   [S][N][pcm_stride]     stream, channel, sample (un-normalised int16 scale)
 *   X     complex64 [S][K][N][T]           subband snapshots, FRAMES CONTIGUOUS
 *   W     complex64 [S or 1][K][N]         beamformer weights,  y = w^H x
 *   Y     complex64 [S][K][T]              beamformed subband frames
 *   out   float32   [S][nblocks*D]         synthesised samples
 *
 * All functions return BTK_OK (0) or a negative error code; btk_last_error() returns the
 * message of the calling thread's last failure (the C++ node layer turns codes into the
 * reference's j_error subclasses, common/jexception.h:26-161).
 */
#ifndef BTKHIP_H
#define BTKHIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define BTK_OK              0
#define BTK_ERR_DIMENSION  -1   /* jdimension_error   */
#define BTK_ERR_CONSISTENCY -2  /* jconsistency_error */
#define BTK_ERR_ALLOCATION -3   /* jallocation_error  */
#define BTK_ERR_PARAMETER  -4   /* jparameter_error   */
#define BTK_ERR_HIP        -5   /* j_error (device runtime failure) */
#define BTK_ERR_NUMERIC    -6   /* jnumeric_error     */

typedef struct btk_fb btk_fb_t;          /* filter-bank plan (analysis or synthesis) */

const char* btk_last_error(void);
int  btk_version(void);
/* Number of HIP devices visible / select one for this thread (one process per GPU). */
int  btk_device_count(void);
int  btk_set_device(int device);
int  btk_synchronize(void* stream);

/* ---- Oversampled modulated-DFT filter bank --------------------------------------------
 * Replaces OverSampledDFTAnalysisBank / OverSampledDFTSynthesisBank
 * (modulated/modulated.h:268-340, modulated/modulated.cc:232-268 ctor delay logic).
 * prototype: [host] m*M float64 coefficients, copied at creation (modulated.cc:243-244).
 * M must be a power of two in [64, 2048]; r in [0, log2(M)]; delay_comp_type in {0,1,2}.   */
int  btk_fb_create(btk_fb_t** fb, int M, int m, int r, int delay_comp_type, int synthesis,
                   const double* prototype);
void btk_fb_destroy(btk_fb_t* fb);
int  btk_fb_processing_delay(const btk_fb_t* fb);   /* processing_delay_ */
int  btk_fb_lookahead(const btk_fb_t* fb);          /* laN_ */
/* frames an analysis bank emits for an nsamples-long channel before jiterator_error:
 * ceil(nsamples/D) - laN + processing_delay   (modulated.cc:419-469).                       */
long btk_fb_analysis_num_frames(const btk_fb_t* fb, long nsamples);
/* blocks a synthesis bank emits when its source ends after nframes: nframes - pd (>= 0)
 * (modulated.cc:569-612).                                                                   */
long btk_fb_synthesis_num_blocks(const btk_fb_t* fb, long nframes);

/* OverSampledDFTAnalysisBank::next for frames [t0, t0+tcount) of every (stream, channel):
 * modulated.cc:375-409.  pcm [dev] [S*N][pcm_stride] with nsamples valid samples per channel
 * (zero outside, like the zero-initialised ring and the end-of-stream padding).
 * X [dev] [S][K][N][T_stride]; frame t is stored at column t - t0.                         */
int  btk_fb_analysis(const btk_fb_t* fb, const float* pcm, long nsamples, long pcm_stride,
                     int S, int N, void* X, long T_stride, long t0, long tcount, void* stream);
/* A bin SHARD of the same transform (frequency-bin sharding): only bins [k0, k1) are written,
 * X [dev] complex64 [S][k1-k0][N][T_stride].  The FFT of a channel yields all bins, so a rank of a bin-sharded run
 * transforms every channel but stores -- the dominant cost of the analysis bank -- only 1/world of the snapshots. */
int  btk_fb_analysis_bins(const btk_fb_t* fb, const float* pcm, long nsamples, long pcm_stride, int S, int N, void* X,
                          long T_stride, long t0, long tcount, int k0, int k1, void* stream);
/* Debug/parity entry: the M real polyphase sums of modulated.cc:384-391 (before the FFT),
 * P [dev] float32 [S*N][tcount][M].  Used to pin the integer polyphase indexing bit-exactly. */
int  btk_fb_analysis_polyphase(const btk_fb_t* fb, const float* pcm, long nsamples, long pcm_stride,
                               int S, int N, float* P, long t0, long tcount, void* stream);
/* OverSampledDFTSynthesisBank::next for blocks [b0, b0+bcount): modulated.cc:553-612.
 * Y [dev] [S][K][T_stride] holding nframes valid frames (frame index < 0 reads as zero == the
 * zeroed ring, modulated.cc:615-621); out [dev] [S][out_stride], block b at offset (b-b0)*D. */
int  btk_fb_synthesis(const btk_fb_t* fb, const void* Y, long nframes, long T_stride, int S,
                      float* out, long out_stride, long b0, long bcount, void* stream);
/* 1: this plan's geometry has a wider kernel form that btk_fb_synthesis takes for ALIGNED launches -- b0 + processing_delay even,
 * T_stride even, out_stride a multiple of 4, Y and out 16-byte aligned -- and whose results differ from the other form's by
 * <= 2 ulp (another FFT factorisation, the same summation order per sample).  A caller that cuts one stream into several launches
 * and needs the same bits for every partition keeps all of them aligned (b0 may be one less than the first block wanted, -1
 * included: blocks before the stream are zeros) or none; 0: one form, every partition gives the same bits anyway.        */
int  btk_fb_synthesis_aligned_form(const btk_fb_t* fb);

/* ---- Sample formats on either side of the path ------------------------------------------------
 * SampleFeature hands the analysis bank UN-NORMALISED floats of 16-bit PCM (feature/feature.cc:265-269) and the reference's
 * scripts write the synthesis output back as int16 (numpy.array(buf, numpy.int16): toward zero,
 * unit_test/test_online_beamforming.py:209).  Utterances cross PCIe as int16 and are widened / narrowed on the device.
 * in, out [dev], n samples.                                                                                            */
int  btk_pcm_i16_to_f32(const short* in, float* out, long n, void* stream);
int  btk_pcm_f32_to_i16(const float* in, short* out, long n, void* stream);
/* A multi-channel recording as stored (frame by frame): in [dev] int16 [L][N] -> out [dev] float32 [N][out_stride], all channels in
 * one pass (SampleFeature::read copies channel chX out of the interleaved frames, once per channel node: feature/feature.cc:333-334). */
int  btk_pcm_i16_deinterleave(const short* in, float* out, long L, int N, long out_stride, void* stream);

/* Rows of samples that lie in SEPARATE host allocations -> one device block, by ONE kernel that reads the host memory itself
 * (round 6; the node layer's 16-bit streams: every channel's SampleFeature owns its utterance, feature/feature.cc:238-389, and a
 * block of a 64-channel graph -- or of 32 graphs -- is 64 ... 2 048 rows; a hipMemcpyAsync per row reaches 27 GB/s at 0.5 MB per row,
 * the kernel the link's 57 GB/s at any row length).  table [PINNED host memory (hipHostMalloc: device-accessible) or dev]: nrows
 * entries; src [pinned host or dev], 16-byte aligned, `bytes` valid bytes (a multiple of 2) -- it must stay untouched until the
 * stream has passed the call, like the source of an asynchronous copy.  Row r goes to dst + r * dst_pitch_bytes [dev]; the bytes
 * from `bytes` up to dst_pitch_bytes are zeroed (bytes <= dst_pitch_bytes).  dst and dst_pitch_bytes multiples of 16.            */
typedef struct { const void* src; long bytes; } btk_row_t;
int  btk_gather_rows(const btk_row_t* table, void* dst, int nrows, long dst_pitch_bytes, void* stream);

/* ---- Fixed-weight beamformer apply ------------------------------------------------------
 * SubbandDS::next (beamformer/beamformer.cc:1095-1157), SubbandGSC::next + calc_gsc_output
 * (:1208-1316), SubbandMVDR::next (:2537-2587), SubbandMVDRGSC::next (:2720-2773):
 *   y_k[t] = w_k^H x_k[t], k = 0..M/2 (mirror bins are conjugates, formed at synthesis).
 * W [dev] complex64 [Sw][K][N] with Sw = S (per-stream weights) or 1 (shared).              */
int  btk_bf_apply(const void* W, int per_stream_weights, const void* X, void* Y,
                  int S, int K, int N, long T_stride, long T, void* stream);

/* Fused OverSampledDFTAnalysisBank x N -> fixed-weight beamformer (the chain SubbandGSC::next pulls per frame,
 * beamformer.cc:1267-1311): Y[s][k][t] = sum_n conj(W[k][n]) X_n[k][t] without materialising the snapshots in HBM
 * (fused kernels: M = 512 and M = 256 with m = 4, r <= 2, and M = 1024 / 2048 with m = 4, r = 1 -- there one stream of a large
 * array is split over channel groups whose partial sums are added in a fixed order; other geometries run btk_fb_analysis +
 * btk_bf_apply through `scratch`, which then needs T_stride == tcount).
 * scratch [dev] of btk_fb_analysis_bf_scratch_bytes(...) bytes, 16-byte aligned (the fused kernel stages its weight
 * pairs [Sw][N][320] float4 there and fetches them by LDS-DMA).  Y rows may be spaced T_stride >= tcount frames apart
 * (fused geometries); rows a multiple of 4 KiB apart are worth padding.  Use the staged calls when a post-filter, the
 * adaptive canceller or covariance accumulation needs the snapshots.                                          */
long btk_fb_analysis_bf_scratch_bytes(const btk_fb_t* fb, int S, int N, int per_stream_weights, long tcount);
/* 1: btk_fb_analysis_bf runs a fused kernel for this plan's geometry (any T_stride >= tcount); 0: the staged pair through
 * `scratch` (a caller that keeps the snapshots anyway then calls btk_fb_analysis + btk_bf_apply itself); < 0: not an analysis plan. */
int  btk_fb_analysis_bf_fused(const btk_fb_t* fb);
int  btk_fb_analysis_bf(const btk_fb_t* fb, const float* pcm, long nsamples, long pcm_stride, int S, int N,
                        const void* W, int per_stream_weights, void* Y, long T_stride, long t0, long tcount,
                        void* scratch, long scratch_bytes, void* stream);

/* The same operator on the samples AS THEY ARE STORED: 16-bit PCM (SampleFeature::read turns a WAV's int16 samples into
 * un-normalised floats, feature/feature.cc:265-269; over PCIe and in HBM they can stay int16).  pcm [dev] int16 [S*N][pcm_stride],
 * widened in registers inside the fused kernel: 2 D N + 8 K bytes per beamformed frame instead of 4 D N + 8 K, and -- the
 * conversion is exact -- the SAME BITS as btk_fb_analysis_bf on the float copies of the same samples.  Geometries:
 * btk_fb_analysis_bf_i16_fused() == 1 (M = 256 / 512 with m = 4, r <= 2, and M = 1024 / 2048 with m = 4, r = 1); for the others widen
 * with btk_pcm_i16_to_f32 and call btk_fb_analysis_bf (BTK_ERR_PARAMETER here).  scratch: btk_fb_analysis_bf_scratch_bytes.   */
int  btk_fb_analysis_bf_i16_fused(const btk_fb_t* fb);
/* The STAGED bank on 16-bit PCM (round 6): btk_fb_analysis with pcm [dev] int16 [S*N][pcm_stride], widened on the way into the
 * kernel's LDS span -- the same bits as btk_fb_analysis on the float copies, 2 D + 8 K instead of 4 D + 8 K bytes per frame and
 * channel, and no btk_pcm_i16_to_f32 pass in front of it (4 D + 2 D bytes per frame and channel more).  What the snapshot
 * consumers of a 16-bit stream run on: post-filters, adaptive cancellers, covariance, WPE (OverSampledDFTAnalysisBank::next over
 * SampleFeature::read, modulated/modulated.cc:375-409 over feature/feature.cc:265-269).  Geometries:
 * btk_fb_analysis_i16_direct() == 1 (M = 256 / 512 / 1024 / 2048, m = 4, r <= 2); BTK_ERR_PARAMETER for the others (widen, then btk_fb_analysis). */
int  btk_fb_analysis_i16_direct(const btk_fb_t* fb);
int  btk_fb_analysis_i16(const btk_fb_t* fb, const short* pcm, long nsamples, long pcm_stride,
                         int S, int N, void* X, long T_stride, long t0, long tcount, void* stream);
int  btk_fb_analysis_bf_i16(const btk_fb_t* fb, const short* pcm, long nsamples, long pcm_stride, int S, int N,
                            const void* W, int per_stream_weights, void* Y, long T_stride, long t0, long tcount,
                            void* scratch, long scratch_bytes, void* stream);

/* ---- Adaptive GSC canceller: leaky power-normalised NLMS ----------------------------------
 * Replaces SubbandGSCLMSBeamformer.__iter__ / reset_stats (lib/pybeamformer.py:659-762), Nc = 1.
 * params [host] 8 floats: beta, gamma(init), regularization_param, energy_floor, sil_thresh,
 *   max_wa_l2norm, min_frames, slowdown_after (pybeamformer.py:597-607).
 * vs [dev] complex64 [K][N]: array manifold / N of bins 0..M/2 (calc_array_manifold_f :284-306;
 *   the upper branch is Yc = vs^H x, the blocking matrix is implied by vs -- see DESIGN.md).
 * State (all [dev], updated in place so consecutive blocks continue the recursion):
 *   u_state complex64 [S][K][N]  = wa^H B^T  (zeros == reset_stats; convert with btk_nlms_*_wa)
 *   sigma2  float32   [S][K]     = _subband_energy          (init_diagonal_load at reset)
 *   stream_state float64 [S][4]  = {_energy, _gamma, _isamp, _ttl_updates}
 * workspace [dev] btk_nlms_workspace_bytes(S,T) bytes.  Y [dev] complex64 [S][K][T_stride].    */
long btk_nlms_workspace_bytes(int S, long T);
int  btk_nlms_process(const float* params, const void* vs, const void* X, void* Y,
                      int S, int M, int N, long T_stride, long T,
                      void* u_state, float* sigma2, double* stream_state, void* workspace, void* stream);
/* Nc > 1 constraints (SubbandGSCLMSBeamformer(..., Nc), lib/pybeamformer.py:588-607, 742): the blocking matrix keeps the
 * first N - Nc Gram-Schmidt columns (calc_blocking_matrix, :309-341), so the canceller's projector loses Nc - 1 more
 * directions: cextra [dev] complex64 [K][NC-1][N], per bin from btk_nlms_constraint_vectors (host, complex128
 * [NC-1][N]; B [N][N-NC] from btk_weights_blocking_matrix).  NC = 1 is btk_nlms_process.  1 <= NC <= 8.              */
int  btk_nlms_process_nc(const float* params, const void* vs, const void* cextra, int NC, const void* X, void* Y,
                         int S, int M, int N, long T_stride, long T,
                         void* u_state, float* sigma2, double* stream_state, void* workspace, void* stream);
int  btk_nlms_constraint_vectors(const double* vs, const double* B, int N, int NC, double* cx);
int  btk_nlms_u_to_wa_nc(const double* u, const double* B, int N, int NC, double* waH);
/* Host-side change of basis between the reference's active weights wa^H (complex128 [N-1], as
 * kept in SubbandGSCLMSBeamformer._waH) and the engine state u = wa^H B^T (complex128 [N]);
 * B [host] complex128 [N][N-1] from btk_weights_blocking_matrix.                               */
int  btk_nlms_wa_to_u(const double* waH, const double* B, int N, double* u);
int  btk_nlms_u_to_wa(const double* u, const double* B, int N, double* waH);

/* ---- Adaptive GSC canceller: recursive least squares (float64 recursion) ---------------------
 * mode 0 replaces SubbandGSCRLS::next + update_active_weight_vector2_ (beamformer/beamformer.cc:1514-1645):
 *   params [host] 6 doubles: mu, diagonal_weight (sigma2 of the ctor, :1447-1467), qctype (0 none,
 *   1 CONSTANT_NORM, 2 THRESHOLD_LIMITATION, beamformer.h:215-219), alpha, normalize_weight, update flag
 *   (update_active_weight_vecotrs, beamformer.h:234);  v = wq (calcMainlobe), bins 1..M/2 adapt.
 * mode 1 replaces SubbandGSCRLSBeamformer.__iter__ / reset_stats (lib/pybeamformer.py:817-925), Nc = 1:
 *   params [host] 10 doubles: beta, gamma, mu, init_diagonal_load, regularization_param, sil_thresh,
 *   constraint_option, alpha2, max_wa_l2norm, min_frames (:776-787);  v = vs (calc_array_manifold_f :284-306).
 * v [dev] complex128 [Sv][K][N] (Sv = S if per_stream_v else 1); the upper branch is v^H x and the blocking
 * matrix is implied by v.  State [dev], updated in place so consecutive blocks continue:
 *   P_state complex128 [S][K][N][N] = B Pz B^H (mode 0) / conj(B) Pz B^T (mode 1)
 *   w_state complex128 [S][K][N]    = wl = B wa (mode 0) / u = wa^H B^T (mode 1)
 *   stream_state float64 [S][4]     = {_energy, -, _isamp, _ttl_updates} (mode 1; untouched in mode 0)
 * btk_rls_init writes P = p0 B B^H resp. p0 conj(B) B^T (closed form from v), w = 0  == init_precision_matrix (p0 = 1/sigma2,
 * beamformer.cc:1482-1494) resp. reset_stats (p0 = 1/init_diagonal_load, pybeamformer.py:921-925).
 * workspace [dev] btk_rls_workspace_bytes(S,T) bytes.  Y [dev] complex64 [S][K][T_stride].
 * N <= 64 with one constraint: P in registers (row and column copies, the reference's two products separately); otherwise, up to
 * N = 128: P as a packed Hermitian matrix in LDS; up to N = 256: P in place in the exported [N][N] state (rls_kernels.hip).
 * btk_rls_init_nc / btk_rls_process_nc: NC >= 1 constraints (SubbandGSCRLSBeamformer(..., Nc), pybeamformer.py:784-797;
 *   SubbandGSCRLS after calc_gsc_weights_2 / _n): cx [dev] complex128 [Sv][K][NC-1][N], the orthonormal directions the blocking
 *   matrix removes besides the one implied by v -- mode 1: btk_nlms_constraint_vectors(vs, B) (conj(B) B^T = I - vs vs^H/|vs|^2 -
 *   sum_j c_j c_j^H), mode 0: their complex conjugates taken with vs = wq (B B^H = I - conj(wq) wq^T/|wq|^2 - sum_j c_j c_j^H).
 *   NC = 1: cx may be NULL (== btk_rls_init / btk_rls_process).                                                               */
long btk_rls_workspace_bytes(int S, long T);
int  btk_rls_init(int mode, const void* v, int per_stream_v, double p0, int S, int K, int N,
                  void* P_state, void* w_state, void* stream);
int  btk_rls_process(int mode, const double* params, const void* v, int per_stream_v,
                     const void* X, void* Y, int S, int M, int N, long T_stride, long T,
                     void* P_state, void* w_state, double* stream_state, void* workspace, void* stream);
int  btk_rls_init_nc(int mode, const void* v, int per_stream_v, const void* cx, int NC, double p0, int S, int K, int N,
                     void* P_state, void* w_state, void* stream);
int  btk_rls_process_nc(int mode, const double* params, const void* v, int per_stream_v, const void* cx, int NC,
                        const void* X, void* Y, int S, int M, int N, long T_stride, long T,
                        void* P_state, void* w_state, double* stream_state, void* workspace, void* stream);

/* ---- Subband acoustic echo cancellation (float64 recursion) -----------------------------------
 * Replaces the next() of the four canceller nodes of aec/aec.cc, per (stream, bin <= M/2) over a block of T frames:
 *   kind 0  NLMSAcousticEchoCancellationFeature          (aec/aec.cc:34-80)    P = 1
 *   kind 1  KalmanFilterEchoCancellationFeature          (aec/aec.cc:85-165)   P = 1
 *   kind 2  BlockKalmanFilterEchoCancellationFeature     (aec/aec.cc:172-307)  P = sample_num
 *   kind 3  DTDBlockKalmanFilterEchoCancellationFeature  (aec/aec.cc:801-942)  P = sample_num
 * params [host] 8 doubles:
 *   kind 0: delta, epsilon, -, threshold                                              (aec.h:36)
 *   kind 1: beta, sigma2, -, threshold                                                (aec.h:73)
 *   kind 2: beta, sigmau2, sigmak2, threshold, -, -, amp4play                         (aec.h:106)
 *   kind 3: beta, sigmau2, sigmak2, snr_threshold, energy_threshold, smooth, amp4play (aec.h:308; the base class's
 *           threshold_ is snr_threshold, aec.cc:805)
 * V (played), A (recorded) [dev] complex64 [S][K][T_stride], K = M/2+1; E [dev] complex64 [S][K][T_stride] = A - R^T v
 * (zdotu, no conjugate; bins above M/2 are the caller's mirror E[M-m] = conj(E[m])).  adapted [dev] uint8 [S][K][T_stride] or
 * NULL: 1 where the frame's update ran (kinds 0-2: |v_0|^2 > threshold after amp4play, strict; kind 3: sf >= 0).
 * State [dev], caller-owned, updated in place so that consecutive blocks continue bit for bit:
 *   R_state   complex128 [S][K][P]     filter (filterCoefficient_)
 *   K_state   complex128 [S][K][P][P]  state error covariance K_k_ (kind 1: the scalar in the real part; kind 0: unused)
 *   sigma2_v  float64    [S][K]        observation noise variance (kinds 1-3)
 *   history   complex128 [S][K][P]     ComplexBuffer_ (aec.h:117-191): slot 0 the newest played frame, scaled by amp4play
 *   dtd_state float64    [S][4]        {EkEnergy_, SkEnergy_, snr_, frames done}; the first three are shared by all bins of a
 *                                      stream and walked in bin order (update_band_, aec.cc:821-853)
 * btk_aec_init writes the constructors' values: R = 0, history = 0, dtd_state = 0; kind 1: sigma2_v = K = sigma2 (aec.cc:95-98);
 * kinds 2, 3: sigma2_v = sigmau2, K = sigmak2 I (aec.cc:190-203).
 * frame_no0: the frame_no argument update_band_ receives (kind 3 only, aec.cc:902): >= 0 the block's frames count up from it;
 * < 0 every frame of the block gets this value (a synthesis bank's next(-5)); BTK_AEC_FRAME_CONTINUE counts up from the state's
 * frames done.  Limits: 1 <= P <= btk_aec_max_filter_length() (64), M <= 2048.  btk_aec_dtd_state_in_lds: 1 when kind 3 keeps K
 * in LDS for the block ((M/2+1) P^2 16 B beside the per-bin vectors), 0 when it updates the exported state in place.           */
#define BTK_AEC_FRAME_CONTINUE (-1073741824L)
int  btk_aec_max_filter_length(void);
int  btk_aec_dtd_state_in_lds(int M, int P);
int  btk_aec_init(int kind, const double* params, int S, int M, int P, void* R_state, void* K_state, double* sigma2_v,
                  void* history, double* dtd_state, void* stream);
int  btk_aec_process(int kind, const double* params, const void* V, const void* A, void* E, void* adapted, int S, int M, int P,
                     long T_stride, long T, long frame_no0, void* R_state, void* K_state, double* sigma2_v, void* history,
                     double* dtd_state, void* stream);

/* ---- Zelinski post-filter -------------------------------------------------------------------
 * Replaces ZelinskiFilter_f / ZelinskiFilter / ZelinskiPostFilter::next
 * (postfilter/postfilter.cc:57-219, 424-491).  Two calls per block:
 * btk_bf_apply_stats = btk_bf_apply plus, from the SAME pass over X, the per-frame statistics of
 *   the time-aligned snapshot x' = conj(d) x:  C = sum_{i<j} x'_i conj(x'_j) (complex64
 *   [S][K][T_stride]) and E = sum_i |x'_i|^2 (float32 [S][K][T_stride]).  D [dev] has W's layout
 *   and holds wq (type & 8, TYPE_ZELINSKI2) or ta_ (postfilter.cc:452-457).
 * btk_zelinski_process = the alpha-recursion on the summed cross/auto spectral densities
 *   (alpha = 0 for the post-filter's first two frames, :460-463), the gain
 *   clamp(f(Phi)/Psi * 2/(N-1), 1e-4, 1) with f = max(Re,0) (type & 1) or |.|, and y <- W y for
 *   frames >= min_frames.  frames_done = frames this post-filter produced before this block.
 *   State [dev]: phi complex64 [S][K], psi float32 [S][K], w_last float32 [S][K] (postfilter_weights()).
 *   Zero the state where the reference re-allocates BeamformerWeights (beamformer.cc:1082-1092).  */
int  btk_bf_apply_stats(const void* W, const void* D, int per_stream_weights, const void* X, void* Y,
                        void* C, float* E, int S, int K, int N, long T_stride, long T, void* stream);
int  btk_zelinski_process(void* Y, const void* C, const float* E, int S, int K, int N, long T_stride, long T,
                          double alpha, int type, int min_frames, long frames_done,
                          void* phi_state, float* psi_state, float* w_last, void* stream);

/* ---- McCowan / Lefkimmiatis post-filters ----------------------------------------------------------
 * Replace McCowanPostFilter::{estimate_average_clean_PSD_, post_filtering_, next} (postfilter/postfilter.cc:798-935)
 * and LefkimmiatisPostFilter::{calc_inverse_noise_spatial_spectral_matrix, calcLambda, estimate_average_noise_PSD_,
 * post_filtering_, next} (:967-1190).  R [dev] complex64 [K][N][N] is the noise coherence matrix R_ (build it with
 * btk_mvdr_diffuse_model == set_diffuse_noise_model :560-618, btk_mvdr_diagonal_loading == set_all_diagonal_loading
 * :620-632).  btk_pf_coherence_coeffs turns it (with threshold_of_Rij_) into the pair-weight matrices Cs (clean PSD)
 * and Cv (noise PSD, may be NULL for McCowan), complex64 [K][N][N].  btk_bf_apply_stats2 = btk_bf_apply plus, from
 * the same snapshots, the per-frame quadratic forms U (and V) complex64 [S][K][T_stride] and E (as btk_bf_apply_stats).
 *   McCowan:      btk_zelinski_process(Y, U, E, ..., type | BTK_PF_MCCOWAN_RULES, ...) -- the gain formula is Zelinski's with the
 *                 weighted sum; with the flag Re or |.| follows type & 1 in every frame, frames below min_frames included
 *                 (:827-832), and the gain is applied to every frame >= min_frames whatever the type (:889-894), so that
 *                 type = 0, 4, 8 or 12 filters as the reference does.
 *   Lefkimmiatis: btk_lefkimmiatis_process(Y, U, V, lambda, fbinX1, ...), lambda [dev] complex64 [K] = d^H pinv(R) d
 *                 from btk_mvdr_lambda (Cholesky with the identity fallback of :975-977), state u/v complex64 [S][K]. */
#define BTK_PF_MCCOWAN_RULES 0x10
int  btk_pf_coherence_coeffs(const void* R, float threshold, int K, int N, void* Cs, void* Cv, void* stream);
int  btk_bf_apply_stats2(const void* W, const void* D, int per_stream_weights, const void* X, void* Y,
                         const void* Cs, const void* Cv, void* U, void* V, float* E,
                         int S, int K, int N, long T_stride, long T, void* stream);
int  btk_lefkimmiatis_process(void* Y, const void* U, const void* V, const void* lambda, int fbinX1,
                              int S, int K, int N, long T_stride, long T, double alpha, int type, int min_frames,
                              long frames_done, void* u_state, void* v_state, float* w_last, void* stream);
int  btk_mvdr_lambda(const void* R, const void* d, void* lambda, int K, int N, float threshold,
                     void* scratch, int* fallback_count, void* stream);

/* ---- Spatial covariance accumulation ----------------------------------------------------------
 * btk_frame_energy: |X_0^H X_0| / M of channel 0 over all M bins, per frame
 *   (MultiChannelSource.update_snapshot_array, lib/pybeamformer.py:263-277); energy [dev] [S][e_stride].
 * btk_cov_frame_gate: w[s][t] = (energy > threshold) * label[s][t] and count[s] += sum_t w
 *   (accu_stats_from_label, pybeamformer.py:967-985; label==NULL means all frames eligible).
 * btk_cov_accumulate: R[s][k] += sum_t tf[s][k][t] * fw[s][t] * x x^H  (either weight may be NULL;
 *   pybeamformer.py:979-981, 1087-1093, 1136-1147).  R [dev] complex64 [S][K][N][N].
 *   use_mfma != 0 selects the v_mfma_f32_32x32x2_f32 kernel, 0 the vector-ALU kernel.
 * btk_cov_scale: R <- float(a * double(R)) on complex64 [S][K][N][N]: the decay step of a recursion R <- a R + sum_t w x x^H
 *   that stays on the device from block to block (btk_cov_accumulate adds the sum).
 * btk_cov_finalize: R <- R/count, then (gamma > 0) improve_matrix_condition
 *   (pybeamformer.py:994-1000, 1200-1207, 1249-1263); count [dev] [S] or [S][K].                  */
int  btk_frame_energy(const void* X, int S, int M, int N, long T_stride, long T, float* energy,
                      long e_stride, void* stream);
int  btk_cov_frame_gate(const float* energy, const float* label, int S, long T_stride, long T,
                        float energy_threshold, float* frame_weights, float* frame_count, void* stream);
int  btk_cov_accumulate(const void* X, const float* tf_weights, const float* frame_weights, void* R,
                        int S, int K, int N, long T_stride, long T, int use_mfma, void* stream);
int  btk_cov_scale(void* R, double a, int S, int K, int N, void* stream);
int  btk_cov_finalize(void* R, const float* count, int count_per_bin, int S, int K, int N, float gamma,
                      void* stream);

/* ---- Batch second-order-statistics beamformers: weight design from accumulated covariances -------
 * btk_cov_mask_count: count[s][k] += sum_t trunc(tf[s][k][t]) * fw[s][t] -- the per-bin integer frame counters of
 *   accu_stats_from_tfmask (lib/pybeamformer.py:1127-1147; the reference's counters are integer arrays, so fractional
 *   mask values weight the covariance but do not count).  count [dev] float32 [S][K].
 * btk_cov_trace_normalize: R <- R / (tr(R)/N) over nbins matrices (SubbandGEVBeamformer.finalize_stats :1326).
 * btk_bmvdr_weights: wqH_k = conj( inv(Rn_k) Rt_k u / (offset + tr(inv(Rn_k) Rt_k)) ), u = e_ref_mic
 *   (SubbandBlindMVDRBeamformer.calc_beamformer_weights :1225-1247).
 * btk_gev_weights: wqH_k = conj of the principal generalised eigenvector of (Rt_k, Rn_k), v^H Rn v = 1, phase of bin
 *   k aligned to bin k-1 (SubbandGEVBeamformer.calc_beamformer_weights :1280-1303).  scipy.linalg.eigh leaves the
 *   phase of each eigenvector to LAPACK; bin 0 is rotated so that its largest component is real positive, i.e. the
 *   result equals the reference's up to one global sign.
 * Rt, Rn [dev] complex64 [nbins][N][N]; WqH [dev] complex64 [nbins][N] (the beamformer output is wqH . x);
 * scratch [dev] btk_sos_scratch_bytes(nbins, N) bytes; *fail_count [dev] += bins whose Rn is not positive definite
 * (the reference raises ArithmeticError there).                                                               */
int  btk_cov_mask_count(const float* tf_weights, const float* frame_weights, int S, int K, long T_stride, long T,
                        float* count, void* stream);
int  btk_cov_trace_normalize(void* R, int nbins, int N, void* stream);
long btk_sos_scratch_bytes(int nbins, int N);
int  btk_bmvdr_weights(const void* Rt, const void* Rn, int nbins, int N, int ref_mic, double offset, void* WqH,
                       void* scratch, int* fail_count, void* stream);
int  btk_gev_weights(const void* Rt, const void* Rn, int K, int N, void* WqH, void* scratch, int* fail_count,
                     void* stream);

/* ---- SubbandMVDR weight design ------------------------------------------------------------------
 * btk_mvdr_diffuse_model: set_diffuse_noise_model (beamformer.cc:2442-2509); mpos [dev] float32 [N][3],
 *   R [dev] complex64 [K][N][N].
 * btk_mvdr_diagonal_loading: set_all_diagonal_loading (beamformer.cc:2511-2523) over nbins matrices.
 * btk_mvdr_weights: calc_mvdr_weights (beamformer.cc:2350-2402): w_k = R_k^-1 d / (N d^H R_k^-1 d),
 *   w_0 = ones; batched complex Cholesky, identity fall-back counted in *fallback_count [dev int]
 *   when a pivot <= threshold (the reference's pseudoinverse() failure path, :262-270, :2381-2383).
 *   wq [dev] complex64 [K][N] = d; W [dev] complex64 [K][N]; scratch [dev] [K][N][N] complex64 only
 *   needed for N > 271 (N <= 136: R_k in LDS; 136 < N <= 271: R_k in the matrix cores' accumulator
 *   registers, read once, never copied; above: panel solver on a copy of R_k); may be NULL otherwise. */
/* btk_mvdr_scratch_bytes: bytes of `scratch` the design entries below (btk_mvdr_weights*, btk_mvdr_lambda) need for K bins of
 *   N channels -- 0 when the solver that will run keeps R_k in LDS or in registers (scratch may then be NULL).            */
long btk_mvdr_scratch_bytes(int K, int N);
int  btk_mvdr_diffuse_model(const float* mpos, int N, int M, float samplerate, float sspeed, void* R, void* stream);
int  btk_mvdr_diagonal_loading(void* R, int nbins, int N, float weight, void* stream);
int  btk_mvdr_weights(const void* R, const void* wq, void* W, int K, int N, float threshold,
                      void* scratch, int* fallback_count, void* stream);
/* btk_mvdr_divide_nondiagonal: divide_nondiagonal_elements / divide_all_nondiagonal_elements (beamformer.cc:2589-2599,
 *   beamformer.h:357-362): R_xy /= (1 + mu), x != y, over nbins matrices.
 * btk_mvdr_weights_flags: btk_mvdr_weights(_shard) that also reports WHICH bins stopped in the Cholesky factorisation
 *   (fail_flags [dev] int32 [K]); btk_mvdr_pinv_fallback re-solves exactly those bins with the reference's own rule -- the
 *   float32-rounded matrix is pseudo-inverted through its SVD, singular values < threshold are zeroed and make the call
 *   "fail", upon which the identity is substituted (pseudoinverse(), beamformer.cc:232-289; :2381-2383) -- and patches W.
 *   It synchronises the stream; *identity_count [host] = bins that ended with the identity.  A Hermitian R_k that is
 *   indefinite but non-singular gets the pseudo-inverse weights the reference computes, not the identity.
 * btk_pinv: that pseudo-inverse for one host matrix A complex128 [M][N] -> invA [N][M]; *below_threshold = number of
 *   singular values zeroed (> 0 == the reference's `return false`).                                                   */
int  btk_mvdr_divide_nondiagonal(void* R, int nbins, int N, float mu, void* stream);
int  btk_mvdr_weights_flags(const void* R, const void* wq, void* W, int K, int N, int first_bin, float threshold,
                            void* scratch, int* fallback_count, int* fail_flags, void* stream);
/* btk_mvdr_weights_streams: the design of S independent streams (each with its own covariance matrices and look direction -- the
 *   SMI-MVDR of S utterances) in ONE launch: R [dev] complex64 [S][K][N][N], wq / W [dev] [S][K][N], fail_flags [dev] int [S*K];
 *   bin 0 of EVERY stream gets the all-ones weight.  The flagged bins go through btk_mvdr_pinv_fallback(R, wq, W, S*K, N, 0, ...)
 *   (a stream's bin 0 is never flagged).  scratch [dev] [S*K][N][N] complex64 for N > 271 only.                                   */
int  btk_mvdr_weights_streams(const void* R, const void* wq, void* W, int S, int K, int N, float threshold,
                              void* scratch, int* fallback_count, int* fail_flags, void* stream);
int  btk_mvdr_pinv_fallback(const void* R, const void* wq, void* W, int K, int N, int first_bin, float threshold,
                            const int* fail_flags, int* identity_count, void* stream);
/* The solve behind it (pinv_kernels.hip), one workgroup per flagged bin, float64 on the float32-rounded matrix: while the matrix
 *   fits in LDS (N <= 70) a one-sided Jacobi SVD with the reference's threshold / identity rule, weights formed without the
 *   inverse; above that the explicit inverse (in-place Gauss-Jordan with row pivoting in a slice of `scratch`) and
 *   1 / sigma_min = || R^-1 ||_2 by power iteration -- the rule only asks whether SOME singular value is below the threshold, and
 *   if none is the pseudo-inverse is the inverse.  btk_mvdr_pinv_fallback_async: on `stream`, no allocation, no host
 *   synchronisation; identity_count [dev int[2]]: [0] += bins that ended with the identity, [1] += bins whose Jacobi sweeps hit
 *   their limit of 60 without converging; scratch [dev] btk_mvdr_pinv_scratch_bytes(K, N) bytes (0 for the LDS form).
 *   btk_mvdr_pinv_not_converged: that second count for this thread's last (blocking) btk_mvdr_pinv_fallback call.
 *   btk_mvdr_pinv_fallback_host: the SVD solve bin by bin on one host thread (the round-2 form; checker / A-B timing only). */
long btk_mvdr_pinv_scratch_bytes(int K, int N);
int  btk_mvdr_pinv_fallback_async(const void* R, const void* wq, void* W, int K, int N, int first_bin, float threshold,
                                  const int* fail_flags, int* identity_count, void* scratch, void* stream);
int  btk_mvdr_pinv_fallback_host(const void* R, const void* wq, void* W, int K, int N, int first_bin, float threshold,
                                 const int* fail_flags, int* identity_count, void* stream);
int  btk_mvdr_pinv_not_converged(void);
int  btk_pinv(const double* A, int M, int N, float threshold, double* invA, int* below_threshold);
/* ---- The reference's float32 csvdc, decision for decision -------------------------------------------
 * pseudoinverse() (beamformer/beamformer.cc:232-289) returns false -- and calc_mvdr_weights (:2379-2384) /
 * LefkimmiatisPostFilter::calc_inverse_noise_spatial_spectral_matrix (postfilter/postfilter.cc:967-980) then use the identity --
 * when LINPACK's float32 csvdc (matrix/linpack_c.cc:9516) reports INFO != 0 (no convergence within 30 QR sweeps) or leaves a
 * singular value below the threshold.  On the 256-microphone diffuse model of BASELINE config C5 INFO != 0 on about half the
 * bins; the decision depends on the float32 roundings, so it is reproduced with the same arithmetic in the same order.
 * btk_csvdc_values: csvdc with job = 0 (no vectors: they never feed back into s, e or INFO) for K matrices A [dev] complex64
 *   [K][n][p] row-major (not modified); s, e [dev] float32 [K][min(n + 1, p)] (either may be NULL), info [dev] int32 [K];
 *   scratch [dev] btk_csvdc_scratch_bytes(K, n, p) bytes (0: the matrix lives in LDS, scratch may be NULL).  Bit-identical to
 *   the reference's compiled csvdc (tests/test_gpu_linpack_rule.py against oracle/_ref and tests/golden/c5_csvdc_info.npz).
 * btk_mvdr_linpack_rule: applies that decision to a design some solver has already written: R [K][N][N], wq [K][N]; every bin
 *   for which pseudoinverse() returns false gets W_k = d / (N d^H d) (W may be NULL) and lambda_k = d^H d (lambda may be NULL)
 *   and its fail_flags entry (may be NULL) is cleared, so btk_mvdr_pinv_fallback afterwards only visits bins that converged but
 *   are not positive definite.  skip_dc != 0: the DC bin (first_bin + k == 0, or k % kper == 0 for kper > 0 stacked streams)
 *   is left alone like calc_mvdr_weights does; the Lefkimmiatis filter decomposes bin 0 too (skip_dc = 0).
 *   counts [dev int[2]] (may be NULL): [0] += bins with INFO != 0, [1] += converged bins with a singular value < threshold.
 *   scratch [dev] btk_mvdr_linpack_rule_scratch_bytes(K, N) bytes.  All on `stream`, no allocation, no synchronisation.      */
long btk_csvdc_scratch_bytes(int K, int n, int p);
int  btk_csvdc_values(const void* A, int K, int n, int p, float* s, float* e, int* info, void* scratch, void* stream);
long btk_mvdr_linpack_rule_scratch_bytes(int K, int N);
int  btk_mvdr_linpack_rule(const void* R, const void* wq, void* W, void* lambda, int K, int N, int first_bin, int kper,
                           int skip_dc, float threshold, int* fail_flags, int* counts, void* scratch, void* stream);
/* ---- The reference's float32 SVD pseudo-inverse itself: csvdc with job = 11 and A+ = V S^-1 U^H -----------------------------
 * The third MVDR rule ("linpack_full"): not only pseudoinverse()'s decision but its matrix.  csvdc's U and V are produced rotation
 * for rotation (matrix/linpack_c.cc:9727-9733, 9777-9783, 9812-9882, 9899-9920 and the csrot / cscal / cswap of the iteration,
 * :10052-10055, 10074-10077, 10133-10148, 10164-10167, 10183-10191), the inverse is assembled from them in the source's order
 * (beamformer/beamformer.cc:262-280) and the weights follow in float64 (:2386-2396).  Sizes: 1 <= n, p <= 256.
 * btk_csvdc_full: K matrices A [dev] complex64 [K][n][p] row-major (not modified) -> s, e [dev] float32 [K][min(n + 1, p)] (either
 *   may be NULL), U [dev] complex64 [K][n][n] and V [K][p][p], each matrix COLUMN-major like the reference's u, v (element (i, k) at
 *   [i + k * n]), info [dev] int32 [K]; scratch [dev] btk_csvdc_full_scratch_bytes(K, n, p) bytes.  Bit-identical to the
 *   reference's compiled csvdc (tests/test_gpu_linpack_full.py).
 * btk_pinv_linpack: pseudoinverse() (beamformer.cc:232-289) of K matrices A [K][M][N], M >= N: invA [dev] complex64 [K][N][M]
 *   row-major, computed for every matrix; ok [dev] int32 [K]: its return value (INFO == 0 and no singular value under the
 *   threshold); info [dev] int32 [K]; scratch [dev] btk_pinv_linpack_scratch_bytes(K, M, N) bytes.
 * btk_mvdr_linpack_full: calc_mvdr_weights (beamformer.cc:2372-2397) / calcLambda (postfilter/postfilter.cc:967-995) for K bins:
 *   R [K][N][N], wq [K][N] -> W [K][N] (may be NULL) and lambda [K] = d^H A+ d (may be NULL), for EVERY bin: from the reference's
 *   inverse where pseudoinverse() returns true, from the identity where not.  first_bin, kper, skip_dc as btk_mvdr_linpack_rule
 *   (a skipped DC bin gets the all-ones weight, :2369-2371, and no lambda); counts [dev int[2]] (may be NULL) as there;
 *   scratch [dev] btk_mvdr_linpack_full_scratch_bytes(K, N) bytes.  All on `stream`, no allocation, no synchronisation.      */
long btk_csvdc_full_scratch_bytes(int K, int n, int p);
int  btk_csvdc_full(const void* A, int K, int n, int p, float* s, float* e, void* U, void* V, int* info, void* scratch, void* stream);
long btk_pinv_linpack_scratch_bytes(int K, int M, int N);
int  btk_pinv_linpack(const void* A, int K, int M, int N, float threshold, void* invA, int* ok, int* info, void* scratch, void* stream);
long btk_mvdr_linpack_full_scratch_bytes(int K, int N);
int  btk_mvdr_linpack_full(const void* R, const void* wq, void* W, void* lambda, int K, int N, int first_bin, int kper, int skip_dc,
                           float threshold, int* counts, void* scratch, void* stream);
/* The same solve for a bin SHARD [first_bin, first_bin + K) of a bin-sharded run: only global bin 0 gets the
 * all-ones weight of calc_mvdr_weights (beamformer.cc:2369-2371).                                                    */
int  btk_mvdr_weights_shard(const void* R, const void* wq, void* W, int K, int N, int first_bin, float threshold,
                            void* scratch, int* fallback_count, void* stream);

/* ---- Multi-channel WPE dereverberation ---------------------------------------------------------
 * Replaces MultiChannelWPEDereverberation::estimate_filter / calc_every_channel_output
 * (dereverberation/dereverberation.cc:312-698).  X [dev] complex64 [S][K][C][T_stride] (the snapshot
 * layout with C channels); L = upperN-lowerN+1 lags, prediction order P = C*L, lag vector ordered
 * channel-major then lag (:540-555).  lower_bw/upper_bw = lower_bandWidthN_/upper_bandWidthN_ (:361-369):
 * bins with lower_bw < k < upper_bw are left untouched.
 * btk_wpe_estimate: `iterations` rounds of { theta = max(|y - g^H ybar|,1e-3)^2 ; R = A diag(1/theta) A^H
 *   + bias I (fp32 MFMA HERK) ; r ; diagonal loading |R_ii| + max|R_ii| 10^(load_db/10) ; Cholesky solve }.
 *   G [dev] complex64 [S][C][K][P] in/out (zeros == a fresh object / next_speaker()).
 *   workspace [dev] btk_wpe_workspace_bytes(...) bytes; *fail_count [dev int] counts failed factorisations
 *   (the reference throws jnumeric_error, :676-680).
 * btk_wpe_apply: OUT[s][k][c][t] = y_c(t) - g_c^H ybar(t) for t >= lowerN using the L-frame ring rule of
 *   :471-480; other frames/bins are copied.                                                          */
long btk_wpe_workspace_bytes(int S, int K, int C, int lowerN, int upperN, long T_stride);
int  btk_wpe_estimate(const void* X, int S, int K, int C, long T_stride, long T, int lowerN, int upperN,
                      int iterations, double load_db, double diagonal_bias, int lower_bw, int upper_bw,
                      void* G, void* workspace, int* fail_count, void* stream);
int  btk_wpe_apply(const void* X, const void* G, void* OUT, int S, int K, int C, long T_stride, long T,
                   int lowerN, int upperN, int lower_bw, int upper_bw, void* stream);

/* ---- Multi-GPU: frequency-bin sharding ---------------------------------------------
 * One process per GPU.  Rank g owns the bins btk_bin_range(K, g, world) = [g ceil(K/world), ...) -- trailing ranks may
 * be short or empty -- for analysis storage (btk_fb_analysis_bins), weight design (btk_mvdr_weights_shard), covariance,
 * beamforming, post-filter; btk_allgather_bins is the ONE collective of the path: every rank contributes its
 * beamformed block Y_local [dev] complex64 [S][k1-k0][T_stride] and receives Y [dev] complex64 [S][K][T_stride] for the
 * synthesis bank.  nccl_comm: an initialised ncclComm_t of `world` ranks (RCCL over xGMI); the collective is enqueued on
 * `stream`.  RCCL is bound at run time, the library does not link it.  Stream sharding needs no entry point: streams are
 * independent (rank = stream mod world, no collective).                                                                 */
void btk_bin_range(int K, int rank, int world, int* k0, int* k1);
int  btk_allgather_bins(void* nccl_comm, const void* Y_local, void* Y, int S, int K, long T_stride, int rank, int world,
                        void* stream);
/* The even form -- north_star's "single RCCL all-gather": Y [dev] complex64 [S][Kp][T_stride] with
 * Kp = btk_bin_rows_padded(K, world) = world ceil(K / world) rows per stream (rows >= K are padding); every rank has written its
 * beamformed bins in place at rows [rank ceil(K/world), ...) (btk_bf_apply straight into that view), and ONE in-place
 * ncclAllGather per stream completes Y on every rank: no staging buffer, no copy.  btk_allgather_bins (grouped broadcasts) remains
 * for callers whose Y has exactly K rows.                                                                                  */
int  btk_bin_rows_padded(int K, int world);
int  btk_allgather_bins_inplace(void* nccl_comm, void* Y, int S, int K, long T_stride, int rank, int world, void* stream);

/* ---- Host-side weight design (double precision, one-off per look direction) -------------
 * BeamformerWeights::calcMainlobe (beamformer.cc:502-565): wq [host] complex128 [M][N].     */
int  btk_weights_mainlobe(int M, int N, float samplerate, const double* delays, double* wq);
/* the same with halfBandShift == true (beamformer.cc:515-527): bin k at (k + 0.5) fs / M, partner of bin k is bin M-1-k */
int  btk_weights_mainlobe_halfband(int M, int N, float samplerate, const double* delays, double* wq);
/* LCMV quiescent weights with two constraints (target + one null): calcMainlobe2 / calcMainlobeN +
 * calc_null_beamformer_ + calc_inverse_22mat_ (beamformer.cc:181-221, 299-363, 572-721); wq [M][N].   */
int  btk_weights_mainlobe_2(int M, int N, float samplerate, const double* delaysT, const double* delaysI, double* wq);
/* BeamformerWeights::calcMainlobeN (beamformer/beamformer.cc:600-721) with NC >= 2 constraints: delaysIs [host]
 * float64 [NC-1][N].  NC = 2 takes the closed-form path above; NC > 2 inverts the NC x NC Gram matrix in float64
 * (the reference: float32 SVD pseudoinverse, :352-355).                                                        */
int  btk_weights_mainlobe_n(int M, int N, float samplerate, const double* delaysT, const double* delaysIs, int NC,
                            double* wq);
/* calc_blocking_matrix_ (beamformer.cc:373-454): a [host] complex128 [N]; B [host] [N][N-NC] */
int  btk_weights_blocking_matrix(const double* a, int N, int NC, double* B);
/* calcSidelobeCancellerU_f (beamformer.cc:752-767): wl = B wa                               */
int  btk_weights_sidelobe(const double* B, const double* wa, int N, int NC, double* wl);
/* Effective GSC weights (wq - wl, optional normalisation of calc_gsc_output :1228-1237) for
 * bins 0..M/2 as complex64 [K][N] ready for btk_bf_apply; bin 0 is wq_0 alone (:1288-1291). */
int  btk_weights_gsc_effective(const double* wq, const double* wl, int M, int N,
                               int normalize, float* w_out);

/* ---- Steered response power: DOAEstimatorSRPBase / DOAEstimatorSRPDSBLA (beamformer.h:466-569) ----------------------
 * The search grid of calc_steering_unit_table_ (beamformer.cc:3052, :3071) in the reference's types: float parameters,
 * n = (unsigned)((max - min) / width + 0.5), theta accumulated in double.  thetas_out [host] float64 [n] or null (count
 * only).  min > max is the parameter error of set_search_param (:2999-3006).                                             */
int  btk_srp_grid(float min_theta, float max_theta, float width_theta, int* n_theta, double* thetas_out);
/* set_look_direction_ (:3193-3207): delays [host] float64 [N], |p_n - p_0| cos(theta), theta rounded to float as there;
 * positions [host] float64 [N] in seconds (positions over the speed of sound).                                           */
int  btk_srp_delays(int N, const double* positions, double theta, double* delays_out);
/* svTbl_ (:3046-3089): out [host] complex128 [n_theta][M/2+1][N]; row [u][k] is wq_k of btk_weights_mainlobe for the
 * delays of theta_u on bins fbin_min .. fbin_max, ones in bin 0, zero elsewhere.                                         */
int  btk_srp_table(int M, int N, float samplerate, const double* positions, int n_theta, const double* thetas,
                   int fbin_min, int fbin_max, double* out);
/* The table in the operand order of the kernel: packed [host] complex64, btk_srp_packed_elems(U, K, N) elements
 * ([K][PP][UP][2], element [k][p][u][h] = sv[u][k][2p+h], zero beyond N and U; PP, UP: pairs / directions rounded up to
 * the register chunk and to 32).  Copy it to the device once per table.                                                  */
long btk_srp_packed_elems(int U, int K, int N);
int  btk_srp_pack_table(const double* table, int U, int K, int N, float* packed);
/* calc_response_power_ for every grid direction and frame of a block, and calc_energy (:3091-3122, :3221-3251), one pass
 * over X [dev] complex64 [S][M/2+1][N][T_stride] on the fp32 matrix cores; the beams are never written.
 *   rp [dev] float32 [S][U][T] = sum_{k=fmin}^{fmax} c_k |sv[u][k]^H x_k[t]|^2 / (fmax - fmin + 1), c_k = 2 (k < M/2), 1
 *   energy [dev] float32 [S][T] = sum_k c_k (sum_n |x_k[n][t]|^2)^2 / (M N)
 * N = 2 .. 256, 1 <= fbin_min <= fbin_max <= M/2.  Directions run in passes of up to 128; for N <= 64 a pass reads X once,
 * for N > 64 the 32-frame strip is fetched again for each of its up to four 32-direction tiles (from cache at best).     */
int  btk_srp_power(const void* X, const void* table_packed, void* rp, void* energy, int S, int M, int N, long T_stride,
                   long T, int U, int fbin_min, int fbin_max, void* stream);
/* The per-frame N-best insertion (strict >, :3157-3187), the energy gate (:3148-3155) and accRPs_ (:3162):
 *   nbest_rp [dev] float32 [S][T][nbest], nbest_idx [dev] int32 [S][T][nbest] (-10e10 / -1 where nothing was inserted),
 *   gate [dev] int32 [S][T] = !(energy < threshold), acc [dev] float64 [S][U] += gate rp, frame by frame in index order
 *   (NULL: no accumulation, for a caller that accumulates frame by frame itself).  nbest <= 16.                          */
int  btk_srp_select(const void* rp, const void* energy, float threshold, int nbest, void* nbest_rp, void* nbest_idx,
                    void* gate, void* acc, int S, int U, long T, void* stream);

/* ---- Maximum-empirical-kurtosis GSC beamformers: SubbandMEKBeamformer / SubbandNMEKBeamformer (lib/pybeamformer.py:1596-1860)
 * Shared inputs, for the bins k < K and the sources s < NS:
 *   X [dev] complex64 [K][N][T_stride]      observation snapshots, frames contiguous
 *   mask [dev] float32 [T] or NULL           only frames with mask != 0 count (the reference's list of observations)
 *   wuH [dev] complex128 [NS][K][N]          upper-branch weights;  BmH [dev] complex128 [NS][K][N-Nc][N]
 *   alpha, beta, gamma                       regulariser, kurtosis constant, norm bound (gamma < 0: ||wuH[s][k]||)
 *   normalize                                0 = MEK, 1 = NMEK (the clamp of normalize_weight, :1845-1855)
 *   prevAvgY2, prevAvgY4 [dev] float64 [K][NS], prevFrameN [dev] int64 [K][NS], or NULL for zero statistics
 * N = 2 .. btk_hos_max_channels() (64), Nc = 1 or 2, NS = 1 or 2, T >= 1; BTK_ERR_DIMENSION otherwise.  All sums are
 * float64 in a fixed order (no atomics): two calls give the same bits.                                                     */
int  btk_hos_max_channels(void);
/* Bytes of device workspace btk_hos_eval / btk_hos_minimize need for these sizes: 0 -- everything the kernels keep between
 * their phases lives in LDS, neither entry takes a workspace argument.  Kept so that callers can size buffers uniformly.
 * A mask that selects no frame, with zero previous statistics, divides by zero exactly as the reference's empty list of
 * observations does: fun, grad and the optimiser's outputs of such a call are NaN, the statistics sums are 0.             */
long btk_hos_workspace_bytes(int K, int N, int Nc, int NS, long T);
/* fun_hos_bf and dfun_hos_bf (:1548-1593) over calc_obj_func and gradient (:1632-1683) at the packed weights
 * x [dev] float64 [K][2 NS (N-Nc)] (NULL: zero), every bin in one launch:
 *   fun [dev] float64 [K];  grad [dev] float64 [K][2 NS (N-Nc)] or NULL (objective only: the snapshots are read once)
 *   stats [dev] float64 [K][2 NS + 2] or NULL: (sum_t |Y_s|^2, sum_t |Y_s|^4) per source, then sum_t m_t and sum_t m_t^2
 *   with m_t = sum_s |Y_s[t]|^2 / NS, the frame terms of store_stats (:1618-1627).                                       */
int  btk_hos_eval(const void* X, const void* mask, const void* wuH, const void* BmH, const void* x, double alpha, double beta,
                  double gamma, int normalize, const void* prevAvgY2, const void* prevAvgY4, const void* prevFrameN, int K,
                  int N, int Nc, int NS, long T_stride, long T, void* fun, void* grad, void* stats, void* stream);
/* The per-bin optimisation of estimate_active_weights (:1802-1827) for every bin in one launch, one workgroup per bin, no host
 * round trip: Polak-Ribiere+ conjugate gradients with Armijo backtracking from x0 [dev] float64 [K][D] (NULL: zero).  Per
 * iteration: stop if ||g|| < gtol; d = -g if g.d >= 0; first trial step 2 / ||g|| in the first iteration, else twice the last
 * accepted one; up to max_halvings halvings until fun(x + a d) <= f + armijo_c1 a g.d, stop if none; then
 * d = -g' + max(0, g'.(g' - g) / g.g) d; stop if |f - f'| < mindelta.
 *   x_out [dev] float64 [K][D], f_out [dev] float64 [K], iters_out [dev] int32 [K]
 *   trace_f [dev] float64 [K][maxiter] accepted objective values (NaN where none)
 *   trace_halvings [dev] int32 [K][maxiter] halvings of each iteration (-1: no step accepted, -2: iteration not reached)  */
int  btk_hos_minimize(const void* X, const void* mask, const void* wuH, const void* BmH, const void* x0, double alpha,
                      double beta, double gamma, int normalize, const void* prevAvgY2, const void* prevAvgY4,
                      const void* prevFrameN, int K, int N, int Nc, int NS, long T_stride, long T, int maxiter, double gtol,
                      double mindelta, int max_halvings, double armijo_c1, void* x_out, void* f_out, void* iters_out,
                      void* trace_f, void* trace_halvings, void* stream);

/* ---- GCC-PHAT time delay of arrival: the front end of unit_test/test_tdoa_estimator.py --------------------------------
 * HammingFeature::next + FFTFeature::next (feature/feature.cc:1177-1200, :1205-1258, :29-43) for a block of frames of
 * pcm [dev] float32 [S][C] rows of len samples, pcm_stride apart.  Frame t covers samples t D .. t D + D - 1, zero beyond len
 * (pad_zeros); T = btk_tdoa_frames(len, D) = ceil(len / D).  window BTK_TDOA_WINDOW_HAMMING: 0.54 - 0.46 cos(2 pi i / (D - 1))
 * and the product in float64, rounded to float32 (the gsl_vector_float of HammingFeature); BTK_TDOA_WINDOW_NONE: the frames as
 * they are (FFTFeature over a source that is no HammingFeature).  Zero padding to L; forward transform, unnormalised.
 *   X [dev] complex64 [S][C][T][L/2+1];  energy [dev] float32 [S][C][T] = 2 sum_{k <= L/2} |X_k|^2 (lib/pytdoa.py:47)
 * L a power of two from 256 to 16384, 2 <= D <= L; BTK_ERR_DIMENSION otherwise, nothing launched.                          */
#define BTK_TDOA_WINDOW_NONE 0
#define BTK_TDOA_WINDOW_HAMMING 1
long btk_tdoa_frames(long len, int D);
int  btk_tdoa_spectra(const float* pcm, long len, long pcm_stride, int S, int C, int D, int L, int window, void* X,
                      void* energy, void* stream);
/* PHATFeature.next + TDOAFeature.next (lib/pytdoa.py:32-54, :87-114) for every listed pair and every frame:
 *   pairs [dev] int32 [P][2] channel indices, in the caller's order ((b, a) is another pair than (a, b))
 *   P_k = X_a[k] conj X_b[k] / |X_a[k] conj X_b[k]|, g = irfft(P) (1/L, imaginary parts of bins 0 and L/2 ignored)
 *   lag [dev] int32 [S][P][T]: the first n with the largest |g[n]|, as n (n < L/2) or n - L;  height [dev] float32 = |g[n]|
 *   gcc [dev] float32 [S][P][T][L] or NULL (the normal case): g itself.
 * No peak -- lag BTK_TDOA_NO_PEAK, height 0 -- where both energies are <= energy_threshold (gcc row: zeros), where a bin of
 * either channel is exactly zero (the reference's 0/0; gcc row: NaN), where g has no positive |g[n]|, and for a pair that
 * names a channel outside 0 .. C-1.                                                                                        */
#define BTK_TDOA_NO_PEAK (-2147483647 - 1)
int  btk_tdoa_gcc_peaks(const void* X, const void* energy, const int* pairs, int P, float energy_threshold, int S, int C,
                        long T, int L, void* lag, void* height, void* gcc, void* stream);

/* ---- EKF / IEKF speaker tracking: the tracker of unit_test/test_source_tracking.py -------------------------------------------
 * ExtendedKalmanFilter.next / KalmanFilter.update / IteratedExtendedKalmanFilter.update (lib/pykalman.py:84-162, :199-216,
 * :232-266) over TDOAFeatureVector.next and the tdoa / linearize / calc_linearized_observation of the three feature vectors
 * (lib/pytdoa.py:213-287, :365-415, :460-516), for S independent streams and the T frames of a block, float64 throughout:
 *   lag [dev] int32 [S][P][T], height [dev] float32 [S][P][T]: the outputs of btk_tdoa_gcc_peaks.  A pair is observed in a
 *     frame where (double)height > threshold and lag != BTK_TDOA_NO_PEAK; its delay is (double)lag * Ts.  A frame with fewer
 *     than minimum_pairs observed pairs leaves the state as it is.
 *   geom [dev] float64 [P][6] per pair (first, second microphone), shared by the streams:
 *     BTK_EKF_MODEL_LINEAR    (n = 1, azimuth):          [d_second - d_first, ...] distances from the first microphone
 *     BTK_EKF_MODEL_CIRCULAR  (n = 2, polar, azimuth):   [p_second - p_first (3), ...]
 *     BTK_EKF_MODEL_CARTESIAN (n = 3, position):         [p_first (3), p_second (3)]
 *   t_begin [dev] int32 [S] or NULL (all 0): the stream's first tracked frame of the block; earlier frames get flags 0.
 *   state [dev] float64 [S][16], read and written: x[3], K_filter[9] (row-major 3 x 3, the leading n x n block is used), time,
 *     lastUpdateT, two spare.  time is the reference's counter at the first tracked frame (set_time), lastUpdateT is -1 before
 *     the first update.  T frames in one call and in consecutive calls give the same bits.
 *   xk [dev] float64 [S][T][3], Kf [dev] float64 [S][T][9]: xk_filter and K_filter after every frame.
 *   flags [dev] int32 [S][T]: BTK_EKF_TRACKED | BTK_EKF_OBSERVED | BTK_EKF_UPDATED (observed and not gated) | rounds of the
 *     IEKF used << BTK_EKF_ROUNDS_SHIFT.
 * The gate is the reference's scipy.stats.chi.cdf(d2, nobs) > gate_prob with d2 the SQUARED Mahalanobis distance (gate_prob 0:
 * no gate).  The nobs x nobs inverse is replaced by the n x n one of sigmaV2 I + H^T H K_predict.
 * BTK_ERR_PARAMETER for a parameter outside its range, BTK_ERR_DIMENSION for S, P, T < 1 or P > 877; nothing is launched.  */
#define BTK_EKF_MODEL_LINEAR 0
#define BTK_EKF_MODEL_CIRCULAR 1
#define BTK_EKF_MODEL_CARTESIAN 2
#define BTK_EKF_TYPE_EKF 0
#define BTK_EKF_TYPE_IEKF 1
#define BTK_EKF_TRACKED 1
#define BTK_EKF_OBSERVED 2
#define BTK_EKF_UPDATED 4
#define BTK_EKF_ROUNDS_SHIFT 8
#define BTK_EKF_MAX_ROUNDS 1000000
typedef struct btk_ekf_params {
  int n, model, type;          /* state length, BTK_EKF_MODEL_*, BTK_EKF_TYPE_* */
  double F[9], U[9];           /* state transition, process noise covariance: row-major 3 x 3, leading n x n block used */
  double sigmaV2, time_delta, gate_prob;
  int num_iterations;          /* IEKF rounds at most (>= 1) */
  double iteration_threshold;  /* the IEKF stops after the round with |eta_i - eta_(i-1)|^2 below it */
  double threshold;            /* peak height above which a pair is observed */
  int minimum_pairs;
  double Ts, c;                /* sampling period in seconds; speed of sound in position units per second */
} btk_ekf_params;
int  btk_ekf_track(const btk_ekf_params* params, const void* lag, const void* height, const void* geom, const void* t_begin,
                   int S, int P, long T, void* state, void* xk, void* Kf, void* flags, void* stream);

/* ---- ASR front end: the nodes of unit_test/log_power_extractor.py and unit_test/mfcc_extractor.py --------------------------
 * Stages: PCM(0) -> SPECTRUM(1) -> POWER(2) -> VTLN(3) -> MEL(4) -> LOG(5) -> CEP(6).  btk_fe_process takes the vectors of stage
 * in_stage and runs the stages after it, up to the last one whose out[] pointer is non-NULL; VTLN is skipped where vtln_rows is
 * NULL, MEL where mel_rows is NULL.  Every requested stage is written: out[stage] [dev] float32 [S][C][T][dim] (SPECTRUM:
 * complex64 [S][C][T][L/2+1]); out[0] is unused.
 *
 * PCM (PreemphasisFeature::next, feature/feature.cc:1128-1144; HammingFeature::next + FFTFeature::next, :1177-1258):
 *   in [dev] float32 [S][C] rows of len samples, pcm_stride apart.  Frame t covers samples t shift .. t shift + D - 1, zero at and
 *   beyond len; 1 <= shift <= D <= L, T frames (btk_fe_frames gives SampleFeature's count).  preemph != 0: sample i becomes
 *   float(x_i - mu prior) with the difference in float64; the prior is the sample before it, for the first sample of frame t > 0
 *   the LAST sample of frame t - 1 (sample (t-1) shift + D - 1, the reference's prior_, also when frames overlap), for t = 0
 *   prior0 [dev] float32 [S][C] (NULL: zero).  window as btk_tdoa_spectra (float64 product rounded to float32), zero padding to L,
 *   forward transform, unnormalised.  L a power of two from 256 to 16384.  With window HAMMING, no pre-emphasis and shift = D
 *   the spectra have the bits of btk_tdoa_spectra.
 * POWER (SpectralPowerFeature::next, :1291-1314): |X_k|^2, k < powN, powN = L/2+1 or L (upper half: the conjugate mirror).
 * VTLN (VTLNFeature::nextOrg / nextFF, :1672-1792), MEL (MelFeature::next over fmatrixBMulot, :2055-2109, :2229-2242),
 * CEP (CepstralFeature::next, :2402-2415): a table applied to the previous stage, accumulated in float64, rounded to float32.
 *   *_rows [dev] int32 [N][3]: (first input index, coefficient count, index of the row's first coefficient in *_w)
 *   vtln_w [dev] float64, mel_w [dev] float32 packed row after row;  dct [dev] float32 [cepN][dimension of LOG], dense.
 *   Coefficients that would read past the input vector are ignored.
 * LOG (LogFeature::next, :2332-2362): float(log_m log10(v + log_a)) with v + log_a <= 0 -> 1.0, or with log_floor != 0
 *   v < 1e-5 -> 1e-5 and log_a unused; evaluated in float64 on the float32 input.
 * The tables are the caller's: a coefficient that would read past the input vector or past *_nw is ignored, nothing else of a
 * table is checked.  Entering at SPECTRUM or later no stage may be longer than 20480 values (BTK_ERR_DIMENSION).
 * in_stage >= POWER: in_dim is the length of the input vectors (any >= 1) and the PCM fields are unused; in_stage == SPECTRUM:
 * in [dev] complex64 [S][C][T][L/2+1].  With in_stage PCM the stage lengths after POWER may not exceed L/2+1 (vtlnN: powN).
 * BTK_ERR_DIMENSION for L, D, shift, powN or a stage length outside these ranges, BTK_ERR_PARAMETER for a null input, an unknown
 * stage or window, or no requested output; nothing is launched.                                                              */
#define BTK_FE_PCM 0
#define BTK_FE_SPECTRUM 1
#define BTK_FE_POWER 2
#define BTK_FE_VTLN 3
#define BTK_FE_MEL 4
#define BTK_FE_LOG 5
#define BTK_FE_CEP 6
typedef struct btk_fe_params {
  int S, C;
  long T;
  int in_stage, in_dim;
  long len, pcm_stride;
  int D, shift, L, window, preemph;
  double mu;
  const float* prior0;
  int powN;
  int vtlnN, vtln_nw;          /* rows, packed weights */
  const int* vtln_rows;
  const double* vtln_w;
  int melN, mel_nw;
  const int* mel_rows;
  const float* mel_w;
  double log_m, log_a;
  int log_floor;
  int cepN;
  const float* dct;
  void* out[7];
} btk_fe_params;
/* frames of SampleFeature(block_len = D, shift_len = shift) over len samples (feature/feature.cc:1050-1108): every start
 * t shift < len with pad_zeros, every start with t shift + D <= len without                                                  */
long btk_fe_frames(long len, int D, int shift, int pad_zeros);
int  btk_fe_process(const btk_fe_params* params, const void* in, void* stream);
/* Host code, no device.  MelFeature::SparseMatrix_::melScaleOrg (version 1) / melScaleFF (version 2), feature/feature.cc:1892-2039
 * with the constructor's up <= 0 -> rate / 2 (:2199-2208), every float of the reference a float32 here:
 *   offset [host] int32 [filterN], count [host] int32 [filterN], coef [host] float32 [coef_cap] packed row after row,
 *   *ncoef: coefficients written.  Version 1 advances the frequency before the coefficient (negative coefficients are kept).
 * BTK_ERR_PARAMETER for low < 0, 2 up > rate, low > up (the reference's j_error) or a version other than 1 and 2;
 * BTK_ERR_DIMENSION for a row with offset + count > powN, a negative count or more than coef_cap coefficients.                 */
int  btk_fe_mel_table(int powN, float rate, float low, float up, int filterN, int version, int* offset, int* count,
                      float* coef, int coef_cap, int* ncoef);
/* VTLNFeature::nextOrg (version 1) / nextFF (version 2), feature/feature.cc:1672-1792, as the operator W [N][inN] on the power
 * vector, out_k = sum_s W[k][s] in_s.  Version 1: the interpolation weights alpha0, ones, alpha1 with the index clamps of
 * :1703-1707.  Version 2 (inN == N): the scatter weights with float32 b, slope1, slope2, sIdx -+ 0.5, dIdx, the k < 0 -> 0 clamp
 * and the k >= N break, each row divided by its normaliser auxV_ where that exceeds 1e-20 (at ratio 1 a normalised
 * [1/2, 1, 1/2] smoothing, not the identity).
 *   offset, count [host] int32 [N]: the span of each row's non-zero weights;  w [host] float64 [w_cap] packed;  *nw: weights written
 * BTK_ERR_PARAMETER for another version, BTK_ERR_DIMENSION for N, inN < 1, version 2 with inN != N or more than w_cap weights.  */
int  btk_fe_vtln_table(int N, int inN, double ratio, double edge, int version, int* offset, int* count, double* w, int w_cap,
                       int* nw);
/* gsl_matrix_float_set_cosine types 0 and 1 (matrix/gslmatrix.cc:107-131) and type 2, CepstralFeature::sphinxLegacy_
 * (feature/feature.cc:2389-2400): dct [host] float32 [cepN][filterN], computed in float64 and rounded.
 * BTK_ERR_PARAMETER for another type, BTK_ERR_DIMENSION for cepN, filterN < 1 (type 0: filterN < 2).                           */
int  btk_fe_dct_table(int type, int cepN, int filterN, float* dct);

/* ---- FFT block convolution: OverlapAdd::next / OverlapSave::next (convolution/convolution.cc:83-131, :196-230) ----------------
 * FIR filtering of whole rows by N-point real transforms (fft_long.h, N a power of two from 256 to 16384), one workgroup per
 * (output row, tile) in the overlap-save arrangement: a span of N samples, forward transform, product with the filter's half
 * spectrum (bins 0 and N/2 real times real, convolution.cc:103-104), inverse transform, Lk samples kept.  P taps are cut into Q
 * partitions of Bp taps (the last may be shorter), Lk + Bp - 1 <= N; a tile costs Q + 1 transforms.  OverlapAdd's float32
 * running sum (convolution.cc:116-127) is not re-enacted: the result is the same linear convolution.
 *
 * Host code, no device: the rule that picks transform, tile and partition for P taps, with N capped by n_max (a power of two
 * from 256 to 16384):  N = min(max(next_pow2(4 P), 8192), n_max);  Bp = P, Q = 1 if P <= N/2 + 1, else Bp = N/2,
 * Q = ceil(P / Bp);  Lk = N - Bp + 1.  (8192 is the length that filtered long rows fastest for short filters; a caller with
 * short rows caps N with n_max.)  BTK_ERR_DIMENSION for P < 1 or a bad n_max, BTK_ERR_PARAMETER for a null pointer.                          */
int  btk_conv_plan(int P, int n_max, int* N, int* Lk, int* Bp, int* Q);
/* The filters' half spectra (OverlapAdd::set_impulse_response_, convolution.cc:43-60, in float32 on the device):
 *   h [dev] float32 [R] rows of P taps, h_stride apart  ->  H [dev] complex64 [R][Q][N/2+1], partition q = taps q Bp ..
 * BTK_ERR_DIMENSION for N no power of two in 256 .. 16384, P < 1, Q Bp < P, (Q - 1) Bp >= P, h_stride < P, R < 1.             */
int  btk_conv_filter_spectra(const float* h, long h_stride, int R, int P, int N, int Bp, int Q, void* H, void* stream);
/* y[s][c][n] = sum_{p < P} h[s or 0][c][p] x[s][n - p],  0 <= n < out_len  (out_len = len: what OverlapAdd hands out,
 * convolution.cc:120-121; len + P - 1: the whole convolution):
 *   x [dev] float32: S row pointers x + s x_stride, each with `len` samples at 0 .. len - 1 and `hist` samples of the stream's
 *     past at -hist .. -1; samples before -hist and from len on are zero and that memory is never read (a second call whose
 *     hist covers P - 1 samples continues the stream of the first)
 *   H [dev] complex64 [S_h][C][Q][N/2+1] from btk_conv_filter_spectra, S_h = 1 (shared) or S
 *   y [dev] float32 [S][C] rows of out_len samples, y_stride apart
 * Tile j holds outputs j Lk ..; a span element no stored output depends on is read as zero, so calls that cut a row at multiples
 * of Lk give the bits of one call.  BTK_ERR_DIMENSION for a bad N, P, Bp, Q (as above), Lk + Bp - 1 > N, S_h not 1 or S,
 * negative lengths, out_len < 1 or strides shorter than the rows; BTK_ERR_PARAMETER for null pointers; nothing is launched.   */
int  btk_conv_apply(const float* x, long len, long hist, long x_stride, int S, const void* H, int S_h, int C, int P, int N, int Lk,
                    int Bp, int Q, float* y, long out_len, long y_stride, void* stream);
/* OverlapSave::next (convolution.cc:196-230) for T stand-alone blocks of L samples, block t at samples t block_step .. of each
 * row (zero from len on): an L-point circular convolution with H [S_h][C][1][L/2+1] (Q = 1, Bp = P, N = L) of which samples
 * P .. L - 1 are kept (:225-226; index P - 1 is dropped as there):  y [dev] float32 [S][C][T][L - P],
 *   y[..][t][j] = sum_{p < P} h[p] x[t block_step + j + P - p].
 * BTK_ERR_DIMENSION for L no power of two in 256 .. 16384, P < 1, P >= L (:180-181), S_h not 1 or S, T < 1, block_step < 1.   */
int  btk_conv_blocks(const float* x, long len, long x_stride, int S, long T, long block_step, const void* H, int S_h, int C, int P,
                     int L, float* y, void* stream);

/* ---- Single-channel enhancement: spectral subtraction, Wiener filter, spectral high-pass (csrc/ss_kernels.hip) ----------------
 * Replace SpectralSubtractor::next with AveragePSDEstimator::add_sample / average / clear / clear_samples
 * (postfilter/spectralsubtraction.cc:216-285, :89-119, :70-87, :57-68, :121-129), WienerFilter::next (:314-362) and
 * HighPassFilter::next (postfilter/postfilter.cc:1215-1239) over a block of T frames.
 * Layouts [dev]: complex64, bins 0 .. M/2 (K = M/2 + 1), T valid frames in rows T_stride apart.  X [S][K][C][T_stride] (the
 * snapshot layout with C = number of channels set), Sx, Nx, Y [S][K][T_stride]; bins above M/2 are the caller's mirror
 * Y[M-m] = conj(Y[m]).  Memory between T and T_stride is neither read nor written.
 * flags [dev] uint8 [T], shared by all streams: the mode of each frame, so that a block computed in one launch follows mode
 * switches between two next() calls (or a VAD label).  NULL: every frame has `mode`.
 *
 * btk_ss_process: per (s, k, t) the channels c = 0 .. C-1 in order, p = |X|^2:
 *   BTK_SS_TRAIN, alpha[c] >= 0 (recursive): the first training frame the channel sees since clear() sets est = p, later ones
 *     est = alpha est + (1 - alpha) p -- BEFORE the frame is subtracted (add_sample precedes estimate(), :227-235)
 *   BTK_SS_TRAIN, alpha[c] < 0 (averaging): acc += p (per bin); est moves in btk_ss_finish_training only
 *   BTK_SS_SUBTRACT: term = X sqrt(S2)/|X|, S2 = max(p - ft est, flooringV) (:267-271; (sqrt(S2), 0) where X = 0, the polar form
 *     with gsl_complex_arg(0) = 0); otherwise term = X
 *   Y = (sum_c term)/C
 *   State [dev], caller-owned, continued bit for bit from block to block: est, acc float64 [S][C][K]; count int64 [S][C]
 *   (training frames summed into acc; averaging channels only); added uint8 [S][C] (sample_added_; recursive channels only).
 *   alpha [host] float64 [C]; alpha, ft and flooringV are rounded to float32, which is what the reference's members hold.
 *   frames_done = frames this node produced before the block: the 64-frame scan chunks of the
 *   recursion sit on multiples of 64 of that counter, so blocks cut at such multiples give the bits of one launch.
 *   Arithmetic: |X|^2, the scan inside a chunk and the subtraction are float32; the carry from chunk to chunk, the state and
 *   the averaging sum (products and sum) are float64.
 *   form: BTK_SS_FORM_AUTO picks the frame-parallel kernel (rows cut along T across workgroups) when no frame can train
 *   (flags == NULL and mode without BTK_SS_TRAIN) and the one-wavefront-per-row scan kernel otherwise; BTK_SS_FORM_ROWS forces
 *   the latter (same bits).
 * btk_ss_finish_training = average() (:70-87): est = acc (1.0/(float)count) on averaging channels (count = 0: 0 x inf = NaN, as there).
 * btk_ss_clear: what = 0 clear_noise_samples() (acc = 0, count = 0), what = 1 clear() (added = 0 as well); est stays in both.
 * btk_wiener_process: bin 0 of Y is Sx's and its state is never touched; for k >= 1
 *     PSDs = a PSDs + (1 - a)|S|^2;  BTK_WIENER_UPDATE_NOISE: PSDn = a PSDn + (1 - a) max(|N|^2, flooringV), else PSDn stays
 *     H = PSDs/(PSDs + beta PSDn),  Y = H S      (0/0 stays NaN)
 *   a = 0 for the stream's first two frames (frame_no_ > 0 is tested before the increment, :323-326), alpha afterwards;
 *   frames_done as above.  State [dev] psd_s, psd_n float64 [S][K] (row 0 unused).  Nx may be NULL when flags == NULL and mode
 *   has no BTK_WIENER_UPDATE_NOISE.
 * btk_spec_highpass: bins 0 .. cutoff-1 of Y are zero (the reference never writes bin 0, so DC goes too), bins cutoff .. M/2 are
 *   X's.  cutoff = (unsigned)(M cutOffFreq/(float)sampleRate) is the caller's; cutoff = 0, with which the reference writes
 *   vector_[M] out of range, copies all K bins here.  X == Y is allowed.
 * Limits: M even, 2 <= M <= 2048, 1 <= C <= btk_ss_max_channels() (64), 1 <= S <= 65535 (a grid dimension), 0 <= T <= T_stride, 0 <= cutoff <= M/2 + 1;
 * BTK_ERR_DIMENSION beyond them, BTK_ERR_PARAMETER for a null pointer, an unknown mode bit, form or what; nothing is launched.   */
#define BTK_SS_TRAIN 1
#define BTK_SS_SUBTRACT 2
#define BTK_WIENER_UPDATE_NOISE 1
#define BTK_SS_FORM_AUTO 0
#define BTK_SS_FORM_ROWS 1
int  btk_ss_max_channels(void);
int  btk_ss_process(const void* X, void* Y, int S, int M, int C, long T_stride, long T, const unsigned char* flags, int mode,
                    double ft, double flooringV, const double* alpha, long frames_done, double* est, double* acc,
                    long long* count, unsigned char* added, int form, void* stream);
int  btk_ss_finish_training(int S, int M, int C, const double* alpha, double* est, const double* acc, const long long* count,
                            void* stream);
int  btk_ss_clear(int S, int M, int C, int what, double* acc, long long* count, unsigned char* added, void* stream);
int  btk_wiener_process(const void* Sx, const void* Nx, void* Y, int S, int M, long T_stride, long T, const unsigned char* flags,
                        int mode, double alpha, double flooringV, double beta, long frames_done, double* psd_s, double* psd_n,
                        void* stream);
int  btk_spec_highpass(const void* X, void* Y, int S, int M, int cutoff, long T_stride, long T, void* stream);

/* ---- Cosine-modulated perfect-reconstruction (PR) banks and the windowed FFT bank (csrc/fb_pr_kernels.hip) --------------------
 * Replace PerfectReconstructionFFTAnalysisBank::next, PerfectReconstructionFFTSynthesisBank::next and NormalFFTAnalysisBank::next
 * (modulated/modulated.cc:683-718, :861-898, :203-227) and get_window (:47-72).  M2 = 2 M, R = 2^r, D = M / R, q = r + 2:
 *   analysis  frame t, newest sample n_t = (t + 1) D - 1:  p[i] = sum_{k<m} (-1)^k h[i + M2 k] x[n_t - q k D - i],
 *             X_t[kappa] = 1/M2 sum_i p[i] e^{-j pi i/M2} e^{+j 2 pi kappa i/M2}, all M2 bins; ceil(nsamples / D) + 2 m - 1 frames
 *   synthesis block b, newest frame f = b + 2 m - 1:  v_f[i] = Re(e^{+j pi i/M2} sum_kappa Y_f[kappa] e^{-j 2 pi kappa i/M2}),
 *             s_b[i] = sum_{k<m} (-1)^{k+m-1} h[i + M2 (m-1-k)] v_{f - q k}[i],  out_b[D-1-d] = sum_{sx<2R} s_{b-(2R-1-sx)}[d + sx D] / R
 *             (float32 running sum in this order); frames and blocks before 0 count as zero; nframes - (2 m - 1) blocks
 *   STFT      X_t[kappa] = sum_{i<M} win[i] x[n_t - M + 1 + i] e^{-j 2 pi kappa i/M}, all M bins; ceil(nsamples / D) + 1 frames
 * Layouts [dev]: pcm float32 [S*N][pcm_stride]; X complex64 [S][M2][N][T_stride] (STFT: [S][M][N][T_stride]), the snapshot
 * layout with K = M2; Y complex64 [S][M2][T_stride]; out float32 [S][out_stride].  A launch covers frames [t0, t0 + tcount) or
 * blocks [b0, b0 + bcount), written from column 0 / sample 0 of the output; any split gives the bits of one launch.
 * prototype [host] float64 [prototype_len]: BTK_ERR_CONSISTENCY unless prototype_len == 2 M m.
 * Limits: PR banks M a power of two in 8 .. 1024 (M2 = 16 .. 2048), 1 <= m <= 64 (m <= 8 compiled in, above that a run-time
 * loop), r <= 2; STFT M a power of two in 8 .. 2048, M >> r >= 1: BTK_ERR_PARAMETER otherwise.  A launch whose tile does not
 * fit 160 KB of LDS (M2 = 2048 with a long prototype) is refused with BTK_ERR_PARAMETER, bad sizes with BTK_ERR_DIMENSION;
 * nothing is launched and the outputs stay untouched.
 * btk_get_window [host]: type 0 rectangular, 2 Hann 0.5 (1 - cos(2 pi i/(len-1))), anything else Hamming 0.54 - 0.46 cos(...).  */
typedef struct btk_prfb btk_prfb_t;
typedef struct btk_stft btk_stft_t;
int  btk_get_window(int type, int len, double* out);
int  btk_prfb_create(btk_prfb_t** fb, int M, int m, int r, int synthesis, const double* prototype, long prototype_len);
void btk_prfb_destroy(btk_prfb_t* fb);
int  btk_prfb_processing_delay(const btk_prfb_t* fb);
long btk_prfb_num_frames(const btk_prfb_t* fb, long nsamples);
long btk_prfb_num_blocks(const btk_prfb_t* fb, long nframes);
int  btk_prfb_analysis(const btk_prfb_t* fb, const float* pcm, long nsamples, long pcm_stride, int S, int N, void* X,
                       long T_stride, long t0, long tcount, void* stream);
int  btk_prfb_synthesis(const btk_prfb_t* fb, const void* Y, long nframes, long T_stride, int S, float* out, long out_stride,
                        long b0, long bcount, void* stream);
int  btk_stft_create(btk_stft_t** fb, int M, int r, int window_type);
void btk_stft_destroy(btk_stft_t* fb);
long btk_stft_num_frames(const btk_stft_t* fb, long nsamples);
int  btk_stft_analysis(const btk_stft_t* fb, const float* pcm, long nsamples, long pcm_stride, int S, int N, void* X,
                       long T_stride, long t0, long tcount, void* stream);

/* ---- Binaural binary-mask filters and threshold estimators (csrc/binaural_kernels.hip) -----------------------------------------
 * Replace KimBinaryMaskFilter::masking1 / IIDBinaryMaskFilter::masking1 (postfilter/binauralprocessing.cc:138-179, :441-485, with
 * calcITDf :17-38), the accumStats1 of KimITDThresholdEstimator, IIDThresholdEstimator and FDIIDThresholdEstimator (:314-353,
 * :548-603, :794-838), their candidate walk and their calc_threshold (:382-407, :632-660, :867-898).
 * Layouts [dev]: XL, XR, Y complex64 [S][K][T_stride], K = M/2 + 1, T valid frames per row; memory between T and T_stride is
 * neither read nor written.  Bins above M/2 are the caller's mirror.
 *
 * btk_binaural_mask: bin 0 of Y is XL's whatever chanX is.  For k >= 1, X = chanX ? XR : XL and
 *     mu_t = alpha mu_{t-1} + (1 - alpha) b_t,   Y_t = mu_t X_t,   b_t in {1, eta}
 *   BTK_BINAURAL_KIM: ITD = min(|d|, |d - 2 pi|, |d + 2 pi|) / (2 pi k / M), d = arg XL - arg XR (arg 0 = 0);
 *     b_t = 1 where (ITD <= threshold) == (chanX == 0).  `thresholds` is ignored, as in the reference.
 *   BTK_BINAURAL_IID: X_T = X, X_I the other input; b_t = eta where |X_T| <= |X_I| + thr, thr = thresholds[k] (float32 [K] [dev])
 *     if given, else threshold.
 *   threshold, alpha, eta are rounded to float32 (the reference's members); (1 - alpha) and (1 - alpha) eta are float32.
 *   prev_mu [dev] float32 [S][K]: prevMu_, the caller initialises it to 1; row 0 is never touched.  Phases, magnitudes and the
 *   comparisons are float64; the recursion is a float32 scan in 64-frame chunks on multiples of 64 of frames_done (frames the
 *   node produced before the block) with the float32 mask carried from chunk to chunk: blocks cut at such multiples give the
 *   bits of one launch.
 * btk_binaural_stats adds T frames to state [dev] float64 and T to count [dev] int64 [S].  cands [dev] float32 [nWalk]: the
 *   candidates; state has nCand >= nWalk slots per stream (see btk_binaural_candidates), those beyond nWalk are not touched.
 *   XL is the target's stream, XR the interferer's (chanX = 0 of the estimators).
 *   KIM   state [S][nCand][5]: sum over frames of R_T R_I, R_T, R_I, R_T^2, R_I^2 with R = (sum_{k in [fbin_min, fbin_max)}
 *         |mu X_k|^2)^power_coeff, (mu_T, mu_I) = (1, eta) where ITD_k <= cand, else (eta, 1).  Bin 0 has ITD x/0: never <=.
 *   IID   state [S][nCand][6]: Y1_T, Y2_T, Y4_T, Y1_I, Y2_I, Y4_I, sums over frames and bins of y, y^2, y^4 with
 *         y = |mu X_k|^(2 power_coeff), mu_T = eta where |XL| <= |XR| + cand, mu_I = eta where |XR| <= |XL| + cand, else 1.
 *   FDIID state [S][K][nCand][3]: Y4, mean, sigma = sums over frames of y_T^4 + y_I^4, y_T + y_I, y_T^2 + y_I^2 per bin 1 .. M/2
 *         (row 0 untouched; fbin_min / fbin_max are ignored).
 *   per_frame [dev] float64 or NULL: KIM [S][T][nCand][2] = R_T, R_I; IID [S][T][nCand][6] = the frame's six sums (FDIID: must be
 *   NULL).  scratch [dev]: btk_binaural_stats_scratch_bytes(kind, S, T, nCand) bytes (0 for FDIID), per-chunk partial sums that
 *   a second launch adds up in chunk order.  No floating-point atomics: same inputs and same block cuts, same bits.
 *   eta and power_coeff are rounded to float32 (the reference's members), everything else is float64.
 * btk_binaural_candidates [host]: the walk `for (float t = min; t <= max; t += width)` into out (at most cap values; out may be
 *   NULL), its length in *nWalk, and *nCand = (int)((max - min)/width + 1.5) (float32 quotient), the size of the reference's
 *   arrays.  The two can differ ((0, 2, 0.1): 20 and 21).  A walk longer than nCand, which in the reference writes past its
 *   arrays, is cut at nCand.
 * btk_binaural_threshold [host]: calc_threshold on downloaded sums of ONE stream (state as above without [S]), count frames.
 *   KIM minimises |rho|, the correlation coefficient of R_T and R_I, first minimum wins; cost[nCand] = E[R_T R_I] (what
 *   cost_function() returns there).  IID maximises cost = E[Y4_T] + E[Y4_I] - beta (E[Y2_T] + E[Y2_I])^2 (sums over bins), first
 *   maximum wins.  FDIID: cost [K][nCand] = E[Y4] - beta E[sigma]^2 per bin; thresholds [K] the per-bin maximiser and *threshold
 *   the maximiser over all bins, LAST maximum wins (<=) in both; thresholds[0] = 0.  Slots beyond nWalk have cost 0 and are not
 *   candidates.  Nothing is modified: calling it again gives the same answer (the reference divides its sums in place).
 * Limits: M even, 2 <= M <= 2048, 1 <= S <= 65535, 0 <= T <= T_stride, 1 <= nCand <= btk_binaural_max_candidates() (4096),
 * 0 <= fbin_min <= fbin_max <= M/2 + 1: BTK_ERR_DIMENSION beyond them; BTK_ERR_PARAMETER for a null pointer, an unknown kind or
 * chanX, a short scratch; nothing is launched and the state stays untouched.   */
#define BTK_BINAURAL_KIM 0
#define BTK_BINAURAL_IID 1
#define BTK_BINAURAL_FDIID 2
int  btk_binaural_max_candidates(void);
int  btk_binaural_mask(const void* XL, const void* XR, void* Y, int S, int M, long T_stride, long T, int kind, int chanX,
                       double threshold, const float* thresholds, double alpha, double eta, long frames_done, float* prev_mu,
                       void* stream);
long btk_binaural_stats_scratch_bytes(int kind, int S, long T, int nCand);
int  btk_binaural_stats(const void* XL, const void* XR, int S, int M, long T_stride, long T, int kind, const float* cands,
                        int nWalk, int nCand, double eta, double power_coeff, int fbin_min, int fbin_max, double* state,
                        long long* count, double* per_frame, void* scratch, long scratch_bytes, void* stream);
int  btk_binaural_candidates(double min, double max, double width, float* out, int cap, int* nWalk, int* nCand);
int  btk_binaural_threshold(int kind, int M, int nCand, int nWalk, const float* cands, const double* state, long long count,
                            double beta, double* threshold, double* cost, double* thresholds);

/* ---- Voice activity detection: the energy family of sad/sad.cc ----------------------------------------------------------
 * Every sum is float64 over float32 inputs in the reference's order, every comparison strict as there: energies, band powers,
 * power / normalised-energy scores, every value and every frame number are the reference's bits (the TSPS score up to the
 * device's float64 log).  A block cut anywhere continues from the state and gives the bits of one launch.
 *
 * btk_vad_frame_energy: energy[s][t] = sum_{n < D} |x[s][t][n]|^2 in index order (EnergyVADMetric::above_threshold_, :520-524;
 *   is_complex: complex64 elements, re^2 + im^2 each, SimpleEnergyVAD::next :165-167).  Element n of frame t of stream s lies at
 *   x + s stream_stride + t frame_stride + n elem_stride (in elements), so the producers' blocks are read as they lie: snapshot
 *   rows complex64 [S][K][T_stride] (frame_stride 1, elem_stride T_stride), feature rows float32 [S][T][D] (D, 1), PCM (shift, 1).
 *   energy [dev] float64 [S][e_stride].  Frame-minor rows may not overlap: T frame_stride <= elem_stride.
 * btk_vad_band_limits [host]: lowX, highX, binN of MultiChannelVADMetric (:629-663): a negative cutoff means 0 / fftLen/2; the
 *   low edge truncates, the high edge adds 0.5; a cutoff >= samplerate / 2 is BTK_ERR_DIMENSION.
 * btk_vad_band_power: spec float32 power spectra, bin k of frame t of channel c of stream s at s stream_stride + c chan_stride +
 *   t frame_stride + k bin_stride.  P[s][c][t] = (sum_{k = lowX .. highX} w_k spec[k]) / M, w_k = 1 for k == 0 or k == M/2 + 1,
 *   else 2 (the reference tests fftLen2_ + 1, so the Nyquist bin is doubled; kept).  P [dev] float64 [S][C][o_stride] or NULL;
 *   score, value [dev] float64 [S][o_stride] (score may be NULL); value = +1 / -1:
 *     BTK_VAD_POWER       score = P_0 / sum_c P_c,                       value = score > E0 / C   (:731-736)
 *     BTK_VAD_NORMALIZED  score = sqrt(P_0) / sum_c sqrt(P_c),           value = score > E0 / C   (:815-827)
 *     BTK_VAD_TSPS        score = log(P_0 / (sum P - P_0)) - log(E0 / sum P), value = score > 0   (:1044-1054)
 * btk_vad_energy_metric: EnergyVADMetric::next (:518-588) over energy [dev] float64 [S][e_stride]: value [dev] float64
 *   [S][v_stride] = 1.0 where energy > sorted window[medianX], evaluated as #{window < energy} > medianX (a NaN energy, on which
 *   the reference's qsort is undefined, is thereby never above and never below), else 0.0; the window takes the energy only while
 *   recognizing == false && abovethresholdN == 0; then the head/tail counters move.  state [dev], per stream
 *   btk_vad_energy_metric_state_bytes(energiesN) = 8 (4 + energiesN) bytes: int64 {ring position, recognizing, abovethresholdN,
 *   belowThresholdN}, then the float64 window as a ring whose oldest entry is at the ring position.  The caller initialises it:
 *   zeros and initialEnergy; a ring position outside 0 .. energiesN - 1 is the caller's error and is not checked on the device.  medianX = unsigned(threshold energiesN) must be < energiesN.
 * btk_vad_simple_energy: SimpleEnergyVAD::next (:165-171) over energy rows: s <- gamma s + (1 - gamma) E (two rounded products,
 *   one rounded sum), is_speech [dev] int32 [S][o_stride] = E / s > threshold, smoothed [dev] float64 [S][o_stride] or NULL = s;
 *   state [dev] float64 [S] = s (spectral_energy_, 0 at the start and after next_speaker()).
 * btk_vad_hangover: the detection rule and the head/tail machine of HangoverVADFeature::next (:1763-1843) on R <= 8 rows of metric
 *   values, values [host] R pointers to [dev] float64 [S][v_stride], thresholds [host] float64 [R]:
 *     BTK_VAD_RULE_SINGLE      values[0] > thresholds[0]                                   (:1763-1771)
 *     BTK_VAD_RULE_MI          R == 3, HangoverMIVADFeature::above_threshold_ (:1859-1885), codes -1, 2, 3, -3
 *     BTK_VAD_RULE_MULTISTAGE  :1910-1951: never with R < 3; values[0] < 0.5 vetoes (code -1); else the first m >= 1 with
 *                              values[m] > 0.5 wins (code m + 1); else code -R
 *   decision [dev] int32 [S][d_stride] or NULL: decision_metric() after each frame (a rule that assigns none leaves the state's).
 *   state [dev] int64 [S][8]: {abovethresholdN, belowThresholdN, recognizing, frames seen, start, end, ended, decision_metric};
 *   the caller starts it as {0, 0, 0, 0, -1, -1, 0, 0}.  start = q - headN + 1 for the first frame q that ends headN consecutive
 *   detections (prefixN()); end = the frame on which the tailN-th consecutive miss falls (exclusive); frame numbers count from
 *   the state's frames seen.  After `ended` the machine rests (decisions are still written).  restart != 0: an end clears the
 *   counters and the machine goes on; every (start, end) completed in this call goes to segments [dev] int64 [S][max_seg][2] in
 *   order and their number to nseg [dev] int32 [S] (it may exceed max_seg: those beyond are not written); a segment still open
 *   stays in the state's start.  headN == 0 is BTK_ERR_DIMENSION.
 * btk_vad_gather: rows [start, end) of the state's segment (end < 0: still open) that lie in src [dev] float32 [S][T][D], whose
 *   row 0 is frame frame_base, to dst [dev] float32 [S][dst_rows][D] at row (frame - start); count [dev] int64 [S] or NULL: rows
 *   copied by this call.  Rows beyond dst_rows are not copied.
 * Limits: 1 <= S <= 65535, 0 <= T <= the row strides, 1 <= energiesN <= 1024, 1 <= C <= 64, 2 <= M <= 2048,
 * 0 <= lowX <= highX <= M/2, 1 <= D <= 65536: BTK_ERR_DIMENSION beyond them, BTK_ERR_PARAMETER for a null pointer or an unknown
 * kind or rule; nothing is launched and the state stays untouched.                                                            */
#define BTK_VAD_POWER 0
#define BTK_VAD_NORMALIZED 1
#define BTK_VAD_TSPS 2
#define BTK_VAD_RULE_SINGLE 0
#define BTK_VAD_RULE_MI 1
#define BTK_VAD_RULE_MULTISTAGE 2
int  btk_vad_frame_energy(const void* x, int is_complex, int S, int D, long T, long stream_stride, long frame_stride,
                          long elem_stride, double* energy, long e_stride, void* stream);
int  btk_vad_band_limits(int fftLen, double samplerate, double lowCutoff, double highCutoff, int* lowX, int* highX, int* binN);
int  btk_vad_band_power(const float* spec, int kind, int S, int C, int M, long T, long stream_stride, long chan_stride,
                        long frame_stride, long bin_stride, int lowX, int highX, double E0, double* P, double* score,
                        double* value, long o_stride, void* stream);
long btk_vad_energy_metric_state_bytes(int energiesN);
int  btk_vad_energy_metric(const double* energy, long e_stride, int S, long T, int energiesN, int medianX, unsigned headN,
                           unsigned tailN, void* state, double* value, long v_stride, void* stream);
int  btk_vad_simple_energy(const double* energy, long e_stride, int S, long T, double gamma, double threshold, double* state,
                           int* is_speech, double* smoothed, long o_stride, void* stream);
int  btk_vad_hangover(const double* const* values, const double* thresholds, int R, int rule, int S, long T, long v_stride,
                      unsigned headN, unsigned tailN, int restart, long long* state, int* decision, long d_stride,
                      long long* segments, int max_seg, int* nseg, void* stream);
int  btk_vad_gather(const float* src, int S, long T, int D, long frame_base, const long long* hangover_state, float* dst,
                    long dst_rows, long long* count, void* stream);

/* ---- Objective measures: objective_measure/objective_measure.cc -----------------------------------------------------------
 * Arithmetic rule: element-wise values (centred and scaled samples, differences, bin powers, ratios) are the reference's float32;
 * sums are float64 in an order fixed by the sample, bin or frame index alone: it depends neither on S, on a pair's place in the
 * batch, on the strides, nor on which optional outputs are asked for.  No floating-point atomics.
 *
 * btk_obj_snr: calcSNR (:42-185) for S pairs.  x1, x2 [dev] float32 [S][stride]; n1, n2 [host] long [S], 1 <= n_c <= stride_c (the distance: 0 <= n_c);
 *   nmin = min(n1, n2).  The inputs are not modified (the reference overwrites them).  option bits:
 *     1  mu_c = f32((sum_{i<n_c} x_c[i]) / n_c), x_c[i] <- f32(x_c[i] - mu_c)                       (else mu_c = 0)
 *   a1 = a2 = 1, then the first of
 *     2  a_c = f32(1 / max(-10000, max_i x_c[i])): the signed maximum with the reference's initial value, not the peak
 *     4  a2 = f32(sqrt((sum x1^2 / n1) / (sum x2^2 / n2)))
 *     8  a2 = f32(sum_{i<n2} x1 x2 / sum_{i<n2} x2^2); needs n1 >= n2 (the reference reads past samp1): BTK_ERR_DIMENSION
 *   v_c[i] = f32(x_c[i] a_c); sum = sum_{i<nmin} (double)v1^2, err = sum_{i<nmin} (double)f32(v1 - v2)^2, and the longer
 *   signal's tail adds its v^2 to both (:159-176).  stats [dev] float64 [S][6] = mu1, mu2, a1, a2, sum, err; btk_obj_snr_db [host]
 *   forms err > 0 ? 10 log10f(f32(sum / err)) : FLT_MAX of them, log10f correctly rounded (the float64 logarithm rounded once).
 *   seg [dev] float64 [S][seg_stride][2] or NULL: sum_b, err_b of the whole segments of seg_len samples below nmin,
 *   b < floor(nmin / seg_len) <= seg_stride (the rows behind a pair's last segment stay untouched).  The segmental SNR made of
 *   them is this project's (the reference's segmentalSNR class is empty).
 *   workspace [dev]: btk_obj_snr_workspace_bytes(S, max n) bytes, need not be initialised.
 * btk_obj_is_distance: calcISDistance (:284-331) for S pairs over the frames of a btk_stft plan, the bits btk_stft_analysis
 *   gives: F = min(btk_stft_num_frames(n1), btk_stft_num_frames(n2)); per frame and bin kappa = 1 .. M/2
 *     P_c = f32((double)re^2 + (double)im^2); P1 > 0 and P2 > 0: ratio = f32(P1 / P2), term = (double)ratio - log(ratio) - 1,
 *     else term = 0;  Eis_t = (sum_kappa term) / (M/2)  (skipped bins stay in the divisor)
 *   dist [dev] float64 [S] = mean of Eis_t over bframe <= t < F and t <= eframe unless eframe < 0, NaN where no frame is in
 *   range; count [dev] int64 [S] frames in range; eis [dev] float64 [S][e_stride], e_stride >= F: the rows t < F (always
 *   written: the mean is taken from them).  btk_obj_is_tile_frames: frames a workgroup transforms at this plan's M.
 * BTK_ERR_DIMENSION for a bad size or length, BTK_ERR_PARAMETER for a null pointer or unknown option bits; nothing is launched
 * and the outputs stay untouched.                                                                                            */
long btk_obj_snr_workspace_bytes(int S, long nmax);
int  btk_obj_snr(const float* x1, long stride1, const float* x2, long stride2, int S, const long* n1, const long* n2, int option,
                 double* stats, long seg_len, double* seg, long seg_stride, void* workspace, void* stream);
float btk_obj_snr_db(double sum, double err);
int  btk_obj_is_tile_frames(const btk_stft_t* fb);
int  btk_obj_is_distance(const btk_stft_t* fb, const float* x1, long stride1, const float* x2, long stride2, int S,
                         const long* n1, const long* n2, long bframe, long eframe, double* dist, long long* count, double* eis,
                         long e_stride, void* stream);

/* ---- Multichannel cross-correlation localisation: SearchGridBuilder / SGB4LinearArray / MCCLocalizer / MCCCalculator
 * (localization/mcc_localizer.h:36-78, :153-260; mcc_localizer.cc) -----------------------------------------------------------
 * Host helpers (no device needed), the reference's types as written:
 * btk_mcc_max_sample_delay: D = (size_t)(fs * maxTimeDelay), a float product (mcc_localizer.cc:273, :326).
 * btk_mcc_sample_delays: tau[c] = (int)(float)(fs * delays[c]), the double product rounded to float and truncated toward zero
 *   (:333-335); delays [host] float64 [n] seconds, tau_out [host] int32 [n].
 * btk_mcc_linear_grid: the far-field walk of SGB4LinearArray (:54-161): positions [host] float64 [N][3] in mm
 *   (setPositionsOfMicrophones; microphone 0 is copied and is pos0, which the reference's loop from 1 never does), or NULL and
 *   `distance` in mm (setDistanceBtwMicrophones).  The walk starts at azimuth 0, goes in steps of _constV in sin(azimuth) up to
 *   pi/2, jumps to 3 pi/2 and ends just below 2 pi.  n_points: the number of grid points; max_time_delay, const_v (may be NULL):
 *   _maxTimeDelay, _constV.  azimuths [host] float64 [max_points], delays [host] float64 [max_points][N]
 *   (calcDelaysOfLinearMicrophoneArray, localization.cc:107-118, 343740 mm/s), tau [host] int32 [max_points][N]: each may be
 *   NULL; all NULL counts only.  More points than max_points (or than 4096): BTK_ERR_DIMENSION.
 * Device entry points.  x [dev] float32 [S][N][len]: S streams of N channels, cut into B blocks of L samples from sample 0
 * (B L <= len).  tau_host [host] int32 [G][N] is checked (|tau| <= D) and copied to tau_dev [dev] int32 [G][N] on the stream.
 * btk_mcc_cost: calcCovarianceMatrix + calcObjectiveFunction (:322-411) of every (stream, block, candidate):
 *     R = (1 / nS) sum_{f < nS} xt[f] xt[f]^T in float64, nS = L - D, xt_c[f] = x_c[f + tau_c], or x_c[L + f + tau_c] where
 *     f + tau_c < 0 (SampleHolder holds the CURRENT block's last D samples, :336: no state crosses a block boundary)
 *     cost [dev] float64 [S][B][G] = sum log d_j - (normalize_variance ? sum log R_ii : 0), d_j the pivots of R = L diag(d) L^T
 *     flag [dev] uint8 [S][B][G] = 1 and cost = 0.0 where a pivot or an R_ii is not > 0 (the zero-eigenvalue branch, :386-397;
 *     the reference takes |lambda| of a negative eigenvalue instead, which an exact Gram matrix has from rounding only)
 *   The summation order depends on (N, L, D) alone: equal tau rows give equal bits, whatever else is in the launch.
 * btk_mcc_select: the N-best insertion of search() (:431-443) in grid order, strict <, every entry starts at cost 100000:
 *   cost [dev] float64 [SB][G] -> nbest_cost [dev] float64 [SB][nbest], nbest_idx [dev] int32 [SB][nbest] (-1 where nothing
 *   was inserted).  nbest = maxSource <= 16.
 * btk_mcc_matrices: R [dev] float64 [P][N][N] (both triangles) of the P pairs (s B + b, g) in pairs_host [host] int32 [P][2],
 *   copied to pairs_dev [dev] int32 [P][2]; the sums of btk_mcc_cost, bit for bit.
 * BTK_ERR_DIMENSION unless 2 <= N <= 64, 1 <= G <= 4096, 2 D <= L <= 65536 ("Data samples are insufficient", :329),
 * |tau| <= D (the reference would read outside its buffers), 1 <= nbest <= 16; nothing is launched then.                    */
long btk_mcc_max_sample_delay(unsigned int fs, float max_time_delay);
int  btk_mcc_sample_delays(unsigned int fs, int n, const double* delays, int* tau_out);
int  btk_mcc_linear_grid(unsigned int fs, int N, const double* positions, float distance, int max_points, int* n_points,
                         float* max_time_delay, float* const_v, double* azimuths, double* delays, int* tau);
int  btk_mcc_cost(const void* x, long len, int S, int N, int B, int L, int D, const int* tau_host, void* tau_dev, int G,
                  int normalize_variance, void* cost, void* flag, void* stream);
int  btk_mcc_select(const void* cost, long SB, int G, int nbest, void* nbest_cost, void* nbest_idx, void* stream);
int  btk_mcc_matrices(const void* x, long len, int S, int N, int B, int L, int D, const int* tau_host, void* tau_dev, int G,
                      const int* pairs_host, void* pairs_dev, int P, void* R, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BTKHIP_H */
