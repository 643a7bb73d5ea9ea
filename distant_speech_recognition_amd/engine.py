"""Block-level Python front-end of the C-ABI (include/btkhip.h).

PyTorch is used only for device memory and streams (tensor.data_ptr()); every computation is a
hand-written HIP kernel in csrc/.  Tensor layouts:

    pcm  float32   [S][N][L]       X  complex64 [S][K][N][T]
    W    complex64 [S|1][K][N]     Y  complex64 [S][K][T]      out float32 [S][B*D]
"""
import collections
import ctypes as C
import os
import sys

import numpy as np
import torch

from . import _lib
from ._lib import check


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(t, name):
    if not t.is_cuda:
        raise ValueError("%s must live in HBM (cuda tensor); the engine has no CPU path" % name)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)


def _check(t, name, dtype, shape, rows=False):
    """The C-ABI sees raw pointers: dtype, residency, contiguity and shape are checked here.  shape: an int (number of
    dimensions) or a tuple whose None entries are free.  rows=True admits a [..., :T] view of a buffer with padded rows
    (padded_rows) and returns the row stride in elements, for the entry points whose T_stride the caller may choose."""
    if rows:
        ts = _row_stride(t, name)
    else:
        _need_cuda(t, name)
        ts = t.shape[-1] if t.dim() else 0
    if t.dtype != dtype:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s must be %s, got %s" % (name, dtype, t.dtype))
    if isinstance(shape, int):
        ok = t.dim() == shape
    else:
        ok = t.dim() == len(shape) and all(e is None or int(e) == int(g) for e, g in zip(shape, t.shape))
    if not ok:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s has shape %s, expected %s" % (name, tuple(t.shape), shape))
    return ts


def rows_like(X, shape, dtype=torch.complex64):
    """Tensor of `shape` [..., T] whose rows are spaced like the rows of X (the C-ABI's per-frame outputs share the snapshots'
    T_stride): contiguous for contiguous X, a [..., :T] view of a padded buffer for row-padded X."""
    ts = X.stride(-2) if X.dim() >= 2 else X.shape[-1]
    T = shape[-1]
    if ts == T:
        return torch.empty(shape, dtype=dtype, device=X.device)
    return torch.empty(tuple(shape[:-1]) + (ts,), dtype=dtype, device=X.device)[..., :T]


def _row_stride(t, name):
    """Row stride (in elements) of a cuda tensor [..., rows, T] whose rows are contiguous and evenly spaced -- a contiguous
    tensor or a [..., :T] view of a buffer with padded rows (the C-ABI takes T_stride >= T everywhere)."""
    if not t.is_cuda:
        raise ValueError("%s must live in HBM (cuda tensor); the engine has no CPU path" % name)
    if t.numel() == 0:                          # an empty bin shard: nothing is read or written, any stride will do
        return max(int(t.shape[-1]), 1) if t.dim() else 1
    if t.dim() < 2 or t.stride(-1) != 1 or t.stride(-2) < t.shape[-1]:
        raise ValueError("%s: rows must be contiguous" % name)
    for i in range(t.dim() - 3, -1, -1):
        if t.shape[i] > 1 and t.stride(i) != t.shape[i + 1] * t.stride(i + 1):
            raise ValueError("%s: rows must be evenly spaced" % name)
    return t.stride(-2)


def padded_rows(shape, dtype, device, row_bytes_quantum=4096, pad=48):
    """Tensor of `shape` whose last-axis rows are `pad` elements apart from being contiguous whenever a contiguous row
    would be a multiple of 4 KiB: power-of-two row strides put the 257 bin rows of a tile on the same HBM channels
    (profiles/pad_ab.py: fused kernel 1.78 -> 1.67 ms, apply 1.66 -> 1.40 ms with 16-48 frames of padding)."""
    T = shape[-1]
    esz = torch.empty((), dtype=dtype).element_size()
    if T == 0 or (T * esz) % row_bytes_quantum:
        return torch.empty(shape, dtype=dtype, device=device)
    buf = torch.empty(tuple(shape[:-1]) + (T + pad,), dtype=dtype, device=device)
    return buf[..., :T]


class FilterBank:
    """Plan of an oversampled modulated-DFT bank (OverSampledDFTFilterBank, modulated.cc:232-268)."""

    def __init__(self, prototype, M, m, r, delay_compensation_type=0, synthesis=False):
        proto = np.ascontiguousarray(prototype, np.float64)
        if proto.shape != (m * M,):
            raise _lib.BtkError(_lib.BTK_ERR_CONSISTENCY,
                                "Prototype sizes do not match (%d vs. %d)." % (proto.size, m * M))
        self.M, self.m, self.r = M, m, r
        self.R = 1 << r
        self.D = M // self.R
        self.K = M // 2 + 1
        self.synthesis = bool(synthesis)
        self._h = C.c_void_p()
        check(_lib.lib().btk_fb_create(C.byref(self._h), M, m, r, delay_compensation_type, int(synthesis), _np_ptr(proto)))
        self.processing_delay = _lib.lib().btk_fb_processing_delay(self._h)
        self.lookahead = _lib.lib().btk_fb_lookahead(self._h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().btk_fb_destroy(h)
            except Exception:
                pass
            self._h = None

    # ---- analysis
    def num_frames(self, nsamples):
        return _lib.lib().btk_fb_analysis_num_frames(self._h, nsamples)

    def analysis(self, pcm, nsamples=None, t0=0, tcount=None, out=None, bins=None, pad_rows=False):
        """pcm float32 [S][N][L] (cuda) -> X complex64 [S][K][N][T]; bins = (k0, k1): only that bin range is computed
        into X [S][k1-k0][N][T] (the bin shard of one rank, sharding.py).  pad_rows: allocate X with padded rows
        (padded_rows: power-of-two row pitches put a tile's rows on the same HBM channels) -- bf_apply and nlms_process
        accept such a view, the other consumers want contiguous snapshots; `out` may itself be a row-padded view.
        pcm may be int16 -- the samples as a WAV stores them (feature/feature.cc:265-269) -- where the geometry has the int16 form of
        the bank (analysis_i16(): btk_fb_analysis_i16, M = 512; the whole bin range): half the PCM bytes, the same bits out."""
        i16 = pcm.dtype == torch.int16
        _check(pcm, "pcm", torch.int16 if i16 else torch.float32, 3)
        if i16 and (bins is not None or not self.analysis_i16()):
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "no int16 analysis kernel for M=%d m=%d r=%d%s: widen with pcm_i16_to_f32 first"
                                % (self.M, self.m, self.r, " on a bin range" if bins is not None else ""))
        S, N, L = pcm.shape
        nsamples = L if nsamples is None else nsamples
        if tcount is None:
            tcount = self.num_frames(nsamples) - t0
        k0, k1 = (0, self.K) if bins is None else (int(bins[0]), int(bins[1]))
        if not (0 <= k0 <= k1 <= self.K):
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "bin range [%d, %d) outside [0, %d]" % (k0, k1, self.K))
        if out is None:
            out = (padded_rows((S, k1 - k0, N, tcount), torch.complex64, pcm.device) if pad_rows
                   else torch.empty((S, k1 - k0, N, tcount), dtype=torch.complex64, device=pcm.device))
        ts = _check(out, "X", torch.complex64, (S, k1 - k0, N, None), rows=True)
        if out.shape[3] < tcount:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "X holds %d frames, %d requested" % (out.shape[3], tcount))
        if i16:
            check(_lib.lib().btk_fb_analysis_i16(self._h, _ptr(pcm), nsamples, L, S, N, _ptr(out), ts, t0, tcount, _stream()))
        elif bins is None:
            check(_lib.lib().btk_fb_analysis(self._h, _ptr(pcm), nsamples, L, S, N, _ptr(out), ts, t0, tcount, _stream()))
        else:
            check(_lib.lib().btk_fb_analysis_bins(self._h, _ptr(pcm), nsamples, L, S, N, _ptr(out), ts, t0, tcount,
                                                  k0, k1, _stream()))
        return out

    def analysis_polyphase(self, pcm, nsamples=None, t0=0, tcount=None):
        """Polyphase sums before the FFT: float32 [S*N][T][M] (parity/debug entry)."""
        _need_cuda(pcm, "pcm")
        S, N, L = pcm.shape
        nsamples = L if nsamples is None else nsamples
        if tcount is None:
            tcount = self.num_frames(nsamples) - t0
        P = torch.empty((S * N, tcount, self.M), dtype=torch.float32, device=pcm.device)
        check(_lib.lib().btk_fb_analysis_polyphase(self._h, _ptr(pcm), nsamples, L, S, N, _ptr(P), t0, tcount, _stream()))
        return P

    def analysis_beamform(self, pcm, W, nsamples=None, t0=0, tcount=None, out=None):
        """Fused analysis -> fixed-weight beamformer: pcm [S][N][L], W complex64 [S|1][K][N] -> Y [S][K][T]
        (the N x K snapshots are not written to HBM).  pcm float32, or int16 -- the samples as a WAV stores them
        (feature/feature.cc:265-269): widened inside the kernel, half the bytes, the same bits out (btk_fb_analysis_bf_i16;
        geometries with an int16 kernel: fused_i16())."""
        i16 = pcm.dtype == torch.int16
        _check(pcm, "pcm", torch.int16 if i16 else torch.float32, 3)
        if i16 and not self.fused_i16():
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "no int16 fused kernel for M=%d m=%d r=%d: widen with pcm_i16_to_f32 first" % (self.M, self.m, self.r))
        S, N, L = pcm.shape
        nsamples = L if nsamples is None else nsamples
        if tcount is None:
            tcount = self.num_frames(nsamples) - t0
        if W.dim() == 2:
            W = W.unsqueeze(0)
        _check(W, "W", torch.complex64, (None, self.K, N))
        if W.shape[0] not in (1, S):
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "weights %s do not match pcm %s" % (tuple(W.shape), tuple(pcm.shape)))
        per_stream = int(W.shape[0] == S and S > 1)
        if out is None:
            # (the staged fall-back of the other geometries needs contiguous rows; the library says which it runs)
            fused = _lib.lib().btk_fb_analysis_bf_fused(self._h) == 1
            out = (padded_rows((S, self.K, tcount), torch.complex64, pcm.device) if fused
                   else torch.empty((S, self.K, tcount), dtype=torch.complex64, device=pcm.device))
        t_stride = _row_stride(out, "Y")          # out may be a [..., :T] view of a row-padded buffer
        if out.dtype != torch.complex64 or tuple(out.shape[:2]) != (S, self.K) or out.shape[2] < tcount:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "Y must be complex64 [%d][%d][>=%d], got %s %s"
                                % (S, self.K, tcount, out.dtype, tuple(out.shape)))
        if tcount == 0:                           # a recording that ends inside the look-ahead: no frames, nothing to launch
            return out
        nb = _lib.lib().btk_fb_analysis_bf_scratch_bytes(self._h, S, N, per_stream, tcount)
        # the weight-pair scratch is written by a kernel of THIS launch's stream: one buffer per (device, stream), so that a plan
        # shared by several streams (serving.BatchBeamformerPipeline next to a caller's own stream) never has two launches
        # re-packing weights into the same bytes
        # The buffers come from torch's stream-aware caching allocator and are RETURNED to it when evicted: it re-issues a block only
        # to the stream that allocated it, so a recycled raw stream handle cannot be handed bytes another stream is still writing.
        # At most eight (device, stream) pairs are kept, least recently used first out: transient torch.cuda.Stream objects do not
        # pile up one buffer each.
        key = (pcm.device.index, int(torch.cuda.current_stream().cuda_stream))
        cache = self.__dict__.setdefault("_bf_scratch", collections.OrderedDict())
        buf = cache.pop(key, None)
        if buf is None or buf.numel() < nb:
            buf = torch.empty(nb, dtype=torch.uint8, device=pcm.device)
        cache[key] = buf
        while len(cache) > 8:
            cache.popitem(last=False)
        fn = _lib.lib().btk_fb_analysis_bf_i16 if i16 else _lib.lib().btk_fb_analysis_bf
        check(fn(self._h, _ptr(pcm), nsamples, L, S, N, _ptr(W), per_stream, _ptr(out), t_stride, t0, tcount, _ptr(buf), buf.numel(), _stream()))
        return out

    def analysis_i16(self):
        """True when analysis() takes int16 samples for this geometry (btk_fb_analysis_i16_direct)."""
        return _lib.lib().btk_fb_analysis_i16_direct(self._h) == 1

    def fused_i16(self):
        """True when analysis_beamform takes int16 samples for this geometry (btk_fb_analysis_bf_i16_fused)."""
        return _lib.lib().btk_fb_analysis_bf_i16_fused(self._h) == 1

    # ---- synthesis
    def num_blocks(self, nframes):
        return _lib.lib().btk_fb_synthesis_num_blocks(self._h, nframes)

    def synthesize(self, Y, nframes=None, b0=0, bcount=None, out=None):
        """Y complex64 [S][K][T] (cuda) -> float32 [S][bcount*D]."""
        t_stride = _row_stride(Y, "Y")            # Y may be a [..., :T] view of a row-padded buffer
        S, K, T = Y.shape
        if K != self.K:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "Y has %d bins, plan has %d" % (K, self.K))
        nframes = T if nframes is None else nframes
        if bcount is None:
            bcount = self.num_blocks(nframes) - b0
        if out is None:
            out = torch.empty((S, bcount * self.D), dtype=torch.float32, device=Y.device)
        check(_lib.lib().btk_fb_synthesis(self._h, _ptr(Y), nframes, t_stride, S, _ptr(out), out.shape[1], b0, bcount, _stream()))
        return out


def bf_apply(W, X, out=None):
    """y_k[t] = w_k^H x_k[t].  W complex64 [S|1][K][N], X complex64 [S][K][N][T] -> Y [S][K][T].  X may be a row-padded view
    (analysis(pad_rows=True)); Y then shares its row stride (the C-ABI has one T_stride for both)."""
    ts = _check(X, "X", torch.complex64, 4, rows=True)
    S, K, N, T = X.shape
    if W.dim() == 2:
        W = W.unsqueeze(0)
    _check(W, "W", torch.complex64, 3)
    if W.shape[1:] != (K, N) or W.shape[0] not in (1, S):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "weights %s do not match X %s" % (tuple(W.shape), tuple(X.shape)))
    if out is None:
        out = rows_like(X, (S, K, T))
    if _check(out, "Y", torch.complex64, (S, K, T), rows=True) != ts and K * T:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "Y rows are %d frames apart, X rows %d: they share T_stride" % (out.stride(-2), ts))
    if K == 0 or T == 0:                       # the empty bin shard of a trailing rank: nothing to launch
        return out
    check(_lib.lib().btk_bf_apply(_ptr(W), int(W.shape[0] == S and S > 1), _ptr(X), _ptr(out), S, K, N, ts, T, _stream()))
    return out


def bf_apply_all_bins(Wfull, X):
    """half_band_shift == true (SubbandDS/GSC::next, beamformer.cc:1113-1128, 1276-1285): every one of the M bins has its
    own weight vector, y_k = w_k^H x_k for k = 0..M-1, where the snapshots of the bins above M/2 are the conjugate mirrors
    the analysis bank of a real signal produces, x_{M-k} = conj(x_k).  Wfull complex64 [M][N], X [S][K][N][T] ->
    Y complex64 [S][M][T]:  y_{M-k} = conj((conj w_{M-k})^H x_k), i.e. two passes of the same apply kernel."""
    _check(X, "X", torch.complex64, 4)
    S, K, N, T = X.shape
    M = 2 * (K - 1)
    _check(Wfull, "W", torch.complex64, (M, N))
    Y = torch.empty((S, M, T), dtype=torch.complex64, device=X.device)
    lo = bf_apply(Wfull[:K].contiguous(), X)
    Y[:, :K] = lo
    W2 = torch.zeros((K, N), dtype=torch.complex64, device=X.device)
    W2[1:K - 1] = torch.conj(Wfull[K:]).flip(0)              # row k' <- conj(w_{M-k'}), k' = 1 .. M/2-1
    up = bf_apply(W2, X)
    Y[:, K:] = torch.conj(up[:, 1:K - 1]).flip(1)
    return Y


# ---------------------------------------------------------------------------- host-side weight design
def weights_mainlobe(M, N, samplerate, delays, half_band_shift=False):
    """BeamformerWeights::calcMainlobe -> wq complex128 [M][N] (half_band_shift: beamformer.cc:515-527)."""
    delays = np.ascontiguousarray(delays, np.float64)
    if delays.shape != (N,):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION,
                            "Number of delays does not match number of channels (%d vs. %d)." % (delays.size, N))
    wq = np.zeros((M, N), np.complex128)
    fn = _lib.lib().btk_weights_mainlobe_halfband if half_band_shift else _lib.lib().btk_weights_mainlobe
    check(fn(M, N, float(samplerate), _np_ptr(delays), _np_ptr(wq)))
    return wq


def weights_mainlobe_2(M, N, samplerate, delays_t, delays_i):
    """LCMV quiescent weights (target + one null): calcMainlobe2 -> wq complex128 [M][N]."""
    dt = np.ascontiguousarray(delays_t, np.float64)
    di = np.ascontiguousarray(delays_i, np.float64)
    if dt.shape != (N,) or di.shape != (N,):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "The number of delays does not match number of channels (%d)" % N)
    wq = np.zeros((M, N), np.complex128)
    check(_lib.lib().btk_weights_mainlobe_2(M, N, float(samplerate), _np_ptr(dt), _np_ptr(di), _np_ptr(wq)))
    return wq


def weights_mainlobe_n(M, N, samplerate, delays_t, delays_is, NC):
    """LCMV quiescent weights (target + NC-1 nulls): calcMainlobeN -> wq complex128 [M][N]; delays_is [NC-1][N]."""
    dt = np.ascontiguousarray(delays_t, np.float64)
    di = np.ascontiguousarray(delays_is, np.float64).reshape(-1, N)
    if dt.shape != (N,) or di.shape != (NC - 1, N):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "The number of delays does not match number of channels (%d)" % N)
    wq = np.zeros((M, N), np.complex128)
    check(_lib.lib().btk_weights_mainlobe_n(M, N, float(samplerate), _np_ptr(dt), _np_ptr(di), int(NC), _np_ptr(wq)))
    return wq


def weights_blocking_matrix(a, NC=1):
    a = np.ascontiguousarray(a, np.complex128)
    N = a.shape[0]
    if N - NC <= 0:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "The number of sensors %d > the number of constraints %d" % (N, NC))
    B = np.zeros((N, N - NC), np.complex128)
    check(_lib.lib().btk_weights_blocking_matrix(_np_ptr(a), N, NC, _np_ptr(B)))
    return B


def weights_sidelobe(B, wa):
    B = np.ascontiguousarray(B, np.complex128)
    wa = np.ascontiguousarray(wa, np.complex128)
    N, bs = B.shape
    wl = np.zeros(N, np.complex128)
    check(_lib.lib().btk_weights_sidelobe(_np_ptr(B), _np_ptr(wa), N, N - bs, _np_ptr(wl)))
    return wl


def weights_gsc_effective(wq, wl, M, normalize=False):
    """complex64 [K][N] numpy array ready for bf_apply (wq - wl, bin 0 = wq_0)."""
    wq = np.ascontiguousarray(wq, np.complex128)
    N = wq.shape[1]
    wlp = None
    if wl is not None:
        wl = np.ascontiguousarray(wl, np.complex128)
        wlp = _np_ptr(wl)
    out = np.zeros((M // 2 + 1, N), np.complex64)
    check(_lib.lib().btk_weights_gsc_effective(_np_ptr(wq), wlp, M, N, int(normalize), _np_ptr(out)))
    return out


# ---------------------------------------------------------------------------- adaptive canceller (NLMS)
NLMS_DEFAULTS = dict(beta=0.97, gamma=0.01, init_diagonal_load=1.0e6, regularization_param=1.0e-4,
                     energy_floor=90.0, sil_thresh=1.0e8, max_wa_l2norm=100.0, min_frames=128,
                     slowdown_after=4096)      # lib/pybeamformer.py:597-607 == unit_test/confs/gsclms.json


class NLMSState:
    """Device-resident state of S independent SubbandGSCLMSBeamformer recursions
    (reset_stats, lib/pybeamformer.py:745-758)."""

    def __init__(self, S, M, N, device, Nc=1, **kw):
        self.p = dict(NLMS_DEFAULTS)
        self.p.update(kw)
        self.S, self.M, self.N, self.K = S, M, N, M // 2 + 1
        self.Nc = int(Nc)
        self.cextra = None                     # Nc > 1: complex64 [K][Nc-1][N], see set_constraints
        self.u = torch.zeros((S, self.K, N), dtype=torch.complex64, device=device)
        self.sigma2 = torch.empty((S, self.K), dtype=torch.float32, device=device)
        self.stream_state = torch.empty((S, 4), dtype=torch.float64, device=device)
        self.reset_stats()
        self._ws = None
        self._ws_groups = {}                   # interleaved launches: a workspace per stream group
        self._streams = None                   # ... and their HIP streams

    def set_constraints(self, vs):
        """Nc > 1: derive the extra projector directions from the array manifold vs complex [K][N] (host)."""
        if self.Nc > 1:
            self.cextra = torch.from_numpy(nlms_constraint_vectors(vs, self.Nc)).to(self.u.device)

    def reset_stats(self):
        self.u.zero_()
        self.sigma2.fill_(self.p["init_diagonal_load"])
        self.stream_state[:, 0] = self.p["init_diagonal_load"]
        self.stream_state[:, 1] = self.p["gamma"]
        self.stream_state[:, 2] = 0
        self.stream_state[:, 3] = 0
        self.frames_done = 0                   # host copy of the streams' frame counter (every stream advances by T per call)

    def params_array(self):
        p = self.p
        return np.array([p["beta"], p["gamma"], p["regularization_param"], p["energy_floor"], p["sil_thresh"],
                         p["max_wa_l2norm"], p["min_frames"], p["slowdown_after"]], np.float32)

    def workspace(self, T):
        need = _lib.lib().btk_nlms_workspace_bytes(self.S, T)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.u.device)
        return self._ws

    def group_workspace(self, g, Sg, T):
        need = _lib.lib().btk_nlms_workspace_bytes(Sg, T)
        w = self._ws_groups.get(g)
        if w is None or w.numel() < need:
            w = self._ws_groups[g] = torch.empty(need, dtype=torch.uint8, device=self.u.device)
        return w

    def group_streams(self, G):
        return side_streams(self.u.device, G)


def nlms_process(vs, X, state, out=None, interleave=None):
    """Adaptive GSC over a block: vs complex64 [K][N] (cuda), X [S][K][N][T] -> Y [S][K][T]; state updated in place.
    X may be a row-padded view (analysis(pad_rows=True)); Y then shares its row stride.
    interleave: None = decide by the launch shape (_nlms_interleave_plan), (1, T) = one launch, (G, chunk) = G stream groups on G
    HIP streams in chunks of `chunk` frames (a multiple of 64)."""
    ts = _check(X, "X", torch.complex64, 4, rows=True)
    S, K, N, T = X.shape
    _check(vs, "vs", torch.complex64, (K, N))
    if (S, K, N) != (state.S, state.K, state.N):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "nlms_process: shapes do not match the state")
    if out is None:
        out = rows_like(X, (S, K, T))
    if _check(out, "Y", torch.complex64, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "Y rows are %d frames apart, X rows %d: they share T_stride" % (out.stride(-2), ts))
    params = state.params_array()
    ws = state.workspace(T)
    Nc = getattr(state, "Nc", 1)
    if Nc > 1:
        cx = getattr(state, "cextra", None)
        if cx is None:
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "nlms_process: Nc = %d needs state.set_constraints(vs) first" % Nc)
        _check(cx, "cextra", torch.complex64, (K, Nc - 1, N))
    cxp = _ptr(state.cextra) if Nc > 1 else None
    plan = _nlms_interleave_plan(S, K, N, T, state) if interleave is None else tuple(interleave)
    G, chunk, stagger = plan[0], plan[1], (plan[2] if len(plan) > 2 else True)
    if G <= 1:
        check(_lib.lib().btk_nlms_process_nc(_np_ptr(params), _ptr(vs), cxp, Nc, _ptr(X), _ptr(out),
                                             S, state.M, N, ts, T, _ptr(state.u), _ptr(state.sigma2), _ptr(state.stream_state),
                                             _ptr(ws), _stream()))
    else:
        # G groups of streams on G HIP streams, frame chunk after frame chunk: every stream is its own recursion and the kernels
        # carry their state from launch to launch (chunks are multiples of 64 frames: the same bits), so the groups may drift
        # apart -- and they do, which is the point (see _nlms_interleave_plan)
        cur = torch.cuda.current_stream()
        streams = state.group_streams(G)
        e0 = torch.cuda.Event()
        e0.record(cur)
        bounds = [(g * S) // G for g in range(G + 1)]
        lib = _lib.lib()
        for st in streams:
            st.wait_event(e0)
        # group g's first chunk is (g + 1) / G of a chunk (in units of 64 frames): the groups' launch boundaries start out spread
        # over the chunk period instead of coinciding
        segs = []
        for g in range(G):
            first = max(64, (chunk * (g + 1) // G) // 64 * 64) if stagger else chunk
            a = 0
            while a < T:
                n = min(first if a == 0 else chunk, T - a)
                segs.append((a, g, n))
                a += n
        for a, g, n in sorted(segs):
            _nlms_group_launch(lib, params, vs, cxp, Nc, X, out, ts, state, bounds[g], bounds[g + 1], a, n, g, chunk, streams[g])
        for st in streams:
            e = torch.cuda.Event()
            e.record(st)
            cur.wait_event(e)
            for t in (X, out, vs, state.u, state.sigma2, state.stream_state):
                t.record_stream(st)
    state.frames_done = getattr(state, "frames_done", 0) + T
    return out


# The engine's side HIP streams, ONE set per device shared by everything that forks work (interleaved canceller launches,
# AdaptiveGSCChain): the runtime maps streams onto a handful of hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and two streams
# that land on one queue run their kernels in turn -- a second pair of streams created after the first made the chain's bank and
# canceller share a queue (9.6 -> 10.7 ms in bench.py, 9.95 with 8 queues).
_SIDE_STREAMS = {}


def side_streams(device, n):
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    pool = _SIDE_STREAMS.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:n]


def _nlms_group_launch(lib, params, vs, cxp, Nc, X, out, ts, state, s0, s1, a, n, g, chunk_cap, st):
    """frames [a, a + n) of the streams [s0, s1) on the HIP stream st (group g's own workspace, sized for chunk_cap frames)"""
    if s1 <= s0 or n <= 0:
        return
    wg = state.group_workspace(g, s1 - s0, max(chunk_cap, n))
    check(lib.btk_nlms_process_nc(_np_ptr(params), _ptr(vs), cxp, Nc, _ptr(X[s0:s1, :, :, a:a + n]), _ptr(out[s0:s1, :, a:a + n]),
                                  s1 - s0, state.M, X.shape[2], ts, n, _ptr(state.u[s0:s1]), _ptr(state.sigma2[s0:s1]),
                                  _ptr(state.stream_state[s0:s1]), _ptr(wg), C.c_void_p(st.cuda_stream)))


# Wavefronts the canceller kernel of a channel count keeps resident on an MI355X (csrc/nlms_kernels.hip: one single-wavefront
# workgroup per (stream, group of bins); 256 CUs x 4 SIMDs x wavefronts per SIMD at the kernel's register count) and bins per
# wavefront.  Every wavefront walks all frames of the launch, so a launch costs (residency rounds) x (one walk): 32 streams x 65
# bin groups = 2 080 workgroups at 64 channels are a round of 2 048 and a round of 32 that takes as long -- 5.0-5.3 ms where 31
# streams take 3.85 (profiles/r06_nlms_residency.txt).  Cut into frame chunks and a few independent groups of streams on their own
# HIP streams, the groups drift out of step, a group's stragglers run beside the next chunk of the others, and the chip stays
# full: 3.75 ms, bit-identical.  Left to themselves the groups sometimes stay in step (one run in five: 5.3-5.6 ms again), so group g's
# first chunk is shortened to (g + 1) / G of a chunk: two groups x 512 frames, staggered, 3.74-3.77 ms five times out of five
# (profiles/r06_nlms_interleave.txt).
_NLMS_RESIDENT = ((8, 8, 3072), (16, 4, 3072), (32, 4, 2048), (64, 4, 2048), (128, 2, 2048), (1 << 30, 1, 2048))


def _nlms_interleave_plan(S, K, N, T, state):
    """(groups, chunk_frames, stagger) for nlms_process: (1, T, False) = one launch"""
    if os.environ.get("BTK_NLMS_INTERLEAVE", "1") == "0" or S < 4 or T < 512:
        return 1, T, False
    if getattr(state, "frames_done", 0) % 64:
        return 1, T, False                     # chunk boundaries must be multiples of 64 of the streams' frame counter
    bpw, slots = next((b, r) for n, b, r in _NLMS_RESIDENT if N <= n)
    nwg = S * ((K + bpw - 1) // bpw)
    if nwg <= slots:
        return 1, T, False
    return 2, (512 if T >= 1024 else 256), True


class AdaptiveGSCChain:
    """The adaptive chain of lib/pybeamformer.py:659-762 over analysis banks, S streams at once:
    PCM -> analysis bank -> snapshots X [S][K][N][T] (HBM) -> NLMS sidelobe canceller -> Y -> synthesis bank -> PCM.

    The canceller is a recursion in t that keeps two wavefronts per SIMD busy at C0 and leaves most of the register file and of
    the HBM bandwidth idle; the analysis bank streams.  So the bank runs AHEAD on one HIP stream, frame chunk after frame chunk
    into the one snapshot buffer, and the canceller follows on a second stream as soon as a chunk's snapshots are complete
    (profiles/adaptive_overlap_ab.py: 10.4 -> 9.7 ms per 32 x 4096 frames at C0).  Chunks are multiples of 64 frames, so the
    output is bit-identical to the one-launch-per-kernel chain (state and scan chunks carry, csrc/nlms_kernels.hip)."""

    def __init__(self, afb, sfb, chunk_frames=512, groups=None):
        if chunk_frames < 64 or chunk_frames % 64:
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "chunk_frames must be a multiple of 64, got %r" % (chunk_frames,))
        self.afb, self.sfb, self.chunk = afb, sfb, int(chunk_frames)
        self.groups = groups                   # canceller stream groups per chunk: None = by the launch shape, 1 = the round-5 form
        self._sa = self._sb = None

    def __call__(self, pcm, vs, state, X, Y, out=None, nsamples=None):
        """pcm [S][N][L]; X [S][K][N][T] and Y [S][K][T] (row-padded views allowed, same row pitch); returns the PCM blocks."""
        T = X.shape[-1]
        if self._sa is None:
            self._sa, self._sb = side_streams(pcm.device, 2)
        if out is None:
            # allocated on the CALLER's stream, where it is consumed: a block taken inside the side stream's context would belong to
            # that stream's pool and could be handed on while the caller still reads it
            out = torch.empty((X.shape[0], self.sfb.num_blocks(T) * self.sfb.D), dtype=torch.float32, device=pcm.device)
        cur = torch.cuda.current_stream()
        ev0 = torch.cuda.Event()
        ev0.record(cur)
        self._sa.wait_event(ev0)
        self._sb.wait_event(ev0)
        S, K, N = X.shape[0], X.shape[1], X.shape[2]
        # round 6 (groups > 1, not the default): the canceller of a chunk as G independent groups of streams, each on its own HIP
        # stream behind the bank's chunk.  It is what makes the canceller ALONE 25 % faster at 32 streams (_nlms_interleave_plan);
        # in the chain the bank's launches already run in the canceller's residency gaps: 9.5 ms with 1 or 2 groups, 10.7-11.8
        # with 4 or 8 (profiles/r06_nlms_interleave.txt).
        G = 1 if self.groups is None else int(self.groups)    # (measured: no gain inside the chain, the bank's kernels already fill the gaps)
        if state.frames_done % 64:
            G = 1
        gstreams = side_streams(pcm.device, 2 + G)[2:] if G > 1 else []
        for st in gstreams:
            st.wait_event(ev0)
        if G > 1:
            ts = _check(X, "X", torch.complex64, 4, rows=True)
            params, lib = state.params_array(), _lib.lib()
            Nc = getattr(state, "Nc", 1)
            cxp = _ptr(state.cextra) if Nc > 1 else None
            bounds = [(g * S) // G for g in range(G + 1)]
        for a in range(0, T, self.chunk):
            n = min(self.chunk, T - a)
            with torch.cuda.stream(self._sa):
                self.afb.analysis(pcm, nsamples=nsamples, t0=a, tcount=n, out=X[..., a:a + n])
                e = torch.cuda.Event()
                e.record(self._sa)
            if G > 1:
                for g, st in enumerate(gstreams):
                    st.wait_event(e)
                    _nlms_group_launch(lib, params, vs, cxp, Nc, X, Y, ts, state, bounds[g], bounds[g + 1], a, n, g, self.chunk, st)
            else:
                self._sb.wait_event(e)
                with torch.cuda.stream(self._sb):
                    nlms_process(vs, X[..., a:a + n], state, out=Y[..., a:a + n], interleave=(1, n))
        if G > 1:
            state.frames_done += T
            for st in gstreams:
                e = torch.cuda.Event()
                e.record(st)
                self._sb.wait_event(e)
        with torch.cuda.stream(self._sb):
            out = self.sfb.synthesize(Y, out=out)
            e = torch.cuda.Event()
            e.record(self._sb)
        cur.wait_event(e)
        for t in (pcm, X, Y, out):                      # the caching allocator must not hand these blocks on before the side streams are done
            for st in [self._sa, self._sb] + list(gstreams):
                t.record_stream(st)
        for st in gstreams:
            for t in (vs, state.u, state.sigma2, state.stream_state):
                t.record_stream(st)
        return out


def constraint_vectors(vs, Nc):
    """The Nc - 1 extra orthonormal directions the Nc-constraint cancellers' projector loses per bin (include/btkhip.h):
    vs complex [K][N] (host) -> complex128 [K][Nc-1][N] (host)."""
    vs = np.ascontiguousarray(vs, np.complex128)
    K, N = vs.shape
    out = np.zeros((K, Nc - 1, N), np.complex128)
    for k in range(K):
        B = weights_blocking_matrix(vs[k], Nc)
        check(_lib.lib().btk_nlms_constraint_vectors(_np_ptr(vs[k]), _np_ptr(B), N, Nc, _np_ptr(out[k])))
    return out


def nlms_constraint_vectors(vs, Nc):
    """constraint_vectors in the NLMS kernel's element type: complex64 [K][Nc-1][N] (host)"""
    return constraint_vectors(vs, Nc).astype(np.complex64)


def nlms_u_to_wa(u, B):
    """wa^H (complex128 [N-Nc]) from the engine state u (complex [N]) and the bin's blocking matrix B [N][N-Nc]."""
    u = np.ascontiguousarray(u, np.complex128)
    B = np.ascontiguousarray(B, np.complex128)
    N = u.shape[0]
    Nc = N - B.shape[1]
    wa = np.zeros(N - Nc, np.complex128)
    check(_lib.lib().btk_nlms_u_to_wa_nc(_np_ptr(u), _np_ptr(B), N, Nc, _np_ptr(wa)))
    return wa


def nlms_wa_to_u(waH, B):
    waH = np.ascontiguousarray(waH, np.complex128)
    B = np.ascontiguousarray(B, np.complex128)
    N = B.shape[0]
    u = np.zeros(N, np.complex128)
    check(_lib.lib().btk_nlms_wa_to_u(_np_ptr(waH), _np_ptr(B), N, _np_ptr(u)))
    return u


# ---------------------------------------------------------------------------- RLS canceller
RLS_PY_DEFAULTS = dict(beta=0.97, gamma=0.04, mu=0.97, init_diagonal_load=1.0e6, regularization_param=1.0e-2,
                       sil_thresh=1.0e8, constraint_option=3, alpha2=10.0, max_wa_l2norm=100.0, min_frames=128)
RLS_CC_DEFAULTS = dict(mu=0.9, diagonal_weight=0.0, qctype=0, alpha=-1.0, normalize_weight=False, update=True)


class RLSState:
    """Device-resident state of S independent RLS sidelobe cancellers.
    mode 1: SubbandGSCRLSBeamformer (lib/pybeamformer.py:765-928); mode 0: SubbandGSCRLS (beamformer.cc:1447-1645).
    v complex128 [K][N] or [S][K][N] (cuda): vs resp. wq of bins 0..M/2."""

    def __init__(self, mode, S, M, N, v, Nc=1, **kw):
        if mode not in (0, 1):
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "RLSState: mode must be 0 or 1")
        self.mode = mode
        self.Nc = int(Nc)
        self.cx = None                         # Nc > 1: complex128 [K][Nc-1][N] on the device, the further blocked directions
        self.p = dict(RLS_PY_DEFAULTS if mode == 1 else RLS_CC_DEFAULTS)
        unknown = set(kw) - set(self.p)
        if unknown:
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "RLSState: unknown parameters %s" % sorted(unknown))
        self.p.update(kw)
        _need_cuda(v, "v")
        self.S, self.M, self.N, self.K = S, M, N, M // 2 + 1
        if v.dtype != torch.complex128 or v.shape[-2:] != (self.K, N) or v.dim() not in (2, 3):
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "RLSState: v must be complex128 [K][N] or [S][K][N]")
        self.v = v.contiguous()
        self.per_stream = 1 if v.dim() == 3 else 0
        dev = v.device
        self.P = torch.empty((S, self.K, N, N), dtype=torch.complex128, device=dev)
        self.w = torch.empty((S, self.K, N), dtype=torch.complex128, device=dev)
        self.stream_state = torch.zeros((S, 4), dtype=torch.float64, device=dev)
        self._ws = None
        if self.Nc > 1:
            if self.per_stream:
                raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "RLSState: Nc > 1 takes one v [K][N] for all streams")
            # conj(B) B^T = I - v v^H/|v|^2 - sum_j c_j c_j^H (mode 1); mode 0: B B^H, i.e. the complex conjugates (include/btkhip.h)
            cx = constraint_vectors(self.v.cpu().numpy(), self.Nc)
            self.cx = torch.from_numpy(np.conj(cx) if mode == 0 else cx).to(dev).contiguous()
        if mode == 1:
            self.reset_stats()

    def init_precision_matrix(self, p0):
        """P = p0 B B^H (mode 0) / p0 conj(B) B^T (mode 1), w = 0 (init_precision_matrix with p0 = 1/sigma2,
        beamformer.cc:1482-1494)"""
        check(_lib.lib().btk_rls_init_nc(self.mode, _ptr(self.v), self.per_stream, None if self.cx is None else _ptr(self.cx), self.Nc,
                                         float(p0), self.S, self.K, self.N, _ptr(self.P), _ptr(self.w), _stream()))

    def reset_stats(self):
        """pybeamformer.py:913-925"""
        self.init_precision_matrix(1.0 / self.p["init_diagonal_load"])
        self.stream_state.zero_()
        self.stream_state[:, 0] = self.p["init_diagonal_load"]

    def params_array(self):
        p = self.p
        if self.mode == 1:
            return np.array([p["beta"], p["gamma"], p["mu"], p["init_diagonal_load"], p["regularization_param"],
                             p["sil_thresh"], p["constraint_option"], p["alpha2"], p["max_wa_l2norm"], p["min_frames"]],
                            np.float64)
        return np.array([p["mu"], p["diagonal_weight"], p["qctype"], p["alpha"], float(bool(p["normalize_weight"])),
                         float(bool(p["update"]))], np.float64)

    def workspace(self, T):
        need = _lib.lib().btk_rls_workspace_bytes(self.S, T)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.P.device)
        return self._ws


def rls_process(X, state, out=None):
    """RLS canceller over a block: X complex64 [S][K][N][T] -> Y [S][K][T]; state updated in place."""
    _check(X, "X", torch.complex64, 4)
    S, K, N, T = X.shape
    if (S, K, N) != (state.S, state.K, state.N):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "rls_process: shapes do not match the state")
    if out is None:
        out = torch.empty((S, K, T), dtype=torch.complex64, device=X.device)
    else:
        _check(out, "Y", torch.complex64, (S, K, T))
    params = state.params_array()
    ws = state.workspace(T)
    check(_lib.lib().btk_rls_process_nc(state.mode, _np_ptr(params), _ptr(state.v), state.per_stream,
                                        None if state.cx is None else _ptr(state.cx), state.Nc, _ptr(X), _ptr(out),
                                        S, state.M, N, T, T, _ptr(state.P), _ptr(state.w), _ptr(state.stream_state),
                                        _ptr(ws), _stream()))
    return out


def rls_state_to_reference(mode, P, w, B):
    """Host change of basis for one bin: engine (P [N][N], w [N]) -> reference (Pz [N-Nc][N-Nc], wa resp. waH [N-Nc])
    with the bin's blocking matrix B [N][N-Nc] (orthonormal columns)."""
    P = np.asarray(P, np.complex128)
    w = np.asarray(w, np.complex128)
    B = np.asarray(B, np.complex128)
    if mode == 1:      # P = conj(B) Pz B^T, u = waH B^T
        return B.T @ P @ np.conj(B), w @ np.conj(B)
    return np.conj(B.T) @ P @ B, np.conj(B.T) @ w      # P = B Pz B^H, wl = B wa


# ---------------------------------------------------------------------------- subband acoustic echo cancellation
AEC_KINDS = {"nlms": 0, "kalman_filter": 1, "block_kalman_filter": 2, "dtd_block_kalman_filter": 3}
# the reference constructors' defaults (aec/aec.h:36,73,106,308)
AEC_DEFAULTS = (
    dict(delta=100.0, epsilon=1.0e-4, threshold=100.0),
    dict(beta=0.95, sigma2=100.0, threshold=100.0),
    dict(beta=0.95, sigmau2=10e-4, sigmak2=5.0, threshold=100.0, amp4play=1.0),
    dict(beta=0.95, sigmau2=10e-4, sigmak2=5.0, snr_threshold=2.0, energy_threshold=100.0, smooth=0.9, amp4play=1.0),
)


class AECState:
    """Device-resident state of S independent subband echo cancellers (aec/aec.cc), bins 0..M/2 only.
    kind 0 NLMS, 1 Kalman, 2 block Kalman, 3 double-talk detecting block Kalman (or the names of AEC_KINDS); P = sample_num.
    R complex128 [S][K][P], K complex128 [S][K][P][P], sigma2_v float64 [S][K], history complex128 [S][K][P] (slot 0 newest, scaled
    by amp4play), dtd float64 [S][4] = {EkEnergy_, SkEnergy_, snr_, frames done}."""

    def __init__(self, kind, S, M, P=1, device="cuda", **kw):
        kind = AEC_KINDS.get(kind, kind)
        if kind not in (0, 1, 2, 3):
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "AECState: kind must be 0..3 or one of %s" % sorted(AEC_KINDS))
        self.kind = kind
        self.p = dict(AEC_DEFAULTS[kind])
        unknown = set(kw) - set(self.p)
        if unknown:
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "AECState: unknown parameters %s" % sorted(unknown))
        self.p.update(kw)
        L = _lib.lib()
        self.S, self.M, self.P, self.Kb = int(S), int(M), int(P), M // 2 + 1
        dev = torch.device(device)
        if min(self.S, self.M, self.P) < 1:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "AECState: S=%d M=%d sample_num=%d" % (S, M, P))
        # (the limits -- filter length, number of subbands, P = 1 for the one-tap kinds -- are btk_aec_init's to refuse)
        self.R = torch.empty((S, self.Kb, P), dtype=torch.complex128, device=dev)
        self.K = torch.empty((S, self.Kb, P, P), dtype=torch.complex128, device=dev)
        self.sigma2_v = torch.empty((S, self.Kb), dtype=torch.float64, device=dev)
        self.history = torch.empty((S, self.Kb, P), dtype=torch.complex128, device=dev)
        self.dtd = torch.empty((S, 4), dtype=torch.float64, device=dev)
        check(L.btk_aec_init(self.kind, _np_ptr(self.params_array()), self.S, self.M, self.P, _ptr(self.R), _ptr(self.K),
                             _ptr(self.sigma2_v), _ptr(self.history), _ptr(self.dtd), _stream()))

    def params_array(self):
        p = self.p
        if self.kind == 0:
            return np.array([p["delta"], p["epsilon"], 0, p["threshold"], 0, 0, 1, 0], np.float64)
        if self.kind == 1:
            return np.array([p["beta"], p["sigma2"], 0, p["threshold"], 0, 0, 1, 0], np.float64)
        if self.kind == 2:
            return np.array([p["beta"], p["sigmau2"], p["sigmak2"], p["threshold"], 0, 0, p["amp4play"], 0], np.float64)
        return np.array([p["beta"], p["sigmau2"], p["sigmak2"], p["snr_threshold"], p["energy_threshold"], p["smooth"],
                         p["amp4play"], 0], np.float64)

    def reset(self):
        """The nodes' reset() (aec.h:41,78,111-114): kinds 0 and 1 zero the filter and nothing else (kind 1 keeps sigma2_v and K);
        kinds 2 and 3 reset their sources only, so all of the adaptive state and the played history survive."""
        if self.kind < 2:
            self.R.zero_()

    def dtd_state_in_lds(self):
        return bool(_lib.lib().btk_aec_dtd_state_in_lds(self.M, self.P))


def aec_process(V, A, state, out=None, frame_no0=None, adapted=None):
    """Echo canceller over a block: played V, recorded A complex64 [S][K][T] (rows may be padded) -> residual E [S][K][T]; state
    updated in place.  frame_no0 (kind 3): None counts the frames up from the state's frames done (explicit frame numbers 0, 1, ...),
    an int >= 0 counts up from it, a negative int is handed to every frame (a consumer that calls next(-5), aec.cc:902).
    adapted: optional uint8 tensor laid out like E, set to 1 where the update ran."""
    ts = _check(V, "V", torch.complex64, (state.S, state.Kb, None), rows=True)
    S, K, T = V.shape
    if _check(A, "A", torch.complex64, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "aec_process: V and A must share one row stride")
    if out is None:
        out = rows_like(V, (S, K, T))
    elif _check(out, "out", torch.complex64, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "aec_process: out must share the row stride of V")
    if adapted is not None and _check(adapted, "adapted", torch.uint8, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "aec_process: adapted must share the row stride of V")
    fn0 = _lib.BTK_AEC_FRAME_CONTINUE if frame_no0 is None else int(frame_no0)
    if frame_no0 is not None and fn0 <= _lib.BTK_AEC_FRAME_CONTINUE:
        raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "aec_process: frame_no0 out of range")
    check(_lib.lib().btk_aec_process(state.kind, _np_ptr(state.params_array()), _ptr(V), _ptr(A), _ptr(out),
                                     None if adapted is None else _ptr(adapted), S, state.M, state.P, ts, T, fn0,
                                     _ptr(state.R), _ptr(state.K), _ptr(state.sigma2_v), _ptr(state.history), _ptr(state.dtd),
                                     _stream()))
    return out


# ---------------------------------------------------------------------------- Zelinski post-filter
class ZelinskiState:
    """Summed CSD / PSD state of S post-filters (the part of BeamformerWeights::CSDs_/wp1_,
    beamformer.cc:874-887, that the Zelinski gain depends on)."""

    def __init__(self, S, K, device):
        self.phi = torch.zeros((S, K), dtype=torch.complex64, device=device)
        self.psi = torch.zeros((S, K), dtype=torch.float32, device=device)
        self.w_last = torch.zeros((S, K), dtype=torch.float32, device=device)
        self.frames_done = 0

    def reset_csd(self):
        """What alloc_bfweight_ does to the post-filter state when weights are recomputed
        (beamformer.cc:1082-1092): CSD history restarts, the frame counter keeps counting."""
        self.phi.zero_()
        self.psi.zero_()
        self.w_last.zero_()


def bf_apply_zelinski(W, D, X, state, alpha=0.6, type_=2, min_frames=0, out=None):
    """Beamform + Zelinski post-filter over a block (ZelinskiPostFilter over SubbandDS/GSC/MVDR).
    W, D complex64 [S|1][K][N]; X [S][K][N][T] -> Y [S][K][T] (post-filtered).  X may be a row-padded view
    (analysis(pad_rows=True)); Y and the per-frame statistics then share its row stride."""
    ts = _check(X, "X", torch.complex64, 4, rows=True)
    S, K, N, T = X.shape
    if W.dim() == 2:
        W, D = W.unsqueeze(0), D.unsqueeze(0)
    _check(W, "W", torch.complex64, (None, K, N)); _check(D, "D", torch.complex64, tuple(W.shape))
    if W.shape[0] not in (1, S):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "weights %s do not match X %s" % (tuple(W.shape), tuple(X.shape)))
    if out is None:
        out = rows_like(X, (S, K, T))
    if _check(out, "Y", torch.complex64, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "Y rows are %d frames apart, X rows %d: they share T_stride" % (out.stride(-2), ts))
    Cc = rows_like(X, (S, K, T))
    Ee = rows_like(X, (S, K, T), dtype=torch.float32)
    L = _lib.lib()
    check(L.btk_bf_apply_stats(_ptr(W), _ptr(D), int(W.shape[0] == S and S > 1), _ptr(X), _ptr(out), _ptr(Cc), _ptr(Ee),
                               S, K, N, ts, T, _stream()))
    check(L.btk_zelinski_process(_ptr(out), _ptr(Cc), _ptr(Ee), S, K, N, ts, T, float(alpha), int(type_), int(min_frames),
                                 state.frames_done, _ptr(state.phi), _ptr(state.psi), _ptr(state.w_last), _stream()))
    state.frames_done += T
    return out


class CoherencePostFilterState:
    """State of S McCowan / Lefkimmiatis post-filters: the recursively averaged weighted CSD sums (see
    csrc/pf_kernels.hip) plus the per-bin pair-weight matrices built from the noise coherence matrix R_."""

    def __init__(self, S, K, N, device, lefkimmiatis=False):
        self.S, self.K, self.N = S, K, N
        self.lefkimmiatis = bool(lefkimmiatis)
        self.u = torch.zeros((S, K), dtype=torch.complex64, device=device)
        self.v = torch.zeros((S, K), dtype=torch.complex64, device=device)     # Lefkimmiatis only
        self.psi = torch.zeros((S, K), dtype=torch.float32, device=device)     # McCowan only
        self.w_last = torch.zeros((S, K), dtype=torch.float32, device=device)
        self.Cs = self.Cv = self.lam = None
        self.frames_done = 0

    def reset_csd(self):
        """As ZelinskiState.reset_csd(): the CSD history restarts, the frame counter keeps counting (beamformer.cc:1082-1092)."""
        self.u.zero_()
        self.v.zero_()
        self.psi.zero_()
        self.w_last.zero_()

    def set_coherence(self, R, threshold=0.99):
        """R complex64 [K][N][N] (cuda): R_ after set_diffuse_noise_model / set_noise_spatial_spectral_matrix /
        diagonal loading (postfilter.cc:536-660); threshold = threshold_of_Rij_."""
        _need_cuda(R, "R")
        K, N = self.K, self.N
        if tuple(R.shape) != (K, N, N):
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "set_coherence: R must be [K][N][N]")
        self.Cs = torch.empty((K, N, N), dtype=torch.complex64, device=R.device)
        self.Cv = torch.empty((K, N, N), dtype=torch.complex64, device=R.device) if self.lefkimmiatis else None
        check(_lib.lib().btk_pf_coherence_coeffs(_ptr(R.contiguous()), float(np.float32(threshold)), K, N, _ptr(self.Cs),
                                                 None if self.Cv is None else _ptr(self.Cv), _stream()))

    def set_lambda(self, R, d, min_sv=1.0e-8, svd_rule=None):
        """Lambda_k = d^H pinv(R_k) d (calcLambda, postfilter.cc:982-995) for all bins; returns the number of bins
        that fell back to the identity (:975-977).  svd_rule as in mvdr_weights(): "linpack" (default) takes the identity
        exactly where the reference's pseudoinverse() returns false (all bins, bin 0 included: postfilter.cc:971)."""
        _need_cuda(R, "R"); _need_cuda(d, "d")
        K, N = self.K, self.N
        rule = svd_rule_default() if svd_rule is None else svd_rule
        if rule not in SVD_RULES:
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "svd_rule must be one of %s, got %r" % (SVD_RULES, rule))
        R, d = R.contiguous(), d.contiguous()
        self.lam = torch.empty((K,), dtype=torch.complex64, device=R.device)
        if rule == "linpack_full":          # d^H A+ d from the reference's own inverse, d^H d where pseudoinverse() returns false
            counts = _linpack_full(R, d, None, self.lam, K, N, 0, 0, 0, min_sv)
            return int(counts.sum().item())
        fb = torch.zeros(1, dtype=torch.int32, device=R.device)
        sb = _lib.lib().btk_mvdr_scratch_bytes(K, N)
        scratch = torch.empty((sb,), dtype=torch.uint8, device=R.device) if sb else None
        check(_lib.lib().btk_mvdr_lambda(_ptr(R), _ptr(d), _ptr(self.lam), K, N, float(min_sv),
                                         None if scratch is None else _ptr(scratch), _ptr(fb), _stream()))
        if rule == "linpack":
            counts = _linpack_rule(R, d, None, self.lam, K, N, 0, 0, 0, min_sv, None)
            return int(counts.sum().item())
        return int(fb.item())


def _pf_args(W, D, X, out):
    """Shape / dtype / row-stride checks shared by the coherence post-filters; returns (T_stride, S, K, N, T, W, D, out)."""
    ts = _check(X, "X", torch.complex64, 4, rows=True)
    S, K, N, T = X.shape
    if W.dim() == 2:
        W, D = W.unsqueeze(0), D.unsqueeze(0)
    _check(W, "W", torch.complex64, (None, K, N)); _check(D, "D", torch.complex64, tuple(W.shape))
    if W.shape[0] not in (1, S):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "weights %s do not match X %s" % (tuple(W.shape), tuple(X.shape)))
    if out is None:
        out = rows_like(X, (S, K, T))
    if _check(out, "Y", torch.complex64, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "Y rows are %d frames apart, X rows %d: they share T_stride" % (out.stride(-2), ts))
    return ts, S, K, N, T, W, D, out


def bf_apply_mccowan(W, D, X, state, alpha=0.6, type_=2, min_frames=0, out=None):
    """Beamform + McCowan post-filter over a block.  W, D complex64 [S|1][K][N]; X [S][K][N][T] -> Y [S][K][T].  X may be a
    row-padded view (analysis(pad_rows=True)); Y and the per-frame statistics then share its row stride."""
    ts, S, K, N, T, W, D, out = _pf_args(W, D, X, out)
    if state.Cs is None:
        raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "McCowanPostFilter:  construct/set a noise coherence matrix")
    U = rows_like(X, (S, K, T))
    Ee = rows_like(X, (S, K, T), dtype=torch.float32)
    L = _lib.lib()
    check(L.btk_bf_apply_stats2(_ptr(W), _ptr(D), int(W.shape[0] == S and S > 1), _ptr(X), _ptr(out), _ptr(state.Cs), None,
                                _ptr(U), None, _ptr(Ee), S, K, N, ts, T, _stream()))
    check(L.btk_zelinski_process(_ptr(out), _ptr(U), _ptr(Ee), S, K, N, ts, T, float(alpha), (int(type_) & 15) | _lib.BTK_PF_MCCOWAN_RULES,
                                 int(min_frames), state.frames_done, _ptr(state.u), _ptr(state.psi), _ptr(state.w_last), _stream()))
    state.frames_done += T
    return out


def bf_apply_lefkimmiatis(W, D, X, state, fbin_x1=0, alpha=0.6, type_=2, min_frames=0, out=None):
    """Beamform + Lefkimmiatis post-filter over a block (D = array manifold); X may be a row-padded view as for McCowan."""
    ts, S, K, N, T, W, D, out = _pf_args(W, D, X, out)
    if state.Cs is None or state.Cv is None or state.lam is None:
        raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "LefkimmiatisPostFilter:  construct/set a noise coherence matrix")
    U = rows_like(X, (S, K, T))
    V = rows_like(X, (S, K, T))
    Ee = rows_like(X, (S, K, T), dtype=torch.float32)
    L = _lib.lib()
    check(L.btk_bf_apply_stats2(_ptr(W), _ptr(D), int(W.shape[0] == S and S > 1), _ptr(X), _ptr(out), _ptr(state.Cs),
                                _ptr(state.Cv), _ptr(U), _ptr(V), _ptr(Ee), S, K, N, ts, T, _stream()))
    check(L.btk_lefkimmiatis_process(_ptr(out), _ptr(U), _ptr(V), _ptr(state.lam), int(fbin_x1), S, K, N, ts, T, float(alpha),
                                     int(type_), int(min_frames), state.frames_done, _ptr(state.u), _ptr(state.v),
                                     _ptr(state.w_last), _stream()))
    state.frames_done += T
    return out


# ---------------------------------------------------------------------------- spectral subtraction, Wiener filter, high-pass
def _frame_flags(flags, T, device, name):
    """uint8 [T] device tensor of per-frame mode bits (or None): a host sequence is uploaded."""
    if flags is None:
        return None
    if not torch.is_tensor(flags):
        flags = torch.from_numpy(np.ascontiguousarray(flags, dtype=np.uint8)).to(device)
    _check(flags, name, torch.uint8, (T,))
    return flags


class SpectralSubtractionState:
    """Noise models of S spectral subtractors with C channels each (the AveragePSDEstimator of every set_channel(),
    postfilter/spectralsubtraction.cc:52-129, :185-189), bins 0..M/2.  alphas: one forgetting factor per channel, < 0 for a channel
    that averages its training frames (the reference's default, -1).  est, acc float64 [S][C][K]; count int64 [S][C] (frames in
    acc, averaging channels); added uint8 [S][C] (sample_added_, recursive channels); frames_done places the scan chunks."""

    def __init__(self, S, C, M, alphas=None, device="cuda"):
        self.S, self.C, self.M, self.Kb = int(S), int(C), int(M), int(M) // 2 + 1
        if self.S < 1 or self.M < 2 or self.M % 2 or self.M > 2048:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "SpectralSubtractionState: S=%d M=%d" % (S, M))
        if not 1 <= self.C <= _lib.lib().btk_ss_max_channels():
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "SpectralSubtractionState: %d channels" % C)
        a = np.full(self.C, -1.0) if alphas is None else np.array(alphas, np.float64).reshape(-1)
        if a.shape != (self.C,):
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "SpectralSubtractionState: %d alphas for %d channels" % (a.size, self.C))
        self.alphas = np.ascontiguousarray(a)
        dev = torch.device(device)
        self.est = torch.zeros((self.S, self.C, self.Kb), dtype=torch.float64, device=dev)
        self.acc = torch.zeros((self.S, self.C, self.Kb), dtype=torch.float64, device=dev)
        self.count = torch.zeros((self.S, self.C), dtype=torch.int64, device=dev)
        self.added = torch.zeros((self.S, self.C), dtype=torch.uint8, device=dev)
        self.frames_done = 0

    def _clear(self, what):
        check(_lib.lib().btk_ss_clear(self.S, self.M, self.C, what, _ptr(self.acc), _ptr(self.count), _ptr(self.added), _stream()))

    def reset_training(self):
        """clear_noise_samples() (:198-202): the averaging sums and their frame counts go, the estimates stay."""
        self._clear(0)

    def clear(self):
        """AveragePSDEstimator::clear() (:63-68): as reset_training(), and the next training frame of a recursive channel is a first
        sample again.  The estimates stay until then."""
        self._clear(1)

    def finish_training(self):
        """stop_training()'s average() (:70-87, :191-196): est = acc (1.0/(float)count) on the averaging channels."""
        check(_lib.lib().btk_ss_finish_training(self.S, self.M, self.C, _np_ptr(self.alphas), _ptr(self.est), _ptr(self.acc),
                                                _ptr(self.count), _stream()))

    def noise_psd(self):
        """A copy of the noise PSD estimates, float64 [S][C][K]."""
        return self.est.clone()

    def set_noise_psd(self, psd, channel=None):
        """Overwrite the estimates (read_estimates, :29-50): psd [K] or [S][K] for one channel, [S][C][K] without `channel`."""
        psd = torch.as_tensor(psd, dtype=torch.float64).to(self.est.device)
        if channel is None:
            self.est.copy_(psd.expand_as(self.est))
        else:
            self.est[:, int(channel)].copy_(psd.expand(self.S, self.Kb))

    def write_noise_file(self, fn, channel=0, stream=0):
        """write_noise_file (spectralsubtraction.h:89): one channel's estimate of one stream, see write_noise_psd_file."""
        return write_noise_psd_file(fn, self.est[int(stream), int(channel)].cpu().numpy())

    def read_noise_file(self, fn, channel=0, stream=None):
        """read_estimates (:17-33) into one channel's estimate (of every stream, or of `stream`); False where the file cannot be
        opened, as there.  (That training ends with it, :204-207, is the caller's mode.)"""
        psd = read_noise_psd_file(fn, self.Kb)
        if psd is None:
            return False
        row = torch.from_numpy(psd).to(self.est.device)           # a short file names the first bins only: the others stay
        if stream is None:
            self.est[:, int(channel), : len(psd)] = row
        else:
            self.est[int(stream), int(channel), : len(psd)] = row
        return True


def write_noise_psd_file(fn, psd):
    """PSDEstimator::write_estimates (spectralsubtraction.cc:35-49): the reference's text format, "%lf\\n" per bin, K lines.  The
    six decimals are part of it: a model read back holds each bin to within 5e-7."""
    try:
        with open(fn, "w") as fp:
            fp.write("".join("%f\n" % v for v in np.asarray(psd, np.float64).reshape(-1)))
    except OSError:
        sys.stderr.write("could not write %s\n" % fn)
        return False
    return True


def read_noise_psd_file(fn, K):
    """PSDEstimator::read_estimates (:17-33): the file's values, float64, at most K of them; None where the file cannot be
    opened.  A file with fewer than K lines yields a shorter array: the reference leaves the bins it does not name as they were,
    and so does SpectralSubtractionState.read_noise_file."""
    try:
        with open(fn) as fp:
            vals = [float(v) for v in fp.read().split()][:K]
    except OSError:
        sys.stderr.write("could not read %s\n" % fn)
        return None
    return np.array(vals, np.float64)


def spectral_subtract(X, state, ft=1.0, floor=0.001, flags=None, train=False, subtract=True, out=None, form=None):
    """Spectral subtraction over a block (SpectralSubtractor::next, :216-285): X complex64 [S][K][C][T] (rows may be padded) ->
    Y [S][K][T], the mean over the channels of X sqrt(max(|X|^2 - ft est, floor))/|X|; state updated in place.
    flags: uint8 [T], bit 0 (BTK_SS_TRAIN) the frame enters the noise model -- before it is subtracted --, bit 1 (BTK_SS_SUBTRACT)
    the frame is subtracted; without flags every frame has the mode (train, subtract).  A block that cannot train runs frame-
    parallel; form=_lib.BTK_SS_FORM_ROWS forces the row scan (same bits)."""
    ts = _check(X, "X", torch.complex64, (state.S, state.Kb, state.C, None), rows=True)
    S, K, C, T = X.shape
    if out is None:
        out = rows_like(X, (S, K, T))
    elif _check(out, "out", torch.complex64, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "spectral_subtract: out must share the row stride of X")
    flags = _frame_flags(flags, T, X.device, "flags")
    mode = (_lib.BTK_SS_TRAIN if train else 0) | (_lib.BTK_SS_SUBTRACT if subtract else 0)
    check(_lib.lib().btk_ss_process(_ptr(X), _ptr(out), S, state.M, C, ts, T, None if flags is None else _ptr(flags), mode,
                                    float(ft), float(floor), _np_ptr(state.alphas), state.frames_done, _ptr(state.est),
                                    _ptr(state.acc), _ptr(state.count), _ptr(state.added),
                                    _lib.BTK_SS_FORM_AUTO if form is None else int(form), _stream()))
    state.frames_done += T
    return out


class WienerState:
    """Recursively averaged target and noise PSDs of S Wiener filters (prev_PSDs_, prev_PSDn_, spectralsubtraction.cc:304-305),
    float64 [S][K] (row 0 is never touched), and the frame counter that decides the two frames without memory.  reset() of the
    node resets its sources only (:364-368): there is nothing to reset here."""

    def __init__(self, S, M, device="cuda"):
        self.S, self.M, self.Kb = int(S), int(M), int(M) // 2 + 1
        if self.S < 1 or self.M < 2 or self.M % 2 or self.M > 2048:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "WienerState: S=%d M=%d" % (S, M))
        self.psd_s = torch.zeros((self.S, self.Kb), dtype=torch.float64, device=torch.device(device))
        self.psd_n = torch.zeros_like(self.psd_s)
        self.frames_done = 0


def wiener_filter(Sx, Nx, state, alpha=0.0, floor=0.001, beta=1.0, flags=None, update_noise=True, out=None):
    """Wiener filter over a block (WienerFilter::next, :314-362): target Sx, noise Nx complex64 [S][K][T] (rows may be padded) ->
    Y = H Sx, H = PSDs/(PSDs + beta PSDn); bin 0 is Sx's.  flags: uint8 [T], bit 0 (BTK_WIENER_UPDATE_NOISE) the frame updates the
    noise PSD; without flags update_noise holds for every frame."""
    ts = _check(Sx, "Sx", torch.complex64, (state.S, state.Kb, None), rows=True)
    S, K, T = Sx.shape
    if _check(Nx, "Nx", torch.complex64, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "wiener_filter: Sx and Nx must share one row stride")
    if out is None:
        out = rows_like(Sx, (S, K, T))
    elif _check(out, "out", torch.complex64, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "wiener_filter: out must share the row stride of Sx")
    flags = _frame_flags(flags, T, Sx.device, "flags")
    check(_lib.lib().btk_wiener_process(_ptr(Sx), _ptr(Nx), _ptr(out), S, state.M, ts, T, None if flags is None else _ptr(flags),
                                        _lib.BTK_WIENER_UPDATE_NOISE if update_noise else 0, float(alpha), float(floor),
                                        float(beta), state.frames_done, _ptr(state.psd_s), _ptr(state.psd_n), _stream()))
    state.frames_done += T
    return out


def highpass_cutoff_bin(M, cut_off_freq, samplerate):
    """HighPassFilter's cut-off bin (postfilter/postfilter.cc:1206-1213): (unsigned)(M cutOffFreq/(float)sampleRate) in float32."""
    return int(np.float32(M) * np.float32(cut_off_freq) / np.float32(samplerate))


def spec_highpass(X, cutoff_bin, out=None):
    """Spectral high-pass (HighPassFilter::next, postfilter/postfilter.cc:1215-1239): X complex64 [S][K][T] (rows may be padded) ->
    Y with bins 0 .. cutoff_bin-1 zero (DC included: the reference never writes it) and the others copied.  cutoff_bin = 0, with
    which the reference writes outside its vector, copies every bin.  out may be X."""
    ts = _check(X, "X", torch.complex64, 3, rows=True)
    S, K, T = X.shape
    if out is None:
        out = rows_like(X, (S, K, T))
    elif _check(out, "out", torch.complex64, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "spec_highpass: out must share the row stride of X")
    check(_lib.lib().btk_spec_highpass(_ptr(X), _ptr(out), S, 2 * (K - 1), int(cutoff_bin), ts, T, _stream()))
    return out


# ---------------------------------------------------------------------------- binaural binary masks and threshold estimators
_BINAURAL_KINDS = {"kim": _lib.BTK_BINAURAL_KIM, "iid": _lib.BTK_BINAURAL_IID, "fdiid": _lib.BTK_BINAURAL_FDIID}
_BINAURAL_NV = {_lib.BTK_BINAURAL_KIM: 5, _lib.BTK_BINAURAL_IID: 6, _lib.BTK_BINAURAL_FDIID: 3}


def _binaural_kind(kind):
    k = _BINAURAL_KINDS.get(kind.lower()) if isinstance(kind, str) else (int(kind) if int(kind) in _BINAURAL_NV else None)
    if k is None:
        raise ValueError("binaural kind %r: 'kim', 'iid' or 'fdiid'" % (kind,))
    return k


def _binaural_pair(XL, XR, who):
    ts = _check(XL, "XL", torch.complex64, 3, rows=True)
    S, K, T = XL.shape
    if K < 2 or 2 * (K - 1) > 2048:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s: %d bins, 2 .. 1025 (M <= 2048) are supported" % (who, K))
    if _check(XR, "XR", torch.complex64, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s: XL and XR must share one row stride" % who)
    return ts, S, K, T


def binaural_mask_state(S, M, device="cuda"):
    """prevMu_ of S binary-mask filters (BinaryMaskFilter's constructor, postfilter/binauralprocessing.cc:71-72): float32 [S][K] of
    ones.  reset() of the filters leaves it as it is."""
    return torch.ones((int(S), int(M) // 2 + 1), dtype=torch.float32, device=torch.device(device))


def binaural_mask(XL, XR, kind, chan, threshold, alpha, eta, state=None, thresholds=None, frames_done=0, out=None):
    """Binary mask over a block (KimBinaryMaskFilter::masking1 / IIDBinaryMaskFilter::masking1, :138-179, :441-485): XL, XR
    complex64 [S][K][T] (rows may be padded) -> Y [S][K][T] = mu X with X = XR if chan else XL and
    mu_t = alpha mu_{t-1} + (1 - alpha) b_t, b_t in {1, eta}; bin 0 is XL's.  kind 'kim': b_t = 1 where the interaural time delay
    is <= threshold (chan 0; the opposite for chan 1); 'iid': b_t = eta where |X_T| <= |X_I| + threshold.  thresholds: float [K],
    one per bin, for 'iid' (Kim ignores it, as the reference does).  state: binaural_mask_state(), updated in place (None: ones);
    frames_done: frames the stream produced before this block, which places the 64-frame scan chunks."""
    kd = _binaural_kind(kind)
    if kd == _lib.BTK_BINAURAL_FDIID:
        raise ValueError("binaural_mask: 'kim' or 'iid'")
    ts, S, K, T = _binaural_pair(XL, XR, "binaural_mask")
    if int(chan) not in (0, 1):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "binaural_mask: chan=%r, 0 or 1" % (chan,))
    if state is None:
        state = binaural_mask_state(S, 2 * (K - 1), XL.device)
    _check(state, "state", torch.float32, (S, K))
    if thresholds is not None:
        if not torch.is_tensor(thresholds):
            thresholds = torch.from_numpy(np.ascontiguousarray(thresholds, dtype=np.float32)).to(XL.device)
        _check(thresholds, "thresholds", torch.float32, (K,))
    if out is None:
        out = rows_like(XL, (S, K, T))
    elif _check(out, "out", torch.complex64, (S, K, T), rows=True) != ts:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "binaural_mask: out must share the row stride of XL")
    check(_lib.lib().btk_binaural_mask(_ptr(XL), _ptr(XR), _ptr(out), S, 2 * (K - 1), ts, T, kd, int(chan), float(threshold),
                                       None if thresholds is None else _ptr(thresholds), float(alpha), float(eta),
                                       int(frames_done), _ptr(state), _stream()))
    return out


def binaural_candidates(min, max, width):
    """The threshold candidates as the estimators walk them (`for(float t=min;t<=max;t+=width)`, :321) and the size nCand_ of their
    arrays, (int)((max-min)/width + 1.5) (:270): (float32 array, nCand).  The walk can be shorter than nCand ((0, 2, 0.1): 20 and
    21); one that is longer, with which the reference writes past its arrays, is cut at nCand."""
    n_walk, n_cand = C.c_int(0), C.c_int(0)
    L = _lib.lib()
    check(L.btk_binaural_candidates(float(min), float(max), float(width), None, 0, C.byref(n_walk), C.byref(n_cand)))
    out = np.zeros(n_walk.value, np.float32)
    check(L.btk_binaural_candidates(float(min), float(max), float(width), _np_ptr(out), out.size, C.byref(n_walk), C.byref(n_cand)))
    return out, n_cand.value


class BinauralStatsState:
    """Sums of S threshold estimators, float64: 'kim' [S][nCand][5] (sums of R_T R_I, R_T, R_I, R_T^2, R_I^2), 'iid' [S][nCand][6]
    (Y1, Y2, Y4 of the target, then of the interferer), 'fdiid' [S][K][nCand][3] (Y4, mean, sigma); count int64 [S] frames."""

    def __init__(self, kind, S, M, n_cand, device="cuda"):
        self.kind, self.S, self.M, self.Kb, self.n_cand = _binaural_kind(kind), int(S), int(M), int(M) // 2 + 1, int(n_cand)
        if self.S < 1 or self.M < 2 or self.M % 2 or self.M > 2048:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "BinauralStatsState: S=%d M=%d" % (S, M))
        if not 1 <= self.n_cand <= _lib.lib().btk_binaural_max_candidates():
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "BinauralStatsState: %d candidates" % n_cand)
        nv = _BINAURAL_NV[self.kind]
        shape = (self.S, self.Kb, self.n_cand, nv) if self.kind == _lib.BTK_BINAURAL_FDIID else (self.S, self.n_cand, nv)
        self.sums = torch.zeros(shape, dtype=torch.float64, device=torch.device(device))
        self.count = torch.zeros((self.S,), dtype=torch.int64, device=torch.device(device))

    def clear(self):
        """reset() of the estimators (:409-426): the sums and the frame count go."""
        self.sums.zero_()
        self.count.zero_()


def _binaural_cands(cands):
    """(float32 walk, nCand) from binaural_candidates()'s pair or from a plain sequence (nCand = its length)."""
    if isinstance(cands, tuple) and len(cands) == 2 and np.ndim(cands[0]) == 1:
        walk, n_cand = np.ascontiguousarray(cands[0], dtype=np.float32), int(cands[1])
    else:
        walk = np.ascontiguousarray(cands, dtype=np.float32).reshape(-1)
        n_cand = walk.size
    if n_cand < 1 or walk.size > n_cand:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "binaural: %d candidates for %d slots" % (walk.size, n_cand))
    return walk, n_cand


def binaural_stats(XL, XR, kind, cands, eta, power_coeff, fbin_min, fbin_max, state=None, per_frame=False):
    """Adds the frames of a block to the sums of the threshold estimators (accumStats1 of KimITDThresholdEstimator,
    IIDThresholdEstimator, FDIIDThresholdEstimator, :314-353, :548-603, :794-838): XL (target), XR (interferer) complex64
    [S][K][T], rows may be padded.  cands: binaural_candidates()'s pair or a sequence of thresholds; bins [fbin_min, fbin_max)
    ('fdiid': always 1 .. M/2).  Returns the state (a new one without `state`); with per_frame=True also the terms of every
    (frame, candidate), float64 [S][T][nCand][2] = R_T, R_I ('kim') or [S][T][nCand][6] = the frame's Y1, Y2, Y4 of target and
    interferer ('iid')."""
    kd = _binaural_kind(kind)
    ts, S, K, T = _binaural_pair(XL, XR, "binaural_stats")
    M = 2 * (K - 1)
    walk, n_cand = _binaural_cands(cands)
    if state is None:
        state = BinauralStatsState(kd, S, M, n_cand, XL.device)
    if (state.kind, state.S, state.M, state.n_cand) != (kd, S, M, n_cand):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "binaural_stats: the state is for kind %d, S=%d, M=%d, %d candidates"
                            % (state.kind, state.S, state.M, state.n_cand))
    if kd != _lib.BTK_BINAURAL_FDIID and not 0 <= int(fbin_min) <= int(fbin_max) <= K:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "binaural_stats: bins [%d, %d) outside 0 .. %d" % (fbin_min, fbin_max, K))
    L = _lib.lib()
    pf = None
    if per_frame:
        if kd == _lib.BTK_BINAURAL_FDIID:
            raise ValueError("binaural_stats: no per-frame terms for 'fdiid'")
        pf = torch.zeros((S, T, n_cand, 2 if kd == _lib.BTK_BINAURAL_KIM else 6), dtype=torch.float64, device=XL.device)
    dc = torch.from_numpy(walk if walk.size else np.zeros(1, np.float32)).to(XL.device)
    nbytes = L.btk_binaural_stats_scratch_bytes(kd, S, T, n_cand)
    scratch = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=XL.device)
    check(L.btk_binaural_stats(_ptr(XL), _ptr(XR), S, M, ts, T, kd, _ptr(dc), walk.size, n_cand, float(eta), float(power_coeff),
                               int(fbin_min), int(fbin_max), _ptr(state.sums), _ptr(state.count),
                               None if pf is None else _ptr(pf), _ptr(scratch), scratch.numel() * 8, _stream()))
    return (state, pf) if per_frame else state


def binaural_threshold(kind, state, cands, stream=0, beta=3.0):
    """calc_threshold of the three estimators (:382-407, :632-660, :867-898) on the sums of one stream: 'kim' minimises the absolute
    correlation coefficient, 'iid' and 'fdiid' maximise the kurtosis-like cost with beta = 3; ties: the first candidate for 'kim'
    and 'iid', the last for 'fdiid'.  Returns (threshold, cost [nCand]) or, for 'fdiid', (threshold, cost [K][nCand], per-bin
    thresholds [K]).  The sums are left as they are."""
    kd = _binaural_kind(kind)
    walk, n_cand = _binaural_cands(cands)
    if state.kind != kd or state.n_cand != n_cand:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "binaural_threshold: the state is for kind %d with %d candidates" % (state.kind, state.n_cand))
    sums = np.ascontiguousarray(state.sums[int(stream)].cpu().numpy())
    count = int(state.count[int(stream)].item())
    fd = kd == _lib.BTK_BINAURAL_FDIID
    cost = np.zeros((state.Kb, n_cand) if fd else (n_cand,), np.float64)
    per_bin = np.zeros(state.Kb, np.float64)
    thr = C.c_double(0.0)
    w = walk if walk.size else np.zeros(1, np.float32)
    check(_lib.lib().btk_binaural_threshold(kd, state.M, n_cand, walk.size, _np_ptr(w), _np_ptr(sums), count, float(beta),
                                            C.byref(thr), _np_ptr(cost), _np_ptr(per_bin)))
    return (thr.value, cost, per_bin) if fd else (thr.value, cost)


# ---------------------------------------------------------------------------- voice activity detection (csrc/vad_kernels.hip)
_VAD_KINDS = {"power": _lib.BTK_VAD_POWER, "normalized": _lib.BTK_VAD_NORMALIZED, "tsps": _lib.BTK_VAD_TSPS}
_VAD_RULES = {"single": _lib.BTK_VAD_RULE_SINGLE, "mi": _lib.BTK_VAD_RULE_MI, "multistage": _lib.BTK_VAD_RULE_MULTISTAGE}
_VAD_E0 = {_lib.BTK_VAD_POWER: 1.0, _lib.BTK_VAD_NORMALIZED: 1.0, _lib.BTK_VAD_TSPS: 5000.0}     # sad.cc:673, :767, :999


def vad_frame_energy(x, frame_len=None, shift=None, layout=None):
    """Frame energies sum_n |x[n]|^2, float64 in index order (EnergyVADMetric::above_threshold_, sad.cc:520-524; for complex input
    re^2 + im^2 per element, SimpleEnergyVAD::next :165-167) -> float64 [S][T].  The blocks are read as their producers leave
    them: layout 'rows' [S][D][T] (the snapshot layout, the default for complex64; rows may be padded), 'frames' [S][T][D] (the
    default for float32), or PCM float32 [S][L] with frame_len and shift (T = (L - frame_len) // shift + 1 whole frames)."""
    if x.dim() == 2:
        _check(x, "x", torch.float32, 2)
        if frame_len is None:
            raise ValueError("vad_frame_energy: PCM needs frame_len")
        S, L = x.shape
        D, sh = int(frame_len), int(frame_len if shift is None else shift)
        if D < 1 or sh < 1:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "vad_frame_energy: frame_len=%d shift=%d" % (D, sh))
        T = (L - D) // sh + 1 if L >= D else 0
        cplx, strides = 0, (L, sh, 1)
    else:
        cplx = 1 if x.dtype == torch.complex64 else 0
        layout = layout or ("rows" if cplx else "frames")
        if layout == "rows":
            ts = _check(x, "x", x.dtype if cplx else torch.float32, 3, rows=True)
            S, D, T = x.shape
            strides = (D * ts, 1, ts)
        elif layout == "frames":
            _check(x, "x", x.dtype if cplx else torch.float32, 3)
            S, T, D = x.shape
            strides = (T * D, D, 1)
        else:
            raise ValueError("vad_frame_energy: layout %r: 'rows' or 'frames'" % (layout,))
    e = torch.empty((S, T), dtype=torch.float64, device=x.device)
    if T == 0:
        return e
    check(_lib.lib().btk_vad_frame_energy(_ptr(x), cplx, S, D, T, strides[0], strides[1], strides[2], _ptr(e), max(T, 1), _stream()))
    return e


def vad_band_limits(fftLen, samplerate, low_cutoff=-1.0, high_cutoff=-1.0):
    """(lowX, highX, binN) of MultiChannelVADMetric (sad.cc:629-663); a cutoff >= samplerate / 2 raises BTK_ERR_DIMENSION."""
    lo, hi, n = C.c_int(0), C.c_int(0), C.c_int(0)
    check(_lib.lib().btk_vad_band_limits(int(fftLen), float(samplerate), float(low_cutoff), float(high_cutoff), C.byref(lo),
                                         C.byref(hi), C.byref(n)))
    return lo.value, hi.value, n.value


def vad_band_power(spec, kind, fftLen, lowX, highX, E0=None):
    """Band powers and decisions of PowerSpectrumVADMetric / NormalizedEnergyMetric / TSPSVADMetric::next (sad.cc:694-739, :777-830,
    :1005-1057): spec float32 [S][C][T][powN] power spectra, channel 0 the target's -> (P float64 [S][C][T], score float64 [S][T],
    value float64 [S][T] = +-1).  kind 'power', 'normalized' or 'tsps'; E0 defaults to the reference's 1, 1, 5000."""
    kd = _VAD_KINDS.get(kind) if isinstance(kind, str) else int(kind)
    if kd not in _VAD_E0:
        raise ValueError("vad_band_power: kind %r: 'power', 'normalized' or 'tsps'" % (kind,))
    _check(spec, "spec", torch.float32, 4)
    S, Cn, T, powN = spec.shape
    if int(highX) >= powN:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "vad_band_power: bin %d of spectra of %d values" % (highX, powN))
    P = torch.empty((S, Cn, T), dtype=torch.float64, device=spec.device)
    score = torch.empty((S, T), dtype=torch.float64, device=spec.device)
    value = torch.empty((S, T), dtype=torch.float64, device=spec.device)
    if T == 0:
        return P, score, value
    check(_lib.lib().btk_vad_band_power(_ptr(spec), kd, S, Cn, int(fftLen), T, Cn * T * powN, T * powN, powN, 1, int(lowX),
                                        int(highX), float(_VAD_E0[kd] if E0 is None else E0), _ptr(P), _ptr(score), _ptr(value),
                                        max(T, 1), _stream()))
    return P, score, value


class EnergyVADState:
    """State of S EnergyVADMetric (sad.cc:472-506): int64 [S][4 + energiesN] = {ring position, recognizing, abovethresholdN,
    belowThresholdN}, then the float64 window of the last energiesN energies as a ring, filled with initialEnergy."""

    def __init__(self, S, energiesN, initial_energy, device="cuda"):
        self.S, self.energiesN, self.initial_energy = int(S), int(energiesN), float(initial_energy)
        if self.S < 1 or _lib.lib().btk_vad_energy_metric_state_bytes(self.energiesN) < 0:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "EnergyVADState: S=%d energiesN=%d (1 .. 1024)" % (S, energiesN))
        self.buf = torch.zeros((self.S, 4 + self.energiesN), dtype=torch.int64, device=torch.device(device))
        self.next_speaker()

    def reset(self):
        """EnergyVADMetric::reset (:493-497): the counters go, the window stays."""
        self.buf[:, 1:4] = 0

    def next_speaker(self):
        """EnergyVADMetric::next_speaker (:499-506): the counters go and the window is initialEnergy again."""
        self.buf[:, :4] = 0
        self.buf[:, 4:] = torch.tensor([self.initial_energy], dtype=torch.float64).view(torch.int64).item()

    def window(self):
        """The windows, oldest energy first: float64 numpy [S][energiesN]."""
        b = self.buf.cpu()
        ring = b[:, 4:].contiguous().view(torch.float64).numpy()
        return np.stack([np.roll(ring[s], -int(b[s, 0])) for s in range(self.S)])

    def energy_percentile(self, percentile, s=0):
        """EnergyVADMetric::energy_percentile (:544-553), the division by energiesN included."""
        if percentile < 0.0 or percentile > 100.0:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "Percentile %g is out of range [0.0, 100.0]." % percentile)
        x = int((percentile / 100.0) * self.energiesN)
        if x >= self.energiesN:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "Percentile %g reads past the window" % percentile)
        return float(np.sort(self.window()[s])[x]) / self.energiesN


def vad_median_index(threshold, energiesN):
    """medianX_ = unsigned(threshold energiesN) (sad.cc:477); an index outside the window (threshold >= 1, where the reference
    reads past its array, or a negative threshold) raises BTK_ERR_DIMENSION."""
    v = float(threshold) * int(energiesN)
    if not (0.0 <= v) or int(v) >= int(energiesN):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "EnergyVADMetric: threshold %g puts the median index outside 0 .. %d"
                            % (threshold, int(energiesN) - 1))
    return int(v)


def vad_energy_metric(energy, state, threshold, headN, tailN):
    """EnergyVADMetric::next over a block (sad.cc:518-588): energy float64 [S][T] -> float64 [S][T] of 1.0 / 0.0; state (an
    EnergyVADState) is carried on, so blocks cut anywhere give the bits of one call."""
    _check(energy, "energy", torch.float64, (state.S, None))
    S, T = energy.shape
    mx = vad_median_index(threshold, state.energiesN)
    value = torch.empty((S, T), dtype=torch.float64, device=energy.device)
    if T == 0:
        return value
    check(_lib.lib().btk_vad_energy_metric(_ptr(energy), max(T, 1), S, T, state.energiesN, mx, int(headN), int(tailN),
                                           _ptr(state.buf), _ptr(value), max(T, 1), _stream()))
    return value


class SimpleEnergyVADState:
    """spectral_energy_ of S SimpleEnergyVAD (sad.cc:140-152): float64 [S], 0 at the start and after next_speaker()."""

    def __init__(self, S, device="cuda"):
        self.S = int(S)
        self.s = torch.zeros((self.S,), dtype=torch.float64, device=torch.device(device))

    def next_speaker(self):
        self.s.zero_()


def vad_simple_energy(energy, state, threshold, gamma):
    """SimpleEnergyVAD::next over a block (sad.cc:165-171): energy float64 [S][T] (vad_frame_energy of the complex frames) ->
    (is_speech int32 [S][T], smoothed float64 [S][T]); s <- gamma s + (1 - gamma) E, is_speech = E / s > threshold."""
    _check(energy, "energy", torch.float64, (state.S, None))
    S, T = energy.shape
    sp = torch.empty((S, T), dtype=torch.int32, device=energy.device)
    sm = torch.empty((S, T), dtype=torch.float64, device=energy.device)
    if T == 0:
        return sp, sm
    check(_lib.lib().btk_vad_simple_energy(_ptr(energy), max(T, 1), S, T, float(gamma), float(threshold), _ptr(state.s), _ptr(sp),
                                           _ptr(sm), max(T, 1), _stream()))
    return sp, sm


class HangoverState:
    """State of S hangover machines (HangoverVADFeature, sad.cc:1712-1761): int64 [S][8] = {abovethresholdN, belowThresholdN,
    recognizing, frames seen, start, end, ended, decision_metric}; start / end are -1 until they are known."""

    def __init__(self, S, device="cuda"):
        self.S = int(S)
        self.buf = torch.empty((self.S, 8), dtype=torch.int64, device=torch.device(device))
        self.reset()

    def reset(self):
        self.buf[:] = torch.tensor([0, 0, 0, 0, -1, -1, 0, 0], dtype=torch.int64)

    def host(self):
        """Downloaded: a list of dicts with start (prefixN()), end, ended, recognizing, frames, decision_metric per stream."""
        b = self.buf.cpu().numpy()
        return [dict(start=int(r[4]), end=int(r[5]), ended=bool(r[6]), recognizing=bool(r[2]), frames=int(r[3]),
                     decision_metric=int(r[7])) for r in b]


def vad_hangover(values, thresholds, rule, headN, tailN, state, restart=False):
    """The detection rule and head/tail machine of HangoverVADFeature / HangoverMIVADFeature / HangoverMultiStageVADFeature
    (sad.cc:1763-1843, :1859-1885, :1910-1951) over a block: values a list of up to 8 float64 [S][T] metric rows (or one tensor
    [R][S][T]), thresholds one per row, rule 'single', 'mi' or 'multistage'.  Returns (decision int32 [S][T], segments int64
    [S][n][2], nseg int32 [S]): the decision_metric() code after each frame and the (start, end) pairs completed in this block;
    the segment found so far is in state.host().  restart: go on after an end and yield every segment."""
    rl = _VAD_RULES.get(rule) if isinstance(rule, str) else int(rule)
    if rl not in (0, 1, 2):
        raise ValueError("vad_hangover: rule %r: 'single', 'mi' or 'multistage'" % (rule,))
    rows = [values[i] for i in range(len(values))]
    R = len(rows)
    if not 1 <= R <= 8 or len(thresholds) != R:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "vad_hangover: %d metric rows (1 .. 8), %d thresholds" % (R, len(thresholds)))
    for i, v in enumerate(rows):
        _check(v, "values[%d]" % i, torch.float64, (state.S, rows[0].shape[-1]))
    S, T = rows[0].shape
    if int(headN) < 1 or int(tailN) < 0:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "vad_hangover: headN=%d (>= 1; the reference divides by it), tailN=%d" % (headN, tailN))
    dev = rows[0].device
    max_seg = T // 2 + 1
    decision = torch.empty((S, T), dtype=torch.int32, device=dev)
    segments = torch.full((S, max_seg, 2), -1, dtype=torch.int64, device=dev)
    nseg = torch.zeros((S,), dtype=torch.int32, device=dev)
    if T == 0:
        return decision, segments, nseg
    ptrs = (C.c_void_p * R)(*[v.data_ptr() for v in rows])
    thr = (C.c_double * R)(*[float(t) for t in thresholds])
    check(_lib.lib().btk_vad_hangover(ptrs, thr, R, rl, S, T, max(T, 1), int(headN), int(tailN), 1 if restart else 0,
                                      _ptr(state.buf), _ptr(decision), max(T, 1), _ptr(segments), max_seg, _ptr(nseg), _stream()))
    return decision, segments, nseg


def vad_gather(src, state, frame_base=0, out=None, dst_rows=None):
    """Source rows [start, end) of the hangover state's segment that lie in src float32 [S][T][D] (row 0 is frame frame_base) ->
    (out float32 [S][dst_rows][D] with the rows at (frame - start), count int64 [S] rows copied by this call)."""
    _check(src, "src", torch.float32, (state.S, None, None))
    S, T, D = src.shape
    if out is None:
        out = torch.zeros((S, int(T if dst_rows is None else dst_rows), D), dtype=torch.float32, device=src.device)
    _check(out, "out", torch.float32, (S, None, D))
    count = torch.zeros((S,), dtype=torch.int64, device=src.device)
    if T == 0 or out.shape[1] == 0:
        return out, count
    check(_lib.lib().btk_vad_gather(_ptr(src), S, T, D, int(frame_base), _ptr(state.buf), _ptr(out), out.shape[1], _ptr(count),
                                    _stream()))
    return out, count


def vad_segments_to_labels(segments, shiftlen, samplerate):
    """Frame segments [(start, end), ...] (end exclusive, ascending, as vad_hangover yields them) as the `vad_label` list
    [[start_s, end_s], ...] that accu_stats_from_label walks (lib/pybeamformer.py:967-985): that loop adds shiftlen / samplerate
    frame by frame and takes a frame as target where start_s <= elapsed <= end_s, so the times are the loop's own sums at frames
    start and end - 1 -- a frame is a target exactly when it lies in a segment."""
    segs = [(int(a), int(b)) for a, b in segments if int(b) > int(a)]
    if not segs:
        return []
    time_delta = int(shiftlen) / float(samplerate)
    elapsed = np.zeros(max(b for _, b in segs), np.float64)
    for t in range(1, elapsed.size):
        elapsed[t] = elapsed[t - 1] + time_delta
    return [[float(elapsed[a]), float(elapsed[b - 1])] for a, b in segs]


# ---------------------------------------------------------------------------- covariance accumulation
def frame_energy(X, M):
    _need_cuda(X, "X")
    S, K, N, T = X.shape
    e = torch.empty((S, T), dtype=torch.float32, device=X.device)
    check(_lib.lib().btk_frame_energy(_ptr(X), S, M, N, T, T, _ptr(e), T, _stream()))
    return e


def cov_frame_gate(energy, label, threshold, count=None):
    """w = (energy > threshold) * label; returns (w [S][T], count [S])."""
    S, T = energy.shape
    w = torch.empty_like(energy)
    if count is None:
        count = torch.zeros(S, dtype=torch.float32, device=energy.device)
    check(_lib.lib().btk_cov_frame_gate(_ptr(energy), None if label is None else _ptr(label), S, T, T, float(threshold),
                                        _ptr(w), _ptr(count), _stream()))
    return w, count


def cov_accumulate(X, R=None, tf_weights=None, frame_weights=None, use_mfma=True):
    """R[s][k] += sum_t tf[s][k][t] fw[s][t] x x^H.  X [S][K][N][T] -> R complex64 [S][K][N][N].  X may be a row-padded view
    (analysis(pad_rows=True)); the per-frame weights, if any, then need the same row stride (rows_like(X, ...))."""
    ts = _check(X, "X", torch.complex64, 4, rows=True)
    S, K, N, T = X.shape
    if R is None:
        R = torch.zeros((S, K, N, N), dtype=torch.complex64, device=X.device)
    _check(R, "R", torch.complex64, (S, K, N, N))
    for w, name, shape in ((tf_weights, "tf_weights", (S, K, T)), (frame_weights, "frame_weights", (S, T))):
        if w is not None and _check(w, name, torch.float32, shape, rows=True) != ts:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s rows are %d frames apart, X rows %d: they share T_stride" % (name, w.stride(-2), ts))
    check(_lib.lib().btk_cov_accumulate(_ptr(X), None if tf_weights is None else _ptr(tf_weights),
                                        None if frame_weights is None else _ptr(frame_weights), _ptr(R),
                                        S, K, N, ts, T, int(use_mfma), _stream()))
    return R


def cov_scale(R, a):
    """R <- float32(a * float64(R)) in place: the decay step of a recursion R <- a R + sum_t w x x^H kept on the device."""
    _check(R, "R", torch.complex64, 4)
    S, K, N, _ = R.shape
    _check(R, "R", torch.complex64, (S, K, N, N))
    check(_lib.lib().btk_cov_scale(_ptr(R), float(a), S, K, N, _stream()))
    return R


def cov_finalize(R, count, gamma=0.0):
    S, K, N, _ = R.shape
    per_bin = int(count.dim() == 2)
    check(_lib.lib().btk_cov_finalize(_ptr(R), _ptr(count), per_bin, S, K, N, float(gamma), _stream()))
    return R


def cov_mask_count(tf_weights, frame_weights=None, count=None):
    """count[s][k] += sum_t trunc(tf[s][k][t]) fw[s][t]  (integer per-bin counters of accu_stats_from_tfmask)."""
    _need_cuda(tf_weights, "tf_weights")
    S, K, T = tf_weights.shape
    if count is None:
        count = torch.zeros((S, K), dtype=torch.float32, device=tf_weights.device)
    check(_lib.lib().btk_cov_mask_count(_ptr(tf_weights), None if frame_weights is None else _ptr(frame_weights), S, K, T, T,
                                        _ptr(count), _stream()))
    return count


def cov_trace_normalize(R):
    N = R.shape[-1]
    check(_lib.lib().btk_cov_trace_normalize(_ptr(R), int(np.prod(R.shape[:-2])), N, _stream()))
    return R


def _sos_weights(which, Rt, Rn, *args):
    _need_cuda(Rt, "Rt"); _need_cuda(Rn, "Rn")
    K, N, _ = Rt.shape
    if Rn.shape != Rt.shape or Rt.dtype != torch.complex64 or Rn.dtype != torch.complex64:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "covariance matrices must both be complex64 [K][N][N]")
    L = _lib.lib()
    W = torch.empty((K, N), dtype=torch.complex64, device=Rt.device)
    scratch = torch.empty(L.btk_sos_scratch_bytes(K, N), dtype=torch.uint8, device=Rt.device)
    fail = torch.zeros(1, dtype=torch.int32, device=Rt.device)
    Rt, Rn = Rt.contiguous(), Rn.contiguous()
    if which == "bmvdr":
        check(L.btk_bmvdr_weights(_ptr(Rt), _ptr(Rn), K, N, int(args[0]), float(args[1]), _ptr(W), _ptr(scratch), _ptr(fail),
                                  _stream()))
    else:
        check(L.btk_gev_weights(_ptr(Rt), _ptr(Rn), K, N, _ptr(W), _ptr(scratch), _ptr(fail), _stream()))
    return W, int(fail.item())


def bmvdr_weights(Rt, Rn, ref_micx=0, offset=0.0):
    """Blind MVDR: wqH [K][N] complex64 (cuda) and the number of bins whose noise covariance is not positive definite."""
    return _sos_weights("bmvdr", Rt, Rn, ref_micx, offset)


def gev_weights(Rt, Rn):
    """GEV: wqH [K][N] complex64 (cuda), equal to the reference's up to one global sign; and the failure count."""
    return _sos_weights("gev", Rt, Rn)


# ---------------------------------------------------------------------------- MVDR weight design
def mvdr_diffuse_model(mpos, M, samplerate, sspeed=343740.0, device=None):
    mp = torch.as_tensor(np.ascontiguousarray(mpos, np.float32)).to(device)
    N = mp.shape[0]
    if mp.shape[1] < 3:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "The microphone positions should be described in the three dimensions")
    R = torch.empty((M // 2 + 1, N, N), dtype=torch.complex64, device=mp.device)
    check(_lib.lib().btk_mvdr_diffuse_model(_ptr(mp), N, M, float(samplerate), float(sspeed), _ptr(R), _stream()))
    return R


def mvdr_diagonal_loading(R, weight):
    nb, N = R.shape[-3], R.shape[-1]
    nb = int(np.prod(R.shape[:-2]))
    check(_lib.lib().btk_mvdr_diagonal_loading(_ptr(R), nb, N, float(weight), _stream()))
    return R


SVD_RULES = ("linpack", "exact", "linpack_full")


def svd_rule_default():
    """The rule that decides where pseudoinverse() 'fails' and the identity replaces inv(R_k) (beamformer.cc:253-270, 2379-2384):
    "linpack" (default) takes the decision of the reference's float32 csvdc, rounding for rounding -- INFO != 0 or a singular
    value under the threshold -- so a design matches the reference bin for bin (on BASELINE config C5 that is delay-and-sum on
    about half the spectrum); "exact" solves every positive definite bin and uses the identity only where a singular value is
    really below the threshold; "linpack_full" computes the reference's weights themselves: csvdc with its singular vectors,
    the pseudo-inverse A+ = V S^-1 U^H assembled in the source's order and the float64 weight step on it, the identity where
    pseudoinverse() returns false (no Cholesky solve, no fall-back; up to 256 channels).  BTK_MVDR_SVD_RULE overrides the default."""
    rule = os.environ.get("BTK_MVDR_SVD_RULE", "linpack")
    if rule not in SVD_RULES:
        raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "BTK_MVDR_SVD_RULE must be one of %s, got %r" % (SVD_RULES, rule))
    return rule


def csvdc_values(A):
    """LINPACK's float32 csvdc with job = 0 (matrix/linpack_c.cc:9516) for a batch: A complex64 [K][n][p] (cuda) ->
    (s float32 [K][m], e float32 [K][m], info int32 [K]), m = min(n + 1, p); bit-identical to the reference's compiled routine."""
    _check(A, "A", torch.complex64, 3)
    K, n, p = A.shape
    m = min(n + 1, p)
    s = torch.zeros((K, m), dtype=torch.float32, device=A.device)
    e = torch.zeros((K, m), dtype=torch.float32, device=A.device)
    info = torch.zeros((K,), dtype=torch.int32, device=A.device)
    if K > 0:
        sb = _lib.lib().btk_csvdc_scratch_bytes(K, n, p)
        scratch = torch.empty((sb,), dtype=torch.uint8, device=A.device) if sb else None
        check(_lib.lib().btk_csvdc_values(_ptr(A), K, n, p, _ptr(s), _ptr(e), _ptr(info), None if scratch is None else _ptr(scratch),
                                          _stream()))
    return s, e, info


def _linpack_rule(R, wq, W, lam, KS, N, first_bin, kper, skip_dc, threshold, flags):
    """btk_mvdr_linpack_rule on the current stream; returns the device counters [INFO != 0, singular value < threshold]."""
    counts = torch.zeros(2, dtype=torch.int32, device=R.device)
    scratch = torch.empty((_lib.lib().btk_mvdr_linpack_rule_scratch_bytes(KS, N),), dtype=torch.uint8, device=R.device)
    check(_lib.lib().btk_mvdr_linpack_rule(_ptr(R), _ptr(wq), None if W is None else _ptr(W), None if lam is None else _ptr(lam),
                                           KS, N, int(first_bin), int(kper), int(skip_dc), float(threshold),
                                           None if flags is None else _ptr(flags), _ptr(counts), _ptr(scratch), _stream()))
    return counts


def csvdc_full(A):
    """LINPACK's float32 csvdc with job = 11 (matrix/linpack_c.cc:9516) for a batch: A complex64 [K][n][p] (cuda) ->
    (s float32 [K][m], e float32 [K][m], U complex64 [K][n][n], V complex64 [K][p][p], info int32 [K]), m = min(n + 1, p);
    U[k, i, j] / V[k, i, j] are the reference's u[i + j * ldu] / v[i + j * ldv] (the tensors are views of column-major storage).
    Bit-identical to the reference's compiled routine; n, p <= 256."""
    _check(A, "A", torch.complex64, 3)
    K, n, p = A.shape
    m = min(n + 1, p)
    s = torch.zeros((K, m), dtype=torch.float32, device=A.device)
    e = torch.zeros((K, m), dtype=torch.float32, device=A.device)
    U = torch.zeros((K, n, n), dtype=torch.complex64, device=A.device)
    V = torch.zeros((K, p, p), dtype=torch.complex64, device=A.device)
    info = torch.zeros((K,), dtype=torch.int32, device=A.device)
    if K > 0:
        scratch = torch.empty((max(_lib.lib().btk_csvdc_full_scratch_bytes(K, n, p), 16),), dtype=torch.uint8, device=A.device)
        check(_lib.lib().btk_csvdc_full(_ptr(A), K, n, p, _ptr(s), _ptr(e), _ptr(U), _ptr(V), _ptr(info), _ptr(scratch), _stream()))
    return s, e, U.transpose(1, 2), V.transpose(1, 2), info


def pinv_linpack(A, threshold=1.0e-8):
    """pseudoinverse() (beamformer/beamformer.cc:232-289) for a batch on the device, the reference's own float32 arithmetic:
    A complex64 [K][M][N] (cuda), M >= N -> (invA complex64 [K][N][M], ok bool [K] -- its return value --, info int32 [K])."""
    _check(A, "A", torch.complex64, 3)
    K, M, N = A.shape
    invA = torch.zeros((K, N, M), dtype=torch.complex64, device=A.device)
    ok = torch.zeros((K,), dtype=torch.int32, device=A.device)
    info = torch.zeros((K,), dtype=torch.int32, device=A.device)
    if M < N:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "pinv_linpack: pseudoinverse() is defined for M >= N, got %d x %d" % (M, N))
    if K > 0:
        scratch = torch.empty((max(_lib.lib().btk_pinv_linpack_scratch_bytes(K, M, N), 16),), dtype=torch.uint8, device=A.device)
        check(_lib.lib().btk_pinv_linpack(_ptr(A), K, M, N, float(threshold), _ptr(invA), _ptr(ok), _ptr(info), _ptr(scratch), _stream()))
    return invA, ok != 0, info


def _linpack_full(R, wq, W, lam, KS, N, first_bin, kper, skip_dc, threshold):
    """btk_mvdr_linpack_full on the current stream; returns the device counters [INFO != 0, singular value < threshold]."""
    counts = torch.zeros(2, dtype=torch.int32, device=R.device)
    scratch = torch.empty((_lib.lib().btk_mvdr_linpack_full_scratch_bytes(KS, N),), dtype=torch.uint8, device=R.device)
    check(_lib.lib().btk_mvdr_linpack_full(_ptr(R), _ptr(wq), None if W is None else _ptr(W), None if lam is None else _ptr(lam),
                                           KS, N, int(first_bin), int(kper), int(skip_dc), float(threshold), _ptr(counts),
                                           _ptr(scratch), _stream()))
    return counts


def mvdr_weights(R, wq, threshold=1.0e-8, first_bin=0, svd_rule=None):
    """R complex64 [K][N][N], wq complex64 [K][N] (cuda) -> (W [K][N], number of bins that ended with the identity).
    first_bin: global index of row 0 when R / wq are one rank's bin range (only global bin 0 gets the all-ones weight).
    svd_rule (svd_rule_default() when None): with "linpack" the bins for which the reference's pseudoinverse() returns false --
    its float32 csvdc does not converge, or leaves a singular value under the threshold -- take the identity exactly as in
    calc_mvdr_weights (beamformer.cc:253-270, 2379-2396); every other bin keeps the Cholesky solution.  Bins whose Cholesky
    factorisation stops (R_k not positive definite) and that the rule did not already decide are re-solved through the
    pseudo-inverse (btk_mvdr_pinv_fallback).  mvdr_weights.last_counts = (INFO != 0, converged but under the threshold,
    identity from the fall-back) of the last call.  With "linpack_full" every bin takes the reference's own float32 SVD
    pseudo-inverse (or the identity where pseudoinverse() returns false) and the float64 weight step: no Cholesky, third count 0.
    S streams at once: R [S][K][N][N], wq [S][K][N] -> W [S][K][N] (btk_mvdr_weights_streams: one launch, every stream's bin 0
    gets the all-ones weight; first_bin must be 0)."""
    rule = svd_rule_default() if svd_rule is None else svd_rule
    if rule not in SVD_RULES:
        raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "svd_rule must be one of %s, got %r" % (SVD_RULES, rule))
    batched = R.dim() == 4
    if batched:
        _check(R, "R", torch.complex64, 4); _check(wq, "wq", torch.complex64, (R.shape[0], R.shape[1], R.shape[2]))
        if first_bin != 0:
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "mvdr_weights: stacked streams are whole bin ranges (first_bin = 0)")
        S, K, N, N2 = R.shape
    else:
        _check(R, "R", torch.complex64, 3); _check(wq, "wq", torch.complex64, (R.shape[0], R.shape[1]))
        S = 1
        K, N, N2 = R.shape
    if N2 != N:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "R must be [K][N][N], got %s" % (tuple(R.shape),))
    W = torch.empty(tuple(wq.shape), dtype=torch.complex64, device=R.device)
    fb = torch.zeros(1, dtype=torch.int32, device=R.device)
    KS = K * S
    flags = torch.zeros(max(KS, 1), dtype=torch.int32, device=R.device)
    nident = 0
    mvdr_weights.last_counts = (0, 0, 0)
    if KS > 0 and rule == "linpack_full":
        R, wq = R.contiguous(), wq.contiguous()
        counts = _linpack_full(R, wq, W, None, KS, N, first_bin, K if batched else 0, 1, threshold)
        c0, c1 = (int(v) for v in counts.tolist())
        nident = c0 + c1
        mvdr_weights.last_counts = (c0, c1, 0)
    elif KS > 0:
        sb = _lib.lib().btk_mvdr_scratch_bytes(KS, N)
        scratch = torch.empty((sb,), dtype=torch.uint8, device=R.device) if sb else None
        sp = None if scratch is None else _ptr(scratch)
        if batched:
            check(_lib.lib().btk_mvdr_weights_streams(_ptr(R), _ptr(wq), _ptr(W), S, K, N, float(threshold), sp, _ptr(fb), _ptr(flags), _stream()))
        else:
            check(_lib.lib().btk_mvdr_weights_flags(_ptr(R), _ptr(wq), _ptr(W), K, N, int(first_bin), float(threshold), sp, _ptr(fb), _ptr(flags),
                                                    _stream()))
        c0 = c1 = 0
        if rule == "linpack":
            counts = _linpack_rule(R, wq, W, None, KS, N, first_bin, K if batched else 0, 1, threshold, flags)
            c0, c1 = (int(v) for v in counts.tolist())
        ni = C.c_int(0)
        if int(fb.item()) > 0 and (rule != "linpack" or int(flags.sum().item()) > 0):
            check(_lib.lib().btk_mvdr_pinv_fallback(_ptr(R), _ptr(wq), _ptr(W), KS, N, int(first_bin), float(threshold),
                                                    _ptr(flags), C.byref(ni), _stream()))
        nident = c0 + c1 + ni.value
        mvdr_weights.last_counts = (c0, c1, ni.value)
    return W, nident


mvdr_weights.last_counts = (0, 0, 0)


def mvdr_divide_nondiagonal(R, mu):
    """divide_all_nondiagonal_elements (beamformer.h:357-362): R_xy /= 1 + mu for x != y, in place; R complex64 [K][N][N]."""
    _check(R, "R", torch.complex64, 3)
    K, N, _ = R.shape
    if K > 0:
        check(_lib.lib().btk_mvdr_divide_nondiagonal(_ptr(R), K, N, float(mu), _stream()))
    return R


def pinv(A, threshold=1.0e-8):
    """pseudoinverse() (beamformer.cc:232-289) of one host matrix: (invA complex128 [N][M], ok) with ok == the reference's
    return value (False when a singular value fell below the threshold)."""
    A = np.ascontiguousarray(A, np.complex128)
    M, N = A.shape
    out = np.zeros((N, M), np.complex128)
    nz = C.c_int(0)
    check(_lib.lib().btk_pinv(_np_ptr(A), M, N, float(threshold), _np_ptr(out), C.byref(nz)))
    return out, nz.value == 0


# ---------------------------------------------------------------------------- WPE dereverberation
def wpe_band(M, band_width, samplerate):
    """set_band_width_ (dereverberation.cc:361-369): (lower_bandWidthN_, upper_bandWidthN_)."""
    if band_width == 0.0:
        lower = M // 2
    else:
        if band_width > samplerate / 2.0:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "Bandwidth is greater than the Nyquist rate.")
        lower = int((band_width / (samplerate / 2.0)) * (M // 2))
    return lower, M - lower


def wpe_estimate(X, M, lower_num=0, upper_num=32, iterations_num=2, load_db=-18.0, band_width=0.0,
                 diagonal_bias=1.0e-4, samplerate=16000.0, G=None):
    """MultiChannelWPEDereverberation::estimate_filter.  X complex64 [S][K][C][T] -> G complex64 [S][C][K][C*L]."""
    _need_cuda(X, "X")
    S, K, Cn, T = X.shape
    L = upper_num - lower_num + 1
    if G is None:
        G = torch.zeros((S, Cn, K, Cn * L), dtype=torch.complex64, device=X.device)
    lo, up = wpe_band(M, band_width, samplerate)
    ws = torch.empty(_lib.lib().btk_wpe_workspace_bytes(S, K, Cn, lower_num, upper_num, T), dtype=torch.uint8, device=X.device)
    fail = torch.zeros(1, dtype=torch.int32, device=X.device)
    check(_lib.lib().btk_wpe_estimate(_ptr(X), S, K, Cn, T, T, lower_num, upper_num, iterations_num, float(load_db),
                                      float(diagonal_bias), lo, up, _ptr(G), _ptr(ws), _ptr(fail), _stream()))
    if int(fail.item()) > 0:
        raise _lib.BtkError(_lib.BTK_ERR_NUMERIC, "MultiChannelWPEDereverberation: Cholesky decomposition failed (%d systems).\n"
                            "Some channels may be too similar. Try to increase 'diagonal_bias'" % int(fail.item()))
    return G


def wpe_apply(X, G, M, lower_num=0, upper_num=32, band_width=0.0, samplerate=16000.0, out=None):
    """calc_every_channel_output for every frame and channel: X [S][K][C][T] -> dereverberated [S][K][C][T]."""
    _need_cuda(X, "X"); _need_cuda(G, "G")
    S, K, Cn, T = X.shape
    if out is None:
        out = torch.empty_like(X)
    lo, up = wpe_band(M, band_width, samplerate)
    check(_lib.lib().btk_wpe_apply(_ptr(X), _ptr(G), _ptr(out), S, K, Cn, T, T, lower_num, upper_num, lo, up, _stream()))
    return out


# ---------------------------------------------------------------------------- steered response power (DOA estimation)
SRP_RESET_RP = -10e10                # the reset value of an N-best entry (beamformer.cc:3131-3135); its DOA is (-pi, -pi), index -1
SRP_MAX_NBEST = 16


def srp_grid(min_theta=-np.pi / 2, max_theta=np.pi / 2, width_theta=0.1):
    """The search grid of DOAEstimatorSRPDSBLA (beamformer.cc:3052, :3071): float parameters, (unsigned)((max - min) / width
    + 0.5) points, the angle accumulated in double -> thetas float64 [nTheta]."""
    n = C.c_int(0)
    L = _lib.lib()
    check(L.btk_srp_grid(float(min_theta), float(max_theta), float(width_theta), C.byref(n), None))
    thetas = np.zeros(n.value, np.float64)
    check(L.btk_srp_grid(float(min_theta), float(max_theta), float(width_theta), C.byref(n), _np_ptr(thetas)))
    return thetas


def srp_delays(positions, theta):
    """set_look_direction_ (beamformer.cc:3193-3207): |p_n - p_0| cos(theta) with theta rounded to float as the reference
    passes it; positions in seconds (metres over the speed of sound)."""
    pos = np.ascontiguousarray(positions, np.float64)
    d = np.zeros(pos.shape[0], np.float64)
    check(_lib.lib().btk_srp_delays(pos.shape[0], _np_ptr(pos), float(theta), _np_ptr(d)))
    return d


def srp_table(M, N, samplerate, positions, thetas, fbin_min=1, fbin_max=None):
    """svTbl_ (beamformer.cc:3046-3089) -> complex128 [nTheta][M/2+1][N]: calcMainlobe rows on bins fbin_min .. fbin_max,
    ones in bin 0, zero elsewhere."""
    pos = np.ascontiguousarray(positions, np.float64)
    th = np.ascontiguousarray(thetas, np.float64)
    if pos.shape != (N,):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "Number of positions does not match number of channels (%d vs. %d)." % (pos.size, N))
    fbin_max = M // 2 if fbin_max is None else int(fbin_max)
    out = np.zeros((th.shape[0], M // 2 + 1, N), np.complex128)
    check(_lib.lib().btk_srp_table(M, N, float(samplerate), _np_ptr(pos), th.shape[0], _np_ptr(th), int(fbin_min), fbin_max, _np_ptr(out)))
    return out


class SRPTable:
    """A steering table on the device in the operand order of srp_power_kernel (btk_srp_pack_table)."""

    def __init__(self, table, device):
        table = np.ascontiguousarray(table, np.complex128)
        if table.ndim != 3:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "steering table has shape %s, expected [U][K][N]" % (table.shape,))
        self.U, self.K, self.N = (int(v) for v in table.shape)
        L = _lib.lib()
        packed = np.zeros(L.btk_srp_packed_elems(self.U, self.K, self.N), np.complex64)
        check(L.btk_srp_pack_table(_np_ptr(table), self.U, self.K, self.N, _np_ptr(packed)))
        self.packed = torch.from_numpy(packed).to(device)


def srp_power(X, table, M, fbin_min=1, fbin_max=None):
    """Response power of every grid direction and frame, and the frame energy, in one pass over X (calc_response_power_ /
    calc_energy, beamformer.cc:3091-3122, 3221-3251).  X complex64 [S][K][N][T] (a row-padded view will do), table an SRPTable
    or a complex128 [U][K][N] array -> (rp float32 [S][U][T], energy float32 [S][T])."""
    ts = _check(X, "X", torch.complex64, 4, rows=True)
    S, K, N, T = X.shape
    if K != M // 2 + 1:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "X has %d bins, M = %d needs %d" % (K, M, M // 2 + 1))
    if not isinstance(table, SRPTable):
        table = SRPTable(table, X.device)
    if (table.K, table.N) != (K, N) or table.packed.device != X.device:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "steering table [%d][%d][%d] does not match X %s" % (table.U, table.K, table.N, tuple(X.shape)))
    fbin_max = M // 2 if fbin_max is None else int(fbin_max)
    rp = torch.empty((S, table.U, T), dtype=torch.float32, device=X.device)
    energy = torch.empty((S, T), dtype=torch.float32, device=X.device)
    check(_lib.lib().btk_srp_power(_ptr(X), _ptr(table.packed), _ptr(rp), _ptr(energy), S, M, N, ts, T, table.U,
                                   int(fbin_min), fbin_max, _stream()))
    return rp, energy


def srp_select(rp, energy, nbest, threshold=0.0, acc=None):
    """Per-frame N-best list (strict >: of equal powers the earlier grid index ranks first), energy gate and accumulated powers
    (beamformer.cc:3131-3187).  rp float32 [S][U][T], energy float32 [S][T] -> (nbest_rp float32 [S][T][nbest], nbest_idx int32
    [S][T][nbest], gate int32 [S][T], acc float64 [S][U]); a gated frame keeps (SRP_RESET_RP, -1); acc is updated in place."""
    _check(rp, "rp", torch.float32, 3)
    S, U, T = rp.shape
    _check(energy, "energy", torch.float32, (S, T))
    if acc is None:
        acc = torch.zeros((S, U), dtype=torch.float64, device=rp.device)
    _check(acc, "acc", torch.float64, (S, U))
    nbest = int(nbest)
    nb_rp = torch.empty((S, T, max(nbest, 0)), dtype=torch.float32, device=rp.device)
    nb_idx = torch.empty((S, T, max(nbest, 0)), dtype=torch.int32, device=rp.device)
    gate = torch.empty((S, T), dtype=torch.int32, device=rp.device)
    check(_lib.lib().btk_srp_select(_ptr(rp), _ptr(energy), float(threshold), nbest, _ptr(nb_rp), _ptr(nb_idx), _ptr(gate),
                                    _ptr(acc), S, U, T, _stream()))
    return nb_rp, nb_idx, gate, acc


def srp_nbest_host(values, nbest):
    """The insertion loop of get_nbest_hypotheses_from_accrp_ (beamformer.cc:2942-2981) over one row of powers: (values, indices),
    (SRP_RESET_RP, -1) where nothing was inserted."""
    best, idx = [SRP_RESET_RP] * nbest, [-1] * nbest
    for u, rp in enumerate(np.asarray(values, np.float64)):
        if rp > best[nbest - 1]:
            for n1 in range(nbest):
                if rp > best[n1]:
                    best[n1 + 1:] = best[n1:nbest - 1]
                    idx[n1 + 1:] = idx[n1:nbest - 1]
                    best[n1], idx[n1] = float(rp), u
                    break
    return np.array(best, np.float64), np.array(idx, np.int64)


class SRPState:
    """What S estimators share and keep between blocks: the grid and the steering table (fixed at construction: another
    geometry, search range or frequency range is another SRPState), the last grid direction's weights, and accRPs_ in float64
    on the device."""

    def __init__(self, S, M, samplerate, positions, device, nbest=1, min_theta=-np.pi / 2, max_theta=np.pi / 2, width_theta=0.1,
                 min_phi=-np.pi / 2, fbin_min=1, fbin_max=None, energy_threshold=0.0):
        self.S, self.M, self.samplerate, self.device, self.nbest = S, M, samplerate, device, int(nbest)
        self.positions = np.ascontiguousarray(positions, np.float64)
        self.N = self.positions.shape[0]
        self.min_phi = float(np.float32(min_phi))
        self.energy_threshold = float(energy_threshold)
        self.fbin_min, self.fbin_max = int(fbin_min), M // 2 if fbin_max is None else int(fbin_max)
        self.thetas = srp_grid(min_theta, max_theta, width_theta)
        self.table_host = srp_table(M, self.N, samplerate, self.positions, self.thetas, self.fbin_min, self.fbin_max)
        self.table = SRPTable(self.table_host, device)
        w_last = self.table_host[-1].astype(np.complex64)         # what next() leaves in vector_: zero outside fbin_min .. fbin_max
        w_last[: self.fbin_min] = 0
        self.w_last = torch.from_numpy(w_last).to(device)
        self.acc = torch.zeros((S, self.thetas.shape[0]), dtype=torch.float64, device=device)

    def init_accs(self):
        self.acc.zero_()

    def process(self, X):
        """One block: (rp, energy, nbest_rp, nbest_idx, gate); acc grows by the block's gated powers."""
        rp, energy = srp_power(X, self.table, self.M, self.fbin_min, self.fbin_max)
        nb_rp, nb_idx, gate, _ = srp_select(rp, energy, self.nbest, self.energy_threshold, self.acc)
        return rp, energy, nb_rp, nb_idx, gate

    def last_beam(self, X):
        """The delay-and-sum output of the last grid direction (what next() leaves in vector_, beamformer.cc:3101-3115):
        complex64 [S][K][T], zero outside fbin_min .. fbin_max."""
        return bf_apply(self.w_last, X)

    def final_nbest_hypotheses(self):
        """final_nbest_hypotheses (beamformer.cc:2942-2981) per stream: (rps float64 [S][nbest], doas float64 [S][nbest][2]) with
        DOA (theta_u, minPhi), (-pi, -pi) where nothing was inserted."""
        acc = self.acc.cpu().numpy()
        rps = np.zeros((self.S, self.nbest)); doas = np.full((self.S, self.nbest, 2), -np.pi)
        for s in range(self.S):
            rps[s], idx = srp_nbest_host(acc[s], self.nbest)
            for j, u in enumerate(idx):
                if u >= 0:
                    doas[s, j] = (self.thetas[u], self.min_phi)
        return rps, doas


# ------------------------------------------------------------------ maximum-empirical-kurtosis beamformers (csrc/hos_kernels.hip)
HOS_DEFAULTS = dict(maxiter=40, gtol=1.0e-2, mindelta=1.0e-5, max_halvings=30, armijo_c1=1.0e-4)


class HOSState:
    """Previous statistics of SubbandMEKBeamformer (reset_stats / store_stats, lib/pybeamformer.py:1613-1627) on the device:
    prevAvgY2, prevAvgY4 float64 [K][NS] and prevFrameN int64 [K][NS]."""

    def __init__(self, K, NS, device):
        self.K, self.NS, self.device = int(K), int(NS), device
        self.reset()

    def reset(self):
        self.prevAvgY2 = torch.zeros((self.K, self.NS), dtype=torch.float64, device=self.device)
        self.prevAvgY4 = torch.zeros((self.K, self.NS), dtype=torch.float64, device=self.device)
        self.prevFrameN = torch.zeros((self.K, self.NS), dtype=torch.int64, device=self.device)

    def store(self, stats, frames):
        """store_stats for every bin and source, as written there: prevFrameN grows FIRST, then every frame adds
        Y2 / prevFrameN and Y4 / prevFrameN with Y2 = sum_s |Y_s|^2 / NS and Y4 = Y2^2 -- not a running mean.  stats: what
        hos_eval returned for the final weights, frames: the number of frames it saw."""
        self.prevFrameN += int(frames)
        n = self.prevFrameN.to(torch.float64)
        NS = self.NS
        self.prevAvgY2 += stats[:, 2 * NS:2 * NS + 1] / n
        self.prevAvgY4 += stats[:, 2 * NS + 1:2 * NS + 2] / n


def _hos_inputs(X, wuH, BmH, Nc, mask, state):
    ts = _check(X, "X", torch.complex64, 3, rows=True)
    K, N, T = X.shape
    _check(wuH, "wuH", torch.complex128, (None, K, N))
    NS = wuH.shape[0]
    _check(BmH, "BmH", torch.complex128, (NS, K, None, N))
    Nc = int(Nc)
    if BmH.shape[2] != N - Nc:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "BmH has %d rows, N - Nc = %d" % (BmH.shape[2], N - Nc))
    if mask is not None:
        _check(mask, "mask", torch.float32, (T,))
    if state is not None:
        _check(state.prevAvgY2, "prevAvgY2", torch.float64, (K, NS))
        _check(state.prevAvgY4, "prevAvgY4", torch.float64, (K, NS))
        _check(state.prevFrameN, "prevFrameN", torch.int64, (K, NS))
    null = C.c_void_p(0)
    prev = (null, null, null) if state is None else (_ptr(state.prevAvgY2), _ptr(state.prevAvgY4), _ptr(state.prevFrameN))
    return ts, K, N, T, NS, Nc, (null if mask is None else _ptr(mask)), prev


def hos_eval(X, wuH, BmH, x=None, Nc=1, alpha=0.01, beta=3.0, gamma=-1.0, normalize=False, mask=None, state=None, grad=True):
    """fun_hos_bf and dfun_hos_bf (lib/pybeamformer.py:1548-1593) of the MEK (normalize=False) or NMEK beamformer for every bin
    in one launch.  X complex64 [K][N][T] (a row-padded view will do), wuH complex128 [NS][K][N], BmH complex128
    [NS][K][N-Nc][N], x float64 [K][2 NS (N-Nc)] packed active weights (None: zero), mask float32 [T] of 0/1 or None, state an
    HOSState or None -> (fun float64 [K], grad float64 [K][D] or None, stats float64 [K][2 NS + 2]).  A mask that selects no
    frame, with zero previous statistics, divides by zero as the reference's empty list of observations does: fun and grad are NaN."""
    ts, K, N, T, NS, Nc, pmask, prev = _hos_inputs(X, wuH, BmH, Nc, mask, state)
    D = 2 * NS * (N - Nc)
    if x is not None:
        _check(x, "x", torch.float64, (K, D))
    fun = torch.empty((K,), dtype=torch.float64, device=X.device)
    g = torch.empty((K, D), dtype=torch.float64, device=X.device) if grad else None
    stats = torch.empty((K, 2 * NS + 2), dtype=torch.float64, device=X.device)
    check(_lib.lib().btk_hos_eval(_ptr(X), pmask, _ptr(wuH), _ptr(BmH), C.c_void_p(0) if x is None else _ptr(x), float(alpha),
                                  float(beta), float(gamma), int(bool(normalize)), prev[0], prev[1], prev[2], K, N, Nc, NS, ts, T,
                                  _ptr(fun), C.c_void_p(0) if g is None else _ptr(g), _ptr(stats), _stream()))
    return fun, g, stats


HOSResult = collections.namedtuple("HOSResult", "x f iters trace_f trace_halvings")


def hos_minimize(X, wuH, BmH, x0=None, Nc=1, alpha=0.01, beta=3.0, gamma=-1.0, normalize=True, mask=None, state=None, **options):
    """The optimisation of every bin in one launch (estimate_active_weights, lib/pybeamformer.py:1802-1827, with the
    Polak-Ribiere+ / Armijo iteration of DESIGN.md 3.15): inputs as hos_eval, options as HOS_DEFAULTS -> HOSResult(x float64
    [K][D], f float64 [K], iters int32 [K], trace_f float64 [K][maxiter], trace_halvings int32 [K][maxiter])."""
    unknown = set(options) - set(HOS_DEFAULTS)
    if unknown:
        raise TypeError("hos_minimize: unknown options %s" % sorted(unknown))
    o = dict(HOS_DEFAULTS, **options)
    ts, K, N, T, NS, Nc, pmask, prev = _hos_inputs(X, wuH, BmH, Nc, mask, state)
    D = 2 * NS * (N - Nc)
    if x0 is not None:
        _check(x0, "x0", torch.float64, (K, D))
    maxiter = int(o["maxiter"])
    dev = X.device
    xo = torch.empty((K, D), dtype=torch.float64, device=dev)
    fo = torch.empty((K,), dtype=torch.float64, device=dev)
    it = torch.empty((K,), dtype=torch.int32, device=dev)
    tf = torch.empty((K, max(maxiter, 0)), dtype=torch.float64, device=dev)
    th = torch.empty((K, max(maxiter, 0)), dtype=torch.int32, device=dev)
    check(_lib.lib().btk_hos_minimize(_ptr(X), pmask, _ptr(wuH), _ptr(BmH), C.c_void_p(0) if x0 is None else _ptr(x0), float(alpha),
                                      float(beta), float(gamma), int(bool(normalize)), prev[0], prev[1], prev[2], K, N, Nc, NS, ts,
                                      T, maxiter, float(o["gtol"]), float(o["mindelta"]), int(o["max_halvings"]),
                                      float(o["armijo_c1"]), _ptr(xo), _ptr(fo), _ptr(it), _ptr(tf), _ptr(th), _stream()))
    return HOSResult(xo, fo, it, tf, th)


# ---- GCC-PHAT time delay of arrival (btk_tdoa_*): HammingFeature + FFTFeature, PHATFeature.next + TDOAFeature.next ------------
TDOA_NO_PEAK = _lib.BTK_TDOA_NO_PEAK


def tdoa_frames(nsamples, D):
    """Frames of SampleFeature(block_len=D, shift_len=D, pad_zeros=True) over nsamples samples: ceil(nsamples / D)."""
    return int(_lib.lib().btk_tdoa_frames(int(nsamples), int(D)))


def tdoa_spectra(pcm, D, L, window=True):
    """Hamming window (float64 product rounded to float32; window=False: none), zero padding to L and forward transform of every
    D-sample frame (feature/feature.cc:1177-1258).  pcm float32 [S][C][len] -> (X complex64 [S][C][T][L/2+1], energy float32 [S][C][T]),
    T = ceil(len / D), energy = 2 sum_k |X_k|^2 (lib/pytdoa.py:47)."""
    _check(pcm, "pcm", torch.float32, 3)
    S, Cn, n = pcm.shape
    D, L = int(D), int(L)
    T = max(-(-n // D), 0) if D > 0 else 0
    X = torch.empty((S, Cn, T, max(L, 0) // 2 + 1), dtype=torch.complex64, device=pcm.device)
    energy = torch.empty((S, Cn, T), dtype=torch.float32, device=pcm.device)
    check(_lib.lib().btk_tdoa_spectra(_ptr(pcm), n, n, S, Cn, D, L, int(bool(window)), _ptr(X), _ptr(energy), _stream()))
    return X, energy


def tdoa_pairs(pairs, C_channels, device):
    """The pair list as the int32 [P][2] device tensor btk_tdoa_gcc_peaks reads; a host list is range-checked here."""
    if isinstance(pairs, torch.Tensor):
        _check(pairs, "pairs", torch.int32, (None, 2))
        return pairs
    a = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    if a.shape[0] < 1 or a.min() < 0 or a.max() >= C_channels:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "pairs must name channels 0 .. %d and be at least one" % (C_channels - 1))
    return torch.from_numpy(a.astype(np.int32)).to(device)


def tdoa_gcc_peaks(X, energy, pairs, energy_threshold, want_gcc=False):
    """Phase transform, inverse transform and peak search of every listed pair and frame (lib/pytdoa.py:32-54, 87-114).
    X complex64 [S][C][T][L/2+1], energy float32 [S][C][T], pairs [P][2] -> (lag int32 [S][P][T], height float32 [S][P][T]
    [, gcc float32 [S][P][T][L]]); lag is TDOA_NO_PEAK and height 0 where a frame has no peak."""
    _check(X, "X", torch.complex64, 4)
    S, Cn, T, K = X.shape
    L = 2 * (K - 1)
    _check(energy, "energy", torch.float32, (S, Cn, T))
    pd = tdoa_pairs(pairs, Cn, X.device)
    P = pd.shape[0]
    lag = torch.empty((S, P, T), dtype=torch.int32, device=X.device)
    height = torch.empty((S, P, T), dtype=torch.float32, device=X.device)
    gcc = torch.empty((S, P, T, L), dtype=torch.float32, device=X.device) if want_gcc else None
    check(_lib.lib().btk_tdoa_gcc_peaks(_ptr(X), _ptr(energy), _ptr(pd), P, float(energy_threshold), S, Cn, T, L, _ptr(lag),
                                        _ptr(height), C.c_void_p(0) if gcc is None else _ptr(gcc), _stream()))
    return (lag, height, gcc) if want_gcc else (lag, height)


def tdoa_estimate(pcm, D, L, pairs, energy_threshold):
    """tdoa_spectra then tdoa_gcc_peaks: pcm float32 [S][C][len] -> (lag int32 [S][P][T], height float32 [S][P][T])."""
    X, energy = tdoa_spectra(pcm, D, L)
    return tdoa_gcc_peaks(X, energy, pairs, energy_threshold)


# ---- EKF / IEKF speaker tracking over the TDOA peaks (btk_ekf_track): lib/pykalman.py over lib/pytdoa.py's observation models ----
EKF_TRACKED, EKF_OBSERVED, EKF_UPDATED, EKF_ROUNDS_SHIFT = 1, 2, 4, 8
EKF_MODELS = {"linear": 0, "circular": 1, "cartesian": 2}          # state length 1, 2, 3
EKF_TYPES = {"ekf": 0, "iekf": 1}


def ekf_params(model, type, F, U, sigmaV2, time_delta, gate_prob=0.0, num_iterations=3, iteration_threshold=1e-4, threshold=0.12,
               minimum_pairs=2, Ts=1.0 / 16000, c=343000.0):
    """The parameter record of btk_ekf_track.  model 'linear' | 'circular' | 'cartesian', type 'ekf' | 'iekf', F and U n x n with
    n the model's state length (1, 2, 3)."""
    F, U = np.asarray(F, np.float64), np.asarray(U, np.float64)
    n = F.shape[0] if F.ndim == 2 else -1
    if model not in EKF_MODELS or type not in EKF_TYPES:
        raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "ekf_params: model %r, type %r" % (model, type))
    if n != EKF_MODELS[model] + 1 or F.shape != (n, n) or U.shape != (n, n):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "ekf_params: F %s and U %s must be %d x %d for the %s model" % (
            F.shape, U.shape, EKF_MODELS[model] + 1, EKF_MODELS[model] + 1, model))
    p = _lib.EkfParams()
    p.n, p.model, p.type = n, EKF_MODELS[model], EKF_TYPES[type]
    F3, U3 = np.zeros((3, 3)), np.zeros((3, 3))
    F3[:n, :n], U3[:n, :n] = F, U
    p.F[:], p.U[:] = F3.ravel().tolist(), U3.ravel().tolist()
    p.sigmaV2, p.time_delta, p.gate_prob = float(sigmaV2), float(time_delta), float(gate_prob)
    p.num_iterations, p.iteration_threshold = int(num_iterations), float(iteration_threshold)
    p.threshold, p.minimum_pairs, p.Ts, p.c = float(threshold), int(minimum_pairs), float(Ts), float(c)
    return p


def ekf_state(x, K, time, device, streams=1, last_update=-1):
    """The float64 [S][16] state record of btk_ekf_track: x, K_filter (3 x 3 row-major, leading n x n block), time, lastUpdateT."""
    x, K = np.asarray(x, np.float64).ravel(), np.asarray(K, np.float64)
    n = len(x)
    rec = np.zeros(16)
    rec[:n] = x
    K3 = np.zeros((3, 3))
    K3[:n, :n] = K
    rec[3:12] = K3.ravel()
    rec[12], rec[13] = time, last_update
    return torch.from_numpy(np.tile(rec, (int(streams), 1))).to(device)


def ekf_track(lag, height, geom, params, state, t_begin=None):
    """Track S independent streams through the T frames of a block of TDOA peaks, in one launch.
    lag int32 [S][P][T], height float32 [S][P][T] (tdoa_gcc_peaks), geom float64 [P][6] (the model's per-pair geometry),
    params an ekf_params record, state float64 [S][16] (ekf_state; updated in place, so the next block continues),
    t_begin int32 [S] or None: the stream's first tracked frame.
    -> (xk float64 [S][T][3], Kf float64 [S][T][9], flags int32 [S][T]): xk_filter, K_filter and EKF_TRACKED | EKF_OBSERVED |
    EKF_UPDATED | rounds << EKF_ROUNDS_SHIFT after every frame."""
    if not isinstance(params, _lib.EkfParams):
        raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "ekf_track: params must come from ekf_params")
    _check(lag, "lag", torch.int32, 3)
    S, P, T = lag.shape
    _check(height, "height", torch.float32, (S, P, T))
    _check(geom, "geom", torch.float64, (P, 6))
    _check(state, "state", torch.float64, (S, 16))
    if t_begin is not None:
        _check(t_begin, "t_begin", torch.int32, (S,))
    xk = torch.empty((S, T, 3), dtype=torch.float64, device=lag.device)
    Kf = torch.empty((S, T, 9), dtype=torch.float64, device=lag.device)
    flags = torch.empty((S, T), dtype=torch.int32, device=lag.device)
    check(_lib.lib().btk_ekf_track(C.cast(C.pointer(params), C.c_void_p), _ptr(lag), _ptr(height), _ptr(geom),
                                   C.c_void_p(0) if t_begin is None else _ptr(t_begin), S, P, T, _ptr(state), _ptr(xk), _ptr(Kf),
                                   _ptr(flags), _stream()))
    return xk, Kf, flags


# ---- ASR front end (btk_fe_*): PreemphasisFeature, HammingFeature + FFTFeature, SpectralPowerFeature, VTLNFeature, MelFeature,
# LogFeature, CepstralFeature (feature/feature.cc:1128-1144, :1177-1314, :1672-1792, :1892-2122, :2326-2415) ---------------------
FE_PCM, FE_SPECTRUM, FE_POWER, FE_VTLN, FE_MEL, FE_LOG, FE_CEP = range(7)
FE_STAGES = ("pcm", "spectrum", "power", "vtln", "mel", "log", "cep")


def _fe_stage(s):
    if isinstance(s, str):
        if s not in FE_STAGES:
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "unknown front-end stage %r (one of %s)" % (s, ", ".join(FE_STAGES)))
        return FE_STAGES.index(s)
    return int(s)


def fe_frames(nsamples, D, shift, pad_zeros=True):
    """Frames of SampleFeature(block_len=D, shift_len=shift, pad_zeros=pad_zeros) over nsamples samples."""
    return int(_lib.lib().btk_fe_frames(int(nsamples), int(D), int(shift), int(bool(pad_zeros))))


class FeTable:
    """A table of the front end: built once on the host (offset, count int32 [rows], coef packed row after row; a cosine table
    is dense, count == cols), uploaded once per device and kept there."""

    def __init__(self, offset, count, coef, cols):
        self.offset, self.count, self.coef, self.cols = offset, count, coef, int(cols)
        self.rows = int(offset.shape[0])
        self.start = np.concatenate(([0], np.cumsum(count)[:-1])).astype(np.int32)
        self._dev = {}

    def matrix(self):
        """The table as a dense float64 [rows][cols] matrix (MelFeature.matrix, VTLNFeature.matrix, CepstralFeature.matrix)."""
        m = np.zeros((self.rows, self.cols), np.float64)
        for j in range(self.rows):
            m[j, self.offset[j]:self.offset[j] + self.count[j]] = self.coef[self.start[j]:self.start[j] + self.count[j]]
        return m

    def abs_column_sum(self):
        """The largest absolute column sum: the table's gain on an l1 perturbation of its input."""
        return float(np.abs(self.matrix()).sum(axis=0).max())

    def on(self, device):
        """(rows int32 [rows][3] = offset, count, start; coef) on the device."""
        key = torch.device(device)
        if key not in self._dev:
            rows = np.ascontiguousarray(np.stack([self.offset, self.count, self.start], axis=1).astype(np.int32))
            self._dev[key] = (torch.from_numpy(rows).to(key), torch.from_numpy(np.ascontiguousarray(self.coef)).to(key))
        return self._dev[key]


def fe_mel_table(powN, rate, low, up, filterN, version=1):
    """MelFeature's band matrix (melScaleOrg: version 1, melScaleFF: version 2; feature/feature.cc:1904-2039), host code."""
    powN, filterN = int(powN), int(filterN)
    offset, count = np.zeros(max(filterN, 1), np.int32), np.zeros(max(filterN, 1), np.int32)
    cap = max(filterN, 1) * max(powN, 1)
    coef = np.zeros(cap, np.float32)
    n = C.c_int(0)
    check(_lib.lib().btk_fe_mel_table(powN, float(rate), float(low), float(up), filterN, int(version), _np_ptr(offset),
                                      _np_ptr(count), _np_ptr(coef), cap, C.byref(n)))
    return FeTable(offset, count, coef[:n.value].copy(), powN)


def fe_vtln_table(N, ratio, edge=1.0, version=1, inN=None):
    """VTLNFeature as an operator on the power vector (nextOrg: version 1, nextFF: version 2; feature/feature.cc:1672-1792),
    float64 weights, host code."""
    N = int(N)
    inN = N if inN is None else int(inN)
    offset, count = np.zeros(max(N, 1), np.int32), np.zeros(max(N, 1), np.int32)
    cap = max(N, 1) * max(inN, 1)
    w = np.zeros(cap, np.float64)
    n = C.c_int(0)
    check(_lib.lib().btk_fe_vtln_table(N, inN, float(ratio), float(edge), int(version), _np_ptr(offset), _np_ptr(count),
                                       _np_ptr(w), cap, C.byref(n)))
    return FeTable(offset, count, w[:n.value].copy(), inN)


def fe_dct_table(type, cepN, filterN):
    """CepstralFeature's cosine table: types 0 and 1 of gsl_matrix_float_set_cosine (matrix/gslmatrix.cc:107-131), type 2 the
    sphinx legacy form (feature/feature.cc:2389-2400); float32 [cepN][filterN], host code."""
    cepN, filterN = int(cepN), int(filterN)
    m = np.zeros((max(cepN, 1), max(filterN, 1)), np.float32)
    check(_lib.lib().btk_fe_dct_table(int(type), cepN, filterN, _np_ptr(m)))
    return FeTable(np.zeros(cepN, np.int32), np.full(cepN, filterN, np.int32), m.reshape(-1), filterN)


def fe_process(x, in_stage="pcm", want=("cep",), D=None, shift=None, L=None, T=None, window=True, preemph=None, prior0=None,
               powN=None, vtln=None, mel=None, log_m=1.0, log_a=1.0, log_floor=False, dct=None, nsamples=None, pad_zeros=True):
    """The front end from the vectors of in_stage up to the last stage of `want`, one launch; -> {stage name: tensor} of the
    wanted stages, float32 [S][C][T][dim] (spectrum: complex64 [S][C][T][L/2+1]).
    in_stage "pcm": x float32 [S][C][len] or [S][len] (one channel; rows may be padded, as FilterBank.synthesize returns them):
      frames of D samples every `shift` (default D), T frames (default fe_frames(len, D, shift, pad_zeros)), pre-emphasis with
      mu = preemph where that is not None (prior0 float32 [S][C]: the sample before the first), Hamming window unless window is
      False, transform length L.  in_stage "spectrum": x complex64 [S][C][T][L/2+1]; later stages: float32 [S][C][T][dim].
    powN: L/2+1 (default) or L.  vtln, mel: FeTable or None (the stage is skipped); dct: FeTable of fe_dct_table."""
    st = _fe_stage(in_stage)
    wanted = sorted(set(_fe_stage(w) for w in ([want] if isinstance(want, (str, int)) else want)))
    if not wanted or wanted[0] <= st or wanted[-1] > FE_CEP:
        raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "fe_process: the wanted stages must come after %s" % FE_STAGES[st])
    if vtln is None:
        wanted = [w for w in wanted if w != FE_VTLN]
    if mel is None and st < FE_MEL:
        wanted = [w for w in wanted if w != FE_MEL]
    if not wanted:
        raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "fe_process: every wanted stage is skipped (no table given)")
    q = _lib.FeParams()
    q.in_stage = st
    dev = x.device
    if st == FE_PCM:
        if x.dim() == 2:
            x = x.unsqueeze(1)
        if x.dtype != torch.float32 or x.dim() != 3 or not x.is_cuda or x.stride(2) != 1:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "fe_process: pcm must be a float32 cuda tensor [S][C][len] with contiguous rows")
        S, Cn, n = x.shape
        stride = x.stride(1) if Cn > 1 else (x.stride(0) if S > 1 else max(n, 1))
        if (Cn > 1 and S > 1 and x.stride(0) != Cn * stride) or stride < n:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "fe_process: pcm rows must be evenly spaced")
        if nsamples is not None and not 0 < int(nsamples) <= n:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "fe_process: nsamples=%d outside the rows' %d samples" % (int(nsamples), n))
        n = n if nsamples is None else int(nsamples)
        if D is None or L is None:
            raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "fe_process: D and L are needed from PCM")
        D, L = int(D), int(L)
        shift = D if shift is None else int(shift)
        T = fe_frames(n, D, shift, pad_zeros) if T is None else int(T)
        q.len, q.pcm_stride, q.D, q.shift, q.L, q.window = n, stride, D, shift, L, int(bool(window))
        q.preemph, q.mu = int(preemph is not None), float(preemph or 0.0)
        if prior0 is not None:
            _check(prior0, "prior0", torch.float32, (S, Cn))
            q.prior0 = prior0.data_ptr()
        n_in = (L // 2 + 1) if powN is None else int(powN)
    elif st == FE_SPECTRUM:
        _check(x, "X", torch.complex64, 4)
        S, Cn, T, K = x.shape
        L = 2 * (K - 1)
        q.L = L
        n_in = (L // 2 + 1) if powN is None else int(powN)
    else:
        _check(x, FE_STAGES[st], torch.float32, 4)
        S, Cn, T, n_in = x.shape
        q.in_dim = n_in
    q.S, q.C, q.T, q.powN = S, Cn, max(T, 0), n_in if st <= FE_SPECTRUM else 0
    keep = []                                          # device tensors the launch reads
    dims = {FE_SPECTRUM: (L // 2 + 1) if st <= FE_PCM else 0, FE_POWER: n_in}
    n = n_in
    last = wanted[-1]
    if st < FE_VTLN and last >= FE_VTLN and vtln is not None:
        rows, w = vtln.on(dev)
        keep += [rows, w]
        q.vtlnN, q.vtln_nw, q.vtln_rows, q.vtln_w = vtln.rows, int(w.numel()), rows.data_ptr(), w.data_ptr()
        dims[FE_VTLN] = n = vtln.rows
    if st < FE_MEL and last >= FE_MEL and mel is not None:
        rows, w = mel.on(dev)
        keep += [rows, w]
        q.melN, q.mel_nw, q.mel_rows, q.mel_w = mel.rows, int(w.numel()), rows.data_ptr(), w.data_ptr()
        dims[FE_MEL] = n = mel.rows
    dims[FE_LOG] = n
    q.log_m, q.log_a, q.log_floor = float(log_m), float(log_a), int(bool(log_floor))
    if last >= FE_CEP:
        if dct is None or dct.cols != n:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "fe_process: cepstra need a cosine table over %d values" % n)
        rows, w = dct.on(dev)
        keep += [w]
        q.cepN, q.dct = dct.rows, w.data_ptr()
        dims[FE_CEP] = dct.rows
    out = {}
    for s in wanted:
        t = torch.empty((S, Cn, max(T, 0), dims[s]), dtype=torch.complex64 if s == FE_SPECTRUM else torch.float32, device=dev)
        out[FE_STAGES[s]] = t
        q.out[s] = t.data_ptr()
    check(_lib.lib().btk_fe_process(C.cast(C.pointer(q), C.c_void_p), _ptr(x), _stream()))
    return out


# ---- FFT block convolution (btk_conv_*): OverlapAdd::next / OverlapSave::next (convolution/convolution.cc:83-131, :196-230) ------
def conv_plan(P, n_max=16384):
    """(N, Lk, Bp, Q) that btk_conv_plan picks for P taps: transform length, outputs per tile, taps per partition, partitions."""
    N, Lk, Bp, Q = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    check(_lib.lib().btk_conv_plan(int(P), int(n_max), C.byref(N), C.byref(Lk), C.byref(Bp), C.byref(Q)))
    return N.value, Lk.value, Bp.value, Q.value


class ConvFilter:
    """Impulse responses as the half spectra btk_conv_apply multiplies with, and the plan they were cut by.
    H complex64 [S_h][C][Q][N/2+1] on the device of h; S_h = 1 for filters shared by every stream."""

    def __init__(self, H, P, N, Lk, Bp, Q):
        self.H, self.P, self.N, self.Lk, self.Bp, self.Q = H, int(P), int(N), int(Lk), int(Bp), int(Q)
        self.S_h, self.C = int(H.shape[0]), int(H.shape[1])


def conv_filter(h, n_max=16384, plan=None):
    """h float32 cuda [C][P] (shared by every stream) or [S][C][P] -> ConvFilter.  Taps given as float64 are rounded to float32
    first.  plan: (N, Lk, Bp, Q) instead of conv_plan(P, n_max)'s, e.g. a tile length that divides a block length."""
    if h.dim() == 2:
        h = h.unsqueeze(0)
    if h.dtype == torch.float64:
        h = h.to(torch.float32)
    h = h.contiguous()
    _check(h, "h", torch.float32, 3)
    S_h, Cn, P = h.shape
    N, Lk, Bp, Q = conv_plan(P, n_max) if plan is None else (int(v) for v in plan)
    H = torch.empty((S_h, Cn, max(Q, 1), max(N, 0) // 2 + 1), dtype=torch.complex64, device=h.device)
    check(_lib.lib().btk_conv_filter_spectra(_ptr(h), P, S_h * Cn, P, N, Bp, Q, _ptr(H), _stream()))
    return ConvFilter(H, P, N, Lk, Bp, Q)


def _conv_rows(x, name):
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_cuda or (x.shape[1] > 1 and x.stride(1) != 1):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s: x must be a float32 cuda tensor [S][samples] with contiguous rows" % name)
    S, n = x.shape
    stride = x.stride(0) if S > 1 else max(n, 1)
    if stride < n:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s: rows of x overlap" % name)
    return x, S, n, stride


def fir_convolve(x, filt, out_len=None, hist=0, out=None):
    """y[s][c][n] = sum_p h[c][p] x[s][hist + n - p]: every row of x float32 [S][hist + len] filtered with every impulse response
    of filt -> float32 [S][C][out_len].  The first `hist` samples of a row are the stream's past (zeros stand in front of them),
    so a call on x[:, a - hist:] with hist >= P - 1 continues a call that ended at sample a; where a is a multiple of filt.Lk
    the bits are those of one call.  out_len: len (default, what OverlapAdd hands out) up to len + P - 1 and beyond (zeros)."""
    x, S, n, stride = _conv_rows(x, "fir_convolve")
    hist = int(hist)
    if hist < 0 or hist > n:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "fir_convolve: hist=%d outside the rows' %d samples" % (hist, n))
    ln = n - hist
    out_len = ln if out_len is None else int(out_len)
    if filt.S_h not in (1, S):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "fir_convolve: filters of %d streams, x has %d" % (filt.S_h, S))
    if out is None:
        out = torch.empty((S, filt.C, max(out_len, 0)), dtype=torch.float32, device=x.device)
    ys = _check(out, "out", torch.float32, (S, filt.C, out_len), rows=True)
    check(_lib.lib().btk_conv_apply(C.c_void_p(x.data_ptr() + 4 * hist), ln, hist, stride, S, _ptr(filt.H), filt.S_h, filt.C,
                                    filt.P, filt.N, filt.Lk, filt.Bp, filt.Q, _ptr(out), out_len, ys, _stream()))
    return out


def conv_blocks(x, filt, L, block_step):
    """OverlapSave::next for every block: x float32 [S][len], block t = samples t block_step .. + L - 1 (every block that fits),
    filt a ConvFilter cut for N = L with Q = 1 (conv_filter(h, plan=(L, L - P + 1, P, 1))) -> float32 [S][C][T][L - P],
    y[..][t][j] = sum_p h[p] x[t block_step + j + P - p]."""
    x, S, n, stride = _conv_rows(x, "conv_blocks")
    L, block_step = int(L), int(block_step)
    if filt.N != L or filt.Q != 1:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "conv_blocks: the filter was cut for N=%d, Q=%d, not for blocks of %d"
                            % (filt.N, filt.Q, L))
    if filt.S_h not in (1, S):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "conv_blocks: filters of %d streams, x has %d" % (filt.S_h, S))
    T = (n - L) // block_step + 1 if (block_step > 0 and n >= L) else 0
    out = torch.empty((S, filt.C, max(T, 0), max(L - filt.P, 0)), dtype=torch.float32, device=x.device)
    check(_lib.lib().btk_conv_blocks(_ptr(x), n, stride, S, T, block_step, _ptr(filt.H), filt.S_h, filt.C, filt.P, L, _ptr(out),
                                     _stream()))
    return out


# ---------------------------------------------------------------------------- PR banks and the windowed FFT bank (fb_pr_kernels.hip)
def get_window(window_type, length):
    """get_window (modulated.cc:47-72): 0 rectangular, 2 Hann, anything else Hamming -> float64 [length].  Host side."""
    w = np.zeros(int(length), np.float64)
    check(_lib.lib().btk_get_window(int(window_type), int(length), _np_ptr(w)))
    return w


class _FrameBank:
    """What PRFilterBank and STFTBank share: a plan handle and the analysis launch over frames [t0, t0 + tcount)."""
    _destroy = _frames = _analysis = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                getattr(_lib.lib(), self._destroy)(h)
            except Exception:
                pass
            self._h = None

    def num_frames(self, nsamples):
        return getattr(_lib.lib(), self._frames)(self._h, nsamples)

    def analysis(self, pcm, nsamples=None, t0=0, tcount=None, out=None):
        """pcm float32 [S][N][L] (cuda) -> X complex64 [S][bins][N][T], every bin of the transform; `out` may be a row-padded view."""
        _check(pcm, "pcm", torch.float32, 3)
        S, N, L = pcm.shape
        nsamples = L if nsamples is None else nsamples
        if tcount is None:
            tcount = self.num_frames(nsamples) - t0
        if out is None:
            out = torch.empty((S, self.bins, N, tcount), dtype=torch.complex64, device=pcm.device)
        ts = _check(out, "X", torch.complex64, (S, self.bins, N, None), rows=True)
        if out.shape[3] < tcount:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "X holds %d frames, %d requested" % (out.shape[3], tcount))
        check(getattr(_lib.lib(), self._analysis)(self._h, _ptr(pcm), nsamples, L, S, N, _ptr(out), ts, t0, tcount, _stream()))
        return out


class PRFilterBank(_FrameBank):
    """Plan of a cosine-modulated perfect-reconstruction bank (PerfectReconstructionFilterBank, modulated.cc:284-300): 2 M complex
    bins per frame, frame shift D = M / 2^r, prototype of length 2 M m."""
    _destroy, _frames, _analysis = "btk_prfb_destroy", "btk_prfb_num_frames", "btk_prfb_analysis"

    def __init__(self, prototype, M, m, r, synthesis=False):
        proto = np.ascontiguousarray(prototype, np.float64).reshape(-1)
        self.M, self.m, self.r = M, m, r
        self.M2 = self.bins = 2 * M
        self.R = 1 << r
        self.D = M // self.R
        self.is_synthesis = bool(synthesis)
        self._h = C.c_void_p()
        check(_lib.lib().btk_prfb_create(C.byref(self._h), M, m, r, int(synthesis), _np_ptr(proto), proto.size))
        self.processing_delay = _lib.lib().btk_prfb_processing_delay(self._h)

    def num_blocks(self, nframes):
        return _lib.lib().btk_prfb_num_blocks(self._h, nframes)

    def synthesis(self, Y, nframes=None, b0=0, bcount=None, out=None):
        """Y complex64 [S][M2][T] (cuda) -> float32 [S][bcount*D], blocks [b0, b0 + bcount)."""
        t_stride = _row_stride(Y, "Y")            # Y may be a [..., :T] view of a row-padded buffer
        if Y.dtype != torch.complex64 or Y.dim() != 3 or Y.shape[1] != self.M2:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "Y must be complex64 [S][%d][T], got %s %s" % (self.M2, Y.dtype, tuple(Y.shape)))
        S, _, T = Y.shape
        nframes = T if nframes is None else nframes
        if bcount is None:
            bcount = self.num_blocks(nframes) - b0
        if out is None:
            out = torch.empty((S, bcount * self.D), dtype=torch.float32, device=Y.device)
        _check(out, "out", torch.float32, (S, None))
        check(_lib.lib().btk_prfb_synthesis(self._h, _ptr(Y), nframes, t_stride, S, _ptr(out), out.shape[1], b0, bcount, _stream()))
        return out

    synthesize = synthesis                        # FilterBank's name for the same launch


class STFTBank(_FrameBank):
    """Plan of the windowed short-time FFT (NormalFFTAnalysisBank, modulated.cc:96-132): M bins per frame, frame shift M / 2^r."""
    _destroy, _frames, _analysis = "btk_stft_destroy", "btk_stft_num_frames", "btk_stft_analysis"

    def __init__(self, M, r=1, window_type=1):
        self.M = self.bins = M
        self.r, self.window_type = r, window_type
        self.R = 1 << r
        self.D = M // self.R
        self._h = C.c_void_p()
        check(_lib.lib().btk_stft_create(C.byref(self._h), M, r, window_type))


# ---------------------------------------------------------------------------- objective measures (obj_kernels.hip)
SNR_MEAN, SNR_PEAK, SNR_POWER, SNR_PROJECT = 1, 2, 4, 8     # option bits of calcSNR (objective_measure.cc:42-185)
FLT_MAX = np.float32(np.finfo(np.float32).max)


def _obj_rows(x, name):
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_cuda or (x.shape[1] > 1 and x.stride(1) != 1):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s must be a float32 cuda tensor [S][samples] with contiguous rows" % name)
    S, n = x.shape
    stride = x.stride(0) if S > 1 else max(n, 1)
    if stride < n:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s: rows overlap" % name)
    return x, S, n, stride


def _obj_pair(x1, x2, n1, n2, name, nlow=1):
    """Rows and lengths of a batch of pairs: x1, x2 float32 cuda [S][>= n]; n1, n2 host integers or sequences (default: the rows)."""
    x1, S, L1, st1 = _obj_rows(x1, name + ": x1")
    x2, S2, L2, st2 = _obj_rows(x2, name + ": x2")
    if S != S2 or x1.device != x2.device:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s: %d and %d signals" % (name, S, S2))
    lens = []
    for n, L in ((n1, L1), (n2, L2)):
        a = np.full(S, L, np.int64) if n is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int64), (S,)))
        if a.min(initial=nlow) < nlow or a.max(initial=0) > L:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s: lengths outside %d .. %d" % (name, nlow, L))
        lens.append(a)
    return x1, st1, x2, st2, S, lens[0], lens[1]


def snr_db(sum_, err):
    """calcSNR's last line on the host: err > 0 ? 10 log10f(float(sum / err)) : FLT_MAX -> float32."""
    sum_, err = np.asarray(sum_, np.float64), np.asarray(err, np.float64)
    f = _lib.lib().btk_obj_snr_db
    return np.array([f(float(s), float(e)) for s, e in zip(sum_.ravel(), err.ravel())], np.float32).reshape(sum_.shape)


def snr(x1, x2, n1=None, n2=None, option=0, segment=None):
    """calcSNR for S pairs, x1 the clean and x2 the enhanced signals (float32 cuda [S][samples], inputs left as they are) ->
    (snr float32 [S], stats float64 [S][6] = mu1, mu2, a1, a2, sum, err) on the host; with segment=L also the rows
    sum_b, err_b float64 cuda [S][B][2] of the whole L-sample segments below min(n1, n2), B = max over the pairs (a pair's rows
    beyond its own floor(nmin / L) are NaN)."""
    x1, st1, x2, st2, S, n1, n2 = _obj_pair(x1, x2, n1, n2, "snr")
    dev = x1.device
    nmax = int(max(n1.max(), n2.max()))
    ws = torch.empty(max(_lib.lib().btk_obj_snr_workspace_bytes(S, nmax), 8) // 8, dtype=torch.float64, device=dev)
    stats = torch.empty((S, 6), dtype=torch.float64, device=dev)
    seg, L, B = None, 0, 0
    if segment is not None:
        L = int(segment)
        if L < 1:
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "snr: segment length %d" % L)
        B = int((np.minimum(n1, n2) // L).max())
        seg = torch.full((S, max(B, 1), 2), float("nan"), dtype=torch.float64, device=dev)
    check(_lib.lib().btk_obj_snr(_ptr(x1), st1, _ptr(x2), st2, S, _np_ptr(n1), _np_ptr(n2), int(option), _ptr(stats), L,
                                 _ptr(seg) if seg is not None else None, max(B, 1), _ptr(ws), _stream()))
    st = stats.cpu().numpy()
    out = (snr_db(st[:, 4], st[:, 5]), st)
    return out + (seg[:, :B],) if seg is not None else out


def segmental_snr(x1, x2, L, n1=None, n2=None, option=0, lo=-10.0, hi=35.0):
    """The segmental SNR (this project's definition; the reference's segmentalSNR class is empty): mean over the B whole
    segments of L samples below min(n1, n2) of 10 log10(sum_b / err_b) in float64 clamped to [lo, hi]; err_b = 0 gives hi,
    sum_b = 0 gives lo, B = 0 gives NaN -> (float64 [S] on the host, the rows as snr(..., segment=L) returns them)."""
    x1, st1, x2, st2, S, n1, n2 = _obj_pair(x1, x2, n1, n2, "segmental_snr")
    _, _, seg = snr(x1, x2, n1, n2, option, segment=L)
    rows = seg.cpu().numpy()
    out = np.full(S, np.nan, np.float64)
    for s in range(S):
        B = int(min(n1[s], n2[s]) // int(L))
        if B:
            out[s] = segment_db(rows[s, :B, 0], rows[s, :B, 1], lo, hi).mean()
    return out, seg


def segment_db(sum_b, err_b, lo=-10.0, hi=35.0):
    """10 log10(sum_b / err_b) in float64 clamped to [lo, hi]; err_b = 0 gives hi, else sum_b = 0 gives lo."""
    sum_b, err_b = np.asarray(sum_b, np.float64), np.asarray(err_b, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.clip(10.0 * np.log10(sum_b / err_b), lo, hi)
    v = np.where(sum_b == 0, lo, v)
    return np.where(err_b == 0, hi, v)


def is_distance(bank, x1, x2, n1=None, n2=None, bframe=0, eframe=-1, rows=False):
    """calcISDistance over the frames of an STFTBank, fused with the transform: -> (distance float64 cuda [S], frames in range
    int64 cuda [S]) and with rows=True also Eis float64 cuda [S][T], T = the largest min(F1, F2) (NaN beyond a pair's own)."""
    x1, st1, x2, st2, S, n1, n2 = _obj_pair(x1, x2, n1, n2, "is_distance", nlow=0)
    dev = x1.device
    T = max(int(bank.num_frames(int(np.minimum(n1, n2).max()))), 1)
    eis = torch.full((S, T), float("nan"), dtype=torch.float64, device=dev) if rows else torch.empty((S, T), dtype=torch.float64, device=dev)
    dist = torch.empty(S, dtype=torch.float64, device=dev)
    count = torch.empty(S, dtype=torch.int64, device=dev)
    check(_lib.lib().btk_obj_is_distance(bank._h, _ptr(x1), st1, _ptr(x2), st2, S, _np_ptr(n1), _np_ptr(n2), int(bframe), int(eframe),
                                         _ptr(dist), _ptr(count), _ptr(eis), T, _stream()))
    return (dist, count, eis) if rows else (dist, count)


# ---------------------------------------------------------------------------- multichannel cross-correlation localisation
MCC_RESET_COST = 100000.0            # the cost an N-best entry starts with (mcc_localizer.h:155); its index is -1
MCC_MAX_NBEST = 16


def mcc_max_sample_delay(fs, max_time_delay):
    """D = (size_t)(fs * maxTimeDelay), the float product of mcc_localizer.cc:273."""
    return int(_lib.lib().btk_mcc_max_sample_delay(int(fs), float(max_time_delay)))


def mcc_sample_delays(fs, delays):
    """tau = (int)(float)(fs * delay) per channel (mcc_localizer.cc:333-335): delays float64 [..., N] seconds -> int32."""
    d = np.ascontiguousarray(delays, np.float64)
    tau = np.zeros(d.shape, np.int32)
    if d.size:
        check(_lib.lib().btk_mcc_sample_delays(int(fs), d.size, _np_ptr(d), _np_ptr(tau)))
    return tau


def mcc_linear_grid(fs, N, spacing=None, positions=None):
    """The far-field walk of SGB4LinearArray (mcc_localizer.cc:54-161) for N microphones `spacing` mm apart or at `positions`
    (mm, [N][3], or [N] along the array's y axis) -> dict(azimuths float64 [G], delays float64 [G][N], tau int32 [G][N],
    D, max_time_delay, const_v)."""
    L = _lib.lib()
    pos = None
    if positions is not None:
        pos = np.asarray(positions, np.float64)
        if pos.ndim == 1:
            pos = np.stack([np.zeros_like(pos), pos, np.zeros_like(pos)], axis=1)
        pos = np.ascontiguousarray(pos)
        if pos.shape != (N, 3):
            raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "The size of the matrix for the geometry of the array should be %d x 3" % N)
    elif spacing is None:
        raise _lib.BtkError(_lib.BTK_ERR_PARAMETER, "mcc_linear_grid: give spacing or positions")
    args = (int(fs), int(N), _np_ptr(pos) if pos is not None else None, float(spacing or 0.0))
    n, mtd, cv = C.c_int(0), C.c_float(0), C.c_float(0)
    check(L.btk_mcc_linear_grid(*args, 0, C.byref(n), C.byref(mtd), C.byref(cv), None, None, None))
    G = n.value
    az, dl, tau = np.zeros(G, np.float64), np.zeros((G, N), np.float64), np.zeros((G, N), np.int32)
    check(L.btk_mcc_linear_grid(*args, G, C.byref(n), C.byref(mtd), C.byref(cv), _np_ptr(az), _np_ptr(dl), _np_ptr(tau)))
    return dict(azimuths=az, delays=dl, tau=tau, D=mcc_max_sample_delay(fs, mtd.value), max_time_delay=mtd.value, const_v=cv.value)


def _mcc_args(x, tau, L, name):
    if x.dim() == 2:
        x = x[None]
    _check(x, "x", torch.float32, 3)
    S, N, n = (int(v) for v in x.shape)
    tau = np.ascontiguousarray(tau.cpu().numpy() if isinstance(tau, torch.Tensor) else tau)
    if tau.ndim == 1:
        tau = tau[None]
    if tau.ndim != 2 or tau.shape[1] != N or not np.issubdtype(tau.dtype, np.integer):
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "%s: tau must be an integer array [G][%d], got %s %s" % (name, N, tau.dtype, tau.shape))
    tau = np.ascontiguousarray(tau, np.int32)
    L = int(L)
    B = n // L if L > 0 else 0
    tau_dev = torch.empty(tau.shape, dtype=torch.int32, device=x.device)
    return x, S, N, n, B, L, tau, tau_dev


def mcc_costs(x, tau, L, D, normalize_variance=True):
    """The MCC objective of every block and candidate (calcCovarianceMatrix + calcObjectiveFunction, mcc_localizer.cc:322-411).
    x float32 cuda [S][N][samples] (or [N][samples]) cut into B = samples // L blocks, tau int [G][N] sample delays, |tau| <= D
    -> (cost float64 [S][B][G], flag uint8 [S][B][G]); flag 1 and cost 0.0 where R is not positive definite or a channel is dead."""
    x, S, N, n, B, L, tau, tau_dev = _mcc_args(x, tau, L, "mcc_costs")
    G = tau.shape[0]
    cost = torch.empty((S, max(B, 0), G), dtype=torch.float64, device=x.device)
    flag = torch.empty((S, max(B, 0), G), dtype=torch.uint8, device=x.device)
    check(_lib.lib().btk_mcc_cost(_ptr(x), n, S, N, B, L, int(D), _np_ptr(tau), _ptr(tau_dev), G, 1 if normalize_variance else 0,
                                  _ptr(cost), _ptr(flag), _stream()))
    return cost, flag


def mcc_select(cost, nbest=1):
    """The N-best insertion of MCCLocalizer::search (mcc_localizer.cc:431-443) over the last axis of cost (float64 cuda
    [...][G]), in grid order with strict < -> (nbest_cost float64 [...][nbest], nbest_idx int32 [...][nbest]); entries nothing
    was inserted into keep (MCC_RESET_COST, -1)."""
    _need_cuda(cost, "cost")
    if cost.dtype != torch.float64 or cost.dim() < 1:
        raise _lib.BtkError(_lib.BTK_ERR_DIMENSION, "cost must be float64 [...][G]")
    G = int(cost.shape[-1])
    SB = int(cost.numel() // max(G, 1))
    nbest = int(nbest)
    shape = tuple(cost.shape[:-1]) + (max(nbest, 0),)
    nb_cost = torch.empty(shape, dtype=torch.float64, device=cost.device)
    nb_idx = torch.empty(shape, dtype=torch.int32, device=cost.device)
    check(_lib.lib().btk_mcc_select(_ptr(cost), SB, G, nbest, _ptr(nb_cost), _ptr(nb_idx), _stream()))
    return nb_cost, nb_idx


def mcc_matrices(x, tau, L, D, pairs):
    """R float64 cuda [P][N][N] of the (block, candidate) pairs in `pairs` (int [P][2]: s B + b, g): the sums mcc_costs works
    from, bit for bit, both triangles."""
    x, S, N, n, B, L, tau, tau_dev = _mcc_args(x, tau, L, "mcc_matrices")
    pairs = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), np.int32)
    P = pairs.shape[0]
    pairs_dev = torch.empty((max(P, 1), 2), dtype=torch.int32, device=x.device)
    R = torch.empty((P, N, N), dtype=torch.float64, device=x.device)
    check(_lib.lib().btk_mcc_matrices(_ptr(x), n, S, N, B, L, int(D), _np_ptr(tau), _ptr(tau_dev), tau.shape[0], _np_ptr(pairs),
                                      _ptr(pairs_dev), P, _ptr(R), _stream()))
    return R


def mcc_localize(x, tau, L, D, nbest=1, want_matrices=False):
    """MCCLocalizer::search for every block: costs of all candidates, then the N-best list -> dict with cost float64
    [S][B][G], flag uint8 [S][B][G], nbest_cost float64 [S][B][nbest], nbest_idx int32 [S][B][nbest] and, with
    want_matrices, R_best float64 [S][B][nbest][N][N] (NaN where the list entry is empty) and R_last float64 [S][B][N][N], the
    matrix of the last grid candidate (what getR() holds after next()).  Asking for the matrices waits for the indices."""
    cost, flag = mcc_costs(x, tau, L, D, True)
    nb_cost, nb_idx = mcc_select(cost, nbest)
    out = dict(cost=cost, flag=flag, nbest_cost=nb_cost, nbest_idx=nb_idx)
    if want_matrices:
        S, B, G = cost.shape
        N = x.shape[-2]
        idx = nb_idx.cpu().numpy().reshape(S * B, -1)
        pairs = np.zeros((S * B, idx.shape[1] + 1, 2), np.int32)
        pairs[:, :, 0] = np.arange(S * B)[:, None]
        pairs[:, :-1, 1] = np.maximum(idx, 0)
        pairs[:, -1, 1] = G - 1
        R = mcc_matrices(x, tau, L, D, pairs).reshape(S, B, idx.shape[1] + 1, N, N)
        Rb = R[:, :, :-1].clone()
        Rb[torch.from_numpy(idx.reshape(S, B, -1) < 0).to(Rb.device)] = float("nan")
        out["R_best"], out["R_last"] = Rb, R[:, :, -1].contiguous()
    return out
