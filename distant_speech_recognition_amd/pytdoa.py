"""btk20.pytdoa -- time delay of arrival (TDOA) features for microphone pairs, the reference's lib/pytdoa.py on this engine.

The names, constructor arguments and methods are the reference's: PHATFeature, TDOAFeature, MicrophonePair,
MicrophonePairObservation, MicrophonePairSource, TDOAFeatureVector, FarfieldLinearArrayTDOAFeatureVector,
FarfieldCircularArrayTDOAFeatureVector, are_collinear_and_consistent_direction, make_tdoa_front_end.

What runs where:
  * the phase transform, the inverse transform and the peak search of every pair are the GPU's (btk_tdoa_gcc_peaks); there is no
    host correlation;
  * make_tdoa_front_end over this package's FFTFeature nodes (each over a HammingFeature over a SampleFeature, one fft_len)
    builds a BATCHED front end: per block of frames the sample blocks of all channels are uploaded once, one btk_tdoa_spectra and
    one btk_tdoa_gcc_peaks launch cover every channel, pair and frame of the block, and next(frame_no), each pair's
    TDOAFeature.next(frame_no) and instantaneous_position(frame_no) are served from that block (launch_count counts: two per
    block, whatever the number of pairs);
  * over any other spectral source (any object with next(frame_no) and reset()) the spectra are pulled frame by frame and
    uploaded, and the same kernel runs on a one-frame block (one launch per frame for all pairs of a front end);
  * the position arithmetic per frame is host float64, a handful of scalars.

A TDOAFeature over a source that is no PHATFeature of this module (a correlation computed elsewhere) has no spectra to give to
the kernel: its peak is the first largest magnitude of that vector, found with numpy.
"""
import numpy
from numpy import linalg  # noqa: F401  (the reference's module exports it)

from .btk20.feature import *  # noqa: F401,F403
from .btk20.feature import FFTFeaturePtr
from .btk20cpp import jindex_error

__all__ = ["PHATFeature", "TDOAFeature", "MicrophonePair", "MicrophonePairObservation", "MicrophonePairSource",
           "TDOAFeatureVector", "are_collinear_and_consistent_direction", "FarfieldLinearArrayTDOAFeatureVector",
           "FarfieldCircularArrayTDOAFeatureVector", "make_tdoa_front_end"]

NO_POSITION = -1e10          # what instantaneous_position returns per coordinate where there is no estimate


class _PairEngine:
    """The spectra and peaks of a set of channel pairs, one frame number at a time, computed a block at a time."""

    def __init__(self, sources, pair_ids, fftlen, energy_threshold, batched=False, block_frames=None):
        self.fftlen, self.K = int(fftlen), int(fftlen) // 2 + 1
        self.threshold = float(energy_threshold)
        # channels are the distinct source objects the pairs name, in order of first use
        self.channels, index = [], {}
        self.pairs = []
        for a, b in pair_ids:
            for c in (a, b):
                if id(sources[c]) not in index:
                    index[id(sources[c])] = len(self.channels)
                    self.channels.append(sources[c])
            self.pairs.append((index[id(sources[a])], index[id(sources[b])]))
        self.batched = bool(batched) and self._nodes_ok()
        self.block_frames = int(block_frames) if block_frames else (self.channels[0].block_frames() if self.batched else 1)
        self.launch_count = 0
        self._pairs_dev = None
        self.block_serial = 0    # counts the blocks computed
        self._clear()

    def _nodes_ok(self):
        ch = self.channels
        return all(isinstance(c, FFTFeaturePtr) and c.has_sample_chain() and c.fftLen() == self.fftlen for c in ch) and \
            len(set(c.windowLen() for c in ch)) == 1

    def _clear(self):
        self.cur = -1            # frame number served last
        self.base = 0            # frame number of the block's first frame
        self.n = 0               # frames in the block
        self.X = self.energy = self.lag = self.height = None
        self.lag_dev = self.height_dev = None      # the block's peaks on the device, int32 / float32 [1][P][n]: what a tracker reads

    def reset(self):
        for c in self.channels:
            c.reset()
        self._clear()

    def _dev(self):
        from ._hostutil import device
        return device()

    def _next_block(self, frame_no):
        import torch
        from . import engine as eng
        dev = self._dev()
        if self._pairs_dev is None:
            self._pairs_dev = eng.tdoa_pairs(self.pairs, len(self.channels), dev)
        if self.batched:
            # channels of unequal length: the stream ends with the shortest one, on the frame where a per-frame graph would end
            # it (n is the smallest count; the next pull finds that chain ended).  The longer chains have then been advanced
            # past blocks nobody reads -- of no consequence, since nothing follows the end of the stream but reset().
            blocks = [c.pull_sample_blocks(self.block_frames) for c in self.channels]
            n = min(b.shape[0] for b in blocks)
            if n == 0:
                raise StopIteration
            D = blocks[0].shape[1]
            pcm = numpy.stack([b[:n].reshape(n * D) for b in blocks])[None]
            self.X, self.energy = eng.tdoa_spectra(torch.from_numpy(pcm).to(dev), D, self.fftlen)
            self.launch_count += 1
        else:
            rows = [numpy.asarray(c.next(frame_no)) for c in self.channels]        # StopIteration ends the stream
            if any(len(r) < self.K for r in rows):
                raise ValueError("a spectral source returned fewer than fftlen/2 + 1 = %d bins" % self.K)
            Xh = numpy.stack([r[:self.K] for r in rows]).astype(numpy.complex64)
            e = 2.0 * numpy.sum(Xh.real.astype(numpy.float64) ** 2 + Xh.imag.astype(numpy.float64) ** 2, axis=-1)
            n = 1
            self.X = torch.from_numpy(Xh[None, :, None, :]).to(dev)
            self.energy = torch.from_numpy(e.astype(numpy.float32)[None, :, None]).to(dev)
        lag, height = eng.tdoa_gcc_peaks(self.X, self.energy, self._pairs_dev, self.threshold)
        self.launch_count += 1
        self.lag, self.height = lag.cpu().numpy()[0], height.cpu().numpy()[0]
        self.lag_dev, self.height_dev = lag, height
        self.block_serial += 1
        self.base, self.n = frame_no, n

    def seek(self, frame_no):
        """Make frame_no the current frame: the same number again is served from the block, the next one advances."""
        if frame_no == self.cur:
            return self.cur - self.base
        if frame_no != self.cur + 1:
            raise jindex_error("TDOA front end: frame %d asked for after frame %d (frames are served in order)" % (frame_no, self.cur))
        if frame_no >= self.base + self.n:
            self._next_block(frame_no)
        self.cur = frame_no
        return self.cur - self.base

    def peak(self, frame_no, p):
        """(lag or None, height) of pair p."""
        from .engine import TDOA_NO_PEAK
        t = self.seek(frame_no)
        lag = int(self.lag[p, t])
        return (None, 0.0) if lag == TDOA_NO_PEAK else (lag, float(self.height[p, t]))

    def gcc(self, frame_no, p):
        """The correlation of pair p as float64 [fftlen]; zeros(1) where the frame is gated (as the reference returns it)."""
        from . import engine as eng
        t = self.seek(frame_no)
        X = self.X[:, :, t:t + 1, :].contiguous()
        e = self.energy[:, :, t:t + 1].contiguous()
        lag, _, g = eng.tdoa_gcc_peaks(X, e, [self.pairs[p]], self.threshold, want_gcc=True)
        g = g.cpu().numpy()[0, 0, 0].astype(numpy.float64)
        if int(lag.cpu().numpy()[0, 0, 0]) == eng.TDOA_NO_PEAK and not numpy.isnan(g[0]):
            return numpy.zeros(1, numpy.float64)
        return g


class PHATFeature:
    """The phase transform of one microphone pair: next(frame_no) is the generalised cross-correlation of the two spectral
    sources, zeros(1) where both frame energies are at or below energy_threshold."""

    def __init__(self, src1, src2, fftlen, energy_threshold=64, _engine=None, _pairx=0):
        self._src1, self._src2 = src1, src2
        self._fftlen2 = fftlen // 2
        self._energy_threshold = energy_threshold
        self._engine = _engine if _engine is not None else _PairEngine([src1, src2], [(0, 1)], fftlen, energy_threshold)
        self._pairx = _pairx
        self.reset()

    def next(self, frame_no):
        return self._engine.gcc(frame_no, self._pairx)

    def peak(self, frame_no):
        """(lag in samples or None, peak height) of the frame: what TDOAFeature reads, without the correlation leaving the GPU."""
        return self._engine.peak(frame_no, self._pairx)

    def __iter__(self):
        while True:
            try:
                block = self.next(self._isamp)
            except StopIteration:
                return
            yield block
            self._isamp += 1

    def reset(self):
        self._isamp = 0
        self._engine.reset()


class TDOAFeature:
    """Peak picking on a cross-correlation: next(frame_no) is [delay in seconds, peak height], [None, 0.0] without a peak."""

    def __init__(self, src, fftlen, samplerate):
        self._src = src
        self._fftlen, self._fftlen2 = fftlen, fftlen // 2
        self._Ts = 1.0 / samplerate
        self.reset()

    def next(self, frame_no):
        if isinstance(self._src, PHATFeature):
            lag, height = self._src.peak(frame_no)
        else:
            mag = numpy.abs(numpy.asarray(self._src.next(frame_no)))
            n = int(numpy.argmax(mag)) if len(mag) else 0            # the first of the largest
            if len(mag) and mag[n] > 0.0:
                lag, height = (n if n < self._fftlen2 else n - self._fftlen), float(mag[n])
            else:
                lag, height = None, 0.0
        if lag is None:
            return [None, 0.0]
        return [float(lag) * self._Ts, height]

    def __iter__(self):
        while True:
            try:
                item = self.next(self._isamp)
            except StopIteration:
                return
            yield item
            self._isamp += 1

    def reset(self):
        self._isamp = 0
        self._src.reset()


class MicrophonePair:
    """The index of a pair and of its two microphones (all from 0)."""

    def __init__(self, pairx, first_micx, second_micx):
        self.pairx, self.first_micx, self.second_micx = pairx, first_micx, second_micx


class MicrophonePairObservation(MicrophonePair):
    """A pair with its observation (the time delay)."""

    def __init__(self, pairx, first_micx, second_micx, observation):
        MicrophonePair.__init__(self, pairx, first_micx, second_micx)
        self.observation = observation


class MicrophonePairSource(MicrophonePair):
    """A pair with the feature that yields its [delay, peak height]."""

    def __init__(self, pairx, first_micx, second_micx, src):
        MicrophonePair.__init__(self, pairx, first_micx, second_micx)
        self._src = src

    def next(self, frame_no):
        return self._src.next(frame_no)

    def reset(self):
        self._src.reset()


class TDOAFeatureVector:
    """The delays of the pairs whose correlation peak exceeds `threshold`, as observations for a position estimate.
    mpos: one position row per microphone; c: speed of sound in position units per second."""

    def __init__(self, mic_pair_srcs, mpos, minimum_pairs=2, threshold=0.12, c=343000.0):
        self._mic_pair_srcs = mic_pair_srcs
        self._mpos = mpos
        self._minimum_pairs = minimum_pairs
        self._threshold = threshold
        self._c = c
        self._tdoabuf = {}
        self._tdoa_frame = None
        self._engine = None
        self.reset()

    @property
    def launch_count(self):
        """Kernel launches the batched front end has made (None for a vector built from foreign pair sources)."""
        return None if self._engine is None else self._engine.launch_count

    # -- the observation model a tracker linearises (positions Cartesian here; the subclasses use angles)
    def _distance(self, x, micx):
        d = x - self._mpos[micx]
        return numpy.sqrt(numpy.dot(d, d))

    def tdoa(self, mic_pair, x_cart):
        return (self._distance(x_cart, mic_pair.first_micx) - self._distance(x_cart, mic_pair.second_micx)) / self._c

    def calc_linearized_observation(self, xk_predict, H, observations):
        yk = numpy.zeros(len(observations), numpy.float64)
        for n, obs in enumerate(observations):
            yk[n] = obs.observation - (self.tdoa(obs, xk_predict) - numpy.dot(H[n, :], xk_predict))
        return yk

    def linearize(self, xk_predict, observations):
        H = numpy.zeros([len(observations), len(xk_predict)], numpy.float64)
        for rowx, obs in enumerate(observations):
            d1, d2 = xk_predict - self._mpos[obs.first_micx], xk_predict - self._mpos[obs.second_micx]
            H[rowx, :] = (d1 / numpy.sqrt(numpy.dot(d1, d1)) - d2 / numpy.sqrt(numpy.dot(d2, d2))) / self._c
        return H

    def _peaks(self, frame_no):
        """[(pair source, delay, height)] of the frame, in pair order."""
        out = []
        for src in self._mic_pair_srcs:
            delay, height = src.next(frame_no)
            out.append((src, delay, height))
        return out

    def next(self, frame_no):
        """The observations of the frame, or None where fewer than minimum_pairs peaks exceed the threshold; mic_pair_tdoa()
        then holds every pair's delay (None without a peak)."""
        observations, buf = [], {}
        for src, delay, height in self._peaks(frame_no):
            buf.setdefault(src.first_micx, {})[src.second_micx] = delay
            if height > self._threshold:
                observations.append(MicrophonePairObservation(src.pairx, src.first_micx, src.second_micx, delay))
        self._tdoabuf, self._tdoa_frame = buf, None
        return observations if len(observations) >= self._minimum_pairs else None

    def instantaneous_position(self, frame_no):
        """A position estimate without trajectory information: the array-specific subclasses provide it."""
        pass

    def mic_pair_tdoa(self):
        if self._tdoa_frame is not None:                 # a frame a tracker served from the device: the table is built on demand
            buf = {}
            for src, delay, _ in self._peaks(self._tdoa_frame):
                buf.setdefault(src.first_micx, {})[src.second_micx] = delay
            self._tdoabuf, self._tdoa_frame = buf, None
        return self._tdoabuf

    def _defer_tdoa(self, frame_no):
        """frame_no is the frame mic_pair_tdoa() is about (the engine's current one), without a next(frame_no) having run."""
        self._tdoa_frame = frame_no

    def _pair_geometry(self, row):
        """float64 [P][6]: row(pair source) -> up to six numbers per pair."""
        g = numpy.zeros((len(self._mic_pair_srcs), 6), numpy.float64)
        for p, src in enumerate(self._mic_pair_srcs):
            r = numpy.ravel(row(src))
            g[p, :len(r)] = r
        return g

    def _track_model(self):
        """(model name, per-pair geometry [P][6]) of engine.ekf_track: the two microphone positions."""
        return "cartesian", self._pair_geometry(lambda s: numpy.concatenate([self._mpos[s.first_micx][:3], self._mpos[s.second_micx][:3]]))

    def __iter__(self):
        while True:
            try:
                obs = self.next(self._isamp)
            except StopIteration:
                return
            yield obs
            self._isamp += 1

    def reset(self):
        self._isamp = 0
        for src in self._mic_pair_srcs:
            src.reset()


def are_collinear_and_consistent_direction(points):
    """True when all points lie on one line and every point lies on the same side of the first one: the normalised inner
    product of (p_1 - p_0) with every (p_i - p_0) is within 0.01 of one and not below it."""
    rel = numpy.array([p - points[0] for p in points])
    x0 = rel[1]
    n0 = numpy.sqrt(numpy.inner(x0, x0))
    for i in range(2, len(points)):
        nip = numpy.inner(x0, rel[i]) / (n0 * numpy.sqrt(numpy.inner(rel[i], rel[i])))
        if abs(nip - 1) > 0.01:
            print("point %d is off the line through points 0 and 1 (normalised inner product %g)" % (i, nip))
            return False
        if nip - 1 < 0:
            print("point %d lies on the other side of point 0 than point 1" % i)
            return False
    return True


class FarfieldLinearArrayTDOAFeatureVector(TDOAFeatureVector):
    """Linear array, far field: the state is the azimuth, a pair's delay is (d_second - d_first) cos(azimuth) / c with d the
    distance of a microphone from the first one."""

    def __init__(self, mic_pair_srcs, mpos, minimum_pairs=2, threshold=0.12, c=343000.0):
        TDOAFeatureVector.__init__(self, mic_pair_srcs, mpos, minimum_pairs, threshold, c)
        if not are_collinear_and_consistent_direction(mpos):
            raise ValueError("a linear array needs collinear microphone positions with the first microphone at one end")
        dist = numpy.zeros((len(mpos), 1), numpy.float64)
        for i in range(1, len(mpos)):
            d = mpos[i] - mpos[0]
            dist[i] = numpy.sqrt(numpy.dot(d, d))
        self._mpos = dist

    def _baseline(self, pair):
        return self._mpos[pair.second_micx] - self._mpos[pair.first_micx]

    def _track_model(self):
        return "linear", self._pair_geometry(self._baseline)

    def tdoa(self, mic_pair, azimuth):
        return numpy.array([self._baseline(mic_pair) * numpy.cos(azimuth) / self._c], numpy.float64)

    def calc_linearized_observation(self, azimuthk_predict, H, observations):
        yk = numpy.zeros(len(observations), numpy.float64)
        for n, obs in enumerate(observations):
            yk[n] = numpy.ravel(obs.observation - (self.tdoa(obs, azimuthk_predict) - numpy.inner(H[n, :], azimuthk_predict)))[0]
        return yk

    def linearize(self, azimuthk_predict, observations):
        H = numpy.zeros([len(observations), len(azimuthk_predict)], numpy.float64)
        for rowx, obs in enumerate(observations):
            H[rowx, :] = numpy.ravel(-self._baseline(obs) * numpy.sin(azimuthk_predict) / self._c)
        return H

    def instantaneous_position(self, frame_no):
        """[mean over the pairs above the threshold of arccos(clamp(delay c / baseline))], or [-1e10]."""
        total, count = 0.0, 0
        for src, delay, height in self._peaks(frame_no):
            if height > self._threshold:
                val = delay * self._c / self._baseline(src)[0]
                val = -1 if val < -1 else (1 if val > 1 else val)
                total += numpy.arccos(val)
                count += 1
        if count < self._minimum_pairs:
            return numpy.array([NO_POSITION])
        return numpy.array([total / float(count)])


class FarfieldCircularArrayTDOAFeatureVector(TDOAFeatureVector):
    """Circular (any non-linear) array, far field: the state is [polar angle, azimuth], a pair's delay is u . (p_second - p_first) / c
    with u the unit vector of that direction."""

    def __init__(self, mic_pair_srcs, mpos, minimum_pairs=2, threshold=0.12, c=343000.0):
        if len(mpos) == 2:
            raise ValueError("two microphones form a line: use FarfieldLinearArrayTDOAFeatureVector")
        for i, p in enumerate(mpos):
            assert len(p) >= 2, "microphone %d needs at least two position coordinates" % i
        TDOAFeatureVector.__init__(self, mic_pair_srcs, mpos, minimum_pairs, threshold, c)

    def _offset(self, pair):
        return self._mpos[pair.second_micx] - self._mpos[pair.first_micx]

    def _track_model(self):
        return "circular", self._pair_geometry(lambda s: self._offset(s)[:3])

    def tdoa(self, mic_pair, polarX):
        theta, phi = polarX[0], polarX[1]
        u = numpy.array([numpy.sin(theta) * numpy.cos(phi), numpy.sin(theta) * numpy.sin(phi), numpy.cos(theta)])
        return numpy.array([numpy.dot(u, self._offset(mic_pair)) / self._c], numpy.float64)

    def calc_linearized_observation(self, polarX, H, observations):
        yk = numpy.zeros(len(observations), numpy.float64)
        for n, obs in enumerate(observations):
            yk[n] = numpy.ravel(obs.observation - (self.tdoa(obs, polarX) - numpy.dot(H[n, :], polarX)))[0]
        return yk

    def linearize(self, polarX, observations):
        theta, phi = polarX[0], polarX[1]
        du_dtheta = numpy.array([numpy.cos(theta) * numpy.cos(phi), numpy.cos(theta) * numpy.sin(phi), -numpy.sin(theta)])
        du_dphi = numpy.array([-numpy.sin(theta) * numpy.sin(phi), numpy.sin(theta) * numpy.cos(phi), 0.0])
        H = numpy.zeros([len(observations), len(polarX)], numpy.float64)
        for rowx, obs in enumerate(observations):
            off = self._offset(obs)
            H[rowx, :] = numpy.array([numpy.dot(du_dtheta, off) / self._c, numpy.dot(du_dphi, off) / self._c])
        return H

    def instantaneous_position(self, frame_no):
        """[polar angle, azimuth] from the least-squares direction A = pinv(P) (c D) of the pairs above the threshold (rows of P:
        their offsets, D: their delays), clamped to [-1, 1] per component, or [-1e10, -1e10] where there is no valid solution.
        With every offset in a plane parallel to xy only A_x and A_y carry information; otherwise A_z takes part."""
        none = numpy.array([NO_POSITION, NO_POSITION])
        P, D = [], []
        for src, delay, height in self._peaks(frame_no):
            if height > self._threshold:
                P.append(self._offset(src))
                D.append(delay)
        if len(D) < self._minimum_pairs:
            return none
        P = numpy.array(P)
        A = numpy.clip(numpy.dot(numpy.linalg.pinv(P), numpy.array(D) * self._c), -1, 1)
        A2 = A * A
        lifted = numpy.count_nonzero(P[:, 2]) != 0
        sxy = A2[0] + A2[1]
        cos_theta2 = 1 - A2[0] - A2[1]
        if not lifted:
            if cos_theta2 < 0 or sxy == 0:
                return none
            theta = numpy.arccos(numpy.sqrt(cos_theta2))
            phi = numpy.arccos(numpy.sqrt(A2[0] / sxy))
            return numpy.array([theta, phi])
        if cos_theta2 + A[2] >= 0:
            theta = numpy.arccos(numpy.sqrt(cos_theta2 + A[2]) / 2.0)
        else:
            theta = numpy.arccos(A[2])
        # up to three expressions of cos^2(phi); the azimuth is the arccos of the mean of the valid roots
        cands = []
        if sxy != 0:
            cands.append(A2[0] / sxy)
        if A2[2] != 1:
            cands.append(-A2[0] / (A2[2] - 1))
            cands.append((A2[1] + A2[2] - 1) / (A2[2] - 1))
        roots = [numpy.sqrt(v) for v in cands if v >= 0]
        if not roots:
            return none
        total = 0.0
        for r in roots:
            total += r
        return numpy.array([theta, numpy.arccos(total / len(roots))])


def make_tdoa_front_end(array_type, pair_ids, spec_sources, fftlen, samplerate, mpos, energy_threshold, minimum_pairs, threshold,
                        sspeed=343000.0, block_frames=None):
    """The TDOA feature vector of an array type ('linear', 'circular'; 'planar' is not supported; anything else gives the plain
    TDOAFeatureVector) over one PHATFeature / TDOAFeature per pair of channel indices.  All pairs share one engine: over this
    package's FFTFeature nodes it computes whole blocks of frames (block_frames: the nodes' own by default)."""
    pair_ids = [(int(a), int(b)) for a, b in pair_ids]
    for a, b in pair_ids:
        assert a >= 0 and b >= 0, "pair (%d, %d): channel indices start at 0" % (a, b)
    engine = _PairEngine(spec_sources, pair_ids, fftlen, energy_threshold, batched=True, block_frames=block_frames)
    srcs = []
    for pairx, (a, b) in enumerate(pair_ids):
        phat = PHATFeature(spec_sources[a], spec_sources[b], fftlen, energy_threshold, _engine=engine, _pairx=pairx)
        srcs.append(MicrophonePairSource(pairx, a, b, TDOAFeature(phat, fftlen, samplerate)))
    if array_type == "planar":
        raise NotImplementedError("no TDOA feature vector for array type %r" % array_type)
    cls = {"linear": FarfieldLinearArrayTDOAFeatureVector, "circular": FarfieldCircularArrayTDOAFeatureVector}.get(array_type, TDOAFeatureVector)
    vec = cls(srcs, mpos, minimum_pairs, threshold, sspeed)
    vec._engine = engine
    return vec
