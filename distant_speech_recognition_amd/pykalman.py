"""btk20.pykalman -- conventional, extended and iterated extended Kalman filters for speaker tracking, the reference's
lib/pykalman.py on this engine.

The names, constructor arguments, attributes and methods are the reference's: KalmanFilter, ExtendedKalmanFilter,
IteratedExtendedKalmanFilter with xk_filter, K_filter, K_predict, time, lastUpdateT, is_observed(), set_time(), next(frame_no),
__iter__, predict, update, calc_innovation, filter_innovation, adjust_boundaries, within_room.

What runs where:
  * HOST PATH: float64, frame by frame, the reference's numpy calls in the reference's order (inv(S) of the nobs x nobs
    innovation covariance included).  It serves KalmanFilter (a fixed H) and every source that is not this package's batched
    TDOA front end, and it is what the GPU tests compare the kernel with.
  * DEVICE PATH: an ExtendedKalmanFilter / IteratedExtendedKalmanFilter over a feature vector of make_tdoa_front_end whose
    engine computes blocks of frames.  The lags and peak heights of the block stay on the GPU; when the tracker first asks for a
    frame of a block, ONE btk_ekf_track launch tracks the rest of that block (whatever the number of pairs), and next() serves
    xk_filter, K_filter, K_predict, the observed flag and the reference's 'Filtering innovation' line from its result.
    launch_count counts those launches.  Changing the tracker's state or time between two frames of a block is honoured: the
    rest of the block is tracked again from the changed state.

The gate is the reference's: scipy.stats.chi.cdf(d2, nobs) > gate_prob with d2 the SQUARED distance, i.e. the regularised
incomplete gamma function P(nobs / 2, d2^2 / 2) (scipy.special.gammainc here; the same number).
"""
from copy import deepcopy

import numpy

from .pytdoa import *  # noqa: F401,F403  (the reference's module re-exports pytdoa)
from . import pytdoa as _pytdoa

__all__ = list(_pytdoa.__all__) + ["KalmanFilter", "ExtendedKalmanFilter", "IteratedExtendedKalmanFilter"]


def _chi_cdf(x, df):
    """scipy.stats.chi.cdf(x, df): P(df / 2, x^2 / 2) for x > 0, else 0."""
    from scipy import special
    return float(special.gammainc(0.5 * df, 0.5 * x * x)) if x > 0 else 0.0


class KalmanFilter:
    """Conventional Kalman filter: source.next(frame_no) is the observation vector (None: no observation), H is fixed."""

    def __init__(self, source, F, U, sigmaV2, sigmaK2, time_delta, initialXk=None, H=None, gate_prob=0.0, boundaries=None):
        self.source = source
        self.F = deepcopy(F)
        self.H = H
        self.U = deepcopy(U)
        self.sigmaV2 = sigmaV2
        self.stateLength = F.shape[0]
        self.I = numpy.identity(self.stateLength, numpy.float64)
        self.time_delta = time_delta
        self.gate_prob = gate_prob
        self.boundaries = boundaries
        self.observed = False
        self.innovationFilter = self.gate_prob != 0.0
        self.K_filter = sigmaK2 * numpy.identity(self.stateLength, numpy.float64)
        self.K_predict = sigmaK2 * numpy.identity(self.stateLength, numpy.float64)
        self.lastUpdateT = -1
        self.time = -1
        self.xk_filter = numpy.zeros(self.stateLength, numpy.float64) if initialXk is None else initialXk

    def is_observed(self):
        return self.observed

    def within_room(self, x):
        if self.boundaries is None:
            return True
        for n in range(len(x)):
            if x[n] < self.boundaries[n][0] or x[n] > self.boundaries[n][1]:
                return False
        return True

    def calc_innovation(self, yk):
        self.S = numpy.dot(numpy.dot(self.H, self.K_predict), numpy.transpose(self.H)) + \
            self.sigmaV2 * numpy.identity(len(yk), numpy.float64)
        self.Sinv = numpy.linalg.inv(self.S)
        self.yk_hat = numpy.dot(self.H, self.xk_predict).flatten()
        self.s = yk - self.yk_hat

    def filter_innovation(self):
        """True where the innovation is to be left out (see the module text for the distribution)."""
        df = len(self.s)
        d2 = numpy.dot(self.s, numpy.dot(self.Sinv, self.s))
        self.gate_cdf = _chi_cdf(d2, df)
        return self.gate_cdf > self.gate_prob

    def predict(self):
        self.xk_predict = numpy.dot(self.F, self.xk_filter)

    def adjust_boundaries(self, xk_filter):
        """Fold the polar angle into [0, pi] and wrap the azimuth into [-pi, pi] (applied to every state, as the reference does)."""
        theta = xk_filter[0]
        phi = xk_filter[1] if len(xk_filter) > 1 else 0
        if theta < 0.0:
            theta = -theta
            phi += numpy.pi
        elif theta > numpy.pi:
            theta -= numpy.pi
            phi += numpy.pi
        if numpy.isfinite(phi):
            while phi < -numpy.pi:
                phi += 2.0 * numpy.pi
            while phi > numpy.pi:
                phi -= 2.0 * numpy.pi
        xk_filter[0] = theta
        if len(xk_filter) > 1:
            xk_filter[1] = phi
        return xk_filter

    def _gated(self):
        if self.filter_innovation():                                  # whatever gate_prob is, as in the reference
            print('Filtering innovation at time step %f' % self.time)
            return True
        return False

    def update(self, yk, elapsed_time):
        """The state update; False where the innovation was gated."""
        self.K_predict = numpy.dot(numpy.dot(self.F, self.K_filter), numpy.transpose(self.F)) + elapsed_time * elapsed_time * self.U
        self.calc_innovation(yk)
        self.rounds = 0
        if self._gated():
            return False
        self.G = numpy.dot(numpy.dot(self.K_predict, numpy.transpose(self.H)), self.Sinv)
        xk_filter = self.xk_predict + numpy.dot(self.G, self.s)
        self.xk_filter = self.adjust_boundaries(xk_filter)
        self.K_filter = numpy.dot((self.I - numpy.dot(self.G, self.H)), self.K_predict)
        self.lastUpdateT = self.time
        return True

    def _observe(self, observation):
        """The observation vector handed to update(): the source's own for the conventional filter."""
        return observation

    def _next_host(self, frame_no):
        self.predict()
        observation = self.source.next(frame_no)
        self.updated = False
        if observation is not None:
            yk = self._observe(observation)
            elapsed_time = (self.time - self.lastUpdateT) * self.time_delta
            self.updated = self.update(yk, elapsed_time)
            self.observed = True
        else:
            self.observed = False
        self.time += 1
        return self.xk_filter

    def next(self, frame_no):
        """Prediction, and correction where the frame has an observation."""
        return self._next_host(frame_no)

    def set_time(self, frame_no):
        self.time = frame_no

    def __iter__(self):
        while True:
            try:
                xk = self.next(self.time)
            except StopIteration:
                return
            yield xk


class ExtendedKalmanFilter(KalmanFilter):
    """Extended Kalman filter over a TDOA feature vector (its tdoa / linearize / calc_linearized_observation are the model)."""

    def __init__(self, source, F, U, sigmaV2, sigmaK2, time_delta, initialXk=None, gate_prob=0.0, boundaries=None):
        KalmanFilter.__init__(self, source, F, U, sigmaV2, sigmaK2, time_delta, initialXk, gate_prob=gate_prob, boundaries=boundaries)
        self.launch_count = 0
        self.use_device = None           # None: the device path where the source allows it; False: the host path always
        self._dev_block = None           # what the last launch left: see _track_block

    def _observe(self, observation):
        self.H = self.source.linearize(self.xk_predict, observation)
        return self.source.calc_linearized_observation(self.xk_predict, self.H, observation)

    # -- device path
    _TYPE = "ekf"

    def _on_device(self):
        if self.use_device is False:
            return False
        eng = getattr(self.source, "_engine", None)
        return eng is not None and eng.batched and \
            type(self.source) in (_pytdoa.TDOAFeatureVector, _pytdoa.FarfieldLinearArrayTDOAFeatureVector,
                                  _pytdoa.FarfieldCircularArrayTDOAFeatureVector)

    def _params(self):
        from . import engine as eng
        src = self.source
        model, _ = src._track_model()
        it = dict(num_iterations=self.num_iterations, iteration_threshold=self.iteration_threshold) if self._TYPE == "iekf" else {}
        return eng.ekf_params(model, self._TYPE, self.F, self.U, self.sigmaV2, self.time_delta, gate_prob=self.gate_prob,
                              threshold=src._threshold, minimum_pairs=src._minimum_pairs, Ts=src._mic_pair_srcs[0]._src._Ts,
                              c=src._c, **it)

    def _state_key(self):
        """What a launch starts from, to notice a state that was changed between two frames of a block."""
        return (self.time, self.lastUpdateT, numpy.asarray(self.xk_filter, numpy.float64).tobytes(),
                numpy.asarray(self.K_filter, numpy.float64).tobytes())

    def _track_block(self, t):
        """One launch for frames t .. of the engine's current block, from the object's present state."""
        import torch
        from . import engine as eng
        pe = self.source._engine
        dev = pe.lag_dev.device
        if getattr(self, "_geom_dev", None) is None:
            self._geom_dev = torch.from_numpy(numpy.ascontiguousarray(self.source._track_model()[1], numpy.float64)).to(dev)
        state = eng.ekf_state(self.xk_filter, self.K_filter, self.time, dev, last_update=self.lastUpdateT)
        tb = torch.tensor([t], dtype=torch.int32, device=dev)
        xk, Kf, flags = eng.ekf_track(pe.lag_dev, pe.height_dev, self._geom_dev, self._params(), state, tb)
        self.launch_count += 1
        self._dev_block = dict(serial=pe.block_serial, xk=xk.cpu().numpy()[0], Kf=Kf.cpu().numpy()[0], flags=flags.cpu().numpy()[0],
                               next_t=t, state=self._state_key())

    def _next_device(self, frame_no):
        from . import engine as eng
        pe = self.source._engine
        t = pe.seek(frame_no)                                         # StopIteration ends the stream
        b = self._dev_block
        if b is None or b["serial"] != pe.block_serial or b["next_t"] != t or b["state"] != self._state_key():
            self._track_block(t)
            b = self._dev_block
        n = self.stateLength
        fl = int(b["flags"][t])
        self.predict()
        self.observed = bool(fl & eng.EKF_OBSERVED)
        self.updated = bool(fl & eng.EKF_UPDATED)
        self.rounds = fl >> eng.EKF_ROUNDS_SHIFT
        if self.observed:
            el = (self.time - self.lastUpdateT) * self.time_delta
            self.K_predict = numpy.dot(numpy.dot(self.F, self.K_filter), numpy.transpose(self.F)) + el * el * self.U
            if not self.updated:
                print('Filtering innovation at time step %f' % self.time)
        if self.updated:
            self.xk_filter = b["xk"][t, :n].copy()
            self.K_filter = b["Kf"][t].reshape(3, 3)[:n, :n].copy()
            self.lastUpdateT = self.time
        self.source._defer_tdoa(frame_no)                             # mic_pair_tdoa() of the served frame
        self.time += 1
        b["next_t"], b["state"] = t + 1, self._state_key()
        return self.xk_filter

    def next(self, frame_no):
        """Prediction, linearisation at the prediction, and correction where the frame has an observation."""
        if self._on_device():
            return self._next_device(frame_no)
        return self._next_host(frame_no)


class IteratedExtendedKalmanFilter(ExtendedKalmanFilter):
    """Iterated extended Kalman filter: up to num_iterations rounds of the update around the same linearisation."""

    _TYPE = "iekf"

    def __init__(self, source, F, U, sigmaV2, sigmaK2, time_delta, initialXk=None, gate_prob=0.0, boundaries=None,
                 num_iterations=3, iteration_threshold=1e-4):
        ExtendedKalmanFilter.__init__(self, source, F, U, sigmaV2, sigmaK2, time_delta, initialXk, gate_prob=gate_prob,
                                      boundaries=boundaries)
        self.num_iterations = num_iterations
        self.iteration_threshold = iteration_threshold

    def update(self, yk, elapsed_time):
        eta = self.xk_predict
        self.K_predict = numpy.dot(numpy.dot(self.F, self.K_filter), numpy.transpose(self.F)) + elapsed_time * elapsed_time * self.U
        self.rounds = 0
        self.round_diffs = []
        for i in range(self.num_iterations):
            self.calc_innovation(yk)
            if self._gated():
                return False
            self.G = numpy.dot(numpy.dot(self.K_predict, numpy.transpose(self.H)), self.Sinv)
            zeta = self.s
            if i > 0:
                zeta -= numpy.dot(self.H, (self.xk_predict - eta))
            eta_prev = eta
            eta = self.xk_predict + numpy.dot(self.G, zeta)
            diff = eta - eta_prev
            self.rounds = i + 1
            self.round_diffs.append(float(numpy.inner(diff, diff)))
            if self.round_diffs[-1] < self.iteration_threshold:
                break
        self.xk_filter = self.adjust_boundaries(eta)
        self.K_filter = numpy.dot((self.I - numpy.dot(self.G, self.H)), self.K_predict)
        self.lastUpdateT = self.time
        return True
