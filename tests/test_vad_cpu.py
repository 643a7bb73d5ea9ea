"""CPU: the closed forms of tests/vad_closed_form.py against a literal, per-frame restatement of the reference's loops
(sad/sad.cc: np.sort of a copied window where the reference calls qsort, the memmove shift, the hangover buffer with its ring
index, the multi-stage walk), and the host-side functions of the engine: vad_band_limits and vad_segments_to_labels."""
import numpy as np
import pytest

from tests import vad_closed_form as cf


# ------------------------------------------------------------------ literal restatements (one object per reference class)
class RefEnergyVADMetric:
    def __init__(self, initial_energy, threshold, headN, tailN, energiesN):
        self.initial, self.headN, self.tailN, self.N = initial_energy, headN, tailN, energiesN
        self.recognizing, self.aboveN, self.belowN = False, 0, 0
        self.energies = np.full(energiesN, initial_energy, np.float64)
        self.medianX = int(threshold * energiesN)
        self.cur_score = None

    def above_threshold(self, vector):
        s = 0.0
        for n in range(len(vector)):
            val = float(vector[n])
            s += val * val
        sorted_e = np.sort(self.energies.copy())
        if not self.recognizing and self.aboveN == 0:
            self.energies[:-1] = self.energies[1:].copy()
            self.energies[-1] = s
        self.cur_score = s
        return s > sorted_e[self.medianX]

    def next(self, vector):
        if self.recognizing:
            if self.above_threshold(vector):
                self.belowN = 0
                return 1.0
            self.belowN += 1
            if self.belowN == self.tailN:
                self.recognizing, self.aboveN = False, 0
            return 0.0
        if self.above_threshold(vector):
            self.aboveN += 1
            if self.aboveN == self.headN:
                self.recognizing, self.belowN = True, 0
            return 1.0
        self.aboveN = 0
        return 0.0


def ref_band_metric(spectra, kind, fftLen, lowX, highX, E0):
    """one frame: spectra [C][powN] float32 -> (powers, score, +-1)"""
    chanN, total, powers = len(spectra), 0.0, []
    for sp in spectra:
        p = 0.0
        for k in range(lowX, highX + 1):
            if k == 0 or k == fftLen // 2 + 1:
                p += float(sp[k])
            else:
                p += 2.0 * float(sp[k])
        p /= fftLen
        total += np.sqrt(p) if kind == cf.NORMALIZED else p
        powers.append(p)
    with np.errstate(all="ignore"):
        if kind == cf.POWER:
            sc = np.float64(powers[0]) / total
            return powers, sc, (1.0 if sc > E0 / chanN else -1.0)
        if kind == cf.NORMALIZED:
            sc = np.sqrt(powers[0]) / total
            return powers, sc, (1.0 if sc > E0 / chanN else -1.0)
        sc = np.log(np.float64(powers[0]) / (total - powers[0])) - np.log(np.float64(E0) / total)
        return powers, sc, (1.0 if sc > 0 else -1.0)


class RefHangover:
    """HangoverVADFeature::next with its buffer; metric values come as rows [R][T]; rule picks above_threshold_"""

    def __init__(self, source, values, thresholds, rule, headN, tailN):
        self.source, self.values, self.thr, self.rule, self.headN, self.tailN = source, values, thresholds, rule, headN, tailN
        self.buffer = [None] * headN
        self.bufferX = self.bufferedN = self.aboveN = self.belowN = self.prefixN_ = 0
        self.recognizing, self.frame_no, self.decision_metric = False, -1, 0
        self.emitted = []                       # source frame numbers, in output order

    def prefixN(self):
        return self.prefixN_ - self.headN

    def _src(self, n):
        if n >= len(self.source):
            raise StopIteration
        return n

    def above_threshold(self, n):
        v = [row[n] for row in self.values]
        if self.rule == cf.SINGLE:
            return v[0] > self.thr[0]
        if self.rule == cf.MI:
            if v[0] < 0.5:
                self.decision_metric = -1
                return False
            if v[1] < 0.5:
                self.decision_metric = 2
                return True
            if v[2] > 0.5:
                self.decision_metric = 3
                return True
            self.decision_metric = -3
            return False
        if len(v) < 3:
            return False
        if v[0] < 0.5:
            self.decision_metric = -1
            return False
        for stageX in range(1, len(v)):
            if v[stageX] > 0.5:
                self.decision_metric = stageX + 1
                return True
            self.decision_metric = -(stageX + 1)
        self.decision_metric = -len(v)
        return False

    def next(self):
        """returns the source frame number served; StopIteration at the source's end; 'end' on the tailN-th miss"""
        frame_no = self.frame_no + 1
        if self.recognizing:
            if self.bufferedN > 0:
                vec = self.buffer[self.bufferX]
                self.bufferX = (self.bufferX + 1) % self.headN
                self.bufferedN -= 1
                self.frame_no += 1
                return vec
            vec = self._src(frame_no + self.prefixN())
            if self.above_threshold(frame_no + self.prefixN()):
                self.belowN = 0
            else:
                self.belowN += 1
                if self.belowN == self.tailN:
                    return "end"
            self.frame_no += 1
            return vec
        while True:
            vec = self._src(self.prefixN_)
            self.buffer[self.bufferX] = vec
            self.bufferX = (self.bufferX + 1) % self.headN
            self.bufferedN = min(self.headN, self.bufferedN + 1)
            n = self.prefixN_
            self.prefixN_ += 1
            if self.above_threshold(n):
                self.aboveN += 1
                if self.aboveN == self.headN:
                    self.recognizing = True
                    vec = self.buffer[self.bufferX]
                    self.bufferX = (self.bufferX + 1) % self.headN
                    self.bufferedN -= 1
                    self.frame_no += 1
                    return vec
            else:
                self.aboveN = 0

    def drain(self):
        out = []
        try:
            while True:
                f = self.next()
                if f == "end":
                    return out, True
                out.append(f)
        except StopIteration:
            return out, False


def ref_label_loop(T, time_delta, target_labs):
    """the label loop of accu_stats_from_label (lib/pybeamformer.py:967-985): True where the frame is a target"""
    elapsed, labx, out = 0.0, 0, []
    for _ in range(T):
        is_target = False
        if labx < len(target_labs):
            if elapsed >= target_labs[labx][0] and (elapsed <= target_labs[labx][1] or target_labs[labx][1] < 0):
                is_target = True
            elif elapsed > target_labs[labx][1]:
                labx += 1
        out.append(is_target)
        elapsed += time_delta
    return np.array(out)


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("D", [1, 7, 160])
def test_frame_energy(D):
    rng = np.random.default_rng(D)
    x = (rng.normal(size=(2, 9, D)) * 100).astype(np.float32)
    z = (rng.normal(size=(2, 9, D)) + 1j * rng.normal(size=(2, 9, D))).astype(np.complex64)
    e, ez = cf.frame_energy(x), cf.frame_energy(z)
    for s in range(2):
        for t in range(9):
            a = b = 0.0
            for n in range(D):
                v = float(x[s, t, n])
                a += v * v
                b += float(z[s, t, n].real) * float(z[s, t, n].real) + float(z[s, t, n].imag) * float(z[s, t, n].imag)
            assert e[s, t] == a and ez[s, t] == b


@pytest.mark.parametrize("energiesN", [1, 5, 200])
@pytest.mark.parametrize("headN,tailN", [(1, 1), (4, 10), (10, 4), (1, 10), (4, 1)])
@pytest.mark.parametrize("threshold", [0.0, 0.5, 0.995])
def test_energy_metric(energiesN, headN, tailN, threshold):
    rng = np.random.default_rng(energiesN * 100 + headN * 10 + tailN)
    S, T, D = 3, 60, 5
    x = rng.normal(size=(S, T, D)).astype(np.float32)
    x[:, 20:35] *= 30.0                                     # a burst, so that the machine moves
    x[1, 40:44] *= 30.0
    energy = cf.frame_energy(x)
    initial = float(np.median(energy))
    st = cf.EnergyMetricState(S, energiesN, initial)
    got = np.concatenate([cf.energy_metric(energy[:, :23], st, threshold, headN, tailN),
                          cf.energy_metric(energy[:, 23:], st, threshold, headN, tailN)], axis=1)
    for s in range(S):
        ref = RefEnergyVADMetric(initial, threshold, headN, tailN, energiesN)
        want = np.array([ref.next(x[s, t]) for t in range(T)])
        assert np.array_equal(got[s], want)
        assert np.array_equal(st.window[s], ref.energies)
        assert (st.recognizing[s], st.above[s], st.below[s]) == (ref.recognizing, ref.aboveN, ref.belowN)
    assert 0 < got.sum() < got.size or threshold in (0.0, 0.995)


@pytest.mark.parametrize("kind", [cf.POWER, cf.NORMALIZED, cf.TSPS])
@pytest.mark.parametrize("M,low,high", [(16, -1, -1), (64, 187, 1000), (16, 0, 7999.9)])
def test_band_power(kind, M, low, high):
    rng = np.random.default_rng(M + kind)
    S, Cn, T = 2, 4, 11
    spec = (rng.chisquare(2, size=(S, Cn, T, M)) * 1e4).astype(np.float32)
    lowX, highX, _ = cf.band_limits(M, 16000.0, low, high)
    P = cf.band_power(spec, M, lowX, highX)
    score, value = cf.band_decision(P, kind)
    for s in range(S):
        for t in range(T):
            p, sc, v = ref_band_metric([spec[s, c, t] for c in range(Cn)], kind, M, lowX, highX, cf.E0_DEFAULT[kind])
            assert np.array_equal(P[s, :, t], np.array(p)) and score[s, t] == sc and value[s, t] == v


def test_band_limits_closed_form_and_engine():
    from distant_speech_recognition_amd import _lib, engine
    assert engine.vad_band_limits(512, 16000, -1, -1) == (0, 256, 513) == cf.band_limits(512, 16000.0, -1, -1)
    # 187 / 16000 x 512 = 5.98 -> 5 (truncated); 1000 / 16000 x 512 + 0.5 = 32.5 -> 32; lowX > 0: 2 (32 - 5 + 1)
    assert engine.vad_band_limits(512, 16000, 187, 1000) == (5, 32, 56) == cf.band_limits(512, 16000.0, 187, 1000)
    # 7999.9 / 16000 x 512 + 0.5 = 256.4968 -> 256
    assert engine.vad_band_limits(512, 16000, 0, 7999.9) == (0, 256, 513) == cf.band_limits(512, 16000.0, 0, 7999.9)
    for lo, hi in [(0, 8000), (8000, -1)]:
        with pytest.raises(_lib.BtkError) as e:
            engine.vad_band_limits(512, 16000, lo, hi)
        assert e.value.code == _lib.BTK_ERR_DIMENSION
        with pytest.raises(ValueError):
            cf.band_limits(512, 16000.0, lo, hi)


def test_simple_energy():
    rng = np.random.default_rng(5)
    energy = rng.chisquare(8, size=(2, 40)) * 1e3
    energy[:, 15:20] *= 50
    sp, sm = cf.simple_energy(energy, np.zeros(2), 2.0, 0.98)
    for s in range(2):
        se = 0.0
        for t in range(40):
            se = 0.98 * se + (1.0 - 0.98) * energy[s, t]
            assert sm[s, t] == se and sp[s, t] == ((energy[s, t] / se) > 2.0)
    assert sp[:, 0].all() and 0 < sp.sum() < sp.size          # the first frame gives E / ((1 - gamma) E) = 50 > 2


def _random_values(rng, R, T, p=0.6):
    v = np.where(rng.random((R, T)) < p, 1.0, 0.0)
    v[1:] = 2.0 * v[1:] - 1.0                               # later stages: +-1, as the power metrics return
    return v


@pytest.mark.parametrize("headN", [1, 4, 10])
@pytest.mark.parametrize("tailN", [1, 4, 10])
@pytest.mark.parametrize("rule,R", [(cf.SINGLE, 1), (cf.MI, 3), (cf.MULTISTAGE, 3), (cf.MULTISTAGE, 5), (cf.MULTISTAGE, 2)])
def test_hangover(headN, tailN, rule, R):
    for seed in range(6):
        rng = np.random.default_rng(seed * 1000 + headN * 100 + tailN * 10 + R)
        T = 60
        values = _random_values(rng, R, T, p=[0.5, 0.8, 0.9][seed % 3])
        thr = [0.5] * R
        above, code = cf.detections(values, thr, rule)
        segs = cf.hangover_segments(above, headN, tailN)
        ref = RefHangover(list(range(T)), values, thr, rule, headN, tailN)
        emitted, ended = ref.drain()
        if not segs:
            assert emitted == [] and not ended
            continue
        start, end = segs[0]
        assert emitted == list(range(start, T if end is None else end))
        assert ended == (end is not None) and ref.prefixN() == start
        # decision_metric() after the last frame the reference evaluated
        last = (end if end is not None else T - 1)
        assert ref.decision_metric == code[last]
        if rule == cf.MULTISTAGE and R < 3:
            assert not above.any()


def test_hangover_restart_is_the_machine_started_again():
    rng = np.random.default_rng(11)
    above = rng.random(60) < 0.7
    segs = cf.hangover_segments(above, 2, 2, restart=True)
    assert len(segs) >= 2
    t0, want = 0, []
    while t0 < 60:                                          # the machine run again from the frame after each end
        ref = RefHangover(list(range(60 - t0)), [np.where(above[t0:], 1.0, 0.0)], [0.5], cf.SINGLE, 2, 2)
        emitted, ended = ref.drain()
        if not emitted:
            break
        want.append((t0 + emitted[0], t0 + emitted[-1] + 1 if ended else None))
        if not ended:
            break
        t0 = t0 + emitted[-1] + 2
    assert segs == want


@pytest.mark.parametrize("shiftlen,samplerate", [(128, 16000), (160, 44100), (256, 48000)])
def test_segments_to_labels_against_the_label_loop(shiftlen, samplerate):
    from distant_speech_recognition_amd import engine
    T = 500
    for segs in ([(0, 5)], [(3, 40), (41, 42), (100, 350)], [(7, 8)], [(10, 20), (22, 500)], [(499, 500)], []):
        labels = engine.vad_segments_to_labels(segs, shiftlen, samplerate)
        want = np.zeros(T, bool)
        for a, b in segs:
            want[a:b] = True
        got = ref_label_loop(T, shiftlen / float(samplerate), labels)
        assert np.array_equal(got, want), segs
        assert labels == cf.segments_to_labels(segs, shiftlen, samplerate)


def test_tsps_closed_form_leaves_out_nothing_on_chi2_spectra():
    """the decision margin of tests/test_gpu_vad.py, checked on the float64 side alone"""
    rng = np.random.default_rng(3)
    spec = (rng.chisquare(2, size=(3, 4, 300, 257)) * 1e4).astype(np.float32)
    P = cf.band_power(spec, 512, 0, 256)
    score, _ = cf.band_decision(P, cf.TSPS)
    bound = 64 * 2.0 ** -52 * cf.tsps_terms(P)
    assert np.isfinite(score).all() and not (np.abs(score) <= bound).any()
