"""GPU: btk_ekf_track (track_kernels.hip) through engine.ekf_track, frame by frame against btk20.pykalman's host classes (which
test_track_cpu.py pins to the reference bit for bit) on every case of tests/golden/pykalman_golden.npz; the state carried from
call to call; the device path of the Python classes and tools/source_tracking.py on the Kinect recording.

Bounds (the figures are in test_track_cpu.py's docstring and DESIGN.md 3.18):
  * flags (tracked, observed, updated, IEKF rounds) are equal: the fixtures keep every branch decision away from its
    threshold (test_track_cpu.py::test_fixture_margins);
  * sigmaK2 <= 1e6: x within 64 e_form (floor 1e-13) and K_filter within 64 e_form of K, e_form being the deviation of the O(P)
    form in numpy from the reference for that case and that quantity -- the margin covers the device's reduction order and its
    sin / cos / sqrt / lgamma, a few ulp per operation over at most 37 frames of a contracting recursion;
  * sigmaK2 = 1e10: the reference's own arithmetic is ill-conditioned there; x within 4 e_sens, e_sens being what the host
    classes themselves move by when the pairs are summed in reverse order; K_filter is not compared.
"""
import contextlib
import io
import json
import wave

import numpy as np
import pytest

from tests import track_closed_form as cf
from tests.test_track_cpu import CASES, NAMES, e_form_of, e_sens_of

pytestmark = pytest.mark.gpu

SINGLE = [n for n in NAMES if not n.startswith("stream")]


@pytest.fixture(scope="module")
def host():
    """the host classes on every case, once"""
    return {name: cf.run_host(CASES[name]) for name in NAMES}


def device_params(case):
    from distant_speech_recognition_amd import engine as eng
    p = case["params"]
    return eng.ekf_params(case["model"], case["type"], p["F"], p["U"], p["sigmaV2"], p["time_delta"], gate_prob=p["gate_prob"],
                          num_iterations=p["num_iterations"], iteration_threshold=p["iteration_threshold"], threshold=p["threshold"],
                          minimum_pairs=p["minimum_pairs"], Ts=p["Ts"], c=p["c"])


def initial_state(cases, dev):
    import torch
    from distant_speech_recognition_amd import engine as eng
    return torch.cat([eng.ekf_state(c["x0"], c["params"]["sigmaK2"] * np.identity(c["n"]), c["t_begin"], dev) for c in cases])


def run_device(cases, dev, split=None):
    """One launch for the streams `cases` (one configuration), or two consecutive ones split at frame `split`.
    -> per stream dict(x [T][n], K [T][n][n], flags [T]), and the final state records."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    c0, n = cases[0], cases[0]["n"]
    lag = torch.from_numpy(np.stack([c["lag"] for c in cases])).to(dev)
    height = torch.from_numpy(np.stack([c["height"] for c in cases])).to(dev)
    geom = torch.from_numpy(cf.pair_geometry(c0["model"], c0["mpos"], c0["pairs"])).to(dev)
    state = initial_state(cases, dev)
    prm = device_params(c0)
    tb = np.array([c["t_begin"] for c in cases], np.int32)
    parts = []
    bounds = [0, lag.shape[2]] if split is None else [0, split, lag.shape[2]]
    for a, b in zip(bounds[:-1], bounds[1:]):
        t_begin = torch.from_numpy(np.maximum(tb - a, 0).astype(np.int32)).to(dev)
        parts.append(eng.ekf_track(lag[:, :, a:b].contiguous(), height[:, :, a:b].contiguous(), geom, prm, state, t_begin))
    xk, Kf, fl = (torch.cat([p[i] for p in parts], dim=1).cpu().numpy() for i in range(3))
    out = [dict(x=xk[s][:, :n], K=Kf[s].reshape(-1, 3, 3)[:, :n, :n], flags=fl[s], xfull=xk[s], Kfull=Kf[s]) for s in range(len(cases))]
    return out, state.cpu().numpy()


def host_flags(h, case):
    from distant_speech_recognition_amd import engine as eng
    return (h["tracked"] * eng.EKF_TRACKED + h["observed"] * eng.EKF_OBSERVED + h["updated"] * eng.EKF_UPDATED +
            (h["rounds"] << eng.EKF_ROUNDS_SHIFT)).astype(np.int32)


def compare(case, got, h):
    name = case["name"]
    assert np.array_equal(got["flags"], host_flags(h, case)), name
    dx = float(np.abs(got["x"] - h["x"]).max())
    if case["params"]["sigmaK2"] == 1e10:
        es = e_sens_of(case)
        print("%s: |x - host| %.3g, e_sens %.3g" % (name, dx, es))
        assert dx <= 4 * es, name
        return
    ex, eK = e_form_of(case)
    dK = float(np.abs(got["K"] - h["K"]).max())
    print("%s: |x - host| %.3g (e_form %.3g), |K - host| %.3g (e_form %.3g)" % (name, dx, ex, dK, eK))
    assert dx <= max(64 * ex, 1e-13), name
    assert dK <= 64 * eK, name
    # outside the leading n x n block the outputs are zero
    n = case["n"]
    assert not got["xfull"][:, n:].any() and not got["Kfull"].reshape(-1, 3, 3)[:, n:, :].any() and \
        not got["Kfull"].reshape(-1, 3, 3)[:, :, n:].any()


@pytest.mark.parametrize("name", SINGLE)
def test_kernel_against_the_host_classes(dev, host, name):
    case = CASES[name]
    got, state = run_device([case], dev)
    compare(case, got[0], host[name])
    # the state record continues where the last frame ended
    T, n = case["lag"].shape[1], case["n"]
    assert np.array_equal(state[0, :n], got[0]["x"][-1]) and np.array_equal(state[0, 3:12], got[0]["Kfull"][-1])
    assert state[0, 12] == case["t_begin"] + (T - case["t_begin"])


def test_three_streams_with_their_own_first_frames(dev, host):
    cases = [CASES["stream%d" % i] for i in range(3)]
    got, _ = run_device(cases, dev)
    for c, g in zip(cases, got):
        compare(c, g, host[c["name"]])
        tb = c["t_begin"]
        assert not g["flags"][:tb].any() and np.array_equal(g["x"][:tb], np.tile(c["x0"], (tb, 1)))
    # a stream tracked on its own gives the bits it gives among others
    alone, _ = run_device(cases[1:2], dev)
    assert np.array_equal(alone[0]["xfull"], got[1]["xfull"]) and np.array_equal(alone[0]["Kfull"], got[1]["Kfull"])


@pytest.mark.parametrize("names", [[n] for n in SINGLE if CASES[n]["lag"].shape[1] == 37] + [["stream0", "stream1", "stream2"]],
                         ids=lambda v: v[0])
def test_state_carries_from_call_to_call(dev, names):
    """37 frames in one call and as 20 + 17 in two: the same bits"""
    cases = [CASES[n] for n in names]
    one, s1 = run_device(cases, dev)
    two, s2 = run_device(cases, dev, split=20)
    for a, b in zip(one, two):
        for k in ("flags", "xfull", "Kfull"):
            assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(s1, s2)


def test_error_reporting(dev):
    import torch
    from distant_speech_recognition_amd import _lib, engine as eng
    case = CASES["linear_ekf_k2"]
    lag = torch.from_numpy(case["lag"][None]).to(dev)
    height = torch.from_numpy(case["height"][None]).to(dev)
    geom = torch.from_numpy(cf.pair_geometry("linear", case["mpos"], case["pairs"])).to(dev)
    state = initial_state([case], dev)
    before = state.clone()

    def code(**change):
        prm = device_params(case)
        for k, v in change.items():
            setattr(prm, k, v)
        with pytest.raises(_lib.BtkError) as e:
            eng.ekf_track(lag, height, geom, prm, state)
        return e.value.code

    assert code(n=2) == _lib.BTK_ERR_PARAMETER and code(n=0) == _lib.BTK_ERR_PARAMETER
    assert code(model=3) == _lib.BTK_ERR_PARAMETER and code(type=2) == _lib.BTK_ERR_PARAMETER
    assert code(sigmaV2=0.0) == _lib.BTK_ERR_PARAMETER and code(c=0.0) == _lib.BTK_ERR_PARAMETER
    assert code(gate_prob=1.5) == _lib.BTK_ERR_PARAMETER and code(minimum_pairs=0) == _lib.BTK_ERR_PARAMETER
    assert code(type=1, num_iterations=0) == _lib.BTK_ERR_PARAMETER
    big = torch.zeros((1, 900, 2), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.BtkError) as e:
        eng.ekf_track(big, torch.zeros((1, 900, 2), dtype=torch.float32, device=dev),
                      torch.zeros((900, 6), dtype=torch.float64, device=dev), device_params(case), state)
    assert e.value.code == _lib.BTK_ERR_DIMENSION
    for bad in (dict(lag=lag.to(torch.int64)), dict(height=height.double()), dict(geom=geom[:5]), dict(state=state[:, :15].contiguous()),
                dict(t_begin=torch.zeros(2, dtype=torch.int32, device=dev))):
        args = dict(lag=lag, height=height, geom=geom, params=device_params(case), state=state)
        args.update(bad)
        with pytest.raises(_lib.BtkError) as e:
            eng.ekf_track(**args)
        assert e.value.code == _lib.BTK_ERR_DIMENSION
    assert torch.equal(state, before)                    # nothing was launched
    with pytest.raises(_lib.BtkError):
        eng.ekf_params("linear", "ekf", np.identity(2), np.identity(2), 1e-4, 0.1)


# ---- the Python classes and the tool on the Kinect recording ----------------------------------------------------------------------
FS, D, L, BLOCK = 16000, 256, 512, 64
KINECT_MPOS = [[-113.0, 0.0, 2.0], [36.0, 0.0, 2.0], [76.0, 0.0, 2.0], [113.0, 0.0, 2.0]]
KINECT_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
SCRIPT = dict(energy_threshold=100, minimum_pairs=3, cc_threshold=0.11, sigmaV2=4.0e-4, sigmaU2=10.0, sigmaK2=1.0e10, gate_prob=0.95,
              num_iterations=3, iteration_threshold=1e-4)


def kinect_front_end(pcm, block_frames=BLOCK):
    from btk20.feature import SampleFeaturePtr, HammingFeaturePtr, FFTFeaturePtr
    from btk20.pytdoa import make_tdoa_front_end
    chans = []
    for x in pcm:
        s = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
        s.set_samples(np.ascontiguousarray(x, np.float32))
        chans.append(FFTFeaturePtr(HammingFeaturePtr(s), L))
    return make_tdoa_front_end("linear", KINECT_PAIRS, chans, L, FS, np.array(KINECT_MPOS), SCRIPT["energy_threshold"],
                               SCRIPT["minimum_pairs"], SCRIPT["cc_threshold"], sspeed=343740.0, block_frames=block_frames)


@pytest.fixture(scope="module")
def kinect_run(dev, kinect_pcm):
    """the class-level run on the device path, as the tool makes it: (first frame, initial state, rows, tracker, tables)"""
    from tools import source_tracking as tool
    fe = kinect_front_end(kinect_pcm)
    first, initial = tool.first_detection(fe)
    settings = tool.Settings(dict(array_type="linear", microphone_positions=KINECT_MPOS,
                                  tracker=dict(SCRIPT, type="iekf", shiftlen=D, fftlen=L, pair_ids=KINECT_PAIRS)))
    trk = tool.build_tracker(fe, settings, initial.copy(), float(D) / FS)
    trk.set_time(first)
    rows, sink = [], io.StringIO()
    before = fe.launch_count
    with contextlib.redirect_stdout(sink):
        for xk in trk:
            rows.append(dict(x=np.array(xk), K=np.array(trk.K_filter), observed=trk.is_observed(), updated=trk.updated,
                             rounds=trk.rounds, tdoa=fe.mic_pair_tdoa(), last=trk.lastUpdateT, time=trk.time))
    # the same tables from a second front end, peak by peak
    fe2 = kinect_front_end(kinect_pcm)
    T = first + len(rows)
    lag = np.full((len(KINECT_PAIRS), T), cf.NO_PEAK, np.int64)
    height = np.zeros((len(KINECT_PAIRS), T), np.float32)
    for t in range(T):
        for p, src in enumerate(fe2._mic_pair_srcs):
            lg, h = src._src._src.peak(t)
            if lg is not None:
                lag[p, t], height[p, t] = lg, h
    return dict(first=first, initial=initial, rows=rows, trk=trk, fe=fe, lag=lag, height=height, T=T,
                front_end_launches=fe.launch_count - before, lines=sink.getvalue().count("Filtering innovation"))


def kinect_case(run):
    prm = dict(F=[[1.0]], U=[[SCRIPT["sigmaU2"]]], sigmaV2=SCRIPT["sigmaV2"], sigmaK2=SCRIPT["sigmaK2"], time_delta=float(D) / FS,
               gate_prob=SCRIPT["gate_prob"], num_iterations=3, iteration_threshold=1e-4, threshold=SCRIPT["cc_threshold"],
               minimum_pairs=SCRIPT["minimum_pairs"], Ts=1.0 / FS, c=343740.0)
    return dict(name="kinect", model="linear", type="iekf", n=1, x0=run["initial"].tolist(), t_begin=run["first"], params=prm,
                lag=run["lag"], height=run["height"], mpos=np.array(KINECT_MPOS), pairs=np.array(KINECT_PAIRS))


def test_device_path_of_the_classes(dev, kinect_run):
    run = kinect_run
    case, first, T = kinect_case(run), run["first"], run["T"]
    assert T >= 200
    margins = {}
    h = cf.run_host(case, margins=margins)
    rev = cf.run_host(case, order=list(range(len(KINECT_PAIRS)))[::-1])
    e_sens = float(np.abs(rev["x"] - h["x"]).max())
    got = {k: np.array([r[k] for r in run["rows"]]) for k in ("x", "observed", "updated", "rounds")}
    dx = float(np.abs(got["x"] - h["x"][first:]).max())
    cdf = np.array(margins["cdf"])
    print("kinect: %d frames from %d, %d observed, %d updated; |x - host| %.3g, e_sens %.3g, min |cdf - gate| %.3g" % (
        T - first, first, got["observed"].sum(), got["updated"].sum(), dx, e_sens, np.abs(cdf - SCRIPT["gate_prob"]).min()))
    for k in ("observed", "updated", "rounds"):
        assert np.array_equal(got[k], h[k][first:]), k
    assert got["observed"].sum() >= 20 and got["updated"].sum() >= 20
    assert dx <= 4 * e_sens
    assert run["lines"] == int((got["observed"] & ~got["updated"]).sum())
    # one tracker launch per block of the front end it touched; the front end's own two per block
    blocks = -(-T // BLOCK) - first // BLOCK
    assert run["trk"].launch_count == blocks
    assert run["front_end_launches"] == 2 * (blocks - (1 if first % BLOCK else 0))   # the scan for the start computed its block
    # attributes frame by frame, and the delays of the served frame
    for t, r in enumerate(run["rows"]):
        assert r["time"] == first + t + 1 and r["K"].shape == (1, 1)
        for p, (a, b) in enumerate(KINECT_PAIRS):
            lg = run["lag"][p, first + t]
            assert r["tdoa"][a][b] == (None if lg == cf.NO_PEAK else float(lg) * (1.0 / FS))   # as TDOAFeature.next forms it
    last = [first + t for t, r in enumerate(run["rows"]) if r["updated"]]
    assert run["rows"][-1]["last"] == last[-1]


def test_changed_state_restarts_the_block(dev, kinect_pcm):
    """set_time or a new xk_filter between two frames of a block: the rest of the block is tracked again from there, as the host
    path would continue"""
    from tools import source_tracking as tool
    fe = kinect_front_end(kinect_pcm)
    first, initial = tool.first_detection(fe)
    settings = tool.Settings(dict(array_type="linear", microphone_positions=KINECT_MPOS,
                                  tracker=dict(SCRIPT, type="iekf", shiftlen=D, fftlen=L, pair_ids=KINECT_PAIRS)))
    trk = tool.build_tracker(fe, settings, initial.copy(), float(D) / FS)
    trk.set_time(first)
    assert first % BLOCK + 7 < BLOCK                                  # the seven frames below lie in one block
    with contextlib.redirect_stdout(io.StringIO()):
        for t in range(first, first + 5):
            trk.next(t)
        assert trk.launch_count == 1
        trk.xk_filter = np.array([1.0])
        trk.next(first + 5)
        assert trk.launch_count == 2
        trk.next(first + 6)
        assert trk.launch_count == 2
    assert trk.time == first + 7


def write_wav(path, x):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(FS)
        w.writeframes(np.asarray(x, np.int16).tobytes())


def test_tool_writes_the_reference_layout(dev, kinect_pcm, kinect_run, tmp_path):
    from tools import source_tracking as tool
    paths = []
    for c in range(4):
        paths.append(str(tmp_path / ("c%d.wav" % (c + 1))))
        write_wav(paths[-1], kinect_pcm[c])
    conf = dict(array_type="linear", microphone_positions=KINECT_MPOS,
                tracker=dict(SCRIPT, type="iekf", shiftlen=D, fftlen=L, pair_ids=KINECT_PAIRS))
    conf_path = str(tmp_path / "conf.json")
    json.dump(conf, open(conf_path, "w"))
    prefix = str(tmp_path / "out" / "kinect")
    with contextlib.redirect_stdout(io.StringIO()):
        trk = tool.main(["-i"] + paths + ["-o", prefix, "-c", conf_path, "-r", str(FS)])
    tdoa = json.load(open(prefix + ".tdoa.json"))
    trj = json.load(open(prefix + ".trj.pos.json"))
    ave = json.load(open(prefix + ".ave.pos.json"))
    run = kinect_run
    first, rows = run["first"], run["rows"]
    assert trk.launch_count >= 1 and list(trj) == ["positions"] and list(ave) == ["positions"]
    assert len(tdoa) == len(rows) and [r[0] for r in tdoa] == pytest.approx([(first + t) * D / FS for t in range(len(rows))], abs=1e-9)
    seen = [(t, r) for t, r in enumerate(rows) if r["observed"]]
    assert len(trj["positions"]) == len(seen)
    for (sec, pos), (t, r) in zip(trj["positions"], seen):
        assert sec == pytest.approx((first + t) * D / FS, abs=1e-9) and pos == [float(r["x"][0]), None, None]
    mean = sum(float(r["x"][0]) for _, r in seen) / len(seen)
    assert ave["positions"][0][0] == 0.0 and ave["positions"][0][1][1:] == [None, None]
    assert ave["positions"][0][1][0] == pytest.approx(mean, rel=1e-12)
    for (sec, buf), r in zip(tdoa, rows):
        assert {int(a): {int(b): v for b, v in row.items()} for a, row in buf.items()} == r["tdoa"]
    with pytest.raises(NotImplementedError):
        tool.build_front_end(paths, tool.Settings(dict(conf, array_type="planar")), FS)
