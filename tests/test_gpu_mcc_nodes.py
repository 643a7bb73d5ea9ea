"""GPU: the node classes of btk20.localization (host/src/mcc_nodes.cc) against engine.mcc_localize / mcc_costs on the same
blocks, and tools/mcc_localizer.py on the committed Kinect recording against the closed form of tests/mcc_closed_form.py.

The nodes call the entry points the engine functions call, on the same float32 samples: positions, delays, costs and matrices
are compared with ==, whatever the number of frames pulled ahead.  getEigenValues() is a host Jacobi over the downloaded R:
within 64 float64 ulp of the largest eigenvalue of numpy.linalg.eigvalsh of that R.

A recording may hold blocks of digital silence (every candidate is flagged, cost 0.0, grid point 0 stays first) and has tied
rows, so the tool's winners are compared with the closed form's under the rule of tests/test_gpu_mcc.py: the delays of the best
candidate are equal wherever the closed form's runner-up with another tau row lies more than twice the cost bound away; at most
5 % of the blocks may be left out.  At 4096 samples per block the committed Kinect recording has no silent block and the rule
leaves none out (smallest gap 6.3e-4 against a bound of at most 8.2e-11; measured on an MI355X: 19 blocks, 0 silent, 0 left out)."""
import json

import numpy as np
import pytest

from tests import mcc_closed_form as cf
from tests.test_gpu_mcc import cost_bound

pytestmark = pytest.mark.gpu

FS, N, L, SPACING, FRAMES = 16000, 8, 6 + 64 * 4 + 1, 20.0, 7
KINECT_MM = [-113.0, 36.0, 76.0, 113.0]


class ArraySource:
    """An array-backed float source: size() / __iter__ / next() / reset()."""

    def __init__(self, x, L):
        self.x, self.L, self.at, self.resets = np.ascontiguousarray(x, np.float32), L, 0, 0

    def size(self):
        return self.L

    def reset(self):
        self.at = 0
        self.resets += 1

    def __iter__(self):
        return self

    def __next__(self):
        if self.at + self.L > len(self.x):
            raise StopIteration
        self.at += self.L
        return self.x[self.at - self.L:self.at]

    next = __next__


@pytest.fixture(scope="module")
def loc_mod(dev):
    import btk20.localization as m
    return m


@pytest.fixture(scope="module")
def signal():
    grid = cf.linear_grid(FS, N, SPACING)
    rng = np.random.default_rng(11)
    x = np.concatenate([cf.synthetic(rng, N, L, grid["tau"][g]) for g in (4, 4, 9, 0, 12, 6, 9)], axis=1)
    assert x.shape == (N, FRAMES * L)
    return x, grid


@pytest.fixture(scope="module")
def expected(dev, signal):
    import torch
    from distant_speech_recognition_amd import engine as eng
    x, grid = signal
    taus = eng.mcc_linear_grid(FS, N, spacing=SPACING)
    out = eng.mcc_localize(torch.from_numpy(x).to(dev), taus["tau"], L, taus["D"], nbest=3, want_matrices=True)
    return taus, {k: v.cpu().numpy()[0] for k, v in out.items()}


def _localizer(m, x, nbest, block_frames):
    g = m.SGB4LinearArrayPtr(N, True, FS)
    g.setDistanceBtwMicrophones(SPACING)
    loc = m.MCCLocalizerPtr(g, maxSource=nbest)
    srcs = [ArraySource(x[c], L) for c in range(N)]
    for s in srcs:
        loc.setChannel(s)
    loc.set_block_frames(block_frames)
    return loc, g, srcs


@pytest.mark.parametrize("block_frames", [1, 3, 0])
def test_localizer_serves_what_the_engine_computes(loc_mod, signal, expected, block_frames):
    x, _ = signal
    taus, want = expected
    loc, g, _ = _localizer(loc_mod, x, 3, block_frames)
    assert loc.size() == 3
    end_az = taus["azimuths"][-1]
    for f in range(FRAMES):
        pos = loc.next()
        idx = want["nbest_idx"][f]
        assert list(pos) == [0.0, taus["azimuths"][idx[0]], 0.0] and np.array_equal(loc.getPosition(), pos)
        assert loc.frame_no() == f
        for j in range(3):
            assert loc.getNthBestPosition(j)[1] == taus["azimuths"][idx[j]]
            assert [loc.getNthBestDelayedSample(j, c) for c in range(N)] == list(taus["tau"][idx[j]])
            assert abs(loc.getNthBestMCCC(j) - (1 - np.exp(want["nbest_cost"][f, j]))) <= 4 * np.spacing(1.0)     # the two exp
        assert loc.getMaxMCCC() == loc.getNthBestMCCC(0) and loc.getDelayedSample(N - 1) == taus["tau"][idx[0]][N - 1]
        assert np.array_equal(loc.getR(), want["R_last"][f])
        ev = loc.getEigenValues()
        ref = np.linalg.eigvalsh(want["R_best"][f, 0])
        assert np.all(np.diff(ev) >= 0) and np.max(np.abs(ev - ref)) <= 64 * np.spacing(ref[-1])
        assert g.getSearchPosition()[1] == end_az          # the builder stands where the walk ends
    with pytest.raises(StopIteration):
        loc.next()
    assert loc.is_end()
    assert loc.launches() == {1: 7, 3: 3, 0: 1}[block_frames]


def test_iterator_protocol_and_reset_replay(loc_mod, signal, expected):
    x, _ = signal
    taus, want = expected
    loc, g, srcs = _localizer(loc_mod, x, 1, 3)
    first = [p.copy() for p in loc]
    assert len(first) == FRAMES and [p[1] for p in first] == [taus["azimuths"][i] for i in want["nbest_idx"][:, 0]]
    loc.reset()
    assert g.getSearchPosition()[1] == 0.0 and all(s.at == 0 for s in srcs)
    a = loc.next().copy()
    b = loc.next(loc.frame_no()).copy()                   # the same frame again
    assert np.array_equal(a, first[0]) and np.array_equal(b, a) and loc.frame_no() == 0
    again = [p.copy() for p in loc]                       # __iter__ resets: a full replay from a half-served block
    assert len(again) == FRAMES and all(np.array_equal(p, q) for p, q in zip(first, again))


def test_short_frames_and_wrong_channel_counts_raise(loc_mod, signal):
    x, _ = signal
    g = loc_mod.SGB4LinearArrayPtr(N, True, FS)
    g.setDistanceBtwMicrophones(SPACING)                    # D = 6
    loc = loc_mod.MCCLocalizerPtr(g)
    for c in range(N):
        loc.setChannel(ArraySource(x[c], 11))               # L = 2 D - 1
    with pytest.raises(Exception, match="insufficient"):
        loc.next()
    few = loc_mod.MCCLocalizerPtr(g)
    few.setChannel(ArraySource(x[0], L))
    with pytest.raises(Exception, match="channels"):
        few.next()
    with pytest.raises(Exception):
        loc_mod.MCCLocalizerPtr(g, maxSource=17)


def test_calculator_cost_mccc_and_delay_changes(dev, loc_mod, signal):
    import torch
    from distant_speech_recognition_amd import engine as eng
    x, grid = signal
    x = x[:, :6 * L]
    xd = torch.from_numpy(x).to(dev)
    D = grid["D"]
    d1, d2 = grid["delays"][4], grid["delays"][9]
    t1, t2 = eng.mcc_sample_delays(FS, d1), eng.mcc_sample_delays(FS, d2)
    assert not np.array_equal(t1, t2)
    for normalize in (True, False):
        c1 = eng.mcc_costs(xd, t1, L, D, normalize_variance=normalize)[0].cpu().numpy()[0, :, 0]
        c2 = eng.mcc_costs(xd, t2, L, D, normalize_variance=normalize)[0].cpu().numpy()[0, :, 0]
        g = loc_mod.SGB4LinearArrayPtr(N, True, FS)
        g.setDistanceBtwMicrophones(SPACING)
        calc = loc_mod.MCCCalculatorPtr(g, normalizeVariance=normalize)
        for c in range(N):
            calc.setChannel(ArraySource(x[c], L))
        calc.set_block_frames(4)
        with pytest.raises(Exception, match="setTimeDelays"):
            calc.next()
        calc.setTimeDelays(d1)
        got = []
        for f in range(6):
            if f == 3:
                calc.setTimeDelays(delays=d2)                # after frame 2 of 6, one frame of the first batch still unserved
            v = calc.next()
            got.append(v[0])
            assert v[1] == 0.0 and v[2] == 0.0 and calc.getCostV() == v[0] and abs(calc.getMCCC() - (1.0 - np.exp(v[0]))) <= 4 * np.spacing(max(1.0, np.exp(v[0])))
            assert calc.getMaxMCCC() == calc.getMCCC()
            assert [calc.getDelayedSample(c) for c in range(N)] == list(t1 if f < 3 else t2)
            R = eng.mcc_matrices(xd, t1 if f < 3 else t2, L, D, [[f, 0]]).cpu().numpy()[0]
            assert np.array_equal(calc.getR(), R)
            ev, ref = calc.getEigenValues(), np.linalg.eigvalsh(R)
            assert np.max(np.abs(ev - ref)) <= 64 * np.spacing(ref[-1])
        assert got[:3] == list(c1[:3]) and got[3:] == list(c2[3:]), normalize
        assert not np.array_equal(c1[3:], c2[3:])
        assert calc.launches() == 3                          # two batches and the frames scored again
        with pytest.raises(StopIteration):
            calc.next()
    far = loc_mod.MCCCalculatorPtr(g)
    for c in range(N):
        far.setChannel(ArraySource(x[c], L))
    far.setTimeDelays(np.full(N, (D + 1.5) / FS))            # |tau| = D + 1: the reference would read outside its buffers
    with pytest.raises(Exception, match="outside"):
        far.next()


def test_grid_builder_through_the_binding(dev, loc_mod):
    from distant_speech_recognition_amd import engine as eng
    for n, spacing, positions in ((8, 20.0, None), (4, None, KINECT_MM)):
        want = eng.mcc_linear_grid(FS, n, spacing=spacing, positions=positions)
        g = loc_mod.SGB4LinearArrayPtr(nChan=n, isFarField=True, samplingFreq=FS)
        if positions is None:
            g.setDistanceBtwMicrophones(distance=spacing)
        else:
            g.setPositionsOfMicrophones(mpos=np.array([[0.0, y, 0.0] for y in positions]))
        assert g.chanN() == n and g.samplingFrequency() == FS and g.maxTimeDelay() == want["max_time_delay"]
        az, dl = [g.getSearchPosition()[1]], [g.getTimeDelays().copy()]
        while g.nextSearchGrid():
            az.append(g.getSearchPosition()[1])
            dl.append(g.getTimeDelays().copy())
        assert not g.nextSearchGrid() and g.getSearchPosition()[1] == az[-1]
        assert np.array_equal(az, want["azimuths"]) and np.array_equal(np.array(dl), want["delays"])
        g.reset()
        assert list(g.getSearchPosition()) == [0.0, 0.0, 0.0] and np.array_equal(g.getTimeDelays(), want["delays"][0])
    base = loc_mod.SearchGridBuilderPtr(4, True)
    assert base.getTimeDelays() is None and not base.nextSearchGrid() and base.maxTimeDelay() == -1.0
    near = loc_mod.SGB4LinearArrayPtr(4, False)
    near.setDistanceBtwMicrophones(40.0)
    with pytest.raises(Exception, match="need to be implemented"):
        near.nextSearchGrid()


def test_star_import_gives_the_four_names(dev):
    ns = {}
    exec("from btk20.localization import *", ns)
    for name in ("SearchGridBuilderPtr", "SGB4LinearArrayPtr", "MCCLocalizerPtr", "MCCCalculatorPtr"):
        assert name in ns
    import btk20
    assert btk20.localization.MCCLocalizerPtr is ns["MCCLocalizerPtr"] and btk20.MCCLocalizerPtr is ns["MCCLocalizerPtr"]


def test_tool_on_the_kinect_recording(dev, kinect_pcm, capsys):
    import os
    from tools import mcc_localizer as tool
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kinect_4ch_16k.npz")
    Lb = 4096
    out = tool.main([path, "--positions"] + [str(v) for v in KINECT_MM] + ["--block", str(Lb), "--nbest", "3"])
    assert json.loads(capsys.readouterr().out) == json.loads(json.dumps(out))
    grid = cf.linear_grid(FS, 4, positions=KINECT_MM)
    taus, D = grid["tau"], grid["D"]
    assert out["grid_points"] == len(taus) == 23 and out["D"] == D == 10 and len(out["blocks"]) == 19
    want, wflag = cf.costs(kinect_pcm, taus, Lb, D)
    left_out = silent = 0
    for b, blk in enumerate(out["blocks"]):
        assert blk["block"] == b and blk["delays"] == blk["nbest"][0]["delays"] and len(blk["nbest"]) == 3
        if wflag[b].all():                                   # digital silence: every candidate is flagged, grid point 0 stays
            silent += 1
            assert blk["delays"] == list(taus[0]) and blk["mccc"] == 0.0 and blk["azimuth"] == 0.0
            continue
        x = kinect_pcm[:, b * Lb:(b + 1) * Lb]
        w = int(cf.nbest(want[b], 1)[1][0])
        live = [g for g in range(len(taus)) if not wflag[b, g]]
        others = [g for g in live if tuple(taus[g]) != tuple(taus[w])]
        bound = max(cost_bound(cf.corr_matrix(x, taus[g], D), cf.abs_sum_matrix(x, taus[g], D), Lb - D)[0] for g in live)
        if others and min(want[b, g] for g in others) - want[b, w] > 2 * bound and not wflag[b].any():
            assert blk["delays"] == [int(t) for t in taus[w]], b
            assert abs(blk["mccc"] - (1 - np.exp(want[b, w]))) <= 2 * bound
            assert abs(blk["azimuth"] - float(grid["azimuths"][w])) <= 4 * np.spacing(np.float32(grid["azimuths"][w]))
        else:
            left_out += 1
    print("kinect: %d blocks, %d silent, %d left out of the comparison" % (len(out["blocks"]), silent, left_out))
    assert left_out <= 0.05 * len(out["blocks"])
