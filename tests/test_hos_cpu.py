"""CPU: the float64 restatement of the maximum-empirical-kurtosis beamformers (tests/hos_closed_form.py) against the reference's
own numbers (tests/golden/pybeamformer_hos_golden.npz), the frame selection and weight packing of the mirror classes, and the
restated optimiser against what the reference's scipy flow reaches.

Bounds: the forward-error bound the restatement carries (classical n u sum |terms|, see its docstring), DOUBLED here because
the golden values are float64 evaluations that round as well."""
import numpy as np
import pytest

from tests import hos_closed_form as cf
from tests import hos_fixture as hf


@pytest.fixture(scope="module")
def G():
    return hf.golden()


@pytest.fixture(scope="module")
def inputs(orc, proto256, kinect_pcm, G):
    T = int(G["meta_T"][0])
    return {"a": hf.frames(orc, proto256, kinect_pcm, T), "b": hf.frames(orc, proto256, kinect_pcm, T, float(G["scale_b"][0]))}


def _labels(a):
    return [tuple(r) for r in np.asarray(a).tolist()]


def _select(X, labs, R=1):
    from distant_speech_recognition_amd.pybeamformer import _hos_select_frames
    return _hos_select_frames(hf.energies(X), 128 / float(hf.FS), labs, hf.ENERGY_THRESHOLD, R)


def _cases():
    for sc in ("a", "b"):
        for NS in (1, 2):
            for Nc in (1, 2):
                if sc == "a" and (NS, Nc) != (1, 1):
                    continue
                for tag, normalize, gamma in hf.VARIANTS:
                    yield sc, NS, Nc, tag, normalize, gamma


def test_selection_logic_matches_reference(inputs, G):
    X = inputs["a"]
    for tag in ("A", "B"):
        for R in (1, 2):
            sel = _select(X, _labels(G["labels_" + tag]), R)
            assert np.array_equal(sel, G["sel_%s_R%d" % (tag, R)]), (tag, R)
    # the `elif` moves to the next segment without looking at the frame again, and an open-ended segment that is reached before its
    # start is skipped (elapsed_time > -1): nothing after 0.7 s of label set B
    assert G["sel_B_R1"].max() * 128 / 16000.0 <= 0.7
    from distant_speech_recognition_amd.pybeamformer import _hos_select_frames
    assert list(_hos_select_frames(np.full(10, 11.0), 1.0, [(2.0, 4.0), (5.0, 7.0)], 10, 1)) == [2, 3, 4, 6, 7]
    assert list(_hos_select_frames(np.full(10, 11.0), 1.0, [(0.0, -1)], 10, 3)) == [0, 3, 6, 9]
    assert list(_hos_select_frames(np.full(4, 10.0), 1.0, [(0.0, -1)], 10, 1)) == []


def test_pack_unpack_weights():
    from distant_speech_recognition_amd.pybeamformer import pack_weights, unpack_weights
    rng = np.random.default_rng(0)
    for NS, dim in ((1, 3), (2, 2), (2, 63)):
        w = rng.normal(size=(NS, dim)) + 1j * rng.normal(size=(NS, dim))
        p = pack_weights(w, NS, dim)
        assert p.shape == (2 * NS * dim,) and p.dtype == np.float64
        for m in range(NS):
            for n in range(dim):
                assert p[2 * (m * dim + n)] == w[m][n].real and p[2 * (m * dim + n) + 1] == w[m][n].imag
        assert np.array_equal(unpack_weights(p, NS, dim), w)
        assert np.array_equal(cf.pack(w), p) and np.array_equal(cf.unpack(p, NS, dim), w)


def _prev(G, key):
    return G[key + "_prevY2"], G[key + "_prevY4"], G[key + "_prevN"]


def test_closed_form_matches_reference_everywhere(inputs, G):
    """fun_hos_bf, dfun_hos_bf, calc_obj_func of every pinned configuration, and the statistics store_stats leaves."""
    bins = G["bins"]
    worst = {"fun": 0.0, "dfun": 0.0, "obj": 0.0, "prev": 0.0}
    for sc, NS, Nc, tag, normalize, gamma in _cases():
        X = inputs[sc]
        dim = hf.N - Nc
        wuH, BmH = G["wuH_ns%d_nc%d" % (NS, Nc)], G["BmH_ns%d_nc%d" % (NS, Nc)]
        pts = G["x_ns%d_nc%d" % (NS, Nc)] if sc == "b" else G["x_ns1_nc1"]
        obsA = hf.observations(X, G["sel_A_R1"])
        key = "%s_%s_ns%d_nc%d" % (sc, tag, NS, Nc)
        # previous statistics: store_stats on the earlier segment at the inside-clamp point
        assert np.array_equal(_select(inputs["a"], _labels(G["labels_prev"])), G["sel_prev"])
        obsP = hf.observations(X, G["sel_prev"])
        r = cf.evaluate(obsP, wuH, BmH, pts[1], 0.01, 3.0, gamma, normalize, want_grad=False)
        zero = (np.zeros((hf.K, NS)), np.zeros((hf.K, NS)), np.zeros((hf.K, NS), np.int64))
        mine = cf.store_stats(zero, r["stats"], r["frames"], NS)
        gold = _prev(G, key)
        assert np.array_equal(mine[2], gold[2])
        for i, col in ((0, 2 * NS), (1, 2 * NS + 1)):
            bound = 2 * (r["stats_err"][:, col:col + 1] / mine[2] + 2 * cf.U * np.abs(gold[i]))
            ratio = np.max(np.abs(mine[i] - gold[i]) / bound)
            worst["prev"] = max(worst["prev"], ratio)
            assert ratio <= 1.0, (key, i, ratio)
        for prev in (0, 1):
            for p in range(3):
                r = cf.evaluate(obsA[bins], wuH[:, bins], BmH[:, bins], pts[p][bins], 0.01, 3.0, gamma, normalize,
                                prev=tuple(q[bins] for q in gold) if prev else None)
                k2 = "%s_prev%d_x%d" % (key, prev, p)
                for name, mine_v, gold_v, bound in (
                        ("fun", r["fun"], G[k2 + "_fun"], r["fun_err"]),
                        ("dfun", r["grad"], G[k2 + "_dfun"], r["grad_err"]),
                        ("obj", r["kurt"] + cf.OFFSET, G[k2 + "_obj"], r["kurt_err"] + cf.U * (np.abs(r["kurt"]) + abs(cf.OFFSET)))):
                    ratio = float(np.max(np.abs(mine_v - gold_v) / (2 * bound)))
                    worst[name] = max(worst[name], ratio)
                    assert ratio <= 1.0, (k2, name, ratio)
    print("largest |closed form - reference| / (2 x bound):", worst)


def test_gradient_convention(inputs, G):
    """dfun_hos_bf is HALF the derivative of fun_hos_bf for MEK (the reference's convention, kept): central differences of the
    restatement's own objective, to the accuracy of the difference quotient."""
    X = inputs["b"]
    obs = hf.observations(X, G["sel_A_R1"])[40:41]
    wuH, BmH = G["wuH_ns1_nc1"][:, 40:41], G["BmH_ns1_nc1"][:, 40:41]
    x = G["x_ns1_nc1"][1][40:41]
    g = cf.evaluate(obs, wuH, BmH, x, 0.01, 3.0, -1.0, False)["grad"][0]
    h = 1e-6
    for i in range(x.shape[1]):
        e = np.zeros_like(x); e[0, i] = h
        fd = (cf.evaluate(obs, wuH, BmH, x + e, 0.01, 3.0, -1.0, False, want_grad=False)["fun"][0]
              - cf.evaluate(obs, wuH, BmH, x - e, 0.01, 3.0, -1.0, False, want_grad=False)["fun"][0]) / (2 * h)
        assert abs(fd - 2 * g[i]) <= 1e-4 * max(abs(fd), 1.0), (i, fd, g[i])


def test_finalize_matches_reference(inputs, G):
    """_woH[.][m] right after finalize_wa_f(m, .) and the statistics it stores on top of the previous ones."""
    X = inputs["b"]
    for sc, NS, Nc, tag, normalize, gamma in _cases():
        if sc != "b":
            continue
        key = "b_%s_ns%d_nc%d" % (tag, NS, Nc)
        wuH, BmH, pts = G["wuH_ns%d_nc%d" % (NS, Nc)], G["BmH_ns%d_nc%d" % (NS, Nc)], G["x_ns%d_nc%d" % (NS, Nc)]
        fb = np.array([8, 72])
        obsA = hf.observations(X, G["sel_A_R1"])
        gold = _prev(G, key)
        r = cf.evaluate(obsA[fb], wuH[:, fb], BmH[:, fb], pts[2][fb], 0.01, 3.0, gamma, normalize,
                        prev=tuple(q[fb] for q in gold), want_grad=False)
        woH = np.moveaxis(r["woH"], 0, 1)                              # [2 bins][NS][N]
        assert np.all(np.abs(woH - G[key + "_fin_woH"]) <= 2 * np.moveaxis(r["woH_err"], 0, 1) + 2 * cf.U * np.abs(woH)), key
        mine = cf.store_stats(tuple(q[fb] for q in gold), r["stats"], r["frames"], NS)
        assert np.array_equal(mine[2], G[key + "_fin_prevN"])
        for i, col, name in ((0, 2 * NS, "_fin_prevY2"), (1, 2 * NS + 1, "_fin_prevY4")):
            bound = 2 * (r["stats_err"][:, col:col + 1] / mine[2] + 4 * cf.U * np.abs(G[key + name]))
            assert np.all(np.abs(mine[i] - G[key + name]) <= bound), (key, name)


OPT = dict(alpha=0.01, beta=3.0, gamma=-1.0, normalize=True)


def test_optimiser_restatement_reaches_the_reference(inputs, G):
    """At scale (b), NMEK, NS = 1, Nc = 1: on every bin with ||g0|| >= gtol the restated optimiser ends at or below
    min(f_CG, f_BFGS) + |f_CG - f_BFGS| of the reference's scipy flow; on the others nothing moves.  No bin is left out."""
    X = inputs["b"]
    obs = hf.observations(X, G["sel_A_R1"])
    wuH, BmH = G["wuH_ns1_nc1"], G["BmH_ns1_nc1"]
    r = cf.minimize(obs, wuH, BmH, None, **OPT)
    # f0 and ||g0|| are the reference's
    e0 = cf.evaluate(obs, wuH, BmH, np.zeros((hf.K, 6)), 0.01, 3.0, -1.0, True)
    assert np.all(np.abs(r["f0"] - G["opt_f0"]) <= 2 * e0["fun_err"])
    assert np.all(np.abs(r["g0norm"] - G["opt_g0norm"]) <= 2 * np.linalg.norm(e0["grad_err"], axis=1))
    gtol = cf.DEFAULTS["gtol"]
    moving = G["opt_g0norm"] >= gtol
    assert np.array_equal(moving, r["g0norm"] >= gtol)
    bad = [k for k in np.where(moving)[0] if not r["f"][k] <= G["opt_f_ref"][k] + G["opt_spread"][k]]
    assert not bad, [(k, r["f"][k], G["opt_f_ref"][k], G["opt_spread"][k]) for k in bad]
    for k in np.where(~moving)[0]:
        assert r["iters"][k] == 0 and r["f"][k] == r["f0"][k]
    # the accepted objective values never increase
    for k in range(hf.K):
        t = np.concatenate([[r["f0"][k]], r["trace_f"][k][: r["iters"][k]]])
        assert np.all(np.diff(t) <= 0)
    print("bins moving: %d of %d, improved over the reference on %d" % (moving.sum(), hf.K, np.sum(r["f"] < G["opt_f_ref"])))


def trace_differs(h1, h2):
    return np.array([not np.array_equal(a, b) for a, b in zip(h1, h2)])


def test_optimiser_restatement_is_stable_under_summation_order(inputs, G):
    """The same optimisation with the frames in reverse order (another summation order): at most 3 % of the bins may take a
    different accept / halve sequence -- the cap the GPU comparison uses."""
    X = inputs["b"]
    obs = hf.observations(X, G["sel_A_R1"])
    wuH, BmH = G["wuH_ns1_nc1"], G["BmH_ns1_nc1"]
    r1 = cf.minimize(obs, wuH, BmH, None, **OPT)
    r2 = cf.minimize(np.ascontiguousarray(obs[:, :, ::-1]), wuH, BmH, None, **OPT)
    diff = trace_differs(r1["trace_halvings"], r2["trace_halvings"])
    print("bins whose halvings trace differs under reversed frame order: %d of %d" % (diff.sum(), hf.K))
    assert diff.sum() <= 0.03 * hf.K
    same = ~diff
    assert np.all(np.abs(r1["f"][same] - r2["f"][same]) <= r1["f_err"][same] + r2["f_err"][same])


def test_workspace_query_answers_zero():
    """btk_hos_workspace_bytes: the kernels keep everything in LDS, at every supported size"""
    from distant_speech_recognition_amd import _lib
    lib = _lib.lib()
    assert lib.btk_hos_max_channels() == 64
    for K, N, Nc, NS, T in ((257, 64, 1, 1, 4096), (129, 4, 2, 2, 160), (1, 2, 1, 1, 1)):
        assert lib.btk_hos_workspace_bytes(K, N, Nc, NS, T) == 0
