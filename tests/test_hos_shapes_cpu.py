"""CPU: the conditions the shape cases of tests/hos_shapes.py must meet before test_gpu_hos_shapes.py may rely on them -- the
lists cover every channel count, block length, source count and mask kind they are meant to; the optimisation runs take their
decisions away from the thresholds; and teeth: a kernel that is wrong in one place would be caught.

Decided bins.  cf.minimize_bin returns, for every comparison of its trace (gnorm < gtol, gd >= 0, each Armijo trial, pr > 0,
df < mindelta), the margin and the bound ONE run may be off by; a bin is decided when every margin exceeds twice its bound
(the kernel and the restatement both round).  A condition on the inputs, checked with the restatement alone; no tolerance.
Counts with the seeds of hs.MIN_SEED: 30 runs, 120 bins, 113 decided (every run at least 3 of 4; the 7 others each by an
Armijo trial whose two sides agree to rounding -- outside the NMEK clamp the objective does not change along the radius).
Among the decided bins 25 end with a "-1" exit (no step accepted; the plain and gamma runs of the two smallest shapes, the
max_halvings = 0 runs) and 49 accept a step after one or more halvings.  The MEK runs are drawn at MEK_SCALE of the amplitude
and started at norm 6: at unit scale the unclamped objective (-|w|^4) overflows within four iterations and decides nothing.

Teeth.  Each change to what the restatement computes (channel N - 1 left out of Y, frame T - 1 lost, frame T - 1 counted twice,
source 0's sums over the frames used for source 1, one masked-out frame let through) moves fun or grad by at least 100 times
the bound the GPU is held to (fun_err, grad_err, taken once).
Smallest move / bound over bins and variants (N = 9, T = 511 | N = 63, T = 513 | N = 64, T = 1025; all NS = 2):
  channel N - 1 dropped 6.8e10 | 3.1e10 | 2.2e10      frame T - 1 dropped 5.6e9 | 1.5e9 | 7.7e8      counted twice 5.6e9 | 1.5e9 | 7.7e8
  source 0's sums for source 1 2.5e11 | 7.1e10 | 5.1e10      one masked-out frame let through 1.5e10 | 2.3e9 | 1.4e9
"""
import numpy as np
import pytest

from tests import hos_closed_form as cf
from tests import hos_shapes as hs


def test_the_cases_cover_what_they_are_meant_to():
    shapes = hs.EVAL_SHAPES
    assert len(set(shapes)) == len(shapes)
    # every (N, Nc) of the list, both source counts on every N, all four (Nc, NS) at 64 channels
    assert {(N, Nc) for N, Nc, NS, T in shapes} == set(hs.EVAL_PAIRS)
    for N in {N for N, _ in hs.EVAL_PAIRS}:
        assert {NS for n, Nc, NS, T in shapes if n == N} == {1, 2}, N
    assert {(Nc, NS) for N, Nc, NS, T in shapes if N == 64} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert {2 * NS * (N - Nc) for N, Nc, NS, T in shapes} >= {252, 248, 126, 124, 2}
    # below 8 channels, no multiple of 8 on either side of every multiple the wavefronts' rounds end at, and the full width
    assert {N for N, _ in hs.EVAL_PAIRS} == {2, 3, 7, 9, 17, 33, 63, 64}
    # every block length, each with an N that is no multiple of the 8 channels of a wavefront and with two sources
    assert {T for N, Nc, NS, T in shapes} == set(hs.EVAL_T) == {1, 63, 64, 65, 511, 512, 513, 1024, 1025}
    for T in hs.EVAL_T:
        assert any(t == T and N % hs.CPW and NS == 2 for N, Nc, NS, t in shapes), T
    # the masks: every kind on some case, with 64 channels and two sources among them; a tile is blanked only where there is a second
    kinds = {}
    for s in shapes:
        for kind in hs.eval_masks(s[3]):
            kinds.setdefault(kind, []).append(s)
    assert set(kinds) == set(hs.MASK_KINDS)
    assert all(any(N == 64 and NS == 2 for N, Nc, NS, T in v) and any(N % hs.CPW for N, Nc, NS, T in v) for v in kinds.values())
    assert all(T > hs.TILE for N, Nc, NS, T in kinds["tile0_blank"]) and all(T >= 65 for N, Nc, NS, T in kinds["random"])
    for T in (65, 513, 1025):
        sel = {k: hs.mask_of(k, T) for k in hs.eval_masks(T)}
        assert sel["none"] == (None, False)
        m, prev = sel["random"]
        assert prev and m[0] == 1 and m[T - 1] == 0 and 0.3 * T < m.sum() < 0.9 * T and set(np.unique(m)) == {0.0, 1.0}
        assert np.flatnonzero(sel["first"][0]).tolist() == [0] and np.flatnonzero(sel["last"][0]).tolist() == [T - 1]
        assert sel["empty_prev"][1] and not sel["empty_noprev"][1]
        assert not sel["empty_prev"][0].any() and not sel["empty_noprev"][0].any()
        if T > hs.TILE:
            assert not sel["tile0_blank"][0][:hs.TILE].any() and sel["tile0_blank"][0][hs.TILE:].all()
    # the problems: three bins, complex64-representable, one point inside and one outside the clamp for both kinds of gamma,
    # previous frame counts above zero, rows in a longer buffer
    for s in shapes:
        c = hs.eval_case(s)
        N, Nc, NS, T = s
        assert c["obs"].shape == (3, N, T) and np.array_equal(c["obs"], c["obs"].astype(np.complex64).astype(np.complex128))
        assert c["wuH"].shape == (NS, 3, N) and c["BmH"].shape == (NS, 3, N - Nc, N) and c["x"].shape == (3, 2 * NS * (N - Nc))
        assert c["stride"] > T and np.all(c["prev"][2] > 0)
        nrm = np.sqrt(np.sum(np.abs(cf.unpack(c["x"], NS, N - Nc)) ** 2, axis=-1))          # [K][NS]
        gam = np.sqrt(np.sum(np.abs(c["wuH"]) ** 2, axis=-1)).T
        assert np.all(nrm[0] < np.minimum(gam[0], 0.4)) and np.all(nrm[1] > np.maximum(gam[1], 0.4))
        # the blocking matrix blocks: BmH wuH^H = 0, what the gradient's meaning rests on
        assert np.max(np.abs(np.einsum("skjn,skn->skj", c["BmH"], np.conj(c["wuH"])))) < 1e-12
    flat, front = hs.padded_rows(hs.eval_case(shapes[0])["obs"], 5)
    assert front > 0 and np.isnan(flat[:front].real).all() and np.isnan(flat[-1].imag) and np.isfinite(flat.real).sum() == 3 * 3 * 1
    # the optimisation runs
    runs = hs.min_runs()
    assert len(runs) == 6 * 4 + 2 * 3 and hs.MIN_SHAPES == ((2, 65, 1, 1), (3, 513, 2, 2), (9, 511, 1, 1), (17, 512, 2, 1),
                                                           (63, 130, 1, 2), (64, 1025, 2, 1))
    assert {s[2] for s in hs.MIN_EXTRA_SHAPES} == {1, 2} and set(hs.MIN_EXTRA_SHAPES) <= set(hs.MIN_SHAPES)
    for name, r in runs.items():
        assert r["obs"].shape == (4, r["N"], r["T"]) and r["opts"]["maxiter"] == 8, name
        busy, mek = name.endswith("_busy"), name.endswith("_mek")
        assert (r["mask"] is not None and r["prev"] is not None and r["stride"] > r["T"]) if busy else \
            (r["mask"] is None and r["prev"] is None and r["stride"] is None), name
        assert (r["x0"] is not None and np.all(np.any(r["x0"] != 0, axis=1))) if busy or mek else r["x0"] is None, name
        assert r["opts"]["normalize"] == (not mek) and r["opts"]["gamma"] == (0.4 if name.endswith("_gamma") else -1.0), name
    print("evaluation cases: %d shapes x %d variants; masks %s" % (len(shapes), len(hs.VARIANTS), {k: len(v) for k, v in kinds.items()}))
    print("optimisation runs: %d" % len(runs))


def test_the_restatement_handles_no_selected_frame():
    """T = 0 after the mask: with previous statistics fun is finite and grad = alpha wa; without, fun and grad are NaN"""
    c = hs.eval_case((9, 2, 2, 511))
    m = np.zeros(511, np.float32)
    with np.errstate(all="ignore"):
        for normalize, gamma in hs.VARIANTS:
            r = hs.evaluate(c, normalize, gamma, mask=m, with_prev=True)
            want = hs.ALPHA * cf.pack(np.moveaxis(r["wa"], 0, -2))
            assert r["frames"] == 0 and np.all(np.isfinite(r["fun"])) and np.array_equal(r["grad"], want) and np.all(r["stats"] == 0)
            assert np.all(np.isfinite(r["fun_err"])) and np.all(r["grad_err"] >= 0) and np.all(r["stats_err"] == 0)
            r = hs.evaluate(c, normalize, gamma, mask=m, with_prev=False)
            assert np.all(np.isnan(r["fun"])) and np.all(np.isnan(r["grad"])) and np.all(r["stats"] == 0)


def _exits(c, k):
    h = c["trace_halvings"][k]
    return bool((h == -1).any()), bool((h > 0).any())


def test_optimisation_runs_are_decided():
    """at least three of the four bins of every run are decided; among the decided bins of all runs there are "-1" exits (no
    step accepted) and accepted steps after halvings; the extra runs stop where they are meant to"""
    total = {"runs": 0, "bins": 0, "decided": 0, "minus1": 0, "halved": 0, "undecided_by": {}}
    for name, run in hs.min_runs().items():
        c = hs.restated(name)
        decided = c["decided"]
        m1 = [k for k in range(hs.K_MIN) if decided[k] and _exits(c, k)[0]]
        hv = [k for k in range(hs.K_MIN) if decided[k] and _exits(c, k)[1]]
        for k in np.flatnonzero(~decided):
            it, kind, m, b = min(c["decisions"][k], key=lambda d: d[2] / d[3] if d[3] > 0 else np.inf)
            total["undecided_by"][kind] = total["undecided_by"].get(kind, 0) + 1
        print("%-28s decided %d of 4 (smallest margin / (2 bound) per bin %s), iterations %s, -1 exit in decided bins %s, halvings > 0 in %s"
              % (name, decided.sum(), ["%.3g" % v for v in c["decided_ratio"]], c["iters"].tolist(), m1, hv))
        assert decided.sum() >= 3, name
        total["runs"] += 1; total["bins"] += hs.K_MIN; total["decided"] += int(decided.sum())
        total["minus1"] += len(m1); total["halved"] += len(hv)
        for k in range(hs.K_MIN):
            n = c["iters"][k]
            assert np.all(np.diff(np.concatenate([[c["f0"][k]], c["trace_f"][k][:n]])) <= 0)
        if name.endswith("_gtol"):
            assert np.all(c["iters"] == 0) and np.all(c["x"] == 0)
        if name.endswith("_mindelta"):
            assert np.all(c["iters"] == (c["trace_halvings"][:, 0] >= 0))
        if name.endswith("_halvings0"):
            assert np.all(c["trace_halvings"] <= 0) and (c["trace_halvings"] == -1).any()
    # the margins are an addition: without them the same keys with the same values, and none of the three new ones
    run = hs.min_runs()["N9_T511_NS1_Nc1_busy"]
    c, plain = hs.restated(run["name"]), cf.minimize(run["obs"], run["wuH"], run["BmH"], run["x0"], hs.ALPHA, hs.BETA, -1.0, True,
                                                     mask=run["mask"], prev=run["prev"], maxiter=hs.MIN_MAXITER)
    assert set(c) - set(plain) == {"decisions", "decided", "decided_ratio"} and set(plain) <= set(c)
    assert all(np.array_equal(plain[k], c[k], equal_nan=True) for k in plain)
    print("optimisation runs:", total)
    assert total["minus1"] >= 1 and total["halved"] >= 1


TEETH_SHAPES = ((9, 2, 2, 511), (63, 1, 2, 513), (64, 1, 2, 1025))


@pytest.mark.parametrize("shape", TEETH_SHAPES, ids=hs.name_of)
def test_teeth(shape):
    c = hs.eval_case(shape)
    assert (c["N"], c["NS"]) in ((9, 2), (63, 2), (64, 2))
    worst = {}
    for normalize, gamma in hs.VARIANTS:
        muts = hs.mutations(c, normalize, gamma)
        assert set(muts) == {"none", "none_masked", "drop_channel", "drop_frame", "double_frame", "source0_v", "mask_leak"}
        for name, (got, mask, r) in muts.items():
            # the largest move over the entries of a bin, in units of the bound the GPU is held to; the smallest over the bins
            ratio = np.maximum(np.abs(got["fun"] - r["fun"]) / r["fun_err"], np.max(np.abs(got["grad"] - r["grad"]) / r["grad_err"], axis=1))
            if name.startswith("none"):
                # from_woH unchanged restates cf.evaluate: both round, so twice the bound
                assert np.all(np.abs(got["fun"] - r["fun"]) <= 2 * r["fun_err"]) and np.all(np.abs(got["grad"] - r["grad"]) <= 2 * r["grad_err"])
                continue
            worst[name] = min(worst.get(name, np.inf), float(ratio.min()))
    print("teeth %-18s smallest move / bound over bins and variants: %s" % (c["name"], {k: "%.3g" % v for k, v in worst.items()}))
    assert min(worst.values()) >= 100.0, worst
