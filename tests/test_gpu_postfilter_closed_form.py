"""GPU: the Zelinski, McCowan and Lefkimmiatis post-filter kernels (csrc/pf_kernels.hip) against the float64 closed forms of
tests/postfilter_closed_form.py, in every frame and bin, under closed_forms.accept: the kernel's error may be FACTOR (4) times
what a straightforward float32 per-pair evaluation of the same inputs achieves, never below FLOOR (2^-22) of the largest value.
Rows are (stream, bin).

Two probes per case:
  gain    W is one-hot on channel 0, so y_t = x_0 exactly; the gain is read back as Re(Y conj(x_0)) / |x_0|^2 (one float32 rounding,
          which the yardstick's gains go through as well) and is 1 where the reference applies none.  state.w_last after every
          launch is compared with the closed form's gain at that launch's last frame: the only view of frames below min_frames.
  output  unit weights; the filtered Y against W_cf y_cf (the y and e sums of each statistics kernel).

A stream is cut into launches and compared, launch by launch, with the closed form of the whole stream.  STREAM = launches of
1, 1, 1, 60, 1, 64, 70, 3, 129 frames (frame bases 0, 1, 2, 3, 63, 64, 128, 198, 201): one-frame launches, scan phase 63, a launch
over three 64-frame scan chunks from a non-zero phase, launches below, at and above 64 frames.

Every case prints its figures (`PFCF` lines); DESIGN.md section 4.2 is where a run's ratios per family are recorded.
"""
import numpy as np
import pytest

from tests import closed_forms as cf
from tests import postfilter_closed_form as pf

pytestmark = pytest.mark.gpu

S = 2
STREAM = (1, 1, 1, 60, 1, 64, 70, 3, 129)
BIG = 100000                                                   # min_frames larger than any stream here


def _rows(a):
    return np.ascontiguousarray(a).reshape(-1, a.shape[-1])


def _masked(arrays, nan):
    return [np.where(nan, 0, a) for a in arrays]


def _family(kind, N, nq):
    if kind == "zelinski":
        return "zelinski/stats"
    if N < 8 or N > 128:
        return kind + "/valu"
    return kind + ("/mfma-2pass" if nq == 2 and N > 64 else "/mfma")


def _accept(tag, got, y32, want, nan_ok):
    """NaN masks equal (a silent bin without memory is 0 / 0 in the reference's arithmetic), the rest under accept."""
    got, y32, want = _rows(got), _rows(y32), _rows(want)
    nan = np.isnan(want.real) if np.iscomplexobj(want) else np.isnan(want)
    g_nan = np.isnan(got.real) | np.isnan(got.imag) if np.iscomplexobj(got) else np.isnan(got)
    assert nan.any() == nan_ok, tag
    assert np.array_equal(g_nan, nan), (tag, np.argwhere(g_nan != nan)[:8].tolist())
    y_nan = np.isnan(y32.real) if np.iscomplexobj(y32) else np.isnan(y32)
    assert np.array_equal(y_nan, nan), tag
    ok, fig = cf.accept(*_masked((got, y32, want), nan))
    print("PFCF %s e_max=%.3g y_max=%.3g e_bin=%.3g y_bin=%.3g ratio=%.3f" % (tag, fig["e_max"], fig["y_max"], fig["e_bin"],
                                                                              fig["y_bin"], fig["ratio"]))
    assert ok, (tag, fig)


def _readback(Y, x0):
    """Re(Y conj(x_0)) / |x_0|^2 in float64 from float32 data; an all-zero x_0 reads the gain as Y / x_0 = NaN like 0 / 0."""
    Y, x0 = Y.astype(np.complex128), x0.astype(np.complex128)
    with np.errstate(all="ignore"):
        return (Y * np.conj(x0)).real / (np.abs(x0) ** 2)


def _run_case(dev, kind, N, K, launches, type_, alpha, minf, thr=0.99, real=False, x1=0, per_stream=False, reset_at=None,
              silent=False, lam=None):
    import torch
    from distant_speech_recognition_amd import engine as eng
    T = int(sum(launches))
    nq = 2 if kind == "lefkimmiatis" else 1
    R, twins = pf.coherence(K, N, thr, real=real) if kind != "zelinski" else (None, None)
    d = pf.alignment(S if per_stream else 1, K, N, seed=N)
    X = pf.snapshots(np.broadcast_to(d, (S, K, N)), T, twins, seed=type_)
    if silent:
        X[1, 2, :, 10:20] = 0
    bases = np.concatenate([[0], np.cumsum(launches)])
    resets = () if reset_at is None else (int(bases[reset_at]),)
    Xd = torch.from_numpy(X).to(dev)
    Dd = torch.from_numpy(d).to(dev)
    Rd = None if R is None else torch.from_numpy(R).to(dev)
    tag0 = "%s N=%d K=%d T=%d type=%d alpha=%g minf=%d thr=%g %s x1=%d%s%s%s" % (
        _family(kind, N, nq), N, K, T, type_, alpha, minf, thr, "real" if real else "cplx", x1, " perstream" if per_stream else "",
        " reset" if resets else "", " silent" if silent else "")
    lam_used = None
    for probe in ("gain", "output"):
        if probe == "gain":
            w = np.zeros((S if per_stream else 1, K, N), np.complex64)
            w[..., 0] = 1.0
        else:
            w = cf.unit_weights(S if per_stream else 1, K, N, seed=N)
        Wd = torch.from_numpy(w).to(dev)
        if kind == "zelinski":
            st = eng.ZelinskiState(S, K, dev)
        else:
            st = eng.CoherencePostFilterState(S, K, N, dev, lefkimmiatis=(nq == 2))
            st.set_coherence(Rd, thr)
            if nq == 2:
                if lam is None:
                    st.set_lambda(Rd, Dd[0].contiguous(), 1.0e-8)
                else:
                    st.lam = torch.from_numpy(np.asarray(lam, np.complex64)).to(dev)
                lam_used = st.lam.cpu().numpy()
                assert np.all(np.isfinite(lam_used.view(np.float32)))
        Ys, wl = [], []
        for i, (a, b) in enumerate(zip(bases[:-1], bases[1:])):
            if reset_at == i:
                st.reset_csd()
            Xb = Xd[..., int(a):int(b)].contiguous()
            if kind == "zelinski":
                Yb = eng.bf_apply_zelinski(Wd, Dd, Xb, st, alpha=alpha, type_=type_, min_frames=minf)
            elif kind == "mccowan":
                Yb = eng.bf_apply_mccowan(Wd, Dd, Xb, st, alpha=alpha, type_=type_, min_frames=minf)
            else:
                Yb = eng.bf_apply_lefkimmiatis(Wd, Dd, Xb, st, fbin_x1=x1, alpha=alpha, type_=type_, min_frames=minf)
            Ys.append(Yb.cpu().numpy())
            wl.append(st.w_last.cpu().numpy().copy())
        assert st.frames_done == T
        Y = np.concatenate(Ys, axis=-1)
        wl = np.stack(wl, axis=-1)                             # [S][K][launches]
        # closed form and yardstick of the whole stream
        y, y32 = pf.beamform(w, X), pf.beamform(w, X, np.float32)
        if probe == "gain":
            assert np.array_equal(y32, X[:, :, 0]) and np.array_equal(y, X[:, :, 0])
        if kind == "zelinski":
            args, kw = (), {}
        elif kind == "mccowan":
            args, kw = (R,), dict(threshold=thr)
        else:
            args, kw = (R, lam_used, x1), dict(threshold=thr)
        f = getattr(pf, kind)
        Wcf, Ocf, _ = f(X, d, y, *args, alpha, type_, minf, resets=resets, **kw)
        W32, O32, _ = f(X, d, y32, *args, alpha, type_, minf, resets=resets, dtype=np.float32, **kw)
        share = pf.clamp_share(Wcf)
        assert share <= 0.5, (tag0, share)                     # a condition on the closed form alone, before anything is compared
        if probe == "gain":
            x0 = X[:, :, 0]
            use = pf.applied(T, minf) & (kind != "zelinski" or type_ != 0)
            want = np.where(np.abs(x0) == 0, np.nan, np.where(use, Wcf, 1.0))      # no gain can be read off a zero sample
            _accept(tag0 + " gain", _readback(Y, x0), _readback(O32, x0), want, silent)
            # w_last in its frames, the closed form elsewhere: the few launch ends are held to the yardstick's error over all frames
            last = bases[1:] - 1
            got = Wcf.copy()
            got[..., last] = wl
            _accept(tag0 + " w_last", got, W32, Wcf, silent and alpha == 0)
        else:
            _accept(tag0 + " output", Y, O32, Ocf, silent and alpha == 0)


# kind, N, K, launches, type, alpha, min_frames, further arguments
ZELINSKI = [
    (2, 5, STREAM, 2, 0.7, 0, {}),
    (15, 5, STREAM, 1, 0.7, 2, {}),
    (16, 9, STREAM, 10, 0.0, 64, {}),
    (17, 5, (300,), 2, 0.7, 0, {}),                            # one launch across the 256-frame block of the statistics kernel
    (33, 5, STREAM, 8, 0.7, BIG, {}),                          # every block ends below min_frames
    (5, 5, STREAM, 0, 0.7, 0, {}),                             # type 0: the densities are updated, no gain
    (16, 5, STREAM, 1, 0.0, 2, dict(per_stream=True, reset_at=6)),
    (17, 5, STREAM, 1, 0.7, 64, dict(per_stream=True, reset_at=3)),
    (33, 5, (40,), 2, 0.0, 0, dict(silent=True)),
    (15, 5, (40,), 1, 0.7, 0, dict(silent=True)),
]
MCCOWAN = [
    (2, 5, STREAM, 1, 0.7, 0, dict(thr=0.99)),                                     # VALU kernel, 8 rows
    (7, 5, STREAM, 2, 0.7, 2, dict(thr=0.5)),
    (8, 9, STREAM, 8, 0.7, 0, dict(thr=0.99, real=True)),                          # matrix cores from 8 channels on, padded
    (16, 5, (1040,), 2, 0.7, 0, dict(thr=0.99)),                                   # second workgroup along the frames (one form: 1024)
    (16, 5, STREAM, 0, 0.0, 64, dict(thr=0.5, real=True)),
    (21, 5, STREAM, 10, 0.7, BIG, dict(thr=0.99)),
    (64, 5, (1, 1, 1, 45), 1, 0.7, 2, dict(thr=0.99, real=True)),
    (64, 5, (50,), 2, 0.0, 0, dict(thr=0.5, silent=True)),
    (128, 5, (1, 1, 38), 2, 0.7, 0, dict(thr=0.99)),                               # eight 16-row blocks
    (130, 5, (1, 1, 38), 1, 0.7, 2, dict(thr=0.5, real=True)),                     # VALU kernel above 128 channels
    (16, 5, STREAM, 1, 0.7, 64, dict(thr=0.99, per_stream=True, reset_at=6)),      # Re below min_frames too: w_last
    (7, 5, STREAM, 8, 0.0, 2, dict(thr=0.99, per_stream=True, reset_at=3)),
]
LEFKIMMIATIS = [
    (2, 5, STREAM, 1, 0.7, 0, dict(thr=0.99, x1=0)),
    (7, 5, STREAM, 1, 0.7, 2, dict(thr=0.5, x1=3, real=True)),
    (8, 9, STREAM, 2, 0.0, 64, dict(thr=0.99, x1=9)),
    (16, 5, (530,), 1, 0.7, 0, dict(thr=0.99, x1=3)),                              # second workgroup along the frames (two forms: 512)
    (21, 5, STREAM, 2, 0.7, BIG, dict(thr=0.5, x1=0, real=True)),
    (64, 5, (1, 1, 1, 45), 2, 0.7, 2, dict(thr=0.99, x1=3)),
    (65, 5, (1, 1, 38), 1, 0.7, 0, dict(thr=0.5, x1=3)),                           # one pass per form above 64 channels
    (100, 5, (40,), 2, 0.0, 0, dict(thr=0.99, x1=0, real=True, silent=True)),
    (130, 5, (1, 1, 38), 2, 0.7, 2, dict(thr=0.99, x1=3)),
    (16, 5, STREAM, 2, 0.7, 0, dict(thr=0.99, x1=3, per_stream=True, reset_at=6)),
    # Lambda set by hand: complex, of order one, so that Re and |.| differ and the noise PSD weighs in every bin
    (16, 5, STREAM, 1, 0.7, 2, dict(thr=0.5, x1=2, lam=[1.5 + 1j, 2 - 1.5j, 1 + 0.5j, 3 + 2j, 2.5 - 1j])),
    (7, 5, STREAM, 2, 0.0, 0, dict(thr=0.99, x1=0, lam=[1.5 + 1j, 2 - 1.5j, 1 + 0.5j, 3 + 2j, 2.5 - 1j])),
]


def _id(c):
    return "N%d-K%d-T%d-type%d-a%g-min%d%s" % (c[0], c[1], sum(c[2]), c[3], c[4], c[5],
                                               "".join("-%s%s" % (k, "" if v is True else v) for k, v in sorted(c[6].items())
                                                       if k != "lam") + ("-lam" if "lam" in c[6] else ""))


@pytest.mark.parametrize("case", ZELINSKI, ids=_id)
def test_zelinski_against_closed_form(dev, case):
    N, K, launches, type_, alpha, minf, kw = case
    _run_case(dev, "zelinski", N, K, launches, type_, alpha, minf, **kw)


@pytest.mark.parametrize("case", MCCOWAN, ids=_id)
def test_mccowan_against_closed_form(dev, case):
    N, K, launches, type_, alpha, minf, kw = case
    _run_case(dev, "mccowan", N, K, launches, type_, alpha, minf, **kw)


@pytest.mark.parametrize("case", LEFKIMMIATIS, ids=_id)
def test_lefkimmiatis_against_closed_form(dev, case):
    N, K, launches, type_, alpha, minf, kw = case
    _run_case(dev, "lefkimmiatis", N, K, launches, type_, alpha, minf, **kw)


@pytest.mark.parametrize("kind", ["zelinski", "mccowan", "lefkimmiatis"])
def test_blocks_on_multiples_of_64_equal_one_launch_bit_for_bit(dev, kind):
    """The scan chunks sit on multiples of 64 of the stream's frame counter, so a stream cut at multiples of 64 sees the same
    chunks, hence the same roundings, as one launch."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    N, K, T = 16, 5, 330
    R, twins = pf.coherence(K, N, 0.99)
    d = pf.alignment(1, K, N)
    X = pf.snapshots(np.broadcast_to(d, (S, K, N)), T, twins)
    Xd, Dd, Rd = torch.from_numpy(X).to(dev), torch.from_numpy(d).to(dev), torch.from_numpy(R).to(dev)
    Wd = torch.from_numpy(cf.unit_weights(1, K, N)).to(dev)

    def run(launches):
        if kind == "zelinski":
            st = eng.ZelinskiState(S, K, dev)
        else:
            st = eng.CoherencePostFilterState(S, K, N, dev, lefkimmiatis=(kind == "lefkimmiatis"))
            st.set_coherence(Rd, 0.99)
            if kind == "lefkimmiatis":
                st.lam = torch.from_numpy(np.array([1.5 + 1j, 2 - 1.5j, 1 + 0.5j, 3 + 2j, 2.5 - 1j], np.complex64)).to(dev)
        out, a = [], 0
        for n in launches:
            Xb = Xd[..., a:a + n].contiguous()
            if kind == "zelinski":
                out.append(eng.bf_apply_zelinski(Wd, Dd, Xb, st, alpha=0.7, type_=2, min_frames=3))
            elif kind == "mccowan":
                out.append(eng.bf_apply_mccowan(Wd, Dd, Xb, st, alpha=0.7, type_=2, min_frames=3))
            else:
                out.append(eng.bf_apply_lefkimmiatis(Wd, Dd, Xb, st, fbin_x1=2, alpha=0.7, type_=2, min_frames=3))
            a += n
        state = [st.w_last] + ([st.phi, st.psi] if kind == "zelinski" else [st.u, st.v, st.psi])
        return torch.cat(out, dim=-1), state

    Y1, s1 = run((330,))
    Y2, s2 = run((64, 128, 138))
    assert torch.equal(Y1, Y2) and all(torch.equal(a, b) for a, b in zip(s1, s2))
    assert float(Y1.abs().max()) > 0
