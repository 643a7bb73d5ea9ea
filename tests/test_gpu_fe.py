"""GPU: the ASR front end (btk_fe_process) stage by stage against the numpy restatement of the reference (tests/fe_closed_form.py).

Bounds, with u = 2^-24 and B = spectra_bound(L) = (log2 L + 1) eta of tests/test_gpu_tdoa.py:
  SPECTRUM  per frame ||X - X64||_2 <= B ||X64||_2.
  POWER     per frame ||P - P64||_1 <= B_P ||P64||_1,  B_P = 2B + B^2 + 3u (1 + B)^2:  |dP_k| <= |dX_k| (2 |X_k| + |dX_k|), summed
            with Cauchy-Schwarz, plus the rounding of two products and a sum of the computed spectrum.
  VTLN, MEL, CEP on the GPU's own previous stage: |out - cf| <= 2u sum |w| |in| (float64 accumulation, one output rounding).
  LOG on the GPU's own previous stage: |out - cf| <= 2u |cf| + 2u, except where the float32 input lies within 4u |in| of a
            branch point (v + a = 0, or v = 1e-5 with flooring); those are left out and counted, at most 1 % of a case.
  LOG end to end: |dlog_j| <= 0.4343 c_W B_P ||P64||_1 / (v64_j + a - c_W B_P ||P64||_1) + 2u |log_j| + 2u with c_W the largest
            absolute column sum of the applied tables (their product where two are applied); elements whose denominator is not
            positive are left out and counted under the same cap.
The kernel carries 4 frames per workgroup at L = 256 and 512, 2 at L = 1024 and 1 from L = 2048; T = 33 is one more than a
multiple of each.
The tone frame's mel bands far from the tone lie below the end-to-end bound's own perturbation term and are the ones left
out there: at most 30 of S C T 30 elements, which is what sets T."""
import math

import numpy as np
import pytest

from tests import fe_closed_form as cf
from tests.test_gpu_tdoa import spectra_bound

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(160, 160, 256), (400, 160, 512), (256, 256, 256), (256, 100, 1024), (800, 320, 2048), (2048, 1000, 4096),
          (4096, 4096, 8192)]
# where the kernel that starts from PCM keeps the VTLN, mel and cosine tables of tables(): staged in LDS behind the frames'
# buffers while both fit 64 KiB (fe_closed_form.pcm_kernel_lds restates the rule), read from global memory otherwise.  At
# L = 2048 the frames take 12 KiB and the tables 44 KiB (VTLN alone 36): LDS; at 4096 and 8192 24 + 87 KiB (VTLN 72) and
# 48 + 172 KiB (VTLN 144): global memory, the VTLN table's first numeric test there (tests/test_fe_cpu.py checks the sizes).
TABLES_IN_LDS = {256: True, 512: True, 1024: True, 2048: True, 4096: False, 8192: False, 16384: False}
S, C, T = 2, 2, 33
PAD = 24                      # pcm_stride - len
MU = 0.95


def power_bound(L):
    B = spectra_bound(L)
    return 2 * B + B * B + 3 * U * (1 + B) ** 2


def _eng():
    from distant_speech_recognition_amd import engine
    return engine


_signals = {}


def signal(D, shift):
    """float32 [S][C][len + PAD] (the PAD samples behind every row hold 1e6: nothing may read them), len ending inside the last
    frame; int16-scale white noise, different in every row, frame 3 all zero, frame 6 of row (1, 0) a pure tone."""
    key = (D, shift)
    if key not in _signals:
        n = (T - 1) * shift + max(shift // 2, 1)
        rng = np.random.default_rng(D * 1000 + shift)
        x = np.full((S, C, n + PAD), 1.0e6, np.float32)
        x[..., :n] = np.round(rng.normal(scale=3000.0, size=(S, C, n))).clip(-32768, 32767)
        x[..., 3 * shift:3 * shift + D] = 0.0
        i = np.arange(6 * shift, min(6 * shift + D, n))
        x[1, 0, i] = np.round(8000.0 * np.sin(2 * np.pi * 1000.0 / 16000.0 * i))
        x[..., n:] = 1.0e6
        _signals[key] = (x, n)
    return _signals[key]


def upload(dev, x, n):
    import torch
    return torch.from_numpy(x).to(dev)[..., :n]


def tables(powN, vtln_version=2):
    eng = _eng()
    key = (powN, vtln_version)
    if key not in _tables:
        _tables[key] = (eng.fe_vtln_table(powN, 0.94, 0.8, vtln_version), eng.fe_mel_table(powN, 16000, 100, 6800, 30, 2),
                        eng.fe_dct_table(1, 13, 30))
    return _tables[key]


_tables = {}
ALL = ("spectrum", "power", "vtln", "mel", "log", "cep")


def closed_frames(x, n, D, shift, mu=None, prior0=None, window=True, frames=T):
    return np.stack([[cf.frames(x[s, c, :n], D, shift, frames, mu, 0.0 if prior0 is None else prior0[s, c], window)
                      for c in range(x.shape[1])] for s in range(x.shape[0])])


def check_spectrum(X, X64, L, label):
    num = np.sqrt(np.sum(np.abs(X.astype(np.complex128) - X64) ** 2, axis=-1))
    den = np.sqrt(np.sum(np.abs(X64) ** 2, axis=-1))
    r = float(np.max(num / np.where(den > 0, den, 1.0)) / spectra_bound(L))
    print("%s spectrum: error/bound %.3f" % (label, r))
    assert np.all(num <= spectra_bound(L) * den), r


def check_rows(out, want, scale, label):
    """|out - want| <= 2u scale"""
    err = np.abs(out.astype(np.float64) - want)
    r = float(np.max(err / np.where(scale > 0, 2 * U * scale, 1.0)))
    print("%s: error/bound %.3f" % (label, r))
    assert np.all(err <= 2 * U * scale), r


def check_log(out, inp, m, a, floor, label):
    inp64 = inp.astype(np.float64)
    want = cf.log_feature(inp, m, a, floor).astype(np.float64)
    near = np.abs(inp64 - 1.0e-5) <= 4 * U * np.abs(inp64) if floor else np.abs(inp64 + a) <= 4 * U * np.abs(inp64)
    err = np.abs(out.astype(np.float64) - want)
    bound = 2 * U * np.abs(want) + 2 * U
    r = float(np.max(np.where(near, 0.0, err / bound)))
    print("%s: error/bound %.3f, left out %d of %d" % (label, r, int(near.sum()), near.size))
    assert near.sum() <= 0.01 * near.size
    assert np.all((err <= bound) | near), r


@pytest.mark.parametrize("shape", SHAPES)
def test_every_stage(dev, shape):
    eng = _eng()
    D, shift, L = shape
    powN = L // 2 + 1
    x, n = signal(D, shift)
    vtln, mel, dct = tables(powN, 1 if L == 512 else 2)
    assert eng.fe_frames(n, D, shift) == T
    assert cf.tables_in_lds(L, vtln, mel, dct) == TABLES_IN_LDS[L], cf.pcm_kernel_lds(L, vtln, mel, dct)
    o = eng.fe_process(upload(dev, x, n), "pcm", ALL, D=D, shift=shift, L=L, vtln=vtln, mel=mel, dct=dct)
    o = {k: v.cpu().numpy() for k, v in o.items()}
    for k, d in (("spectrum", powN), ("power", powN), ("vtln", powN), ("mel", 30), ("log", 30), ("cep", 13)):
        assert o[k].shape == (S, C, T, d), (k, o[k].shape)
    label = "D=%d shift=%d L=%d" % shape
    X64 = cf.spectrum64(closed_frames(x, n, D, shift), L)
    check_spectrum(o["spectrum"], X64, L, label)
    assert np.all(o["spectrum"][..., 0].imag == 0) and np.all(o["spectrum"][..., L // 2].imag == 0)
    # POWER end to end
    P64 = cf.power64(X64, powN)
    num, den = np.abs(o["power"] - P64).sum(axis=-1), P64.sum(axis=-1)
    r = float(np.max(num / np.where(den > 0, den, 1.0)) / power_bound(L))
    print("%s power: error/bound %.3f" % (label, r))
    assert np.all(num <= power_bound(L) * den), r
    # the silent frame (3; without overlap nothing else touches it)
    assert np.all(o["power"][:, :, 3] == 0) and np.all(o["log"][:, :, 3] == 0) and np.all(o["cep"][:, :, 3] == 0)
    # each later stage on the GPU's own previous stage
    P = o["power"].astype(np.float64)
    fn = cf.vtln_org if L == 512 else cf.vtln_ff
    Vw = fn(P.reshape(-1, powN).T, powN, 0.94, 0.8).T.reshape(P.shape)
    check_rows(o["vtln"], Vw, np.abs(P) @ np.abs(vtln.matrix()).T, label + " vtln")
    off, cnt, rows = cf.mel_table(powN, 16000, 100, 6800, 30, 2)
    check_rows(o["mel"], cf.mel_apply(o["vtln"], off, cnt, rows), cf.mel_abs(o["vtln"], off, cnt, rows), label + " mel")
    check_log(o["log"], o["mel"], 1.0, 1.0, False, label + " log")
    Dm = cf.dct_table(1, 13, 30).astype(np.float64)
    check_rows(o["cep"], o["log"].astype(np.float64) @ Dm.T, np.abs(o["log"].astype(np.float64)) @ np.abs(Dm).T, label + " cep")
    # LOG end to end
    cW = vtln.abs_column_sum() * mel.abs_column_sum()
    v64 = cf.mel_apply(P64 @ vtln.matrix().T, off, cnt, rows)
    dv = cW * power_bound(L) * den[..., None]
    lg64 = np.log10(np.where(v64 + 1.0 > 0, v64 + 1.0, 1.0))
    ok = v64 + 1.0 - dv > 0
    bound = 0.4343 * dv / np.where(ok, v64 + 1.0 - dv, 1.0) + 2 * U * np.abs(lg64) + 2 * U
    err = np.abs(o["log"] - lg64)
    r = float(np.max(np.where(ok, err / bound, 0.0)))
    print("%s log end to end: error/bound %.3f, left out %d of %d" % (label, r, int((~ok).sum()), ok.size))
    assert (~ok).sum() <= 0.01 * ok.size and np.all((err <= bound) | ~ok), r


@pytest.mark.parametrize("shape", [(160, 160, 256), (256, 256, 256), (400, 400, 512), (256, 256, 1024), (800, 800, 2048),
                                   (2048, 2048, 4096), (4096, 4096, 8192)])
def test_spectra_have_the_bits_of_tdoa_spectra(dev, shape):
    import torch
    eng = _eng()
    D, shift, L = shape
    x, n = signal(D, shift)
    xd = torch.from_numpy(np.ascontiguousarray(x[..., :n])).to(dev)
    X = eng.fe_process(xd, "pcm", "spectrum", D=D, shift=D, L=L)["spectrum"]
    Xt, _ = eng.tdoa_spectra(xd, D, L)
    assert X.shape == Xt.shape and torch.equal(torch.view_as_real(X), torch.view_as_real(Xt))
    # and without the window
    X = eng.fe_process(xd, "pcm", "spectrum", D=D, shift=D, L=L, window=False)["spectrum"]
    Xt, _ = eng.tdoa_spectra(xd, D, L, window=False)
    assert torch.equal(torch.view_as_real(X), torch.view_as_real(Xt))


def test_log_power_and_its_branches(dev):
    """LOG straight on the power vector (the log-power chain), a = 0 and the sphinx floor; silent frames give exactly 0."""
    eng = _eng()
    D, shift, L = 160, 160, 256
    x, n = signal(D, shift)
    xd = upload(dev, x, n)
    for kw in (dict(log_a=1.0), dict(log_a=0.0), dict(log_m=10.0, log_floor=True)):
        o = eng.fe_process(xd, "pcm", ("power", "log"), D=D, shift=shift, L=L, **kw)
        assert sorted(o) == ["log", "power"] and o["log"].shape == (S, C, T, L // 2 + 1)
        P, lg = o["power"].cpu().numpy(), o["log"].cpu().numpy()
        # the silent frame sits exactly on the branch point of a = 0 (v + a = 0): it is pinned to its exact value below and
        # the bound, with its count of elements near a branch, is asked of the other frames
        live = [t for t in range(T) if t != 3]
        check_log(lg[:, :, live], P[:, :, live], kw.get("log_m", 1.0), kw.get("log_a", 1.0), kw.get("log_floor", False),
                  "log power %s" % kw)
        if not kw.get("log_floor"):
            assert np.all(P[:, :, 3] == 0) and np.all(lg[:, :, 3] == 0)     # a = 1: log10(1); a = 0: the -> 1.0 branch
        else:
            assert np.all(lg[:, :, 3] == np.float32(10.0 * math.log10(1.0e-5)))


@pytest.mark.parametrize("shape", [(160, 160, 256), (400, 160, 512), (256, 100, 1024), (2048, 1000, 4096)])
def test_preemphasis(dev, shape):
    import torch
    eng = _eng()
    D, shift, L = shape
    x, n = signal(D, shift)
    xd = upload(dev, x, n)
    rng = np.random.default_rng(5)
    p0 = np.round(rng.normal(scale=3000.0, size=(S, C))).astype(np.float32)
    for prior0 in (None, p0):
        X = eng.fe_process(xd, "pcm", "spectrum", D=D, shift=shift, L=L, preemph=MU,
                           prior0=None if prior0 is None else torch.from_numpy(prior0).to(dev))["spectrum"].cpu().numpy()
        X64 = cf.spectrum64(closed_frames(x, n, D, shift, MU, prior0), L)
        check_spectrum(X, X64, L, "pre-emphasis D=%d shift=%d L=%d prior0 %s" % (D, shift, L, prior0 is not None))
    off = eng.fe_process(xd, "pcm", "spectrum", D=D, shift=shift, L=L)["spectrum"].cpu().numpy()
    assert not np.array_equal(off, X)
    # T frames in one call and in two consecutive calls: the same bits (prior0 of the second call = the last sample of frame T1 - 1)
    T1 = 14
    one = eng.fe_process(xd, "pcm", ("spectrum", "power"), D=D, shift=shift, L=L, preemph=MU)
    last = (T1 - 1) * shift + D - 1
    prior = np.ascontiguousarray(x[..., last]) if last < n else np.zeros((S, C), np.float32)
    a = eng.fe_process(xd, "pcm", ("spectrum", "power"), D=D, shift=shift, L=L, preemph=MU, T=T1)
    b = eng.fe_process(xd[..., T1 * shift:], "pcm", ("spectrum", "power"), D=D, shift=shift, L=L, preemph=MU, T=T - T1,
                       prior0=torch.from_numpy(prior).to(dev))
    for k in ("spectrum", "power"):
        two = torch.cat([a[k], b[k]], dim=2)
        assert torch.equal(torch.view_as_real(two) if k == "spectrum" else two,
                           torch.view_as_real(one[k]) if k == "spectrum" else one[k]), k


def test_partial_workgroup_and_single_row(dev):
    """S C T no multiple of the frames per workgroup: the last workgroup holds frames that do not exist."""
    import torch
    eng = _eng()
    D, shift, L = 400, 160, 512
    x, n = signal(D, shift)
    vtln, mel, dct = tables(L // 2 + 1, 1)
    xd = upload(dev, x, n)
    full = eng.fe_process(xd, "pcm", ALL, D=D, shift=shift, L=L, vtln=vtln, mel=mel, dct=dct)
    part = eng.fe_process(xd[1:, 1:], "pcm", ALL, D=D, shift=shift, L=L, vtln=vtln, mel=mel, dct=dct)     # 33 frames, 4 per workgroup
    for k in ALL:
        assert part[k].shape[:3] == (1, 1, T)
        assert torch.equal(torch.view_as_real(part[k]) if k == "spectrum" else part[k],
                           torch.view_as_real(full[k][1:, 1:]) if k == "spectrum" else full[k][1:, 1:]), k


def test_stage_entry_at_power(dev):
    import torch
    eng = _eng()
    rng = np.random.default_rng(11)
    P = (rng.uniform(0.0, 4.0e9, size=(S, C, 5, 17))).astype(np.float32)
    P[0, 0, 2] = 0.0
    mel = eng.fe_mel_table(17, 16000, 0, 8000, 12, 2)
    dct = eng.fe_dct_table(1, 5, 12)
    o = eng.fe_process(torch.from_numpy(P).to(dev), "power", ("mel", "log", "cep"), mel=mel, dct=dct)
    o = {k: v.cpu().numpy() for k, v in o.items()}
    assert o["mel"].shape == (S, C, 5, 12) and o["cep"].shape == (S, C, 5, 5)
    off, cnt, rows = cf.mel_table(17, 16000, 0, 8000, 12, 2)
    check_rows(o["mel"], cf.mel_apply(P, off, cnt, rows), cf.mel_abs(P, off, cnt, rows), "entry at power: mel")
    check_log(o["log"], o["mel"], 1.0, 1.0, False, "entry at power: log")
    Dm = cf.dct_table(1, 5, 12).astype(np.float64)
    check_rows(o["cep"], o["log"].astype(np.float64) @ Dm.T, np.abs(o["log"].astype(np.float64)) @ np.abs(Dm).T, "entry at power: cep")
    assert np.all(o["cep"][0, 0, 2] == 0)
    # entering at LOG gives the cepstra of the same log vector, bit for bit
    c2 = eng.fe_process(torch.from_numpy(o["log"]).to(dev), "log", "cep", dct=dct)["cep"].cpu().numpy()
    assert np.array_equal(c2, o["cep"])


def test_entry_at_spectrum_and_upper_half(dev):
    import torch
    eng = _eng()
    D, shift, L = 400, 160, 512
    x, n = signal(D, shift)
    vtln, mel, dct = tables(L // 2 + 1, 1)
    xd = upload(dev, x, n)
    kw = dict(vtln=vtln, mel=mel, dct=dct)
    full = eng.fe_process(xd, "pcm", ALL, D=D, shift=shift, L=L, **kw)
    late = eng.fe_process(full["spectrum"], "spectrum", ALL[1:], **kw)
    for k in ALL[1:]:
        assert torch.equal(late[k], full[k]), k
    # powN = L: the upper half is the mirror, from PCM and from the spectrum; LOG over all L values
    for src, st, a in ((xd, "pcm", dict(D=D, shift=shift, L=L)), (full["spectrum"], "spectrum", {})):
        up = eng.fe_process(src, st, ("power", "log"), powN=L, **a)
        assert up["power"].shape == (S, C, T, L) and up["log"].shape == (S, C, T, L)
        assert torch.equal(up["power"][..., :L // 2 + 1], full["power"])
        assert torch.equal(up["power"][..., L // 2 + 1:], full["power"][..., 1:L // 2].flip(-1))
        assert torch.equal(up["log"][..., L // 2 + 1:], up["log"][..., 1:L // 2].flip(-1))


def test_skipped_stages(dev):
    import torch
    eng = _eng()
    D, shift, L = 160, 160, 256
    x, n = signal(D, shift)
    vtln, mel, dct = tables(L // 2 + 1)
    xd = upload(dev, x, n)
    full = eng.fe_process(xd, "pcm", ALL, D=D, shift=shift, L=L, vtln=vtln, mel=mel, dct=dct)
    # no VTLN: MEL reads the power vector
    o = eng.fe_process(xd, "pcm", ALL, D=D, shift=shift, L=L, mel=mel, dct=dct)
    assert "vtln" not in o and torch.equal(o["power"], full["power"])
    m = eng.fe_process(full["power"], "power", "mel", mel=mel)["mel"]
    assert torch.equal(o["mel"], m) and not torch.equal(o["mel"], full["mel"])
    # no MEL: LOG reads the VTLN vector, the cosine table spans all of it
    d129 = eng.fe_dct_table(1, 13, L // 2 + 1)
    o = eng.fe_process(xd, "pcm", ALL, D=D, shift=shift, L=L, vtln=vtln, dct=d129)
    assert "mel" not in o and torch.equal(o["vtln"], full["vtln"]) and o["log"].shape[-1] == L // 2 + 1
    check_log(o["log"].cpu().numpy(), o["vtln"].cpu().numpy(), 1.0, 1.0, False, "no mel: log")
    # a wanted stage whose table is missing is left out of the result; nothing else wanted: refused
    from distant_speech_recognition_amd import _lib
    with pytest.raises(_lib.BtkError) as e:
        eng.fe_process(xd, "pcm", ("vtln", "mel"), D=D, shift=shift, L=L)
    assert e.value.code == _lib.BTK_ERR_PARAMETER
    # neither: the reference script's default wiring, 13 cepstra from 129 log-power values
    o = eng.fe_process(xd, "pcm", ALL, D=D, shift=shift, L=L, dct=d129)
    assert sorted(o) == ["cep", "log", "power", "spectrum"]
    lg = o["log"].cpu().numpy().astype(np.float64)
    Dm = cf.dct_table(1, 13, L // 2 + 1).astype(np.float64)
    check_rows(o["cep"].cpu().numpy(), lg @ Dm.T, np.abs(lg) @ np.abs(Dm).T, "log power cepstra")


def test_refusals_leave_outputs_untouched(dev):
    import ctypes
    import torch
    from distant_speech_recognition_amd import _lib
    n = 2000
    x = torch.zeros((1, 1, n), dtype=torch.float32, device=dev)
    X = torch.full((1, 1, 64, 8193, 2), 7.0, dtype=torch.float32, device=dev)
    P = torch.full((1, 1, 64, 16384), 7.0, dtype=torch.float32, device=dev)

    def call(D=160, shift=160, L=256, powN=129):
        q = _lib.FeParams()
        q.S, q.C, q.T, q.in_stage, q.len, q.pcm_stride = 1, 1, 4, 0, n, n
        q.D, q.shift, q.L, q.window, q.powN = D, shift, L, 1, powN
        q.out[1], q.out[2] = X.data_ptr(), P.data_ptr()
        rc = _lib.lib().btk_fe_process(ctypes.cast(ctypes.pointer(q), ctypes.c_void_p), ctypes.c_void_p(x.data_ptr()), None)
        torch.cuda.synchronize()
        return rc

    for kw in (dict(L=128), dict(L=300), dict(L=32768), dict(D=300, shift=100), dict(shift=161), dict(shift=0), dict(powN=100)):
        assert call(**kw) == _lib.BTK_ERR_DIMENSION, kw
        assert bool((X == 7.0).all()) and bool((P == 7.0).all()), kw
    assert call() == _lib.BTK_OK                                   # four frames of 129 values, back to back
    assert bool((P.view(-1)[:4 * 129] == 0).all()) and bool((P.view(-1)[4 * 129:] == 7.0).all())
    assert bool((X.view(-1)[:4 * 129 * 2] == 0).all()) and bool((X.view(-1)[4 * 129 * 2:] == 7.0).all())


def test_device_hand_over_from_the_synthesis_bank(dev, proto256):
    """fe_process on the tensor FilterBank.synthesize returns == fe_process on an upload of its host copy."""
    import torch
    eng = _eng()
    h, g = proto256
    M, m, r = 256, 4, 1
    fb = eng.FilterBank(g, M, m, r, synthesis=True)
    rng = np.random.default_rng(2)
    Y = (rng.normal(size=(2, M // 2 + 1, 40)) + 1j * rng.normal(size=(2, M // 2 + 1, 40))).astype(np.complex64) * 1000
    pcm = fb.synthesize(torch.from_numpy(Y).to(dev))
    assert pcm.is_cuda and pcm.dim() == 2
    vtln, mel, dct = tables(129)
    kw = dict(D=400, shift=160, L=512, preemph=MU)
    mel2 = eng.fe_mel_table(257, 16000, 100, 6800, 30, 2)
    a = eng.fe_process(pcm, "pcm", ("power", "mel", "cep"), mel=mel2, dct=dct, **kw)
    b = eng.fe_process(torch.from_numpy(pcm.cpu().numpy()).to(dev), "pcm", ("power", "mel", "cep"), mel=mel2, dct=dct, **kw)
    assert a["cep"].shape == (2, 1, eng.fe_frames(pcm.shape[1], 400, 160), 13)
    for k in a:
        assert torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k]).all()), k
    assert float(a["power"].abs().max()) > 0


def test_longest_transform_and_long_vectors_at_stage_entry(dev):
    """L = 16384: one frame per workgroup, tables read from global memory; entering at SPECTRUM with powN = L the vectors
    take one frame per workgroup in the stage kernel too.  Spectra with the bits of btk_tdoa_spectra, the rest bit-equal
    between the two kernels and, stage by stage on the GPU's own previous stage, within the bounds of the closed form."""
    import torch
    from distant_speech_recognition_amd import _lib
    eng = _eng()
    D, L = 8192, 16384
    rng = np.random.default_rng(9)
    x = np.round(rng.normal(scale=3000.0, size=(1, 2, 2 * D + 100))).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    mel = eng.fe_mel_table(L // 2 + 1, 16000, 100, 6800, 30, 2)
    dct = eng.fe_dct_table(1, 13, 30)
    o = eng.fe_process(xd, "pcm", ("spectrum", "power", "mel", "cep"), D=D, L=L, mel=mel, dct=dct)
    Xt, _ = eng.tdoa_spectra(xd, D, L)
    assert o["spectrum"].shape == (1, 2, 3, L // 2 + 1) and torch.equal(torch.view_as_real(o["spectrum"]), torch.view_as_real(Xt))
    check_spectrum(o["spectrum"].cpu().numpy(), cf.spectrum64(closed_frames(x, x.shape[2], D, D, frames=3), L), L, "L=16384")
    late = eng.fe_process(o["spectrum"], "spectrum", ("power", "mel", "cep"), mel=mel, dct=dct)
    for k in ("power", "mel", "cep"):
        assert torch.equal(late[k], o[k]), k
    up = eng.fe_process(o["spectrum"], "spectrum", ("power", "log"), powN=L)
    assert up["power"].shape[-1] == L and torch.equal(up["power"][..., :L // 2 + 1], o["power"])
    assert torch.equal(up["power"][..., L // 2 + 1:], o["power"][..., 1:L // 2].flip(-1))
    with pytest.raises(_lib.BtkError) as e:                          # nsamples beyond the rows
        eng.fe_process(xd, "pcm", "power", D=D, L=L, nsamples=x.shape[2] + 1)
    assert e.value.code == _lib.BTK_ERR_DIMENSION
    # the later stages against the closed form, each on the GPU's own previous stage, as in test_every_stage; with the VTLN
    # table too, which like the others is read from global memory at this length
    powN = L // 2 + 1
    vtln = eng.fe_vtln_table(powN, 0.94, 0.8, 2)
    assert not cf.tables_in_lds(L, None, mel, dct) and not cf.tables_in_lds(L, vtln, mel, dct) and not TABLES_IN_LDS[L]
    off, cnt, rows = cf.mel_table(powN, 16000, 100, 6800, 30, 2)
    Dm = cf.dct_table(1, 13, 30).astype(np.float64)
    P = o["power"].cpu().numpy()
    check_rows(o["mel"].cpu().numpy(), cf.mel_apply(P, off, cnt, rows), cf.mel_abs(P, off, cnt, rows), "L=16384 mel on power")
    a = eng.fe_process(xd, "pcm", ALL, D=D, L=L, vtln=vtln, mel=mel, dct=dct)
    assert torch.equal(torch.view_as_real(a["spectrum"]), torch.view_as_real(o["spectrum"])) and torch.equal(a["power"], o["power"])
    late = eng.fe_process(a["spectrum"], "spectrum", ALL[1:], vtln=vtln, mel=mel, dct=dct)
    for k in ALL[1:]:
        assert torch.equal(late[k], a[k]), k
    a = {k: v.cpu().numpy() for k, v in a.items()}
    for k, d in (("vtln", powN), ("mel", 30), ("log", 30), ("cep", 13)):
        assert a[k].shape == (1, 2, 3, d), (k, a[k].shape)
    P64 = P.astype(np.float64)
    Vw = cf.vtln_ff(P64.reshape(-1, powN).T, powN, 0.94, 0.8).T.reshape(P64.shape)
    check_rows(a["vtln"], Vw, table_abs_apply(vtln, P64), "L=16384 vtln")
    check_rows(a["mel"], cf.mel_apply(a["vtln"], off, cnt, rows), cf.mel_abs(a["vtln"], off, cnt, rows), "L=16384 mel")
    check_log(a["log"], a["mel"], 1.0, 1.0, False, "L=16384 log")
    lg = a["log"].astype(np.float64)
    check_rows(a["cep"], lg @ Dm.T, np.abs(lg) @ np.abs(Dm).T, "L=16384 cep")


def table_abs_apply(tab, v):
    """sum |w| |in| per output row of an FeTable, row by row: np.abs(v) @ np.abs(tab.matrix()).T without the dense matrix"""
    v = np.abs(np.asarray(v, np.float64))
    w = np.abs(np.asarray(tab.coef, np.float64))
    out = np.zeros(v.shape[:-1] + (tab.rows,))
    for j in range(tab.rows):
        o_, c_, s_ = int(tab.offset[j]), int(tab.count[j]), int(tab.start[j])
        out[..., j] = v[..., o_:o_ + c_] @ w[s_:s_ + c_]
    return out
