"""GPU: the fused analysis -> beamformer kernels (fb_analysis512.hip, fb_fast.hip, fb_fused_big.hip) and the synthesis kernels
against the float64 closed forms of tests/closed_forms.py -- every stream, bin and frame, dense and shipped prototypes,
unit-modulus and one-hot weights, integer PCM in the int16 range.

Bound (closed_forms.accept): e_max and the worst bin's e_bin of the kernel <= 4 x the same figure of a plain float32 / complex64
numpy evaluation of the same inputs (the yardstick), never below 2^-22 of max|Y_cf|; a closed form that is identically zero must
be matched exactly.  The factor covers what two correct float32 evaluations differ by (FFT factorisation, fmaf, sum order) and sits
28 x under the smallest seeded fault (tap 1 of the shipped prototype dropped, N = 64: 112 x the yardstick, test_closed_forms_cpu.py).

Kernel / yardstick ratio per case (the larger of the e_max and the e_bin ratio; worst stream and frame range), MI355X, kernels
as they were before this module existed -- every entry is <= 4:

    case (worst stream / chunk)                    dense  shipped
    512 r1 N=1                                      2.20     1.70
    512 r1 N=2                                      2.06     1.86
    512 r1 N=3                                      1.97     1.98
    512 r1 N=63                                     1.87     1.60
    512 r1 N=64                                     1.47     2.09
    512 r1 N=65                                     1.99     2.12
    512 r1 N=128                                    1.57     1.47
    512 r1 T=1 first frames                         2.08     1.40
    512 r1 T=15 first frames                        2.00     1.96
    512 r1 T=15 whole                               2.33     1.72
    512 r1 T=16 first frames                        1.63     1.74
    512 r1 T=16 whole                               2.25     2.28
    512 r1 T=17 first frames                        1.93     1.92
    512 r1 T=17 whole                               2.00     1.96
    512 r1 T=112 first frames                       1.86     2.32
    512 r1 T=112 whole                              2.05     1.97
    512 r1 T=129 first frames                       1.70     1.81
    512 r1 T=129 whole                              1.50     1.49
    512 r1 T=271 first frames                       1.71     1.82
    512 r1 T=271 whole                              1.87     2.16
    512 r1 S=1 per-stream W                         1.82     1.89
    512 r1 S=2 per-stream W                         1.82     1.89
    512 r1 S=2 shared W                             1.82     1.89
    512 r1 S=9 per-stream W                         2.04     1.89
    512 r1 S=9 shared W                             2.15     2.38
    512 r1 S=33 per-stream W                        2.08     2.26
    512 r1 S=33 shared W                            2.15     2.38
    512 r0 N=3                                      2.16     1.60
    512 r0 N=64                                     2.14     1.76
    512 r0 one-hot                                  2.48     2.60
    512 r1 one-hot                                  2.56     2.03
    512 r2 N=3                                      2.02     1.59
    512 r2 N=64                                     1.70     1.63
    512 r2 one-hot                                  1.44     2.40
    512 r1 ranges                                   2.36     2.30
    512 r1 dct0 L=1                                 2.38     1.90
    512 r1 dct0 L=255                               1.85     1.91
    512 r1 dct0 L=257                               2.20     1.98
    512 r1 dct0 L=5887                              1.89     2.00
    512 r1 dct0 L=5889                              1.81     1.67
    512 r1 dct0 L=2306                              1.48     1.69
    512 r1 dct0 L=2311                              2.32     2.17
    512 r1 dct2 L=5887                              1.89     2.00
    512 r1 dct2 L=5889                              1.81     1.67
    512 r1 dct2 L=2306                              1.48     1.69
    512 r1 dct2 L=2311                              2.32     2.17
    512 r1 rows float32                             1.54     1.61
    512 r1 rows int16                               1.54     1.61
    512 r0 float32 entry                            1.94     1.55
    512 r0 int16 entry                              1.94     1.55
    512 r1 float32 entry                            1.33     1.95
    512 r1 int16 entry                              1.33     1.95
    512 r2 float32 entry                            2.15     1.47
    512 r2 int16 entry                              2.15     1.47
    C0                                              1.54     1.27
    512 r1 form 1                                   1.84     1.50
    512 r2 form 1                                   1.86     1.90
    512 r1 form 3                                   1.84     1.50
    512 r1 form 7                                   1.84     1.50
    512 r1 form 15                                  1.84     1.50
    512 r1 form 31                                  1.84     1.50
    512 r1 form 79                                  1.84     1.50
    512 r1 form 207                                 1.69     1.50
    512 r1 form 463                                 1.69     1.50
    512 r1 form 33231                               1.69     1.50
    512 r1 form 1031                                1.84     1.50
    256 r0 N=1 S=9                                  2.68     2.42
    256 r0 N=2 S=1                                  1.69     1.55
    256 r0 N=65 S=1                                 2.09     1.41
    256 r0 N=65 S=9 shared W                        1.95     2.08
    256 r0 one-hot                                  2.02     2.54
    256 r0 N=65 S=1 int16                           1.88     1.28
    256 r1 N=1 S=9                                  2.03     2.49
    256 r1 N=2 S=1                                  1.89     1.05
    256 r1 N=65 S=1                                 1.80     1.45
    256 r1 N=65 S=9 shared W                        2.35     1.81
    256 r1 one-hot                                  1.78     2.42
    256 r1 N=65 S=1 int16                           1.75     1.45
    256 r2 N=1 S=9                                  2.26     2.31
    256 r2 N=2 S=1                                  1.85     1.22
    256 r2 N=65 S=1                                 1.67     1.35
    256 r2 N=65 S=9 shared W                        2.58     1.78
    256 r2 one-hot                                  1.90     1.92
    256 r2 N=65 S=1 int16                           1.67     1.31
    1024 r1 N=1 S=9                                 2.48     2.21
    1024 r1 N=2 S=1                                 2.05     1.65
    1024 r1 N=65 S=1                                0.51     0.65
    1024 r1 N=65 S=9 shared W                       0.89     0.81
    1024 r1 one-hot                                 2.82     2.22
    1024 r1 N=65 S=1 int16                          0.51     0.65
    2048 r1 N=1 S=9                                 2.44     2.41
    2048 r1 N=2 S=1                                 2.09     1.80
    2048 r1 N=65 S=1                                0.60     0.81
    2048 r1 N=65 S=9 shared W                       0.74     0.78
    2048 r1 one-hot                                 2.41     2.51
    2048 r1 N=65 S=1 int16                          0.60     0.78
    synthesis 512 T=5                               1.13        -
    synthesis 512 T=20                              1.39        -
    synthesis 512 T=21                              1.72        -
    synthesis 512 T=300                             1.62        -
    synthesis 256 T=5                               1.72        -
    synthesis 256 T=20                              2.04        -
    synthesis 256 T=21                              1.38        -
    synthesis 256 T=300                             1.81        -
    synthesis 1024 T=5                              1.41        -
    synthesis 1024 T=20                             1.94        -
    synthesis 1024 T=21                             1.81        -
    synthesis 1024 T=300                            1.81        -
    synthesis 2048 T=5                              2.14        -
    synthesis 2048 T=20                             1.74        -
    synthesis 2048 T=21                             1.96        -
    synthesis 2048 T=300                            1.95        -
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import closed_forms as cf
from tests.util import design_prototype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
m, DCT = 4, 2
_FB, _PROTO = {}, {}


def _proto(M, name, kind="h"):
    key = (M, name, kind)
    if key not in _PROTO:
        _PROTO[key] = cf.dense_prototype(M, m, seed=kind == "g") if name == "dense" else design_prototype(M, m, kind)
    return _PROTO[key]


def _bank(M, r, name, dct=DCT, synthesis=False):
    from distant_speech_recognition_amd import engine as eng
    key = (M, r, name, dct, synthesis)
    if key not in _FB:
        _FB[key] = eng.FilterBank(_proto(M, name, "g" if synthesis else "h"), M, m, r, dct, synthesis=synthesis)
    return _FB[key]


_judge = cf.judge                                              # print the figures, then assert the rule


def _reference(M, r, name, pcm_s, W_s, dct=DCT):
    h = _proto(M, name)
    return cf.fused_cf(h, M, m, r, dct, pcm_s, W_s), cf.plain_f32(h, M, m, r, dct, pcm_s, W_s)


def _fused_case(dev, label, M, r, N, S, L, name, weights="unit", per_stream=True, tcount=None, i16=False, dct=DCT, seed=0, chunks=()):
    """One launch of FilterBank.analysis_beamform over the whole recording (or its first tcount frames), every stream against the
    closed form; then each (t0, tc) of chunks: equal to the slice of the whole launch bit for bit when asked, and against the
    closed form."""
    import torch
    fb = _bank(M, r, name, dct)
    K = M // 2 + 1
    pcm = cf.int_pcm(S, N, L, seed=seed + 13 * N + L)
    if weights == "onehot":
        W = cf.one_hot_weights(K, N)[None]
    else:
        W = cf.unit_weights(S if per_stream else 1, K, N, seed=seed + N)
    T = cf.num_frames(L, M, m, r, dct)
    assert fb.num_frames(L) == T
    p = torch.from_numpy(pcm.astype(np.int16) if i16 else pcm).to(dev)
    Wd = torch.from_numpy(W if W.shape[0] > 1 else W[0]).to(dev)
    tc = T if tcount is None else tcount
    assert tc <= T
    Yd = fb.analysis_beamform(p, Wd, tcount=tc)
    Y = Yd.cpu().numpy()
    assert Y.shape == (S, K, tc)
    if tc == 0:
        return Y
    refs = []
    for s in range(S):
        Ycf, Y32 = _reference(M, r, name, pcm[s], W[s if W.shape[0] > 1 else 0], dct)
        assert Ycf.shape == (K, T)
        refs.append((Ycf, Y32))
        _judge("%s s=%d" % (label, s), Y[s], Y32[:, :tc], Ycf[:, :tc])
        if weights == "onehot" and s == 0:                     # bin k is channel k mod N's own analysis
            for n in range(N):
                Xn = cf.analysis_cf(_proto(M, name), M, m, r, dct, pcm[s, n])[:tc, n:K:N].T
                assert np.array_equal(Ycf[n::N, :tc], Xn)
    for (t0, c, bits) in chunks:
        part = fb.analysis_beamform(p, Wd, t0=t0, tcount=c)
        assert part.shape == (S, K, c)
        if bits:
            assert torch.equal(part, Yd[:, :, t0:t0 + c]), (label, t0, c)
        pn = part.cpu().numpy()
        for s in range(S):
            _judge("%s s=%d t0=%d tc=%d" % (label, s, t0, c), pn[s], refs[s][1][:, t0:t0 + c], refs[s][0][:, t0:t0 + c])
    return Y


PROTOS = ("dense", "shipped")


# ---- M = 512: one function per axis -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 128])
def test_m512_channels(dev, N, name):
    _fused_case(dev, "512 r1 N=%d %s" % (N, name), 512, 1, N, 2, cf.num_samples(21, 512, m, 1, DCT) + 2, name)


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("T", [1, 15, 16, 17, 7 * 16, 8 * 16 + 1, 17 * 16 - 1])
def test_m512_frames(dev, T, name):
    """1, 1, 1, 2, 7, 9, 17 tiles over the eight XCD groups; ragged last tiles; launches of the first T frames of a recording
    (a whole recording has at least pd = 7 frames) and, from T = 15 on, a recording of exactly T frames."""
    L = cf.num_samples(max(T, 7), 512, m, 1, DCT)
    _fused_case(dev, "512 r1 T=%d first frames %s" % (T, name), 512, 1, 3, 2, L + 512, name, tcount=T)
    if T >= 15:
        _fused_case(dev, "512 r1 T=%d whole %s" % (T, name), 512, 1, 3, 2, L, name)


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("S,per_stream", [(1, True), (2, True), (2, False), (9, True), (9, False), (33, True), (33, False)])
def test_m512_streams(dev, S, per_stream, name):
    _fused_case(dev, "512 r1 S=%d %s W %s" % (S, "per-stream" if per_stream else "shared", name), 512, 1, 3, S,
                cf.num_samples(37, 512, m, 1, DCT) + 1, name, per_stream=per_stream)


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("r", [0, 1, 2])
def test_m512_decimation(dev, r, name):
    for N in (3, 64):
        _fused_case(dev, "512 r%d N=%d %s" % (r, N, name), 512, r, N, 2, cf.num_samples(40, 512, m, r, DCT) + 3, name)
    _fused_case(dev, "512 r%d one-hot %s" % (r, name), 512, r, 5, 1, cf.num_samples(40, 512, m, r, DCT) + 3, name, weights="onehot")


@pytest.mark.parametrize("name", PROTOS)
def test_m512_frame_ranges(dev, name):
    """[t0, t0 + tcount) as the frame-sharded callers launch it: the chunk is the slice of the whole launch bit for bit, and
    matches the closed form on its own."""
    T = 137
    chunks = [(t0, c, True) for t0 in (1, 15, 16, 1000 % T) for c in (1, 16, 100) if t0 + c <= T]
    assert len(chunks) >= 9
    _fused_case(dev, "512 r1 ranges %s" % name, 512, 1, 4, 2, cf.num_samples(T, 512, m, 1, DCT), name, chunks=chunks)


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("dct", [0, 2])
def test_m512_short_and_odd_recordings(dev, dct, name):
    """Recordings shorter than one tile's window span (every tile an edge tile, zero fill on both sides), lengths that are no
    multiple of D, L % 4 in {1, 2, 3} (no vector loads).  With dct = 2 a recording that ends inside the look-ahead has no frames."""
    D, SPAN = 256, 15 * 256 + 4 * 512
    seen = 0
    for L in (1, D - 1, D + 1, SPAN - 1, SPAN + 1, 9 * D + 2, 9 * D + 7):
        Y = _fused_case(dev, "512 r1 dct%d L=%d %s" % (dct, L, name), 512, 1, 3, 2, L, name, dct=dct)
        seen += Y.shape[-1] > 0
    assert seen == (7 if dct == 0 else 4)


def _raw_launch(dev, fb, buf_t, L, pitch, S, N, Wd, per_stream, Y, T, i16):
    """btk_fb_analysis_bf / _i16 through the C-ABI with the caller's own pointers and pitches."""
    import ctypes as C
    import torch
    from distant_speech_recognition_amd import engine as eng
    lib = eng._lib.lib()
    nb = lib.btk_fb_analysis_bf_scratch_bytes(fb._h, S, N, per_stream, T)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    fn = lib.btk_fb_analysis_bf_i16 if i16 else lib.btk_fb_analysis_bf
    eng.check(fn(fb._h, C.c_void_p(buf_t.data_ptr()), L, pitch, S, N, C.c_void_p(Wd.data_ptr()), per_stream,
                 C.c_void_p(Y.data_ptr()), Y.stride(1), 0, T, C.c_void_p(scratch.data_ptr()), nb, None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("i16", [False, True])
def test_m512_rows_pitch_and_alignment(dev, i16, name):
    """Rows L + 3 apart with nsamples = L, the base pointer 4 bytes past a 16-byte boundary (one float; two int16 samples -- the int16
    entry demands 4-byte alignment), Y contiguous and row-padded: the guarded loads and T_stride.  Both entries against the
    closed form, and the same bits from both."""
    import torch
    M, r, N, S, L = 512, 1, 5, 2, cf.num_samples(35, 512, m, 1, DCT) + 6
    fb = _bank(M, r, name)
    K, T, pitch = M // 2 + 1, fb.num_frames(L), L + 3
    pcm = cf.int_pcm(S, N, L, seed=91)
    W = cf.unit_weights(S, K, N, seed=5)
    Wd = torch.from_numpy(W).to(dev)
    off = 2 if i16 else 1
    flat = torch.zeros(S * N * pitch + off + 64, dtype=torch.int16 if i16 else torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    rows = flat[off: off + S * N * pitch].view(S, N, pitch)
    rows[..., :L] = torch.from_numpy(pcm.astype(np.int16) if i16 else pcm).to(dev)
    rows[..., L:] = 12345                                       # beyond nsamples: must not be read as signal
    assert rows.data_ptr() % 16 == 4
    Yc = torch.empty((S, K, T), dtype=torch.complex64, device=dev)
    Yp = torch.empty((S, K, T + 4 + (T % 2 == 0)), dtype=torch.complex64, device=dev)[..., :T]
    assert Yp.stride(1) % 2 == 1
    for Y in (Yc, Yp):
        _raw_launch(dev, fb, rows, L, pitch, S, N, Wd, 1, Y, T, i16)
    assert torch.equal(Yc, Yp)
    other = fb.analysis_beamform(torch.from_numpy(pcm if i16 else pcm.astype(np.int16)).to(dev), Wd)     # the other sample type, aligned
    assert torch.equal(Yc, other[..., :T])
    Yn = Yc.cpu().numpy()
    for s in range(S):
        Ycf, Y32 = _reference(M, r, name, pcm[s], W[s])
        _judge("512 r1 rows %s %s s=%d" % ("int16" if i16 else "float32", name, s), Yn[s], Y32, Ycf)


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("r", [0, 1, 2])
def test_m512_int16_entry(dev, r, name):
    args = (512, r, 6, 2, cf.num_samples(50, 512, m, r, DCT) + 1, name)
    Yf = _fused_case(dev, "512 r%d float32 entry %s" % (r, name), *args)
    Yi = _fused_case(dev, "512 r%d int16 entry %s" % (r, name), *args, i16=True)
    assert np.array_equal(Yf.view(np.uint32), Yi.view(np.uint32))


# ---- the C0 launch -------------------------------------------------------------------------------------------------------
def test_c0_launch_against_closed_form(dev):
    """S = 32, N = 64, T = 4096, shared W (the benchmark's launch): streams 0, 17 and 31 on every frame and bin with the dense
    prototype, stream 31 with the shipped one; the float32 yardstick on stream 31."""
    import torch
    M, r, S, N, T = 512, 1, 32, 64, 4096
    K, L = M // 2 + 1, cf.num_samples(T, M, m, r, DCT)
    g = torch.Generator(device=dev).manual_seed(20)
    p = (torch.randn((S, N, L), device=dev, generator=g) * 3000.0).round_().clamp_(-32767, 32767)
    W = cf.unit_weights(1, K, N, seed=3)[0]
    Wd = torch.from_numpy(W).to(dev)
    host = {s: p[s].cpu().numpy() for s in (0, 17, 31)}
    fig32 = None
    for name, streams in (("shipped", (31,)), ("dense", (31, 0, 17))):
        Y = _bank(M, r, name).analysis_beamform(p, Wd)
        assert Y.shape == (S, K, T)
        h = _proto(M, name)
        for s in streams:
            Ys = Y[s].cpu().numpy()
            Ycf = cf.fused_cf(h, M, m, r, DCT, host[s], W)
            if s == 31:
                Y32 = cf.plain_f32(h, M, m, r, DCT, host[s], W)
                fig32 = _judge("C0 %s s=31" % name, Ys, Y32, Ycf)
            else:                                               # yardstick figures of stream 31: same statistics, same sizes
                em, eb = cf.e_max(Ys, Ycf), float(np.max(cf.e_bin(Ys, Ycf)))
                print("CFRATIO %-58s ratio %7.3f  e_max %.3e (f32 %.3e)  e_bin %.3e (f32 %.3e)" %
                      ("C0 %s s=%d (yardstick of s=31)" % (name, s), max(em / fig32["y_max"], eb / fig32["y_bin"]), em, fig32["y_max"], eb, fig32["y_bin"]))
                assert em <= cf.FACTOR * fig32["y_max"] and eb <= cf.FACTOR * fig32["y_bin"], (name, s, em, eb, fig32)


# ---- the kept forms of the M = 512 kernel (BTK_FUSED_VAR is read once per process: one child each) -----------------------
FORM_CASES = [(3, 37, 0, "dense"), (3, 37, 3, "dense"), (64, 37, 0, "dense"), (64, 37, 3, "dense"), (64, 37, 3, "shipped")]   # N, T, extra samples, prototype

_FORM_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from distant_speech_recognition_amd import engine as eng
from tests import closed_forms as cf
from tests import test_gpu_fused_closed_form as t
dev = torch.device("cuda", 0)
out = {}
for r in [int(a) for a in sys.argv[3].split(",")]:
    for i, (N, T, extra, name) in enumerate(t.FORM_CASES):
        pcm, W, L = t._form_inputs(r, N, T, extra)
        Y = t._bank(512, r, name).analysis_beamform(torch.from_numpy(pcm).to(dev), torch.from_numpy(W).to(dev))
        out["r%d_%d" % (r, i)] = Y.cpu().numpy()
np.savez(sys.argv[2], **out)
"""


def _form_inputs(r, N, T, extra):
    L = cf.num_samples(T, 512, m, r, DCT) + extra
    return cf.int_pcm(2, N, L, seed=700 + N + extra), cf.unit_weights(2, 257, N, seed=9), L


def test_m512_kept_kernel_forms(dev):
    """Every form launch512_bf still dispatches, each in a process of its own, one after another, none started after a failure.
    The forms that read the window straight from HBM (7 and up) exist for r = 1; form 1 also runs at r = 2, where 3 is the default.
    33231 (the default at r = 1) differs from 463 only in the wave priority of the polyphase stage: equal bits."""
    forms = [("1", "1,2"), ("3", "1"), ("7", "1"), ("15", "1"), ("31", "1"), ("79", "1"), ("207", "1"), ("463", "1"), ("33231", "1"), ("1031", "1")]
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for var, rs in forms:
            env = dict(os.environ)
            env["BTK_FUSED_VAR"] = var
            path = os.path.join(tmp, "form_%s.npz" % var)
            res = subprocess.run([sys.executable, "-c", _FORM_CHILD, ROOT, path, rs], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
            assert res.returncode == 0, (var, res.stdout[-800:], res.stderr[-800:])          # no further child after a failure
            with np.load(path) as z:
                got[var] = {k: z[k] for k in z.files}
    refs = {}
    for var, rs in forms:
        for r in [int(a) for a in rs.split(",")]:
            for i, (N, T, extra, name) in enumerate(FORM_CASES):
                if (r, i) not in refs:
                    pcm, W, L = _form_inputs(r, N, T, extra)
                    refs[(r, i)] = [_reference(512, r, name, pcm[s], W[s]) for s in range(2)]
                Y = got[var]["r%d_%d" % (r, i)]
                assert Y.shape == (2, 257, cf.num_frames(_form_inputs(r, N, T, extra)[2], 512, m, r, DCT))
                for s in range(2):
                    _judge("512 r%d form %s N=%d +%d %s s=%d" % (r, var, N, extra, name, s), Y[s], refs[(r, i)][s][1], refs[(r, i)][s][0])
    for k in got["463"]:
        assert np.array_equal(got["463"][k].view(np.uint32), got["33231"][k].view(np.uint32)), k


# ---- the siblings: M = 256 (fb_fast.hip), M = 1024 / 2048 (fb_fused_big.hip) -----------------------------------------------
@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("M,r", [(256, 0), (256, 1), (256, 2), (1024, 1), (2048, 1)])
def test_sibling_geometries(dev, M, r, name):
    L = cf.num_samples(29, M, m, r, DCT) + 3                   # ragged last tile, L % 4 = 3
    tag = "%d r%d" % (M, r)
    i16 = _bank(M, r, name).fused_i16()
    _fused_case(dev, "%s N=1 S=9 %s" % (tag, name), M, r, 1, 9, L, name, chunks=[(5, 13, False)])
    _fused_case(dev, "%s N=2 S=1 %s" % (tag, name), M, r, 2, 1, L, name, chunks=[(17, 12, False)])
    Yf = _fused_case(dev, "%s N=65 S=1 %s" % (tag, name), M, r, 65, 1, L, name, chunks=[(3, 20, False)])
    _fused_case(dev, "%s N=65 S=9 shared W %s" % (tag, name), M, r, 65, 9, L - 3, name, per_stream=False)
    _fused_case(dev, "%s one-hot %s" % (tag, name), M, r, 5, 1, L, name, weights="onehot")
    if i16:
        Yi = _fused_case(dev, "%s N=65 S=1 int16 %s" % (tag, name), M, r, 65, 1, L, name, i16=True)
        assert np.array_equal(Yf.view(np.uint32), Yi.view(np.uint32))


# ---- synthesis ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [512, 256, 1024, 2048])
def test_synthesis_against_closed_form(dev, M):
    """synthesize with the dense g and random complex Y in bins 0 .. M/2 (the closed form gets the Hermitian extension), whole runs
    and [b0, b0 + bcount) pieces with b0 + pd odd and even (the wide form of M = 512 needs it even), contiguous Y and rows an odd
    number of frames apart (the narrow form)."""
    import torch
    r, S, K = 1, 2, M // 2 + 1
    D = M >> r
    g = _proto(M, "dense", "g")
    sfb = _bank(M, r, "dense", synthesis=True)
    pd = cf.fb_delays(m, r, True, DCT)[0]
    assert sfb.processing_delay == pd
    rng = np.random.default_rng(M)
    for T in (pd + 1, pd + 16, pd + 17, 300):
        Yn = ((rng.normal(size=(S, K, T)) + 1j * rng.normal(size=(S, K, T))) * 1000.0).astype(np.complex64)
        Yc = torch.from_numpy(Yn).to(dev)
        Yp = torch.empty((S, K, T + 2 + (T % 2 == 0)), dtype=torch.complex64, device=dev)[..., :T]
        Yp.copy_(Yc)
        assert Yp.stride(1) % 2 == 1
        B = T - pd
        assert sfb.num_blocks(T) == B
        refs = []
        for s in range(S):
            full = cf.hermitian(Yn[s], M)
            refs.append((cf.synthesis_cf(g, M, m, r, DCT, full).reshape(B, D), cf.synthesis_f32(g, M, m, r, DCT, full).reshape(B, D)))
        pieces = sorted({(0, B)} | {(b0, min(c, B - b0)) for b0, c in ((1, 20), (2, 21), (B - 1, 1)) if B - b0 >= 1})
        for kind, Yd in (("contiguous", Yc), ("odd stride", Yp)):
            for b0, c in pieces:
                out = sfb.synthesize(Yd, b0=b0, bcount=c).cpu().numpy()
                assert out.shape == (S, c * D)
                for s in range(S):
                    _judge("synthesis %d T=%d %s b0=%d bc=%d s=%d" % (M, T, kind, b0, c, s), out[s].reshape(c, D),
                           refs[s][1][b0:b0 + c], refs[s][0][b0:b0 + c])
