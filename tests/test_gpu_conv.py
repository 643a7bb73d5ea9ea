"""GPU: btk_conv_filter_spectra / btk_conv_apply / btk_conv_blocks (engine.conv_filter, fir_convolve, conv_blocks) against the
float64 direct sums of tests/conv_closed_form.py on the float32 inputs.  Every sample of every output is compared.

Bound of one tile (derived, not tuned).  u = 2^-24; mu, eta and B = B_N = (log2 N + 1) eta as in DESIGN 3.17 / tests/test_gpu_tdoa.py:
a real N-point transform of the kernel (N/2-point complex transform from fft_long.h plus the split or pre-twist step) returns
X^ with |X^ - X|_2 <= B |X|_2 over the N bins.  By Parseval |X|_2 = sqrt(N) |x|_2, and |X|_inf <= |x|_1.

A tile transforms, per partition q, the span x_q (N samples; zero wherever the kernel reads zero) and multiplies with the stored
spectrum of the taps h_q, itself a computed transform of float32 taps:
    X^_q = X_q + dX_q,  |dX_q|_2 <= B sqrt(N) |x_q|_2;        H^_q = H_q + dH_q,  |dH_q|_2 <= B sqrt(N) |h_q|_2.
The bin product is a complex product with one fused multiply-add per component, relative error <= sqrt(2) gamma_2 (Higham,
Lemma 3.5; bins 0 and N/2 take the real parts of operands whose exact values are real, which moves them no further from those),
and the Q products are added in ascending order, Q - 1 float additions: c = sqrt(2) gamma_2 + (Q - 1) u relative to each product.
With G = sum_q X_q H_q the exact spectrum of the section and |A o B|_2 <= |A|_2 |B|_inf:
    |X^_q H^_q - X_q H_q|_2 <= |dX_q|_2 |H_q|_inf + |X_q|_inf |dH_q|_2 + |dX_q|_2 |dH_q|_2  =  sqrt(N) d_q,
    d_q = B |x_q|_2 |h_q|_1 + B |x_q|_1 |h_q|_2 + B^2 sqrt(N) |x_q|_2 |h_q|_2,
    |X^_q H^_q|_2 <= sqrt(N) (|x_q|_2 |h_q|_1 + d_q),
    |G^ - G|_2 <= sqrt(N) e_G,     e_G = sum_q [(1 + c) d_q + c |x_q|_2 |h_q|_1].
The inverse transform of G^ (scaled by 1/N, a power of two: exact) errs by at most B |G^|_2 / sqrt(N) in the 2-norm of the N
section samples, and |G^|_2 / sqrt(N) <= sum_q |x_q|_2 |h_q|_1 + e_G (Young's inequality for the circular convolutions).  So
    |y^ - y|_2 over the samples a tile stores  <=  e_G + B (sum_q |x_q|_2 |h_q|_1 + e_G),
two transforms' worth on |x_q|_2 |h_q|_1, one on |x_q|_1 |h_q|_2, the products' c, and the second-order terms written out; no
factor is fitted.  conv_closed_form.apply_tile_bounds / blocks_tile_bounds evaluate it tile by tile; a tile whose spans are all
zero must be exactly zero.  Every test prints its largest error / bound ratio (pytest -s shows them).

Bits.  A span element no stored sample depends on is read as zero, so an output's bits depend on its tile's position, the
samples its sums name and the filter: cutting a row at a multiple of Lk, the other streams of the launch and memory outside
[-hist, len) leave them as they are.
"""
import ctypes as C

import numpy as np
import pytest

from tests import conv_closed_form as cf

pytestmark = pytest.mark.gpu


def _eng():
    from distant_speech_recognition_amd import engine
    return engine


def _signal(seed, S, n):
    rng = np.random.default_rng(seed)
    return cf.f32(rng.normal(size=(S, n)) * 1000.0)


def _taps(seed, shape):
    rng = np.random.default_rng(seed)
    P = shape[-1]
    return cf.f32(rng.normal(size=shape) * np.exp(-3.0 * np.arange(P) / P))


def _check_apply(name, y, x, h, plan, out_len, hist=0):
    """y [S][C][out_len] against the direct sums of x [S][hist + len] with h [S_h][C][P], tile by tile; -> worst error / bound"""
    S, Cn = y.shape[:2]
    worst = 0.0
    for s in range(S):
        for c in range(Cn):
            hc = h[s if h.shape[0] > 1 else 0, c]
            ref = cf.direct(x[s], hc, out_len, hist)
            worst = max(worst, cf.worst_ratio(y[s, c], ref, cf.apply_tile_bounds(x[s], hc, plan, out_len, hist)))
    print("%s: largest tile error / bound = %.2e" % (name, worst))
    assert np.all(np.isfinite(y)) and worst <= 1.0
    return worst


def _run(dev, x, h, plan, out_len=None, hist=0):
    import torch
    eng = _eng()
    filt = eng.conv_filter(torch.from_numpy(h).to(dev), plan=plan)
    y = eng.fir_convolve(torch.from_numpy(x).to(dev), filt, out_len=out_len, hist=hist)
    return y.cpu().numpy(), filt


@pytest.mark.parametrize("P", [157, 1])
def test_full_section_n256(dev, P):
    # Lk + P - 1 = N at P = 157: the section is exactly full
    plan = (256, 100, P, 1)
    S, Cn, n = 2, 2, 730                                    # eight tiles, the last one partial
    x, h = _signal(1, S, n), _taps(2, (1, Cn, P))
    for out_len in (n, n + P - 1):
        y, _ = _run(dev, x, h, plan, out_len)
        assert y.shape == (S, Cn, out_len)
        _check_apply("N=256 Lk=100 P=%d out_len=%d" % (P, out_len), y, x, h, plan, out_len)
    if P == 1:                                              # one tap: a gain
        assert np.allclose(y[0, 0], x[0] * h[0, 0, 0], rtol=1e-5, atol=1e-3)


@pytest.fixture(scope="module")
def partitioned(dev):
    """N = 512, Bp = 200, Q = 3, P = 523 (the last partition has 123 taps), Lk = 313; len ends inside the fifth tile.  The rows
    lie in a buffer filled with NaN in front of and behind them; row 1 of the three-stream signal is all zero."""
    import torch
    plan, P, n = (512, 313, 200, 3), 523, 4 * 313 + 150
    S, Cn, front, back = 3, 3, 40, 77
    x = _signal(3, S, n)
    x[1] = 0.0
    h = _taps(4, (S, Cn, P))
    buf = torch.full((S, front + n + back), float("nan"), dtype=torch.float32, device=dev)
    buf[:, front:front + n] = torch.from_numpy(x).to(dev)
    return dict(plan=plan, P=P, n=n, S=S, C=Cn, x=x, h=h, buf=buf, front=front)


@pytest.mark.parametrize("per_stream", [False, True])
def test_partitioned_n512(dev, partitioned, per_stream):
    import torch
    eng, p = _eng(), partitioned
    h = p["h"] if per_stream else p["h"][:1]
    filt = eng.conv_filter(torch.from_numpy(h).to(dev), plan=p["plan"])
    assert tuple(filt.H.shape) == (h.shape[0], p["C"], 3, 257)
    xv = p["buf"][:, p["front"]:p["front"] + p["n"]]        # a view: NaN on both sides of every row
    for out_len in (p["n"], p["n"] + p["P"] - 1):
        y = eng.fir_convolve(xv, filt, out_len=out_len).cpu().numpy()
        _check_apply("N=512 Bp=200 Q=3 P=523 S_h=%d out_len=%d" % (h.shape[0], out_len), y, p["x"], h, p["plan"], out_len)
        assert not np.any(y[1])                             # an all-zero row gives exactly 0
    # a stream alone has the bits it has among the others
    alone = eng.fir_convolve(xv[2:3], eng.conv_filter(torch.from_numpy(h[-1:]).to(dev), plan=p["plan"]), out_len=out_len)
    assert np.array_equal(alone.cpu().numpy()[0], y[2])


def test_two_calls_continue_a_stream_bit_for_bit(dev, partitioned):
    import torch
    eng, p = _eng(), partitioned
    P, n, Lk, front = p["P"], p["n"], p["plan"][1], p["front"]
    filt = eng.conv_filter(torch.from_numpy(p["h"][:1]).to(dev), plan=p["plan"])
    xv = p["buf"][:, front:front + n]
    whole = eng.fir_convolve(xv, filt).cpu().numpy()
    a = 2 * Lk                                              # the cut lies on a tile boundary
    first = eng.fir_convolve(p["buf"][:, front:front + a], filt).cpu().numpy()
    assert np.array_equal(first, whole[:, :, :a])
    for hist in (P - 1, a):                                 # the samples the sums reach, or more of the past
        second = eng.fir_convolve(p["buf"][:, front + a - hist:front + n], filt, hist=hist).cpu().numpy()
        assert second.shape[-1] == n - a and np.array_equal(second, whole[:, :, a:])
    # a history shorter than P - 1 is a history with zeros in front of it
    hist = 100
    short = eng.fir_convolve(p["buf"][:, front + a - hist:front + n], filt, hist=hist)
    z = torch.zeros((p["S"], P - 1 + n - a), dtype=torch.float32, device=dev)
    z[:, P - 1 - hist:] = p["buf"][:, front + a - hist:front + n]
    padded = eng.fir_convolve(z, filt, hist=P - 1)
    assert torch.equal(short, padded)
    xs = np.concatenate([p["x"][:, a - hist:a], p["x"][:, a:]], axis=1)
    _check_apply("hist=100 < P-1", short.cpu().numpy(), xs, p["h"][:1], p["plan"], n - a, hist)
    # out= is written in place
    out = torch.full((p["S"], p["C"], n), 5.0, dtype=torch.float32, device=dev)
    assert eng.fir_convolve(xv, filt, out=out) is out and np.array_equal(out.cpu().numpy(), whole)


def test_largest_transform_n16384(dev):
    plan, P = (16384, 8192, 8193, 1), 8193
    n = 2 * 8192 + 5000                                     # three tiles
    x, h = _signal(5, 1, n), _taps(6, (1, 1, P))
    for out_len in (n, n + P - 1):
        y, _ = _run(dev, x, h, plan, out_len)
        _check_apply("N=16384 Lk=8192 P=8193 out_len=%d" % out_len, y, x, h, plan, out_len)
    assert _eng().conv_plan(P) == plan


@pytest.mark.parametrize("case", cf.CASES, ids=[c[0] for c in cf.CASES])
def test_every_length(dev, case):
    """N = 1024 ... 8192 (conv_closed_form.CASES): a section exactly full and a three-partition filter with a short last
    partition at each, and at N = 8192, the one length compiled under a register cap, the plans the rule itself picks."""
    name, plan, P, S_h, rule = case
    S, Cn, n = cf.CASE_S, cf.CASE_C, cf.case_len(plan)
    seed = 100 + [c[0] for c in cf.CASES].index(name)
    x, h = _signal(seed, S, n), _taps(seed + 50, (S if S_h == 0 else 1, Cn, P))
    if rule is not None:
        assert _eng().conv_plan(*rule) == plan
    for out_len in (n, n + P - 1):
        y, filt = _run(dev, x, h, plan, out_len)
        assert y.shape == (S, Cn, out_len) and tuple(filt.H.shape) == (h.shape[0], Cn, plan[3], plan[0] // 2 + 1)
        _check_apply("%s N=%d Lk=%d Bp=%d Q=%d P=%d S_h=%d out_len=%d" % ((name,) + plan + (P, h.shape[0], out_len)), y, x, h, plan,
                     out_len)
    if rule is not None and rule[1] == 16384:               # the default call picks the same plan
        import torch
        f = _eng().conv_filter(torch.from_numpy(h).to(dev))
        assert (f.N, f.Lk, f.Bp, f.Q) == plan and torch.equal(torch.view_as_real(f.H), torch.view_as_real(filt.H))


@pytest.mark.parametrize("plan,P", [((256, 100, 157, 1), 157), ((512, 313, 200, 3), 523)], ids=["n256_q1", "n512_q3"])
def test_truncated_output(dev, plan, P):
    """out_len < len: the row is cut inside a tile, and inside the first tile (a single partial tile, out_len < Lk).  The
    samples that are stored have the bits of the untruncated call: a tile's position and its sums are the same."""
    Lk = plan[1]
    S, Cn, n = 2, 2, 4 * Lk + 50
    x, h = _signal(30 + plan[3], S, n), _taps(31 + plan[3], (1, Cn, P))
    whole, _ = _run(dev, x, h, plan, n)
    for out_len in (2 * Lk + 37, Lk - 41):
        assert out_len < n and out_len % Lk != 0
        y, _ = _run(dev, x, h, plan, out_len)
        assert y.shape == (S, Cn, out_len)
        _check_apply("truncated N=%d Q=%d out_len=%d < len=%d" % (plan[0], plan[3], out_len, n), y, x, h, plan, out_len)
        full_tiles = out_len // Lk * Lk                     # the tiles in front of the cut one see the same spans
        assert np.array_equal(y[..., :full_tiles], whole[..., :full_tiles])


def test_out_view_of_a_wider_buffer(dev):
    """out= as a [..., :out_len] view of a buffer with padded rows: the padding keeps its sentinel and the samples are those of
    the contiguous call, bit for bit."""
    import torch
    eng = _eng()
    plan, P = (512, 313, 200, 3), 523
    S, Cn, n, pad = 2, 2, 2 * 313 + 150, 24
    x, h = _signal(40, S, n), _taps(41, (1, Cn, P))
    xd = torch.from_numpy(x).to(dev)
    filt = eng.conv_filter(torch.from_numpy(h).to(dev), plan=plan)
    for out_len in (n, n + P - 1, 313 - 41):
        want = eng.fir_convolve(xd, filt, out_len=out_len)
        wide = torch.full((S, Cn, out_len + pad), -7.0, dtype=torch.float32, device=dev)
        got = eng.fir_convolve(xd, filt, out_len=out_len, out=wide[..., :out_len])
        assert got.data_ptr() == wide.data_ptr() and tuple(got.shape) == (S, Cn, out_len)
        assert bool((wide[..., out_len:] == -7.0).all())
        assert torch.equal(wide[..., :out_len], want)
    _check_apply("out= view, out_len=%d" % out_len, wide[..., :out_len].cpu().numpy(), x, h, plan, out_len)
    # a view whose rows are not contiguous is refused and nothing is written
    wide = torch.full((S, Cn, 2 * n), -7.0, dtype=torch.float32, device=dev)
    from distant_speech_recognition_amd import _lib
    with pytest.raises((ValueError, _lib.BtkError)):
        eng.fir_convolve(xd, filt, out=wide[..., ::2])
    assert bool((wide == -7.0).all())


def test_default_plan_and_unit_tap(dev):
    import torch
    eng = _eng()
    # a unit tap at delay d reproduces the input, shifted
    d, n = 300, 2000
    x = _signal(7, 2, n)
    h = np.zeros((1, 1, d + 1), np.float32)
    h[0, 0, d] = 1.0
    filt = eng.conv_filter(torch.from_numpy(h[0]).to(dev))  # [C][P]: shared filters
    plan = (filt.N, filt.Lk, filt.Bp, filt.Q)
    assert plan == eng.conv_plan(d + 1) == (8192, 7892, 301, 1)
    y = eng.fir_convolve(torch.from_numpy(x).to(dev), filt).cpu().numpy()
    _check_apply("unit tap at 300", y, x, h, plan, n)
    assert np.allclose(y[:, 0, d:], x[:, :n - d], rtol=0, atol=1e-2) and np.allclose(y[:, 0, :d], 0, atol=1e-2)
    # float64 taps are rounded to float32
    h64 = np.random.default_rng(8).normal(size=(2, 40))
    f64 = eng.conv_filter(torch.from_numpy(h64).to(dev), n_max=256)
    f32 = eng.conv_filter(torch.from_numpy(h64.astype(np.float32)).to(dev), n_max=256)
    assert (f64.N, f64.Q, f64.C, f64.S_h) == (256, 1, 2, 1) and torch.equal(f64.H, f32.H)
    # partitioning chosen by the rule at a small cap
    hp = _taps(9, (1, 2, 300))
    fp = eng.conv_filter(torch.from_numpy(hp).to(dev), n_max=256)
    assert (fp.N, fp.Lk, fp.Bp, fp.Q) == (256, 129, 128, 3)
    yp = eng.fir_convolve(torch.from_numpy(x).to(dev), fp, out_len=n + 299).cpu().numpy()
    _check_apply("n_max=256 P=300 Q=3", yp, x, hp, (256, 129, 128, 3), n + 299)


@pytest.mark.parametrize("step", [100, 256])
def test_block_form(dev, step):
    import torch
    eng = _eng()
    L, P, S, Cn, n = 256, 17, 2, 2, 1300
    x, h = _signal(10 + step, S, n), _taps(11, (1, Cn, P))
    filt = eng.conv_filter(torch.from_numpy(h).to(dev), plan=(L, L - P + 1, P, 1))
    y = eng.conv_blocks(torch.from_numpy(x).to(dev), filt, L, step).cpu().numpy()
    T = (n - L) // step + 1
    assert y.shape == (S, Cn, T, L - P)
    worst = 0.0
    for s in range(S):
        for c in range(Cn):
            ref, bounds = cf.blocks_direct(x[s], h[0, c], L, step), cf.blocks_tile_bounds(x[s], h[0, c], L, step)
            for t in range(T):
                worst = max(worst, float(np.sqrt(np.sum((y[s, c, t] - ref[t]) ** 2))) / bounds[t])
    print("block form L=256 P=17 step=%d: largest block error / bound = %.2e" % (step, worst))
    assert worst <= 1.0
    # every block stands alone: block t of the row is block 0 of the row cut there
    t = 3
    one = eng.conv_blocks(torch.from_numpy(x[:, t * step:t * step + L].copy()).to(dev), filt, L, step).cpu().numpy()
    assert one.shape[2] == 1 and np.array_equal(one[:, :, 0], y[:, :, t])


@pytest.mark.parametrize("L,P,step,T", [(1024, 17, 700, 3),     # another length, overlapping blocks
                                         (8192, 17, 8192, 2),    # the length under the register cap, blocks back to back
                                         (256, 1, 100, 4),       # P = 1: o = 1, n_out = L - 1
                                         (256, 255, 256, 3),     # P = L - 1: one output per block
                                         (256, 17, 300, 4)])     # a step above L: the samples between blocks are read by nobody
def test_block_form_parameters(dev, L, P, step, T):
    import torch
    eng = _eng()
    S, Cn = 2, 2
    n = (T - 1) * step + L + min(step, L) // 2              # T blocks fit, a rest behind the last one belongs to no block
    x, h = _signal(20 + P + step, S, n), _taps(21 + L, (1, Cn, P))
    if step > L:                                            # what lies between the blocks must not matter: NaN there
        for t in range(T):
            x[:, t * step + L:(t + 1) * step] = np.nan
    filt = eng.conv_filter(torch.from_numpy(h).to(dev), plan=(L, L - P + 1, P, 1))
    y = eng.conv_blocks(torch.from_numpy(x).to(dev), filt, L, step).cpu().numpy()
    assert (n - L) // step + 1 == T and y.shape == (S, Cn, T, L - P) and np.all(np.isfinite(y))
    xz = np.nan_to_num(x, nan=0.0)                          # the closed form reads only inside the blocks; its norms want numbers
    worst = 0.0
    for s in range(S):
        for c in range(Cn):
            ref, bounds = cf.blocks_direct(xz[s], h[0, c], L, step), cf.blocks_tile_bounds(xz[s], h[0, c], L, step)
            assert ref.shape == (T, L - P) and len(bounds) == T
            for t in range(T):
                worst = max(worst, float(np.sqrt(np.sum((y[s, c, t] - ref[t]) ** 2))) / bounds[t])
    print("block form L=%d P=%d step=%d T=%d: largest block error / bound = %.2e" % (L, P, step, T, worst))
    assert worst <= 1.0
    # every block stands alone: block t of the row is block 0 of the row cut there
    t = T - 1
    one = eng.conv_blocks(torch.from_numpy(x[:, t * step:t * step + L].copy()).to(dev), filt, L, step).cpu().numpy()
    assert one.shape[2] == 1 and np.array_equal(one[:, :, 0], y[:, :, t])


def test_refusals_leave_outputs_untouched(dev):
    import torch
    from distant_speech_recognition_amd import _lib
    eng, lib = _eng(), _lib.lib()
    x = torch.from_numpy(_signal(12, 2, 1000)).to(dev)
    h = torch.from_numpy(_taps(13, (1, 3, 157))).to(dev)
    filt = eng.conv_filter(h, plan=(256, 100, 157, 1))
    y = torch.full((2, 3, 1000), 7.0, dtype=torch.float32, device=dev)
    H = torch.full((1, 3, 1, 129), 7.0, dtype=torch.complex64, device=dev)
    p, null = (lambda t: C.c_void_p(t.data_ptr())), C.c_void_p(0)

    def apply(xp=None, Hp=None, yp=None, S_h=1, P=157, N=256, Lk=100, Bp=157, Q=1):
        return lib.btk_conv_apply(p(x) if xp is None else xp, 1000, 0, 1000, 2, p(filt.H) if Hp is None else Hp, S_h, 3, P, N, Lk, Bp,
                                  Q, p(y) if yp is None else yp, 1000, 1000, null)

    D, PAR = _lib.BTK_ERR_DIMENSION, _lib.BTK_ERR_PARAMETER
    assert [apply(N=300), apply(N=128), apply(Lk=101), apply(Q=2, Bp=70), apply(P=0), apply(S_h=3)] == [D] * 6
    assert [apply(xp=null), apply(Hp=null)] == [PAR] * 2
    assert lib.btk_conv_blocks(p(x), 1000, 1000, 2, 3, 100, p(filt.H), 1, 3, 256, 256, p(y), null) == D
    assert lib.btk_conv_blocks(p(x), 1000, 1000, 2, 3, 100, p(filt.H), 1, 3, 17, 200, p(y), null) == D
    assert lib.btk_conv_blocks(null, 1000, 1000, 2, 3, 100, p(filt.H), 1, 3, 17, 256, p(y), null) == PAR
    assert lib.btk_conv_filter_spectra(p(h), 157, 3, 157, 300, 157, 1, p(H), null) == D
    assert lib.btk_conv_filter_spectra(p(h), 157, 3, 157, 256, 100, 1, p(H), null) == D
    assert lib.btk_conv_filter_spectra(null, 157, 3, 157, 256, 157, 1, p(H), null) == PAR
    torch.cuda.synchronize()
    assert bool(torch.all(y == 7.0)) and bool(torch.all(H == 7.0))
    # the engine's own checks
    with pytest.raises(_lib.BtkError):
        eng.fir_convolve(x, eng.conv_filter(torch.zeros((3, 3, 157), device=dev), plan=(256, 100, 157, 1)))   # filters of 3 streams, 2 rows
    with pytest.raises(_lib.BtkError):
        eng.conv_blocks(x, filt, 512, 100)                  # the filter was cut for another block length
    with pytest.raises(_lib.BtkError):
        eng.fir_convolve(x, filt, hist=1001)
    with pytest.raises(_lib.BtkError):
        eng.conv_filter(h, n_max=1000)


def test_result_feeds_the_analysis_bank_and_the_tdoa_front_end(dev):
    import torch
    from tests.util import design_prototype
    eng = _eng()
    M, m = 128, 4
    S, Cn, n = 2, 3, 4000
    x = torch.from_numpy(_signal(14, S, n)).to(dev)
    filt = eng.conv_filter(torch.from_numpy(_taps(15, (Cn, 200))).to(dev))
    y = eng.fir_convolve(x, filt)                           # [S][C][len]: an array recording from S dry sources
    assert y.dtype == torch.float32 and tuple(y.shape) == (S, Cn, n) and y.is_contiguous()
    afb = eng.FilterBank(design_prototype(M, m), M, m, 1, 2)
    X = afb.analysis(y)
    back = torch.from_numpy(y.cpu().numpy().copy()).to(dev)  # the same samples after a host round trip
    assert torch.equal(torch.view_as_real(X), torch.view_as_real(afb.analysis(back)))
    Z, e = eng.tdoa_spectra(y, 400, 512)
    Zb, eb = eng.tdoa_spectra(back, 400, 512)
    assert torch.equal(torch.view_as_real(Z), torch.view_as_real(Zb)) and torch.equal(e, eb)
