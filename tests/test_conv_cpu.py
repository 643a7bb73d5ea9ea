"""CPU: the yardstick of the block-convolution tests against itself (the restated OverlapAdd / OverlapSave bodies equal the
direct sums within the float32 running-sum bound), btk_conv_plan, every refusal of the ABI (called with null pointers: nothing
can be launched) and the nodes' constructors and sizes (construction touches no device)."""
import ctypes as C

import numpy as np
import pytest

from tests import conv_closed_form as cf


def _blocks(x, L, shift):
    """SampleFeature(block_len=L, shift_len=shift, pad_zeros=True) over x"""
    out = []
    cur = 0
    while cur < len(x):
        b = np.zeros(L, np.float32)
        seg = x[cur:cur + L]
        b[:len(seg)] = seg
        out.append(b)
        cur += shift
    return np.stack(out)


@pytest.mark.parametrize("L,shift,P,n", [(64, 32, 20, 500),      # overlapping source blocks
                                         (16, 16, 50, 300),      # P - 1 > L: the tail spans several blocks
                                         (32, 32, 1, 200),       # P = 1
                                         (64, 64, 64, 640)])
def test_overlap_add_restated_is_the_convolution_of_the_blocks_as_served(L, shift, P, n):
    rng = np.random.default_rng(L * 1000 + P)
    x = cf.f32(rng.normal(size=n) * 1000)
    h = cf.f32(rng.normal(size=P)).astype(np.float64)
    blocks = _blocks(x, L, shift)
    served = blocks.reshape(-1)
    out = cf.overlap_add_restated(blocks, h).reshape(-1)
    ref = cf.direct(served, h)
    bound = cf.running_sum_bound(blocks, served, h, len(served))
    ratio = np.max(np.abs(out - ref) / np.where(bound > 0, bound, 1.0))
    print("OverlapAdd restated: L=%d shift=%d P=%d largest error / bound = %.3f" % (L, shift, P, ratio))
    assert out.shape == served.shape and np.all(np.abs(out - ref) <= bound)
    assert ratio > 0 or P == 1                              # the running sum really is float32
    # an explicit transform length gives the same sums; one that is too short is refused as the reference refuses it
    out2 = cf.overlap_add_restated(blocks, h, fft_len=cf.next_pow2(L + P - 1)).reshape(-1)
    assert np.array_equal(out2, out)
    with pytest.raises(ValueError):
        cf.overlap_add_restated(blocks, h, fft_len=L + P - 2)


@pytest.mark.parametrize("L,P", [(64, 17), (32, 1), (64, 63)])
def test_overlap_save_restated_is_the_block_sum(L, P):
    rng = np.random.default_rng(L + P)
    x = cf.f32(rng.normal(size=5 * L) * 1000)
    h = cf.f32(rng.normal(size=P)).astype(np.float64)
    blocks = _blocks(x, L, L)
    out = cf.overlap_save_restated(blocks, h)
    ref = cf.blocks_direct(x, h, L, L)
    bound = cf.block_rounding_bound(blocks, h, cf.blocks_direct(np.abs(x), np.abs(h), L, L))
    assert out.shape == (5, L - P) and np.all(np.abs(out - ref) <= bound)
    with pytest.raises(ValueError):
        cf.overlap_save_restated(blocks, np.ones(L))


@pytest.fixture(scope="module")
def engine():
    from distant_speech_recognition_amd import engine
    return engine


PLAN_CASES = [  # P, n_max -> N, Lk, Bp, Q
    (1, 16384, (8192, 8192, 1, 1)),          # short filters: 8192 where the cap admits it
    (64, 16384, (8192, 8129, 64, 1)),
    (64, 1024, (1024, 961, 64, 1)),
    (2048, 16384, (8192, 6145, 2048, 1)),
    (2049, 16384, (16384, 14336, 2049, 1)),  # 4 P leaves 8192
    (100, 512, (512, 413, 100, 1)),
    (129, 256, (256, 128, 129, 1)),          # P = N/2 + 1: still one partition
    (130, 256, (256, 129, 128, 2)),          # P = N/2 + 2: partitioned
    (523, 512, (512, 257, 256, 3)),
    (8000, 16384, (16384, 8385, 8000, 1)),
    (8193, 16384, (16384, 8192, 8193, 1)),
    (8194, 16384, (16384, 8193, 8192, 2)),
    (32000, 16384, (16384, 8193, 8192, 4)),
    (100000, 16384, (16384, 8193, 8192, 13)),
]


@pytest.mark.parametrize("P,n_max,want", PLAN_CASES)
def test_plan(engine, P, n_max, want):
    N, Lk, Bp, Q = engine.conv_plan(P, n_max)
    assert (N, Lk, Bp, Q) == want
    assert Lk + Bp - 1 <= N and Q * Bp >= P > (Q - 1) * Bp and 256 <= N <= n_max


@pytest.mark.parametrize("case", cf.CASES, ids=[c[0] for c in cf.CASES])
def test_listed_plans_are_consistent_and_their_tiles_cover_the_output_once(engine, case):
    name, (N, Lk, Bp, Q), P, S_h, rule = case
    assert Q * Bp >= P > (Q - 1) * Bp and Lk + Bp - 1 <= N and N in (1024, 2048, 4096, 8192) and S_h in (0, 1)
    if rule is not None:
        assert engine.conv_plan(*rule) == (N, Lk, Bp, Q) and rule[0] == P
    elif Q == 1:
        assert Bp == P and Lk + P - 1 == N                  # the section exactly full
    else:
        assert Q == 3 and 0 < P - 2 * Bp < Bp and Lk + Bp - 1 == N   # a short last partition
    n = cf.case_len((N, Lk, Bp, Q))
    assert 2 * Lk < n < 3 * Lk                              # the row ends inside the third tile
    x, h = np.ones(n, np.float32), np.ones(P, np.float32)
    for out_len in (n, n + P - 1, Lk - 1, Lk, Lk + 1):
        tiles = cf.apply_tile_bounds(x, h, (N, Lk, Bp, Q), out_len)
        seen = np.zeros(out_len, np.int64)
        for first, cnt, bound in tiles:
            assert 0 <= first and 1 <= cnt <= Lk and first + cnt <= out_len and bound > 0
            seen[first:first + cnt] += 1
        assert np.all(seen == 1)


def test_every_transform_length_has_its_two_listed_plans():
    by_n = {}
    for name, plan, P, S_h, rule in cf.CASES:
        if rule is None:
            by_n.setdefault(plan[0], []).append(plan[3])
    assert by_n == {1024: [1, 3], 2048: [1, 3], 4096: [1, 3], 8192: [1, 3]}
    assert any(c[3] == 0 for c in cf.CASES)                 # per-stream filters somewhere
    assert len(set(c[0] for c in cf.CASES)) == len(cf.CASES)


def test_plan_refusals(engine):
    from distant_speech_recognition_amd import _lib
    for P, n_max in ((0, 16384), (-3, 16384), (10, 100), (10, 384), (10, 32768), (10, 128)):
        with pytest.raises(_lib.BtkError) as e:
            engine.conv_plan(P, n_max)
        assert e.value.code == _lib.BTK_ERR_DIMENSION
    assert _lib.lib().btk_conv_plan(10, 256, None, None, None, None) == _lib.BTK_ERR_PARAMETER


def test_abi_refusals_with_null_pointers():
    """Dimensions are judged before pointers and both before any device call: every refusal is reachable without a device."""
    from distant_speech_recognition_amd import _lib
    lib = _lib.lib()
    null = C.c_void_p(0)
    DIM, PAR = _lib.BTK_ERR_DIMENSION, _lib.BTK_ERR_PARAMETER

    def spectra(R=2, P=157, N=256, Bp=157, Q=1, stride=None):
        return lib.btk_conv_filter_spectra(null, P if stride is None else stride, R, P, N, Bp, Q, null, null)

    def apply(ln=1000, hist=0, S=2, S_h=1, Cn=3, P=157, N=256, Lk=100, Bp=157, Q=1, out_len=1000, xs=None, ys=None):
        return lib.btk_conv_apply(null, ln, hist, ln + hist if xs is None else xs, S, null, S_h, Cn, P, N, Lk, Bp, Q, null, out_len,
                                  out_len if ys is None else ys, null)

    def blocks(ln=1000, S=2, T=3, step=100, S_h=1, Cn=3, P=17, L=256):
        return lib.btk_conv_blocks(null, ln, ln, S, T, step, null, S_h, Cn, P, L, null, null)

    assert spectra() == PAR and apply() == PAR and blocks() == PAR and apply(S_h=2) == PAR and blocks(S_h=2) == PAR
    for N in (128, 300, 32768, 0, -256):                                      # N no power of two from 256 to 16384
        assert spectra(N=N) == DIM and apply(N=N) == DIM and blocks(L=N) == DIM
    assert apply(Lk=101) == DIM and apply(Lk=0) == DIM                        # Lk + Bp - 1 > N
    assert spectra(P=523, N=512, Bp=200, Q=2) == DIM and apply(P=523, N=512, Lk=313, Bp=200, Q=2) == DIM   # Q Bp < P
    assert spectra(P=523, N=512, Bp=200, Q=4) == DIM                          # a partition without taps
    assert spectra(P=0, Bp=1) == DIM and apply(P=0, Bp=1) == DIM and blocks(P=0) == DIM   # P < 1
    assert blocks(P=256) == DIM and blocks(P=300) == DIM                      # P >= L in the block form
    assert apply(S=3, S_h=2) == DIM and blocks(S=3, S_h=2) == DIM and apply(S_h=0) == DIM   # S_h neither 1 nor S
    assert spectra(R=0) == DIM and spectra(stride=100) == DIM
    assert apply(S=0) == DIM and apply(Cn=0) == DIM and apply(out_len=0) == DIM and apply(ln=-1) == DIM and apply(hist=-1) == DIM
    assert apply(ys=999) == DIM and apply(hist=10, xs=1000) == DIM
    assert blocks(T=0) == DIM and blocks(step=0) == DIM and blocks(S=0) == DIM
    assert b"btk_conv_blocks" in lib.btk_last_error()


def _source(L, shift=None):
    from btk20.feature import SampleFeaturePtr
    return SampleFeaturePtr(block_len=L, shift_len=L if shift is None else shift, pad_zeros=True)


def test_node_constructors_and_sizes():
    from btk20.convolution import OverlapAddPtr, OverlapSavePtr
    from distant_speech_recognition_amd.btk20cpp import j_error, jdimension_error
    h = np.arange(1, 158, dtype=np.float64)
    oa = OverlapAddPtr(_source(100), h)
    assert oa.size() == 100 and oa.taps() == 157 and oa.fftLen() == 256 and oa.launches() == 0
    # the plan's tile cut to the block (launches end on tile boundaries) and the shortest transform that holds it: exactly full
    assert oa.plan() == (256, 100, 157, 1)
    assert OverlapAddPtr(_source(2048, 1024), np.ones(2048), fftLen=4096).plan() == (4096, 2048, 2048, 1)
    assert OverlapAddPtr(_source(320), np.ones(100000)).plan() == (16384, 320, 8192, 13)
    assert OverlapAddPtr(_source(10000), np.ones(8000)).plan() == (16384, 5000, 8000, 1)
    assert OverlapAddPtr(_source(100), h, fftLen=256, nm="x").name() == "x"
    assert OverlapAddPtr(_source(100), impulse_response=h, fft_len=512).fftLen() == 512
    for bad in (255, 128, 300):                             # too short (convolution.cc:75-77); long enough but no power of two
        with pytest.raises(jdimension_error):
            OverlapAddPtr(_source(100), h, fftLen=bad)
    with pytest.raises(j_error):
        OverlapAddPtr(_source(100), np.zeros(0))
    os_ = OverlapSavePtr(_source(256), np.ones(17))
    assert os_.size() == 239 and os_.taps() == 17 and os_.plan() == (256, 240, 17, 1) and os_.launches() == 0
    assert OverlapSavePtr(_source(256), impulseResponse=np.ones(255), nm="y").size() == 1
    for L, P in ((256, 256), (256, 300), (100, 17), (320, 17), (128, 17), (32768, 17)):   # P >= L (:180-181); L the device cannot run
        with pytest.raises(jdimension_error):
            OverlapSavePtr(_source(L), np.ones(P))
    # block service knobs
    assert oa.block_frames() == 64
    oa.set_block_frames(7)
    assert oa.block_frames() == 7
    assert OverlapAddPtr(_source(100), h, block_frames=3).block_frames() == 3


def test_modules_and_keywords():
    import btk20
    import btk20.convolution as conv
    import distant_speech_recognition_amd.btk20.convolution as conv2
    from distant_speech_recognition_amd.btk20cpp import _signatures as S, _signatures_alt as A
    assert conv is conv2 and btk20.convolution is conv
    assert sorted(conv.__all__) == ["OverlapAdd", "OverlapAddPtr", "OverlapSave", "OverlapSavePtr"]
    assert [p for p, _ in S.CTORS["OverlapAddPtr"]] == ["samp", "impulseResponse", "fftLen", "nm"]
    assert [p for p, _ in S.CTORS["OverlapSavePtr"]] == ["samp", "impulseResponse", "nm"]
    assert [p for p, _ in A.CTOR_KWARGS["OverlapAddPtr"]] == ["samp", "impulse_response", "fft_len", "nm"]
    # the legacy spellings unit_test/correlate.py uses for its sample source
    s = btk20.SampleFeaturePtr(blockLen=2048, shiftLen=1024, padZeros=True)
    assert s.size() == 2048
