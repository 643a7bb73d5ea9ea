"""GPU: the synthesis bank beyond r = 1 against the float64 closed form of tests/closed_forms.py -- r = 0 and r = 2 (the ring kernels,
the only form R = 4 has), delay compensation 0 and 1, and the generic kernel of fb_kernels.hip (M = 64 / 128, m = 2 / 3, and M = 2048
r = 2 with its one-frame-per-round fall-back).  test_gpu_fused_closed_form.py::test_synthesis_against_closed_form holds r = 1, dct = 2.

Scheme as there: the dense g, random complex64 Y x 1000 in bins 0 .. M/2 (the closed form gets the Hermitian extension), contiguous rows
and rows an odd number of frames apart, whole runs and [b0, b0 + bcount) pieces with b0 + pd even and odd.  The output goes into a
buffer of the test's own between two guard bands of 4096 bytes, which must keep their fill.

Bound: closed_forms.accept, FACTOR = 4 and FLOOR = 2^-22 unchanged; the yardstick is cf.synthesis_f32 on the same Y.

Kernel / yardstick ratio per case (worst stream, row spacing and piece), MI355X:

    case                                            dense
    synthesis 512 m4 r0 dct0 T=8                     1.70
    synthesis 512 m4 r0 dct0 T=23                    2.40
    synthesis 512 m4 r0 dct0 T=24                    2.05
    synthesis 512 m4 r0 dct0 T=300                   2.11
    synthesis 512 m4 r0 dct2 T=3                     1.85
    synthesis 512 m4 r0 dct2 T=18                    2.44
    synthesis 512 m4 r0 dct2 T=19                    1.53
    synthesis 512 m4 r0 dct2 T=300                   1.59
    synthesis 512 m4 r2 dct1 T=16                    1.94
    synthesis 512 m4 r2 dct1 T=31                    1.96
    synthesis 512 m4 r2 dct1 T=32                    2.14
    synthesis 512 m4 r2 dct1 T=300                   2.00
    synthesis 512 m4 r2 dct2 T=9                     1.89
    synthesis 512 m4 r2 dct2 T=24                    1.78
    synthesis 512 m4 r2 dct2 T=25                    2.75
    synthesis 512 m4 r2 dct2 T=300                   1.82
    synthesis 256 m4 r0 dct1 T=4                     1.76
    synthesis 256 m4 r0 dct1 T=19                    2.46
    synthesis 256 m4 r0 dct1 T=20                    1.85
    synthesis 256 m4 r0 dct1 T=300                   2.50
    synthesis 256 m4 r2 dct2 T=9                     2.12
    synthesis 256 m4 r2 dct2 T=24                    1.65
    synthesis 256 m4 r2 dct2 T=25                    1.51
    synthesis 256 m4 r2 dct2 T=300                   1.56
    synthesis 1024 m4 r0 dct2 T=3                    1.51
    synthesis 1024 m4 r0 dct2 T=18                   1.86
    synthesis 1024 m4 r0 dct2 T=19                   1.62
    synthesis 1024 m4 r0 dct2 T=300                  2.10
    synthesis 1024 m4 r2 dct0 T=8                    1.87
    synthesis 1024 m4 r2 dct0 T=23                   2.12
    synthesis 1024 m4 r2 dct0 T=24                   1.81
    synthesis 1024 m4 r2 dct0 T=300                  1.71
    synthesis 2048 m4 r0 dct0 T=8                    2.31
    synthesis 2048 m4 r0 dct0 T=23                   1.57
    synthesis 2048 m4 r0 dct0 T=24                   1.86
    synthesis 2048 m4 r0 dct0 T=300                  2.08
    synthesis 2048 m4 r2 dct2 T=9                    1.76
    synthesis 2048 m4 r2 dct2 T=24                   1.88
    synthesis 2048 m4 r2 dct2 T=25                   1.83
    synthesis 2048 m4 r2 dct2 T=150                  2.03
    synthesis 2048 m2 r2 dct1 T=8                    2.36
    synthesis 2048 m2 r2 dct1 T=23                   1.62
    synthesis 2048 m2 r2 dct1 T=24                   1.86
    synthesis 2048 m2 r2 dct1 T=150                  2.03
    synthesis 64 m4 r1 dct1 T=8                      1.57
    synthesis 64 m4 r1 dct1 T=23                     1.76
    synthesis 64 m4 r1 dct1 T=24                     2.49
    synthesis 64 m4 r1 dct1 T=300                    1.63
    synthesis 128 m2 r2 dct0 T=4                     1.72
    synthesis 128 m2 r2 dct0 T=19                    2.04
    synthesis 128 m2 r2 dct0 T=20                    1.55
    synthesis 128 m2 r2 dct0 T=300                   1.77
    synthesis 512 m3 r1 dct2 T=4                     1.99
    synthesis 512 m3 r1 dct2 T=19                    2.57
    synthesis 512 m3 r1 dct2 T=20                    1.68
    synthesis 512 m3 r1 dct2 T=300                   1.94

The helpers below (prototypes, plans, the guarded buffer, the case lists of the switch children) are shared with
test_gpu_analysis_closed_form.py.
"""
import numpy as np
import pytest

from tests import closed_forms as cf
from tests.util import design_prototype

pytestmark = pytest.mark.gpu

DCT = 2
GUARD = 4096                                                   # bytes of guard band on either side of a guarded buffer
_FB, _PROTO = {}, {}


def _proto(M, mm, name, kind="h"):
    key = (M, mm, name, kind)
    if key not in _PROTO:
        _PROTO[key] = cf.dense_prototype(M, mm, seed=kind == "g") if name == "dense" else design_prototype(M, mm, kind)
    return _PROTO[key]


def _bank(M, mm, r, name, dct=DCT, synthesis=False):
    from distant_speech_recognition_amd import engine as eng
    key = (M, mm, r, name, dct, synthesis)
    if key not in _FB:
        _FB[key] = eng.FilterBank(_proto(M, mm, name, "g" if synthesis else "h"), M, mm, r, dct, synthesis=synthesis)
    return _FB[key]


def _same_bits(a, b):
    import torch
    a, b = (torch.view_as_real(t.contiguous()) if t.is_complex() else t.contiguous() for t in (a, b))
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _guarded(dev, shape, dtype, row=None):
    """A tensor of `shape` -- the [..., :shape[-1]] view of rows `row` elements apart when row is given -- in a buffer of its own with
    GUARD bytes before and after it, everything filled with a sentinel.  -> (view, check); check() asserts that every element outside
    the view (padding columns and both guard bands) still holds the sentinel."""
    import torch
    row = shape[-1] if row is None else row
    assert row >= shape[-1]
    g = GUARD // torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape[:-1])) * row
    sentinel = complex(-7777.25, 4321.5) if dtype.is_complex else -7777.25
    flat = torch.full((g + n + g,), sentinel, dtype=dtype, device=dev)
    inner = lambda t: t[g:g + n].view(*shape[:-1], row)[..., :shape[-1]]
    view = inner(flat)
    assert view.data_ptr() % 16 == 0
    before = flat.clone()

    def check():
        after = flat.clone()
        inner(after)[...] = sentinel
        assert torch.equal(after, before), "written outside the output: %d elements" % int((after != before).sum())
    return view, check


# ---- synthesis cases (also run by the switch children of test_gpu_analysis_closed_form.py) --------------------------------
SYN_GEOMS = [(512, 4, 0, 0), (512, 4, 0, 2), (512, 4, 2, 1), (512, 4, 2, 2), (256, 4, 0, 1), (256, 4, 2, 2), (1024, 4, 0, 2), (1024, 4, 2, 0),
             (2048, 4, 0, 0), (2048, 4, 2, 2), (2048, 2, 2, 1), (64, 4, 1, 1), (128, 2, 2, 0), (512, 3, 1, 2)]            # M, m, r, dct
S = 2


def _syn_frames(M, mm, r, dct):
    """Workgroup runs are 16 blocks long at this S: 300 frames prime the frame ring many times (150 at M = 2048, r = 2: one frame per round)."""
    pd = cf.fb_delays(mm, r, True, dct)[0]
    return [pd + 1, pd + 16, pd + 17, 150 if (M, r) == (2048, 2) else 300]


def _syn_input(M, mm, r, dct, T):
    rng = np.random.default_rng(100003 * M + 1009 * mm + 101 * r + 11 * dct + T)
    K = M // 2 + 1
    return ((rng.normal(size=(S, K, T)) + 1j * rng.normal(size=(S, K, T))) * 1000.0).astype(np.complex64)


def _syn_refs(M, mm, r, dct, Yn):
    g, D = _proto(M, mm, "dense", "g"), M >> r
    B = Yn.shape[2] - cf.fb_delays(mm, r, True, dct)[0]
    refs = []
    for s in range(S):
        full = cf.hermitian(Yn[s], M)
        refs.append((cf.synthesis_cf(g, M, mm, r, dct, full).reshape(B, D), cf.synthesis_f32(g, M, mm, r, dct, full).reshape(B, D)))
    return refs


def _syn_pieces(B, reduced=False):
    want = ((1, 20),) if reduced else ((1, 20), (2, 21), (B - 1, 1))
    return sorted({(0, B)} | {(b0, min(c, B - b0)) for b0, c in want if B - b0 >= 1})


def _syn_device_inputs(dev, Yn):
    """Y contiguous, and in rows an odd number of frames apart."""
    import torch
    T = Yn.shape[2]
    Yc = torch.from_numpy(Yn).to(dev)
    Yp = torch.empty(Yn.shape[:2] + (T + 2 + (T % 2 == 0),), dtype=torch.complex64, device=dev)[..., :T]
    Yp.copy_(Yc)
    assert Yp.stride(1) % 2 == 1
    return (("contiguous", Yc), ("odd stride", Yp))


def _syn_launches(dev, M, mm, r, dct, T, reduced=False):
    """Every launch of one (geometry, T): yields (label, b0, bcount, out [S][bcount D] numpy); the guard bands are checked here."""
    import torch
    sfb = _bank(M, mm, r, "dense", dct, synthesis=True)
    pd, D = cf.fb_delays(mm, r, True, dct)[0], M >> r
    assert sfb.processing_delay == pd and sfb.num_blocks(T) == T - pd
    for kind, Yd in _syn_device_inputs(dev, _syn_input(M, mm, r, dct, T)):
        for b0, c in _syn_pieces(T - pd, reduced):
            out, check = _guarded(dev, (S, c * D), torch.float32)
            sfb.synthesize(Yd, b0=b0, bcount=c, out=out)
            host = out.cpu().numpy()
            check()
            yield "%s b0=%d bc=%d" % (kind, b0, c), b0, c, host


def _syn_tag(M, mm, r, dct, T):
    return "synthesis %d m%d r%d dct%d T=%d" % (M, mm, r, dct, T)


def _syn_judge(tag, M, mm, r, dct, T, launches):
    refs = _syn_refs(M, mm, r, dct, _syn_input(M, mm, r, dct, T))
    D, worst, seen = M >> r, None, 0
    for label, b0, c, out in launches:
        assert out.shape == (S, c * D)
        for s in range(S):
            fig = cf.judge("%s %s s=%d" % (tag, label, s), out[s].reshape(c, D), refs[s][1][b0:b0 + c], refs[s][0][b0:b0 + c], show=False)
            worst = fig if worst is None or fig["ratio"] > worst["ratio"] else worst
            seen += 1
    assert seen >= 2 * S
    print(cf.cfratio_line(tag, worst))


@pytest.mark.parametrize("M,mm,r,dct", SYN_GEOMS)
def test_synthesis_geometries_against_closed_form(dev, M, mm, r, dct):
    for T in _syn_frames(M, mm, r, dct):
        _syn_judge(_syn_tag(M, mm, r, dct, T), M, mm, r, dct, T, _syn_launches(dev, M, mm, r, dct, T))


# the reduced list of the switch children: the geometries whose kernel a switch changes (BTK_DISABLE_SYNTHESIS512, BTK_DISABLE_FAST,
# BTK_SYN_NARROW: the narrow forms exist for r <= 1), two frame counts, two pieces
SYN_SWITCH_GEOMS = [(512, 4, 0, 2), (512, 4, 1, 2), (512, 4, 2, 1), (256, 4, 2, 2), (1024, 4, 0, 2), (1024, 4, 1, 2), (1024, 4, 2, 0)]


def _syn_switch_frames(M, mm, r, dct):
    return [cf.fb_delays(mm, r, True, dct)[0] + 17, 100]
