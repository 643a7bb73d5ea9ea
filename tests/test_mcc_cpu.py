"""CPU: the closed form of the MCC localiser (tests/mcc_closed_form.py) against known answers, and the host side of the C-ABI
(btk_mcc_max_sample_delay, btk_mcc_sample_delays, btk_mcc_linear_grid, the refusals of the device entry points) against it.

The grid walk is float32 arithmetic through sinf / asinf.  The restatement takes them correctly rounded (the float64 function
rounded once); the C library's may differ from that by a unit in the last place, so the angles are pinned to 4 float32 ulp and
not to bits, and a tau row is pinned only where fs d lies further than 1e-3 from an integer (the truncation cannot flip there).
Under numpy's own float32 sin / arcsin the restatement gives the same 23, 13, 15 and 120 grid points with D = 10, 5, 6 and 58
for the four geometries below at 16 kHz (pinned too), but its angles are no yardstick: numpy's float32 sine is a few units less
exact, the walk feeds sin(asin(.)) back into itself and asin near 1 magnifies the loss.  Measured on the build machine against
the library: at most 1 ulp for the first three geometries, 44 ulp at the last step below pi/2 of 63 x 20 mm -- where the
library lies within 1 ulp of the correctly rounded walk."""
import ctypes as C

import numpy as np
import pytest

from tests import mcc_closed_form as cf

KINECT_MM = [-113.0, 36.0, 76.0, 113.0]
GEOMETRIES = [  # (N, spacing, positions, grid points, D)
    (4, None, KINECT_MM, 23, 10),
    (4, 40.0, None, 13, 5),
    (8, 20.0, None, 15, 6),
    (64, 20.0, None, 120, 58),
]


@pytest.fixture(scope="module")
def eng():
    from distant_speech_recognition_amd import engine
    return engine


@pytest.fixture(scope="module")
def lib():
    from distant_speech_recognition_amd import _lib
    return _lib


def test_two_channels_give_log_one_minus_rho_squared():
    rng = np.random.default_rng(1)
    for D, L, tau in ((0, 64, (0, 0)), (5, 300, (0, -5)), (7, 257, (3, 7)), (10, 20, (-10, 10))):
        x = cf.synthetic(rng, 2, L, [0, 2], noise_db=-3.0)
        xt = cf.shifted(x, tau, D)
        rho = float(xt[0] @ xt[1]) / np.sqrt(float(xt[0] @ xt[0]) * float(xt[1] @ xt[1]))
        cost, flag = cf.cost_of(cf.corr_matrix(x, tau, D))
        assert not flag and abs(cost - np.log1p(-rho * rho)) <= 1e-12 * max(1.0, abs(cost)), (D, L, tau)
        raw, _ = cf.cost_of(cf.corr_matrix(x, tau, D), normalize=False)
        assert abs(raw - cost - np.log(float(xt[0] @ xt[0]) / xt.shape[1]) - np.log(float(xt[1] @ xt[1]) / xt.shape[1])) <= 1e-9


def test_window_wraps_into_the_blocks_own_tail():
    L, D = 12, 3
    x = np.arange(2 * L, dtype=np.float32).reshape(2, L)
    xt = cf.shifted(x, [-3, 3], D)
    assert xt.shape == (2, L - D)
    assert list(xt[0]) == [9, 10, 11, 0, 1, 2, 3, 4, 5]           # f + tau < 0 reads x[L + f + tau]
    assert list(xt[1]) == [L + 3 + f for f in range(L - D)]       # the last sample read is L - 1
    with pytest.raises(AssertionError):
        cf.shifted(x, [-4, 0], D)


def test_minimum_sits_at_the_true_delay_row():
    rng = np.random.default_rng(2)
    N, L, D = 4, 1024, 6
    true = np.array([0, -2, -4, -6])
    x = cf.synthetic(rng, N, 3 * L, true)
    taus = np.array([[0, -k, -2 * k, -3 * k] for k in range(-2, 3)])
    cost, flag = cf.costs(x, taus, L, D)
    assert not flag.any() and np.all(np.argmin(cost, axis=1) == 4)
    assert np.all(np.sort(cost, axis=1)[:, 1] - cost[:, 4] > 0.99)
    assert np.all(cost <= 1e-9)                                   # Hadamard: det R <= prod R_ii


def test_nbest_insertion_keeps_grid_order_among_equals():
    c, i = cf.nbest([3.0, 1.0, 1.0, 2.0, 1.0], 3)
    assert list(i) == [1, 2, 4] and list(c) == [1.0, 1.0, 1.0]
    c, i = cf.nbest([3.0, 1.0], 4)
    assert list(i) == [1, 0, -1, -1] and list(c) == [1.0, 3.0, cf.RESET_COST, cf.RESET_COST]
    c, i = cf.nbest([cf.RESET_COST, 200000.0], 1)
    assert list(i) == [-1]                                        # strict <: the reset value itself is not inserted


def test_sample_delays_truncate_toward_zero_through_float32(eng):
    fs = 16000
    d = np.array([0.0, 1.0 / fs, -1.0 / fs, 2.9999 / fs, -2.9999 / fs, 0.49 / fs, -0.49 / fs, -57.99 / fs, 58.0 / fs,
                  2.99999999 / fs, -2.99999999 / fs])          # the last two are 3 and -3 once rounded to float32
    want = cf.sample_delays(fs, d)
    assert list(want) == [0, 1, -1, 2, -2, 0, 0, -57, 58, 3, -3]
    assert np.array_equal(eng.mcc_sample_delays(fs, d), want)
    assert eng.mcc_sample_delays(fs, d.reshape(1, -1)).shape == (1, d.size)
    assert eng.mcc_max_sample_delay(16000, np.float32(226.0 / cf.SSPEED)) == 10
    assert eng.mcc_max_sample_delay(16000, 0.0) == 0


@pytest.mark.parametrize("N,spacing,positions,points,D", GEOMETRIES)
def test_linear_grid_follows_the_float32_walk(eng, N, spacing, positions, points, D):
    fs = 16000
    want = cf.linear_grid(fs, N, spacing, positions)
    assert len(want["azimuths"]) == points and want["D"] == D
    loose = cf.linear_grid(fs, N, spacing, positions, numpy_f32=True)
    assert len(loose["azimuths"]) == points and loose["D"] == D
    got = eng.mcc_linear_grid(fs, N, spacing=spacing, positions=positions)
    assert len(got["azimuths"]) == points and got["D"] == D
    assert np.float32(got["const_v"]) == want["const_v"] and np.float32(got["max_time_delay"]) == want["max_time_delay"]
    az = got["azimuths"].astype(np.float32)
    assert np.array_equal(az.astype(np.float64), got["azimuths"])              # float32 values
    ulp = np.spacing(np.maximum(np.abs(want["azimuths"]), np.float32(1e-30)))
    worst = float(np.max(np.abs(az.astype(np.float64) - want["azimuths"].astype(np.float64)) / ulp))
    drift = float(np.max(np.abs(az.astype(np.float64) - loose["azimuths"].astype(np.float64)) / ulp))
    print("N=%d: %d points, D=%d, largest azimuth difference %.1f float32 ulp (%.1f from the walk on numpy's float32 sin / arcsin)"
          % (N, points, D, worst, drift))
    assert worst <= 4.0
    assert az[0] == 0.0 and np.all(np.diff(az) > 0) and az[-1] < 2 * np.pi
    assert np.max(np.abs(got["delays"] - want["delays"])) <= 8 * 2.0 ** -24 * want["max_time_delay"]
    safe = np.abs(want["prod"] - np.rint(want["prod"])) > 1e-3
    assert safe.mean() > 0.5 and np.array_equal(got["tau"][safe], want["tau"][safe])
    assert np.array_equal(got["tau"], eng.mcc_sample_delays(fs, got["delays"]))
    assert np.max(np.abs(got["tau"])) <= D and np.all(got["tau"][:, 0] == 0)


def test_linear_grid_refusals(eng, lib):
    with pytest.raises(lib.BtkError) as e:
        eng.mcc_linear_grid(16000, 1, spacing=20.0)
    assert e.value.code == lib.BTK_ERR_DIMENSION
    with pytest.raises(lib.BtkError):
        eng.mcc_linear_grid(16000, 4, spacing=0.0)
    with pytest.raises(lib.BtkError):
        eng.mcc_linear_grid(16000, 4, positions=[0.0, 1.0, 2.0])                 # three positions for four microphones
    n = C.c_int(0)
    az = np.zeros(5)
    rc = lib.lib().btk_mcc_linear_grid(16000, 4, None, 40.0, 5, C.byref(n), None, None, az.ctypes.data_as(C.c_void_p), None, None)
    assert rc == lib.BTK_ERR_DIMENSION and b"max_points" in lib.lib().btk_last_error()


def _cost_rc(lib, N, L, D, tau, S=1, B=1, G=None):
    tau = np.ascontiguousarray(tau, np.int32).reshape(-1, N) if N > 0 else np.zeros((1, 1), np.int32)
    G = tau.shape[0] if G is None else G
    return lib.lib().btk_mcc_cost(None, B * L, S, N, B, L, D, tau.ctypes.data_as(C.c_void_p), None, G, 1, None, None, None)


def test_refusals_come_before_any_launch(lib):
    """Every limit is refused with BTK_ERR_DIMENSION on a machine without a device, all device pointers null: nothing is
    launched.  Sizes within the limits then reach the null-pointer check (BTK_ERR_PARAMETER)."""
    DIM, PAR = lib.BTK_ERR_DIMENSION, lib.BTK_ERR_PARAMETER
    assert _cost_rc(lib, 1, 64, 4, np.zeros((1, 1))) == DIM
    assert _cost_rc(lib, 65, 64, 4, np.zeros((1, 65))) == DIM
    assert _cost_rc(lib, 2, 7, 4, np.zeros((1, 2))) == DIM                       # L = 2 D - 1
    assert b"insufficient" in lib.lib().btk_last_error()
    assert _cost_rc(lib, 2, 8, 4, np.zeros((1, 2))) == PAR                       # L = 2 D passes the size checks
    assert _cost_rc(lib, 2, 65537, 4, np.zeros((1, 2))) == DIM
    assert _cost_rc(lib, 2, 64, 4, [[0, 5]]) == DIM and _cost_rc(lib, 2, 64, 4, [[-5, 0]]) == DIM     # |tau| = D + 1
    assert _cost_rc(lib, 2, 64, 4, [[4, -4]]) == PAR
    assert _cost_rc(lib, 2, 64, 4, np.zeros((1, 2)), G=0) == DIM
    assert _cost_rc(lib, 2, 64, 4, np.zeros((1, 2)), G=4097) == DIM
    assert _cost_rc(lib, 64, 64, 4, np.zeros((4096, 64))) == PAR
    L = lib.lib()
    assert L.btk_mcc_select(None, 1, 4, 17, None, None, None) == DIM             # maxSource = 17
    assert L.btk_mcc_select(None, 1, 4, 0, None, None, None) == DIM
    assert L.btk_mcc_select(None, 1, 4, 16, None, None, None) == PAR
    tau = np.zeros((1, 2), np.int32)
    pairs = np.array([[0, 1]], np.int32)                                        # candidate 1 of 1
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.btk_mcc_matrices(None, 64, 1, 2, 1, 64, 4, p(tau), None, 1, p(pairs), None, 1, None, None) == DIM
    pairs[0, 1] = 0
    assert L.btk_mcc_matrices(None, 64, 1, 2, 1, 64, 4, p(tau), None, 1, p(pairs), None, 1, None, None) == PAR
    assert L.btk_mcc_matrices(None, 64, 1, 1, 1, 64, 4, p(tau), None, 1, p(pairs), None, 1, None, None) == DIM
