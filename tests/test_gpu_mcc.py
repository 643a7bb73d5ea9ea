"""GPU: the MCC kernels (csrc/mcc_kernels.hip through engine.mcc_costs / mcc_select / mcc_matrices / mcc_localize) against the
closed form of tests/mcc_closed_form.py on the same float32 blocks.

Inputs: a smoothed common source with per-channel integer delays plus independent noise 10 dB below it, rounded to integers at
PCM scale (cf.synthetic).  The closed form's condition number kappa(R) stays below 1000 on the shapes of this file (printed).

Shapes.  The kernel takes four samples per matrix instruction, issues the loads of four such steps together (16 samples) and
deals the steps over four wavefronts (a quarter each): the window nS = L - D is chosen below one step (3), below two (7), at
L = 2 D exactly (nS = D), one more than a multiple of 64 = 4 x 16 (a wavefront's last batch holds one live sample), and 4038
(L = 4096, D = 58, N = 64); always nS > N, so that R is not singular by construction.  N in {2, 3, 8, 17, 33, 48, 64} covers one to four 16-channel tiles with full and ragged last tiles.  One work unit is
one workgroup -- the kernel forms no groups of candidates -- so G = 1, 2 and 5 and S x B = 1 x 1 and 2 x 5 cover the indexing.
Integer samples below 2^15 make every partial sum exact, so R differs from the closed form by the scaling alone (error 0 in the
printed lines); n8_fraction divides the samples by three, which makes the additions round.
Every case holds a tau row that reaches -D on one channel (the wrap reads the block's tail) and +D on another (the last sample
read is L - 1).

Bounds, u = 2^-53, A_ij = (1 / nS) sum_f |xt_i xt_j|:
  R     |dR_ij| <= (nS + 2) u A_ij: nS - 1 additions and the scaling, each one rounding of a partial sum no larger than nS A_ij
        (the products of two float32 are exact in float64), one more for the closed form's own scaling.
  cost  first-order perturbation of log det R - sum log R_ii under that dR, with the closed form's own inverse:
        sum_ij |Rinv_ij| (nS + 2) u A_ij + sum_i dR_ii / R_ii, plus the factorisation's backward error N (N + 1) u kappa(R).
Largest error / bound measured on an MI355X (each case prints its own; DESIGN 3.26 has the table): R 0.0096 (n8_fraction; 0 on
integer samples), cost 0.42 with and 0.51 without the variances (n3_seven_samples: seven samples, where the logarithms'
own rounding is as large as the factorisation's); from N = 8 upwards at most 0.011."""
import numpy as np
import pytest

from tests import mcc_closed_form as cf

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# name: (N, L, D, S, B, G)
CASES = {
    "n2_L2D": (2, 10, 5, 1, 1, 1),
    "n2_three_samples": (2, 3, 0, 1, 1, 2),
    "n3_seven_samples": (3, 13, 6, 2, 5, 2),
    "n3_tail": (3, 6 + 64 * 3 + 1, 6, 2, 5, 5),
    "n8_grid": (8, 6 + 64 * 8 + 1, 6, 2, 5, 0),          # G = 0: the 15 rows of the 7 x 20 mm grid (rows repeat)
    "n8_fraction": (8, 6 + 64 * 8 + 1, 6, 1, 2, 3),
    "n17_L2D": (17, 80, 40, 1, 1, 2),
    "n33_tail": (33, 20 + 64 * 4 + 1, 20, 1, 1, 5),
    "n33_L2D": (33, 160, 80, 1, 1, 1),
    "n48": (48, 500, 30, 1, 1, 2),
    "n64": (64, 4096, 58, 1, 2, 5),
}
worst = {"R": 0.0, "cost": 0.0}


@pytest.fixture(scope="module")
def eng(dev):
    from distant_speech_recognition_amd import engine
    return engine


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def _taus(rng, N, D, G):
    """G rows: the true delays (a ramp), a row that reaches -D on channel 1 and +D on the last channel, random rows within +-D."""
    true = -np.round(np.linspace(0, D, N)).astype(np.int64)
    edge = rng.integers(-D, D + 1, N)
    edge[0], edge[1], edge[-1] = 0, -D, D
    if N == 2:
        edge = np.array([-D, D])
    rows = [edge, true] + [rng.integers(-D, D + 1, N) for _ in range(max(G - 2, 0))]
    return np.array(rows[:G], np.int64), true


_made = {}


def make(name):
    """(x float32 [S][N][B L], taus, closed-form cost [S][B][G], flag, true row) of a case, computed once."""
    if name not in _made:
        N, L, D, S, B, G = CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        if G == 0:
            taus = cf.linear_grid(16000, N, 20.0)["tau"]
            true = taus[0]                               # broadside: the row the grid holds three times (points 0, 1, 14)
        else:
            taus, true = _taus(rng, N, D, G)
        x = np.stack([cf.synthetic(rng, N, B * L + min(3, L - 1), true) for _ in range(S)])
        if name.endswith("fraction"):                    # samples that are no integers: the sums round
            x = (x * np.float32(1.0 / 3.0)).astype(np.float32)
        want = [cf.costs(x[s], taus, L, D) for s in range(S)]
        _made[name] = (x, taus, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), true)
    return _made[name]


def cost_bound(R, A, nS, normalize=True):
    N = len(R)
    dR = (nS + 2) * U * A
    lam = np.linalg.eigvalsh(R)
    kappa = float(lam[-1] / lam[0])
    pert = float(np.sum(np.abs(np.linalg.inv(R)) * dR))
    if normalize:
        pert += float(np.sum(np.diag(dR) / np.diag(R)))
    return pert + N * (N + 1) * U * kappa, kappa


@pytest.mark.parametrize("name", list(CASES))
def test_matrices_and_costs_meet_their_bounds(eng, torch_, dev, name):
    N, L, D, S, B, _ = CASES[name]
    x, taus, want, wflag, _ = make(name)
    G, nS = len(taus), L - D
    xd = torch_.from_numpy(x).to(dev)
    cost, flag = eng.mcc_costs(xd, taus, L, D)
    raw, rflag = eng.mcc_costs(xd, taus, L, D, normalize_variance=False)
    pairs = np.array([[sb, g] for sb in range(S * B) for g in range(G)])
    R = eng.mcc_matrices(xd, taus, L, D, pairs).cpu().numpy().reshape(S, B, G, N, N)
    cost, flag, raw, rflag = cost.cpu().numpy(), flag.cpu().numpy(), raw.cpu().numpy(), rflag.cpu().numpy()
    assert cost.shape == (S, B, G) and flag.shape == (S, B, G) and flag.dtype == np.uint8
    rR = rC = rW = kmax = 0.0
    for s in range(S):
        for b in range(B):
            blk = x[s, :, b * L:(b + 1) * L]
            for g in range(G):
                Rw, A = cf.corr_matrix(blk, taus[g], D), cf.abs_sum_matrix(blk, taus[g], D)
                assert np.array_equal(R[s, b, g], R[s, b, g].T)
                err = np.abs(R[s, b, g] - Rw)
                bound = (nS + 2) * U * A
                assert np.all(err <= bound), (name, s, b, g, float(np.max(err - bound)))
                rR = max(rR, float(np.max(err / np.maximum(bound, 1e-300))))
                if wflag[s, b, g]:
                    assert flag[s, b, g] == 1 and cost[s, b, g] == 0.0
                    continue
                assert flag[s, b, g] == 0 and rflag[s, b, g] == 0
                cb, kappa = cost_bound(Rw, A, nS)
                kmax = max(kmax, kappa)
                e = abs(cost[s, b, g] - want[s, b, g])
                assert e <= cb, (name, s, b, g, e, cb)
                rC = max(rC, e / cb)
                wr, _ = cf.cost_of(Rw, normalize=False)
                cbr, _ = cost_bound(Rw, A, nS, normalize=False)
                er = abs(raw[s, b, g] - wr)
                assert er <= cbr, (name, s, b, g, er, cbr)
                rW = max(rW, er / cbr)
    worst["R"], worst["cost"] = max(worst["R"], rR), max(worst["cost"], rC, rW)
    print("%s: N=%d L=%d D=%d SxB=%dx%d G=%d  error/bound: R %.3g, cost %.3g, cost without variances %.3g;  kappa <= %.1f"
          % (name, N, L, D, S, B, G, rR, rC, rW, kmax))


def test_equal_rows_blocks_and_candidates_give_equal_bits(eng, torch_, dev):
    name = "n8_grid"
    N, L, D, S, B, _ = CASES[name]
    x, taus, _, _, _ = make(name)
    taus = np.concatenate([taus, taus[5:6], taus[:1]])      # two more copies, far from their originals in the grid
    G = len(taus)
    xd = torch_.from_numpy(x).to(dev)
    cost = eng.mcc_costs(xd, taus, L, D)[0].cpu().numpy()
    again = eng.mcc_costs(xd, taus, L, D)[0].cpu().numpy()
    assert np.array_equal(cost, again)                       # two runs, the same bits
    rows = {}
    for g in range(G):
        rows.setdefault(tuple(taus[g]), []).append(g)
    assert max(len(v) for v in rows.values()) >= 3            # the float32 truncation maps several grid points to one row
    for gs in rows.values():
        for g in gs[1:]:
            assert np.array_equal(cost[:, :, g], cost[:, :, gs[0]]), (gs[0], g)
    for s, b in ((0, 0), (0, 3), (1, 4)):                    # a block launched alone
        alone = eng.mcc_costs(xd[s:s + 1, :, b * L:(b + 1) * L].contiguous(), taus, L, D)[0].cpu().numpy()
        assert alone.shape == (1, 1, G) and np.array_equal(alone[0, 0], cost[s, b])
    for g in (0, 7, G - 1):                                  # a candidate launched alone
        alone = eng.mcc_costs(xd, taus[g:g + 1], L, D)[0].cpu().numpy()
        assert np.array_equal(alone[:, :, 0], cost[:, :, g])
    one = eng.mcc_costs(xd[1], taus, L, D)[0].cpu().numpy()  # [N][samples] is one stream
    assert np.array_equal(one[0], cost[1])


@pytest.mark.parametrize("name", ["n8_grid", "n3_tail", "n64"])
def test_selection(eng, torch_, dev, name):
    N, L, D, S, B, _ = CASES[name]
    x, taus, want, _, true = make(name)
    G, nS = len(taus), L - D
    xd = torch_.from_numpy(x).to(dev)
    for nbest in (1, 3, 16):
        out = eng.mcc_localize(xd, taus, L, D, nbest=nbest)
        cost = out["cost"].cpu().numpy()
        nc, ni = out["nbest_cost"].cpu().numpy(), out["nbest_idx"].cpu().numpy()
        assert nc.shape == (S, B, nbest) and ni.dtype == np.int32
        for s in range(S):
            for b in range(B):
                wc, wi = cf.nbest(cost[s, b], nbest)          # the closed form's insertion on the GPU's own costs: exact
                assert np.array_equal(ni[s, b], wi) and np.array_equal(nc[s, b], wc), (nbest, s, b)
        if nbest > G:
            assert np.all(ni[..., G:] == -1) and np.all(nc[..., G:] == cf.RESET_COST)
    # against the closed form's costs: the best index, wherever the runner-up with another tau row is further than twice the bound
    ni = eng.mcc_localize(xd, taus, L, D, nbest=1)["nbest_idx"].cpu().numpy()
    left_out = 0
    for s in range(S):
        for b in range(B):
            blk = x[s, :, b * L:(b + 1) * L]
            w = int(cf.nbest(want[s, b], 1)[1][0])
            others = [g for g in range(G) if tuple(taus[g]) != tuple(taus[w])]
            bound = max(cost_bound(cf.corr_matrix(blk, taus[g], D), cf.abs_sum_matrix(blk, taus[g], D), nS)[0] for g in range(G))
            gap = min(want[s, b, g] for g in others) - want[s, b, w] if others else np.inf
            if gap > 2 * bound:
                assert ni[s, b, 0] == w, (s, b, gap)
            else:
                left_out += 1
            assert tuple(taus[w]) == tuple(true)
    assert left_out <= 0.05 * S * B


def test_duplicated_rows_fill_consecutive_slots(eng, torch_, dev):
    name = "n8_grid"
    N, L, D, S, B, _ = CASES[name]
    x, taus, _, _, true = make(name)
    xd = torch_.from_numpy(x).to(dev)
    ni = eng.mcc_localize(xd, taus, L, D, nbest=3)["nbest_idx"].cpu().numpy()
    same = [g for g in range(len(taus)) if tuple(taus[g]) == tuple(true)]
    assert len(same) >= 2
    k = min(len(same), 3)
    assert np.all(ni[:, :, :k] == np.array(same[:k]))         # the same row in several slots, in grid order


@pytest.mark.parametrize("normalize", [True, False])
def test_dead_channel_gives_zero_cost_and_the_flag(eng, torch_, dev, normalize):
    name = "n3_tail"
    N, L, D, S, B, _ = CASES[name]
    x, taus, _, _, _ = make(name)
    x = x.copy()
    x[0, 1, 2 * L:3 * L] = 0.0                               # stream 0, block 2: channel 1 is silent
    x[1, :, 0:L] = 0.0                                       # stream 1, block 0: digital silence
    xd = torch_.from_numpy(x).to(dev)
    cost, flag = (t.cpu().numpy() for t in eng.mcc_costs(xd, taus, L, D, normalize_variance=normalize))
    dead = np.zeros((S, B), bool)
    dead[0, 2] = dead[1, 0] = True
    assert np.all(flag[dead] == 1) and np.all(cost[dead] == 0.0) and not np.signbit(cost[dead]).any()
    assert np.all(flag[~dead] == 0)
    if normalize:
        assert np.all(cost[~dead] < 0.0)                     # Hadamard: a live candidate lies below 0.0 ...
        idx = eng.mcc_select(torch_.from_numpy(cost).to(dev), 1)[1].cpu().numpy()
        assert np.all(idx[dead] == 0)                        # every candidate of a silent block is dead: the first one stays
        mixed = cost.copy()
        mixed[:, :, 0] = 0.0                                 # ... so a dead candidate in front of live ones wins no block
        idx = eng.mcc_select(torch_.from_numpy(mixed).to(dev), 1)[1].cpu().numpy()
        assert np.all(idx[~dead] > 0)


def test_localize_hands_out_the_winners_and_the_last_candidates_matrix(eng, torch_, dev):
    name = "n8_grid"
    N, L, D, S, B, _ = CASES[name]
    x, taus, _, _, _ = make(name)
    G = len(taus)
    xd = torch_.from_numpy(x).to(dev)
    out = eng.mcc_localize(xd, taus, L, D, nbest=16, want_matrices=True)
    ni = out["nbest_idx"].cpu().numpy()
    Rb, Rl = out["R_best"].cpu().numpy(), out["R_last"].cpu().numpy()
    assert Rb.shape == (S, B, 16, N, N) and Rl.shape == (S, B, N, N)
    allp = np.array([[sb, g] for sb in range(S * B) for g in range(G)])
    R = eng.mcc_matrices(xd, taus, L, D, allp).cpu().numpy().reshape(S, B, G, N, N)
    assert np.array_equal(Rl, R[:, :, G - 1])
    for s in range(S):
        for b in range(B):
            for j in range(16):
                if ni[s, b, j] < 0:
                    assert j >= G and np.isnan(Rb[s, b, j]).all()
                else:
                    assert np.array_equal(Rb[s, b, j], R[s, b, ni[s, b, j]])


def test_engine_refuses_what_the_kernel_could_not_read(eng, torch_, dev):
    from distant_speech_recognition_amd import _lib
    x = torch_.zeros((1, 2, 64), dtype=torch_.float32, device=dev)
    for tau, L, D in (([[0, 5]], 64, 4), ([[0, 0]], 7, 4), ([[0, 0, 0]], 64, 4), ([[0, 0]], 128, 4)):
        with pytest.raises(_lib.BtkError) as e:
            eng.mcc_costs(x, np.array(tau), L, D)
        assert e.value.code == _lib.BTK_ERR_DIMENSION
    with pytest.raises(_lib.BtkError):
        eng.mcc_select(torch_.zeros((1, 4), dtype=torch_.float64, device=dev), 17)
    with pytest.raises(_lib.BtkError):
        eng.mcc_matrices(x, np.array([[0, 0]]), 64, 4, [[1, 0]])                # block 1 of 1
    with pytest.raises(_lib.BtkError):
        eng.mcc_costs(x, np.array([[0.0, 1.0]]), 64, 4)                        # delays in seconds are not sample delays


def test_zz_report():
    print("largest error / bound over this file: R %.3g, cost %.3g" % (worst["R"], worst["cost"]))
