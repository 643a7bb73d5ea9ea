"""GPU: what the node layer reports WHILE it streams (host/src/btk_nodes.cc).  The other node tests compare a stream's contents and
look at a node's state once the stream has ended; these poll the state after every call of a 16-bit stream that stages its input
ahead (SubbandGraphPool::stage_round_, SubbandBeamformer::prefetch_next_):

  A. is_end: of every graph of a pool after every next() / next_round(), of a single graph's synthesis bank after every next();
  B. errors and resets in the middle of a stream: new samples under a running 16-bit stream, reset() with a staged round pending;
  C. the bytes that come back to the host per round (btk_node_d2h_bytes): a graph that ends in a synthesis bank brings back its PCM.

Every comparison is equality -- of bits, of call sequences, of byte counts against a bound read from the code; no tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_node_i16 import _float_path, _graph, _same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, m, r = 4, 4, 1
AZ = (-1.306379, 0.3, 1.1, -0.4, 0.8)


def _protos(M):
    from tests.util import design_prototype
    return design_prototype(M, m), design_prototype(M, m, "g")


def _utt(L, seed):
    from tests.util import synthetic_pcm
    return synthetic_pcm(1, N, L, seed=seed)[0][0]


def _delays(i):
    from tests.util import la_delays, ula_positions
    return la_delays(ula_positions(N), AZ[i % len(AZ)])


def _pool_of(utts, M, block_frames):
    from distant_speech_recognition_amd.btk20 import SubbandGraphPoolPtr
    h, g = _protos(M)
    pool, keep = SubbandGraphPoolPtr(), []
    for i, u in enumerate(utts):
        k, bf, sfb = _graph(u, h, g, M, m, r, _delays(i), block_frames)
        pool.add(bf, sfb)
        keep.append((k, bf, sfb))
    return pool, keep


def _drain(node):
    """next() until StopIteration, WITHOUT the reset of __iter__"""
    out = []
    while True:
        try:
            out.append(np.array(node.next()))
        except StopIteration:
            return out


# ================================================================================ A. the end of a stream, polled after every call
POOL_GEOMETRIES = [(256, 16), (512, 16), (1024, 24)]          # (M, block_frames) at m = 4, r = 1: the three fused routes a pool accepts


def _pool_lens(M, B):
    D = M >> r
    # ends in the last round / in a middle round / on an exact round boundary / inside the first round / one sample past a boundary
    return [4 * B * D + 11 * D, 2 * B * D + 9 * D + 19, 2 * B * D, 3 * D, B * D + 1]


def _pool_trace(M, B, by_round):
    """one pool of five ragged graphs, driven to its end by next() (by_round: next_round()).  Per call and graph: how many blocks came
    out and what is_end(g) said afterwards; the blocks themselves; the state after exhaustion and after reset()"""
    lens = _pool_lens(M, B)
    pool, keep = _pool_of([_utt(L, 300 + i) for i, L in enumerate(lens)], M, B)
    G = len(lens)
    assert [pool.is_end(g) for g in range(G)] == [False] * G
    seq, blocks = [], [[] for _ in range(G)]
    while True:
        if by_round:
            outs = pool.next_round()
            if outs is None:
                break
            n = [int(a.shape[0]) for a in outs]
            for g, a in enumerate(outs):
                blocks[g] += [np.array(b) for b in a]
        else:
            try:
                outs = pool.next()
            except StopIteration:
                break
            n = [0 if o is None else 1 for o in outs]
            for g, o in enumerate(outs):
                if o is not None:
                    blocks[g].append(np.array(o))
        seq.append([[n[g], bool(pool.is_end(g))] for g in range(G)])
        assert len(seq) < 100000
    after = [[bool(pool.is_end(g)), pool.output(g) is None] for g in range(G)]
    i16 = [bool(k[1].i16_stream()) for k in keep]
    pool.reset()
    after_reset = [bool(pool.is_end(g)) for g in range(G)]
    return {"seq": seq, "blocks": [np.concatenate(b) if b else np.zeros(0, np.float32) for b in blocks], "after": after,
            "after_reset": after_reset, "i16": i16}


def _check_trace(tr, M, B):
    G = len(tr["after"])
    seq = tr["seq"]
    lens = _pool_lens(M, B)
    for g in range(G):
        delivered = [i for i, c in enumerate(seq) if c[g][0] > 0]
        ends = [c[g][1] for c in seq]
        assert delivered, g
        # 1. not ended as long as a later call still delivers a block of this graph
        early = [i for i in range(delivered[-1]) if ends[i]]
        assert not early, "graph %d: is_end true after calls %s, blocks still came out up to call %d" % (g, early[:8], delivered[-1])
        # 2. once true it stays true
        if True in ends:
            assert all(ends[ends.index(True):]), (g, ends)
        # every sample of the utterance came out (whole blocks: the source pads its last block with zeros)
        assert tr["blocks"][g].size >= lens[g], (g, tr["blocks"][g].size, lens[g])
    # 3. after exhaustion: ended, and no block to show
    assert tr["after"] == [[True, True]] * G, tr["after"]
    # ... until reset()
    assert tr["after_reset"] == [False] * G


CHILD = r'''
import json, sys
sys.path.insert(0, %r)
import numpy as np
from tests.test_gpu_node_midstream import _pool_trace
out = {}
for by_round in (False, True):
    tr = _pool_trace(%d, %d, by_round)
    np.save(sys.argv[1] + ("_round" if by_round else "_next") + ".npy", np.concatenate(tr["blocks"]))
    out["round" if by_round else "next"] = {"seq": tr["seq"], "after": tr["after"], "after_reset": tr["after_reset"], "i16": tr["i16"],
                                            "sizes": [int(b.size) for b in tr["blocks"]]}
print("TRACE " + json.dumps(out))
'''


@pytest.mark.parametrize("M,B", POOL_GEOMETRIES)
def test_pool_is_end_polled_after_every_call(dev, tmp_path, M, B):
    """five graphs whose utterances end in the last round, in middle rounds, on a round boundary, inside the first round and one
    sample past a boundary.  A 16-bit pool stages round r + 1 while round r is served; what it learns there about a graph's end
    belongs to round r + 1: is_end(g) must not be true while a later call still delivers a block of g, stays true once it is, and
    the per-call sequence of (blocks delivered, is_end) and the blocks are those of the float path (BTK_NODE_I16=0: nothing is
    staged ahead) and of a 16-bit pool without the staging (BTK_NODE_PREFETCH=0: read once per process, hence a child process)"""
    runs = {}
    for by_round in (False, True):
        tr = _pool_trace(M, B, by_round)
        assert all(tr["i16"])
        with _float_path():
            tf = _pool_trace(M, B, by_round)
        assert not any(tf["i16"])
        runs[by_round] = (tr, tf)
    env = dict(os.environ)
    env["BTK_NODE_PREFETCH"] = "0"
    env.pop("BTK_NODE_I16", None)
    stem = str(tmp_path / "noprefetch")
    res = subprocess.run([sys.executable, "-c", CHILD % (ROOT, M, B), stem], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    child = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("TRACE ")][-1][6:])
    for by_round in (False, True):
        tr, tf = runs[by_round]
        tc = child["round" if by_round else "next"]
        assert all(tc["i16"])
        tc["blocks"] = np.split(np.load(stem + ("_round" if by_round else "_next") + ".npy"), np.cumsum(tc["sizes"])[:-1])
        # 1. - 3. on every run: the float path and the pool without staging stage nothing ahead, they say what the sequence is ...
        _check_trace(tf, M, B)
        _check_trace(tc, M, B)
        _check_trace(tr, M, B)
        # 4. ... and the staged 16-bit pool reports the same, call by call
        assert tr["seq"] == tf["seq"] == tc["seq"], by_round
        # 5. the same blocks, bit for bit
        for g in range(len(tr["blocks"])):
            assert float(np.max(np.abs(tr["blocks"][g]))) > 100
            assert _same_bits(tr["blocks"][g], tf["blocks"][g]), (by_round, g)
            assert _same_bits(tr["blocks"][g], np.asarray(tc["blocks"][g], np.float32)), (by_round, g)
    # a round at a time or a block at a time: the same blocks
    for g in range(len(runs[False][0]["blocks"])):
        assert _same_bits(runs[False][0]["blocks"][g], runs[True][0]["blocks"][g]), g


def test_single_graph_is_end_polled_after_every_next(dev):
    """a single 16-bit graph plans and uploads its next block ahead too (prefetch_next_): the synthesis bank's is_end() is false
    after every next() that returned a block and true after the one that raised StopIteration.  (This held before the pool's
    is_end was mended too: the bank sets is_end only where it raises.)"""
    M, B = 512, 16
    D = M >> r
    h, g = _protos(M)
    _, bf, sfb = _graph(_utt(2 * B * D + 9 * D + 19, 77), h, g, M, m, r, _delays(0), B)
    sfb.reset()
    n = 0
    while True:
        try:
            sfb.next()
        except StopIteration:
            break
        n += 1
        assert not sfb.is_end(), n
    assert bf.i16_stream() and n == 2 * B + 10 and sfb.is_end()


# ================================================================================ B. errors and resets in the middle of a 16-bit stream
BM, BB, BLEN, BLEN2 = 512, 32, 200, 120          # M, block_frames, blocks of the utterances, blocks of the utterance that replaces one


def _after_change(call, ref, got0):
    """200 more calls after the samples changed.  call() returns the blocks one call delivered as [(graph, block)], raises at the end
    of the stream or on an error.  Returns the errors in call order, after checking
      1. that every block delivered is, bit for bit, the block at its position in the untouched run `ref` (per graph), and
      3. that from the first error on every call raises and nothing is delivered any more."""
    pos = list(got0)
    errors, first = [], None
    for i in range(200):
        try:
            got = call()
        except StopIteration:
            raise AssertionError("call %d after the change ended the stream as if nothing had happened (first error: call %s)" % (i, first))
        except Exception as e:           # noqa: BLE001 -- whatever the binding raises is recorded and looked at by the caller
            errors.append(e)
            first = i if first is None else first
            continue
        assert first is None, "call %d delivered a block after call %d had raised %r" % (i, first, str(errors[0])[:120])
        for gph, b in got:
            assert pos[gph] < len(ref[gph]), (i, gph)
            assert _same_bits(b, ref[gph][pos[gph]]), "call %d: block %d of graph %d is not the original utterance's" % (i, pos[gph], gph)
            pos[gph] += 1
    assert first is not None, "200 calls after the change and no error"
    assert len(errors) == 200 - first
    return errors


def test_changed_samples_under_a_16_bit_graph(dev):
    """set_samples() on every source of a running 16-bit graph, without reset().  The blocks that still come out are the original
    utterance's (computed, or at least uploaded, before the change); the first load that would read the source again raises and
    names the 16-bit stream, BEFORE it commits the block that was planned ahead; the failure is latched until reset(); after
    reset() the new utterance streams with the bits of a fresh graph.
    (The upload of the block planned ahead reads the source's pinned int16 copy on the copy stream.  set_samples() waits for that
    stream before it rewrites the copy in place; without the wait a block could hold samples of both utterances.  That race has no
    deterministic test -- the comparison with the untouched run above cannot catch it reliably.)"""
    from distant_speech_recognition_amd.btk20 import j_error
    D = BM >> r
    h, g = _protos(BM)
    pcm, pcm2 = _utt(BLEN * D, 5), _utt(BLEN2 * D, 6)
    _, _, sfb0 = _graph(pcm, h, g, BM, m, r, _delays(0), BB)
    sfb0.reset()
    ref = _drain(sfb0)
    assert len(ref) == BLEN
    keep, bf, sfb = _graph(pcm, h, g, BM, m, r, _delays(0), BB)
    sfb.reset()
    for i in range(40):
        assert _same_bits(np.array(sfb.next()), ref[i])
    assert bf.i16_stream()
    for c in range(N):
        keep[2 * c].set_samples(pcm2[c])
    errors = _after_change(lambda: [(0, np.array(sfb.next()))], [ref], [40])
    assert isinstance(errors[0], j_error) and "16-bit" in str(errors[0]), errors[0]                  # 2.
    assert all(isinstance(e, j_error) and "16-bit" in str(e) for e in errors)
    sfb.reset()                                                                                     # 4.
    out = np.concatenate(_drain(sfb))
    _, bf2, sfb2 = _graph(pcm2, h, g, BM, m, r, _delays(0), BB)
    sfb2.reset()
    fresh = np.concatenate(_drain(sfb2))
    assert bf.i16_stream() and bf2.i16_stream() and out.size == BLEN2 * D and _same_bits(out, fresh)


def test_changed_samples_under_a_16_bit_pool(dev):
    """the same under a pool of three: the sources of ONE graph change.  No graph's blocks mix utterances, the round that was staged
    before the change is refused before it is made current (a failed staging must leave nothing a later call takes for a staged
    round), every later call raises until reset(), and after reset() the pool streams the new utterance beside the two old ones
    with the bits of a fresh pool"""
    from distant_speech_recognition_amd.btk20 import j_error
    D = BM >> r
    utts = [_utt(BLEN * D, 50 + i) for i in range(3)]
    pcm2 = _utt(BLEN2 * D, 60)

    def blocks_of(pool):
        return [(gph, np.array(o)) for gph, o in enumerate(pool.next()) if o is not None]

    def drain(pool):
        out = [[] for _ in range(3)]
        while True:
            try:
                for gph, b in blocks_of(pool):
                    out[gph].append(b)
            except StopIteration:
                return out

    pool0, keep0 = _pool_of(utts, BM, BB)
    ref = drain(pool0)
    assert [len(x) for x in ref] == [BLEN] * 3
    pool, keep = _pool_of(utts, BM, BB)
    got = [0, 0, 0]
    for _ in range(40):
        for gph, b in blocks_of(pool):
            assert _same_bits(b, ref[gph][got[gph]])
            got[gph] += 1
    assert all(k[1].i16_stream() for k in keep) and got == [40] * 3
    for c in range(N):
        keep[1][0][2 * c].set_samples(pcm2[c])
    errors = _after_change(lambda: blocks_of(pool), ref, got)
    assert all(isinstance(e, j_error) and "16-bit" in str(e) for e in errors), errors[0]
    pool.reset()
    out = drain(pool)
    poolf, keepf = _pool_of([utts[0], pcm2, utts[2]], BM, BB)
    fresh = drain(poolf)
    assert all(k[1].i16_stream() for k in keep) and [len(x) for x in out] == [BLEN, BLEN2, BLEN]
    for gph in range(3):
        assert _same_bits(np.concatenate(out[gph]), np.concatenate(fresh[gph])), gph


def test_reset_in_the_middle_of_a_16_bit_stream(dev):
    """1.5 rounds into a 16-bit stream the next block (single graph) / round (pool) is already planned and on its way up; reset()
    then, and the stream from its start has the bits of a first pass: the staged input nobody asked for leaves no trace.
    (Every utterance reaches beyond the staged round, blocks 2 B .. 3 B - 1: a SampleFeature that was pulled to its end has dropped
    its samples, as the reference's does, and a reset() then restarts an empty stream whether anything was staged or not.)"""
    M, B = 512, 16
    D = M >> r
    h, g = _protos(M)
    lens = [70 * D + 19, 4 * B * D, 60 * D]
    utts = [_utt(L, 80 + i) for i, L in enumerate(lens)]
    # a single graph
    _, bf0, sfb0 = _graph(utts[0], h, g, M, m, r, _delays(0), B)
    sfb0.reset()
    first = np.concatenate(_drain(sfb0))
    _, bf, sfb = _graph(utts[0], h, g, M, m, r, _delays(0), B)
    sfb.reset()
    for _ in range(B + B // 2):
        sfb.next()
    assert bf.i16_stream()
    sfb.reset()
    again = np.concatenate(_drain(sfb))
    assert bf.i16_stream() and float(np.max(np.abs(first))) > 100 and _same_bits(again, first)
    # a pool
    def drain(pool):
        out = [[] for _ in utts]
        while True:
            try:
                for gph, o in enumerate(pool.next()):
                    if o is not None:
                        out[gph].append(np.array(o))
            except StopIteration:
                return [np.concatenate(x) for x in out]

    pool0, keep0 = _pool_of(utts, M, B)
    first = drain(pool0)
    pool, keep = _pool_of(utts, M, B)
    for _ in range(B + B // 2):
        pool.next()
    assert all(k[1].i16_stream() for k in keep)
    pool.reset()
    again = drain(pool)
    assert all(k[1].i16_stream() for k in keep)
    for gph in range(3):
        assert first[gph].size >= lens[gph] and _same_bits(again[gph], first[gph]), gph


# ================================================================================ C. what comes back to the host
CM, CB, CROUNDS = 512, 64, 6


def _d2h_rounds(step, round_id):
    """drives a stream to its end with step() (returns the number of blocks one call delivered, raises StopIteration at the end) and
    returns per round -- the calls between two changes of round_id() -- [bytes that came back to the host, blocks delivered]"""
    from distant_speech_recognition_amd import btk20cpp
    rounds, cur = [], None
    while True:
        b0 = btk20cpp.node_d2h_bytes()
        try:
            n = step()
        except StopIteration:
            n = None
        rid = round_id()
        if rid != cur or not rounds:
            rounds.append([0, 0])
            cur = rid
        rounds[-1][0] += btk20cpp.node_d2h_bytes() - b0
        rounds[-1][1] += n or 0
        if n is None:
            return rounds


def _check_d2h(rounds, D, what):
    print(what, "[bytes, blocks] per round:", rounds)
    assert len(rounds) >= CROUNDS, (what, rounds)
    assert sum(x[1] for x in rounds) >= CROUNDS * CB
    for i, (nbytes, nblocks) in enumerate(rounds[1:], 1):
        assert nbytes <= 4 * D * (nblocks + 1), "%s: round %d brought %d bytes back for %d blocks (bound %d)" % (what, i, nbytes, nblocks, 4 * D * (nblocks + 1))


@pytest.mark.parametrize("what", ["fused", "staged", "zelinski", "pool"])
def test_only_the_pcm_comes_back_to_the_host(dev, what):
    """a graph pulled through its synthesis bank: beamformer (fused / staged with snapshots / with a Zelinski post-filter behind it)
    and synthesis hand their blocks over on the device, and a round of T frames brings back the PCM of its output blocks only.
    Bound per round after the first (which also sets up weights and the like): 4 D (blocks delivered + 1) bytes -- 66 560 for 64 blocks of
    D = 256, where ONE [K][T] complex64 spectrum is 8 * 257 * 64 = 131 584.
    The + 1: OverSampledDFTSynthesisBank::run_window_ starts an aligned launch one block early when (b_first - w0 + pd) is odd and
    computes nblocks_ + lead blocks, lead in {0, 1}.  As the code stands the lead block stays on the device -- the copy is
    d2h_async(hb, first, 4 * nblocks_ * D), and the pool's hipMemcpy2DAsync starts at dO + lead * D -- so the exact figure is
    4 * D * nblocks_ per round (per graph in a pool); the bound leaves room for a download that takes the lead block along.
    (A pool copies a rectangle [G][nb D]: the graphs here are equally long, a graph that has ended would still have its row copied.)
    Measured before the post-filter kept its block and its spectral densities on the device: 230 016 bytes per 64-block round of
    the Zelinski graph (65 536 of PCM, 131 584 of spectrum, 32 896 of densities); the other three graphs were within the bound."""
    D = CM >> r
    h, g = _protos(CM)
    L = CROUNDS * CB * D
    if what == "pool":
        pool, keep = _pool_of([_utt(L, 90 + i) for i in range(3)], CM, CB)

        def step():
            return sum(o is not None for o in pool.next())
        rounds = _d2h_rounds(step, pool.rounds)
        assert all(k[1].i16_stream() for k in keep)
    else:
        keep, bf, sfb = _graph(_utt(L, 90), h, g, CM, m, r, _delays(0), CB, staged=what == "staged", postfilter=what == "zelinski")
        sfb.reset()

        def step():
            sfb.next()
            return 1
        rounds = _d2h_rounds(step, bf.chunk_base)
        assert bf.i16_stream() and bf.fused_path() == (what == "fused") and bf.snapshots_materialised() == (what != "fused")
    _check_d2h(rounds, D, what)


def test_post_filter_pulled_frame_by_frame_still_serves_its_frames(dev):
    """the post-filter's own next() serves frames from a host mirror of its block and keeps that download: frame by frame it hands
    out, bit for bit, the blocks the same graph holds on the device while a synthesis bank pulls it (device_block(): the host view
    of the block the synthesis bank was handed)"""
    from distant_speech_recognition_amd import btk20cpp
    M, B = 512, 64
    D, K = M >> r, M // 2 + 1
    h, g = _protos(M)
    pcm = _utt(3 * B * D + 5 * D + 7, 95)
    keep, bf, sfb = _graph(pcm, h, g, M, m, r, _delays(0), B, postfilter=True)
    pf = keep[-1]
    sfb.reset()
    blocks, base = [], -1
    while True:
        try:
            sfb.next()
        except StopIteration:
            break
        if pf._block_base() != base:
            base = pf._block_base()
            blocks.append(np.array(pf.device_block())[0])                          # [K][T]
    Y = np.concatenate(blocks, axis=1)
    keep2, bf2, _ = _graph(pcm, h, g, M, m, r, _delays(0), B, postfilter=True)
    pf2 = keep2[-1]
    pf2.reset()
    b0 = btk20cpp.node_d2h_bytes()
    frames = _drain(pf2)
    assert bf.i16_stream() and bf2.i16_stream()
    assert len(frames) == Y.shape[1] and len(frames) > 3 * B and float(np.max(np.abs(Y))) > 100, (len(frames), Y.shape)
    F = np.stack(frames)                                                           # [T][M] complex128, conjugate mirror above M/2
    assert np.array_equal(F[:, :K], Y.T.astype(np.complex128))
    assert np.array_equal(F[:, K:], np.conj(F[:, 1:M // 2][:, ::-1]))
    assert btk20cpp.node_d2h_bytes() - b0 >= 8 * K * len(frames)                   # every block's spectrum came to the host
