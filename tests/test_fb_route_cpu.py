"""CPU: the filter-bank route table (csrc/fb_route.h) -- which kernel covers a plan, what the five queries of the C-ABI answer and
how much scratch btk_fb_analysis_bf asks for -- against a table WRITTEN OUT here from the contract in include/btkhip.h and the
dispatch as it stood before the route existed.  tests/cpp/fb_route_table.cc (a plain C++ program, only fb_route.h) prints the
route's side for every M in 64 ... 2048, m in {2, 4}, r in 0 ... 3, whole plans and bin shards, float and int16 samples, under the
default switches and under each switch on its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distant_speech_recognition_amd", "csrc")
MS = (64, 128, 256, 512, 1024, 2048)
SHAPES = ((1, 1, 0, 1), (2, 3, 1, 2), (32, 64, 0, 4096), (1, 64, 0, 512))     # S, N, per_stream, tcount

# ---- the expected table, m = 4, whole bin range; one word per r = 0, 1, 2, 3 (m = 2 and bin shards: see expected()) ----------------
G4, S4 = "GENERIC GENERIC GENERIC GENERIC", "STAGED STAGED STAGED STAGED"
ANA = {64: G4, 128: G4, 256: "FAST FAST FAST GENERIC", 512: "A512 A512 A512 GENERIC", 1024: "FAST FAST FAST GENERIC", 2048: "FAST FAST FAST GENERIC"}
# (M = 2048, r = 2: the frame ring of the fb_fast.hip synthesis kernel does not fit the LDS)
SYN = {64: G4, 128: G4, 256: "FAST FAST FAST GENERIC", 512: "S512 S512 S512 GENERIC", 1024: "FAST FAST FAST GENERIC", 2048: "FAST FAST GENERIC GENERIC"}
ALIGNED = {64: "0 0 0 0", 128: "0 0 0 0", 256: "0 0 0 0", 512: "1 1 0 0", 1024: "1 1 0 0", 2048: "1 1 0 0"}
FUSED = {64: S4, 128: S4, 256: "FAST256 FAST256 FAST256 STAGED", 512: "BFZ512 FUSED512 BFZ512 STAGED", 1024: "STAGED BIG STAGED STAGED", 2048: "STAGED BIG STAGED STAGED"}
NONE = {M: G4 for M in MS}
DEFAULT = {"ana": ANA, "syn": SYN, "aligned": ALIGNED, "fused": FUSED, "fused_i16": FUSED}
OLD512 = {**FUSED, 512: "BFZ512 BFZ512 BFZ512 STAGED"}                        # analysis512_bfz_kernel for every r <= 2
TABLE = {
    "default": DEFAULT,
    "BTK_DISABLE_ANALYSIS512": {**DEFAULT, "ana": {**ANA, 512: "FAST FAST FAST GENERIC"}},
    "BTK_DISABLE_SYNTHESIS512": {**DEFAULT, "syn": {**SYN, 512: "FAST FAST FAST GENERIC"}, "aligned": {**ALIGNED, 512: "0 0 0 0"}},
    # (the float fused kernel of M = 256 stays, its int16 form goes: an asymmetry of long standing, recorded in fb_route.h)
    "BTK_DISABLE_FAST": {"ana": {**NONE, 512: ANA[512]}, "syn": {**NONE, 512: SYN[512]}, "aligned": {**ALIGNED, 1024: "0 0 0 0", 2048: "0 0 0 0"},
                         "fused": FUSED, "fused_i16": {**FUSED, 256: S4}},
    "BTK_DISABLE_FUSED": {**DEFAULT, "fused": {M: S4 for M in MS}, "fused_i16": {M: S4 for M in MS}},
    "BTK_SYN_NARROW": {**DEFAULT, "aligned": {M: "0 0 0 0" for M in MS}},
    "BTK_FUSED_VAR": {**DEFAULT, "fused": OLD512, "fused_i16": OLD512},
    "BTK_FUSED512_NEW=0": {**DEFAULT, "fused": OLD512, "fused_i16": OLD512},
}


def big_cg(S, N, tcount):
    """channel groups of the M = 1024 / 2048 fused launch (8-frame tiles; fb_fused_big.hip)"""
    tiles, cg = (tcount + 7) // 8 * S, 1
    while cg < 16 and tiles * cg < 384 and N // (2 * cg) >= 8:
        cg *= 2
    return cg


def consumed(route, M, S, N, per_stream, tcount):
    """bytes of `scratch` the launch of a route touches, from the layouts in the kernels' sources"""
    K, Sw = M // 2 + 1, (S if per_stream else 1)
    if route in ("FUSED512", "BFZ512"):
        return 16 * Sw * N * 320                                              # weight pairs [Sw][N][320] float4
    if route == "FAST256":
        return 8 * Sw * N * K                                                 # transposed weights [Sw][N][K] complex64
    if route == "BIG":                                                        # pairs [Sw][N][M/2 + 16] float4 + partial sums [CG][S][K][tcount]
        cg = big_cg(S, N, tcount)
        return 16 * Sw * N * (M // 2 + 16) + (8 * cg * S * K * tcount if cg > 1 else 0)
    assert route == "STAGED"
    return 8 * S * K * N * tcount                                             # snapshots [S][K][N][tcount] complex64


def expected(sw, M, m, r, whole):
    t = TABLE[sw]
    row = {k: (t[k][M].split()[r] if m == 4 else {"aligned": "0", "fused": "STAGED", "fused_i16": "STAGED"}.get(k, "GENERIC")) for k in t}
    if not whole:                                                             # a bin shard (btk_fb_analysis_bins) has staged kernels only
        row["fused"] = row["fused_i16"] = "STAGED"
    return row


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fb_route") / "fb_route_table")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "fb_route_table.cc"), "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-3000:]
    rows = {}
    for line in run.stdout.splitlines():
        w = line.split()
        assert [w[5], w[7], w[9], w[11], w[13], w[18]] == ["ana", "fused", "fused_i16", "syn", "queries", "bytes"], line
        rows[(w[0], int(w[1]), int(w[2]), int(w[3]), w[4] == "whole")] = dict(
            ana=w[6], fused=w[8], fused_i16=w[10], syn=w[12], queries=[int(x) for x in w[14:18]], bytes=[int(x) for x in w[19:23]], bytes_i16=[int(x) for x in w[23:27]])
    return rows


def test_route_header_is_host_only():
    src = open(os.path.join(CSRC, "fb_route.h")).read()
    assert "#include" not in src and "getenv" not in src


def test_route_table(table):
    keys = [(sw, M, m, r, whole) for sw in TABLE for M in MS for m in (2, 4) for r in range(4) for whole in (True, False)]
    assert sorted(table) == sorted(keys)
    for key in keys:
        sw, M, m, r, whole = key
        got, exp = table[key], expected(*key)
        assert {k: got[k] for k in ("ana", "fused", "fused_i16", "syn")} == {k: exp[k] for k in ("ana", "fused", "fused_i16", "syn")}, key
        # btk_fb_analysis_i16_direct, btk_fb_synthesis_aligned_form, btk_fb_analysis_bf_fused, btk_fb_analysis_bf_i16_fused
        assert got["queries"] == [int(exp["ana"] != "GENERIC"), int(exp["aligned"]), int(exp["fused"] != "STAGED"), int(exp["fused_i16"] != "STAGED")], key
        # the int16 query is 1 exactly where the fused int16 route is not STAGED
        assert got["queries"][3] == int(got["fused_i16"] != "STAGED"), key
        for which, route in (("bytes", exp["fused"]), ("bytes_i16", exp["fused_i16"])):
            for shape, nb in zip(SHAPES, got[which]):
                need = consumed(route, M, *shape)
                # btk_fb_analysis_bf_scratch_bytes: what the route's launch consumes (M = 1024 / 2048: and 16 bytes more, as ever)
                assert nb >= need and nb == need + (16 if route == "BIG" else 0), (key, which, shape, nb, need)


def test_m512_r3_is_sized_as_staged(table):
    """M = 512, m = 4, r = 3 has no fused kernel: sized as the staged pair (the dispatch once demanded 16 Sw 320 N bytes of weight-pair
    scratch for it and refused short blocks that came with exactly btk_fb_analysis_bf_scratch_bytes)"""
    got = table[("default", 512, 4, 3, True)]
    assert got["fused"] == "STAGED" and got["bytes"][:2] == [8 * 257, 8 * 2 * 257 * 3 * 2] and got["bytes"][1] < 16 * 2 * 320 * 3
