"""CPU: the float64 restatement of the echo cancellers (tests/aec_closed_form.py) against itself -- identities between the kinds,
the branch structure of the double-talk detector, float64 against longdouble on the inputs of tests/test_gpu_aec.py -- and the
pieces of the feature that need no GPU: the import names, the reference script's call shapes, the C-ABI table."""
import ast
import builtins
import ctypes
import os
import re

import numpy as np
import pytest

from tests import aec_closed_form as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SCRIPT = "/root/reference/btk20_src/unit_test/test_subband_aec.py"
# not provided by this engine, by decision: they share one skip counter across all bins and frames, use a
# function-local static loading constant and invert through GSL's Hermitian eigen-solver -- nothing a float64 closed form can pin
NOT_PROVIDED = {"InformationFilterEchoCancellationFeaturePtr", "SquareRootInformationFilterEchoCancellationFeaturePtr"}


def test_block_kalman_with_one_tap_is_the_kalman_filter():
    """(a) kind 2 with P = 1 and amp4play = 1 equals kind 1 when sigma2 = sigmau2 = sigmak2 (initial sigma2_v, K and the process
    noise coincide); with sigmak2 != sigma2 it equals kind 1 started from K = sigmak2 and differs from kind 1 proper"""
    V, A = cf.make_inputs(7, 6, 150, 1)
    s2 = 40.0
    k1 = cf.new_state(1, 6, 1, sigma2=s2)
    E1, f1, _ = cf.run(1, V, A, k1)
    k2 = cf.new_state(2, 6, 1, sigmau2=s2, sigmak2=s2)
    E2, f2, _ = cf.run(2, V, A, k2)
    sc = np.max(np.abs(E1))
    assert np.array_equal(f1, f2) and f1.sum() < f1.size
    assert np.max(np.abs(E1 - E2)) <= 1e-10 * sc
    assert np.max(np.abs(k1["R"] - k2["R"])) <= 1e-10 * np.max(np.abs(k1["R"]))
    assert np.max(np.abs(k1["K"] - k2["K"])) <= 1e-10 * np.max(np.abs(k1["K"])) and np.max(np.abs(k1["sig"] - k2["sig"])) <= 1e-10 * np.max(k1["sig"])
    # sigmak2 != sigma2: predicted by kind 1 started from K = sigmak2
    k2b = cf.new_state(2, 6, 1, sigmau2=s2, sigmak2=5.0)
    E2b, _, _ = cf.run(2, V, A, k2b)
    k1b = cf.new_state(1, 6, 1, sigma2=s2)
    k1b["K"][...] = 5.0
    E1b, _, _ = cf.run(1, V, A, k1b)
    assert np.max(np.abs(E1b - E2b)) <= 1e-10 * sc
    assert np.max(np.abs(E1 - E2b)) > 1e-6 * sc


def test_dtd_constant_negative_frame_number_skips_only_on_negative_snr():
    """(b) with next()'s default frame number the 'first 100 frames' branch always holds (aec.cc:825,841): sf = -1 is never
    assigned, a bin is skipped only where snr_ < 0 made sf negative -- and that does happen, the smoothing factor exceeds 1"""
    V, A = cf.make_inputs(11, 5, 140, 4, pause=(30, 32))
    st = cf.new_state(3, 5, 4, **cf.DTD_GATE)
    tr = []
    E, fl, mg = cf.run(3, V, A, st, frame_no0=-5, trace=tr)
    assert len(tr) == 5 * 140
    skipped = 0
    for t, m, snr, sf in tr:
        if snr >= 0:
            assert sf >= 0 and fl[m, t] == 1
        else:
            assert sf < 0 and fl[m, t] == 0            # from the formula, 2 / (1 + exp(-snr_)) - 1 (it rounds to -1 for large |snr_|)
            skipped += 1
    assert 0 < skipped == fl.size - fl.sum()
    # with explicit frame numbers the branch ends at frame 100 and the gate can close with sf = -1
    st2 = cf.new_state(3, 5, 4, **cf.DTD_GATE)
    V2, A2 = cf.make_inputs(11, 5, 180, 4)
    tr2 = []
    cf.run(3, V2, A2, st2, trace=tr2)
    assert any(sf == -1.0 for t, m, snr, sf in tr2 if t >= 100) and not any(sf == -1.0 for t, m, snr, sf in tr2 if t < 100)


@pytest.mark.parametrize("case", cf.CASES, ids=[c[0] for c in cf.CASES])
def test_float64_and_longdouble_take_the_same_decisions(case):
    """(c) on the inputs of the GPU tests: identical gate decisions, E within 1e-9, and every decision at least 1e-8 from its branch"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("longdouble is float64 on this platform")
    r64, rld = cf.case_reference(case), cf.case_reference(case, np.longdouble)
    for s, (a, b) in enumerate(zip(r64, rld)):
        assert a[2].smallest() >= 1e-8 and b[2].smallest() >= 1e-8, (case[0], s, a[2].smallest())
        assert np.array_equal(a[1], b[1]), (case[0], s)
        assert np.max(np.abs(a[0] - b[0])) <= 1e-9 * np.max(np.abs(b[0])), (case[0], s)


def test_dtd_cases_cover_both_state_placements():
    from distant_speech_recognition_amd import _lib
    L = _lib.lib()
    assert L.btk_aec_max_filter_length() == 64
    assert L.btk_aec_dtd_state_in_lds(32, 24) == 1 and L.btk_aec_dtd_state_in_lds(32, 25) == 0
    assert L.btk_aec_dtd_state_in_lds(256, 36) == 0 and L.btk_aec_dtd_state_in_lds(256, 2) == 1
    ps = {c[4] for c in cf.CASES if c[1] == 3 and c[3] == 32}
    assert {24, 25} <= ps
    # kind 2: both sides of every register-tile boundary
    assert {4, 5, 8, 9, 16, 17, 32, 33} <= {c[4] for c in cf.CASES if c[1] == 2}


def test_btk20_aec_import_names_resolve():
    """(d) `from btk20.aec import *` gives the four classes, under the reference's module name"""
    ns = {}
    exec("from btk20.aec import *", ns)
    for n in ("NLMSAcousticEchoCancellationFeaturePtr", "KalmanFilterEchoCancellationFeaturePtr",
              "BlockKalmanFilterEchoCancellationFeaturePtr", "DTDBlockKalmanFilterEchoCancellationFeaturePtr"):
        assert n in ns, n
    import btk20
    import btk20.aec
    assert btk20.aec is btk20.__dict__["aec"]
    assert not (NOT_PROVIDED & set(ns)), "no stub classes for the information filters"
    from distant_speech_recognition_amd.btk20cpp import _signatures as S
    assert [p for p, _ in S.CTORS["NLMSAcousticEchoCancellationFeaturePtr"]][:2] == ["original", "distorted"]
    assert [p for p, _ in S.CTORS["DTDBlockKalmanFilterEchoCancellationFeaturePtr"]][:3] == ["played", "recorded", "sample_num"]


@pytest.mark.skipif(not os.path.exists(REF_SCRIPT), reason="the reference tree is only mounted in the dev container")
def test_reference_aec_script_resolves_in_the_mirror():
    """(d) unit_test/test_subband_aec.py, translated in memory: every name, constructor keyword and method it uses exists"""
    import inspect
    from tests.test_reference_callers_resolve import _load
    import distant_speech_recognition_amd.btk20 as b20
    import distant_speech_recognition_amd.btk20.aec as aec
    from distant_speech_recognition_amd.btk20cpp import _signatures as S
    mod, tree = _load("test_subband_aec.py")
    defined = set(mod.__dict__) | set(dir(builtins))
    for n in ast.walk(tree):
        if isinstance(n, ast.Name) and isinstance(n.ctx, (ast.Store, ast.Del)):
            defined.add(n.id)
        elif isinstance(n, (ast.FunctionDef, ast.ClassDef)):
            defined.add(n.name)
        elif isinstance(n, ast.arg):
            defined.add(n.arg)
        elif isinstance(n, ast.alias):
            defined.add((n.asname or n.name).split(".")[0])
    missing = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load) and n.id not in defined}
    assert missing == NOT_PROVIDED, "beyond the two information filters the mirror lacks: %s" % sorted(missing - NOT_PROVIDED)
    # constructor keywords of every btk20 class the script builds
    checked = 0
    for n in ast.walk(tree):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id.endswith("Ptr") and n.func.id not in NOT_PROVIDED:
            names = [p for p, _ in S.CTORS[n.func.id]]
            for kw in n.keywords:
                assert kw.arg in names, (n.func.id, kw.arg)
            checked += 1
    assert checked >= 7
    for cname in ("NLMSAcousticEchoCancellationFeaturePtr", "DTDBlockKalmanFilterEchoCancellationFeaturePtr"):
        assert getattr(mod, cname) is getattr(aec, cname)
    mirror = set()
    for _, cls in inspect.getmembers(b20, inspect.isclass):
        mirror |= set(dir(cls))
    import argparse, json, pickle, wave, sys, numpy
    other = set()
    for o in (list, dict, str, bytes, numpy, numpy.ndarray, wave, wave.Wave_write, argparse, argparse.ArgumentParser, json, pickle, os, os.path, sys,
              type(open(os.devnull))):
        other |= set(dir(o))
    called = {n.func.attr for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}
    missing = sorted(a for a in called if a not in mirror and a not in other)
    assert not missing, missing


def test_abi_declares_exports_and_binds_the_aec_entries():
    """(e) btk_aec_* in the header, the library and the ctypes table"""
    from distant_speech_recognition_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "btkhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(btk_aec_[a-z0-9_]+)\s*\(", txt))
    assert {"btk_aec_init", "btk_aec_process"} <= declared
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(L, s) and s in _lib.SIGNATURES, s
    # a clean error above the limits, without a device
    import numpy
    p = numpy.zeros(8)
    one = ctypes.c_void_p(8)
    rc = _lib.lib().btk_aec_process(2, p.ctypes.data_as(ctypes.c_void_p), one, one, one, None, 1, 64, 65, 8, 8, 0, one, one, one, one, one, None)
    assert rc == _lib.BTK_ERR_DIMENSION and b"sample_num" in _lib.lib().btk_last_error()
    rc = _lib.lib().btk_aec_process(3, p.ctypes.data_as(ctypes.c_void_p), one, one, one, None, 1, 4096, 4, 8, 8, 0, one, one, one, one, one, None)
    assert rc == _lib.BTK_ERR_DIMENSION and b"2048" in _lib.lib().btk_last_error()


def test_tool_refuses_the_information_filters_by_name(tmp_path):
    import json
    from tools import subband_aec
    for kind in subband_aec.UNSUPPORTED:
        with pytest.raises(KeyError, match="not supported"):
            subband_aec.make_canceller(None, None, {"type": kind})
        conf = tmp_path / ("%s.json" % kind)
        conf.write_text(json.dumps({"type": kind}))
        assert subband_aec.main(["-c", str(conf), "-q"]) == 2
    assert subband_aec.DEFAULT_CONF["type"] == "dtd_block_kalman_filter" and subband_aec.DEFAULT_CONF["filter_length"] == 36
