"""CPU, dev container only (skipped where /root/reference is absent): the checks of test_reference_callers_resolve.py applied to
the reference's unit_test/test_tdoa_estimator.py -- loaded in memory against this repo's `btk20` import names (nothing is
written to this repository): every name it imports or uses, every keyword it passes and every method it calls must exist."""
import ast
import builtins
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/btk20_src/unit_test"
SCRIPT = "test_tdoa_estimator.py"

pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is only mounted in the dev container")


def _load():
    src = open(os.path.join(REF, SCRIPT)).read() + "\n"
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    mod = types.ModuleType("ref_test_tdoa_estimator")
    mod.__dict__["__name__"] = "ref_test_tdoa_estimator"         # not "__main__": only definitions run
    exec(compile(src, SCRIPT, "exec"), mod.__dict__)             # `from btk20.feature import *`, `from btk20.pytdoa import *`
    return mod, ast.parse(src)


def test_names_resolve_in_the_mirror():
    mod, tree = _load()
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
    assert not missing, "names the reference script uses that the mirror lacks: %s" % sorted(missing)
    for name in ("SampleFeaturePtr", "HammingFeaturePtr", "FFTFeaturePtr", "make_tdoa_front_end"):
        assert name in mod.__dict__, name


def test_keywords_are_accepted():
    """keywords of Python callables against their signatures, keywords of bound classes against the table generated from the
    reference's SWIG interface (which the binding's constructors are called through)"""
    import inspect
    from distant_speech_recognition_amd.btk20cpp import _signatures as S
    mod, tree = _load()
    bad, checked = [], 0
    for n in ast.walk(tree):
        if not (isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.keywords):
            continue
        obj = mod.__dict__.get(n.func.id)
        if obj is None:
            continue
        if getattr(obj, "__module__", "").startswith("distant_speech_recognition_amd"):
            accepted = set(inspect.signature(obj).parameters)
        elif n.func.id in S.CTORS:
            accepted = {p for p, _ in S.CTORS[n.func.id]}
        else:
            continue
        checked += 1
        bad += [(n.func.id, kw.arg) for kw in n.keywords if kw.arg is not None and kw.arg not in accepted]
    assert not bad, bad
    assert checked >= 2                                         # SampleFeaturePtr(...) and make_tdoa_front_end(...)


def test_method_names_exist_in_the_mirror():
    import argparse
    import inspect
    import json
    import numpy
    import distant_speech_recognition_amd.btk20 as b20
    import distant_speech_recognition_amd.pytdoa as pt
    mod, tree = _load()
    mirror = set()
    for m in (b20, pt):
        for _, cls in inspect.getmembers(m, inspect.isclass):
            mirror |= set(dir(cls))
    other = set()
    for o in (list, dict, str, tuple, float, int, numpy, numpy.ndarray, argparse.ArgumentParser, argparse.Namespace, argparse, json,
              os, os.path, sys, type(open(os.devnull))):
        other |= set(dir(o))
    called = {n.func.attr for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}
    missing = sorted(a for a in called if a not in mirror and a not in other)
    assert not missing, missing
    for a in ("read", "instantaneous_position", "mic_pair_tdoa"):
        assert a in called and a in mirror


def test_bound_constructors_take_the_reference_keywords():
    """the calls of the script, spelled with its keywords, construct (no samples, no GPU work: nothing is pulled)"""
    from btk20.feature import SampleFeaturePtr, HammingFeaturePtr, FFTFeaturePtr
    s = SampleFeaturePtr(block_len=8192, shift_len=8192, pad_zeros=True)
    h = HammingFeaturePtr(s)
    f = FFTFeaturePtr(h, 16384)
    assert f.size() == 16384 and h.size() == 8192 and f.fftLen() == 16384 and f.windowLen() == 8192
    f2 = FFTFeaturePtr(samp=HammingFeaturePtr(samp=s, nm="Hamming"), fft_len=512, nm="FFT")
    assert f2.size() == 512
