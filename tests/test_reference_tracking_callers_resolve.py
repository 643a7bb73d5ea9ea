"""CPU, dev container only (skipped where /root/reference is absent): the checks of test_reference_tdoa_callers_resolve.py applied
to the reference's unit_test/test_source_tracking.py -- loaded in memory against this repo's `btk20` import names (nothing is
written to this repository): every name it imports or uses, every keyword it passes (those of the two tracker constructors
among them) and every method it calls must exist."""
import ast
import builtins
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/btk20_src/unit_test"
SCRIPT = "test_source_tracking.py"

pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is only mounted in the dev container")


def _load():
    src = open(os.path.join(REF, SCRIPT)).read() + "\n"
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    mod = types.ModuleType("ref_test_source_tracking")
    mod.__dict__["__name__"] = "ref_test_source_tracking"         # not "__main__": only definitions run
    exec(compile(src, SCRIPT, "exec"), mod.__dict__)             # `from btk20.pykalman import *` and the two of the TDOA script
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
    for name in ("SampleFeaturePtr", "HammingFeaturePtr", "FFTFeaturePtr", "make_tdoa_front_end", "ExtendedKalmanFilter",
                 "IteratedExtendedKalmanFilter"):
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
    assert checked >= 4                                         # SampleFeaturePtr, make_tdoa_front_end and the two trackers
    for cls in ("ExtendedKalmanFilter", "IteratedExtendedKalmanFilter"):
        assert any(isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == cls and n.keywords for n in ast.walk(tree))
        assert mod.__dict__[cls].__module__ == "distant_speech_recognition_amd.pykalman"


def test_method_names_exist_in_the_mirror():
    import argparse
    import inspect
    import json
    import numpy
    import distant_speech_recognition_amd.btk20 as b20
    import distant_speech_recognition_amd.pykalman as pk
    import distant_speech_recognition_amd.pytdoa as pt
    mod, tree = _load()
    mirror = set()
    for m in (b20, pt, pk):
        for _, cls in inspect.getmembers(m, inspect.isclass):
            mirror |= set(dir(cls))
    other = set()
    for o in (list, dict, str, tuple, float, int, numpy, numpy.ndarray, argparse.ArgumentParser, argparse.Namespace, argparse, json,
              os, os.path, sys, type(open(os.devnull))):
        other |= set(dir(o))
    called = {n.func.attr for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}
    missing = sorted(a for a in called if a not in mirror and a not in other)
    assert not missing, missing
    for a in ("read", "instantaneous_position", "mic_pair_tdoa", "set_time", "is_observed"):
        assert a in called and a in mirror


def test_tracker_constructors_take_the_reference_keywords():
    """the two constructor calls of the script, spelled with its keywords, construct and carry the reference's attributes"""
    import numpy
    from btk20.pykalman import ExtendedKalmanFilter, IteratedExtendedKalmanFilter, KalmanFilter
    kw = dict(F=numpy.identity(2), U=10.0 * numpy.identity(2), sigmaV2=4.0e-4, sigmaK2=1.0e10, time_delta=0.256,
              initialXk=numpy.zeros(2), gate_prob=0.95, boundaries=numpy.array(None))
    ekf = ExtendedKalmanFilter(None, **kw)
    iekf = IteratedExtendedKalmanFilter(None, num_iterations=3, iteration_threshold=1e-4, **kw)
    assert isinstance(iekf, ExtendedKalmanFilter) and isinstance(ekf, KalmanFilter)
    for t in (ekf, iekf):
        assert t.time == -1 and t.lastUpdateT == -1 and not t.is_observed()
        assert numpy.array_equal(t.K_filter, 1.0e10 * numpy.identity(2)) and numpy.array_equal(t.K_predict, t.K_filter)
        assert numpy.array_equal(t.xk_filter, numpy.zeros(2))
        t.set_time(7)
        assert t.time == 7
        for m in ("next", "__iter__", "predict", "update", "calc_innovation", "filter_innovation", "adjust_boundaries", "within_room"):
            assert callable(getattr(t, m))
