"""CPU, dev container only (skipped where the reference tree is absent): the reference's unit_test/correlate.py against this
repository's `btk20` names.  The script does its work at import and cannot run as written, so it is NOT executed: it is parsed,
only its `from btk20.... import *` lines run, and then every keyword of every ...Ptr(...) call must be accepted -- by the table
generated from the reference's SWIG interface or by the alternates -- and every method it calls must exist.  The chain is also
constructed with the script's own keywords (no samples, no device).  The script's one undefined name is asserted to be exactly
`chirpSignal`: the test documents the defect instead of hiding it."""
import ast
import builtins
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/btk20_src/unit_test"
SCRIPT = "correlate.py"

pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is only mounted in the dev container")


def _load():
    tree = ast.parse(open(os.path.join(REF, SCRIPT)).read())
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    ns, ran = {}, []
    for node in tree.body:
        if isinstance(node, ast.ImportFrom) and node.module and node.module.startswith("btk20"):
            exec(compile(ast.Module(body=[node], type_ignores=[]), SCRIPT, "exec"), ns)
            ran.append(node.module)
    return ns, tree, ran


def test_imports_resolve_and_chirpSignal_is_the_one_undefined_name():
    ns, tree, ran = _load()
    assert ran == ["btk20.stream", "btk20.common", "btk20.feature", "btk20.convolution"]
    defined = set(ns) | set(dir(builtins))
    for n in ast.walk(tree):
        if isinstance(n, ast.Name) and isinstance(n.ctx, (ast.Store, ast.Del)):
            defined.add(n.id)
        elif isinstance(n, ast.arg):
            defined.add(n.arg)
        elif isinstance(n, ast.alias):
            defined.add((n.asname or n.name).split(".")[0])
        elif isinstance(n, ast.FunctionDef):
            defined.add(n.name)
    missing = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load) and n.id not in defined}
    assert missing == {"chirpSignal"}, sorted(missing)      # the script's own defect: it reads the chirp into impulseResponse
    for name in ("SampleFeaturePtr", "OverlapAddPtr", "OverlapSavePtr"):
        assert name in ns, name


def test_keywords_are_accepted():
    from distant_speech_recognition_amd.btk20cpp import _signatures as S, _signatures_alt as A
    ns, tree, _ = _load()
    bad, seen = [], {}
    for n in ast.walk(tree):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id.endswith("Ptr"):
            name = n.func.id
            assert name in S.CTORS, name
            tables = [{p for p, _ in S.CTORS[name]}] + ([{p for p, _ in A.CTOR_KWARGS[name]}] if name in A.CTOR_KWARGS else [])
            kws = {kw.arg for kw in n.keywords if kw.arg is not None}
            seen.setdefault(name, set()).update(kws)
            if not any(kws <= t for t in tables):           # one table must know all keywords of a call
                bad.append((name, sorted(kws)))
    assert not bad, bad
    assert seen == {"SampleFeaturePtr": {"blockLen", "shiftLen", "padZeros"}, "OverlapAddPtr": {"fftLen"}}
    assert "fftLen" in {p for p, _ in S.CTORS["OverlapAddPtr"]}                 # the generated table knows the script's keyword
    assert "blockLen" not in {p for p, _ in S.CTORS["SampleFeaturePtr"]}        # the legacy spellings are the alternates' business


def test_methods_exist():
    import copy
    import wave
    import distant_speech_recognition_amd.btk20 as b20
    ns, tree, _ = _load()
    mirror = set()
    for _, cls in inspect.getmembers(b20, inspect.isclass):
        mirror |= set(dir(cls))
    other = set(dir(copy)) | set(dir(wave)) | set(dir(np.ndarray))
    called = {n.func.attr for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}
    missing = sorted(a for a in called if a not in mirror and a not in other)
    assert not missing, missing
    assert {"read", "next"} <= called and {"read", "next"} <= mirror


def test_the_chain_constructs_with_the_scripts_keywords():
    from btk20.feature import SampleFeaturePtr
    from btk20.convolution import OverlapAddPtr
    from distant_speech_recognition_amd.btk20cpp import jdimension_error
    M = 2048
    chirpFeature = SampleFeaturePtr(blockLen=M, shiftLen=M, padZeros=True)
    assert chirpFeature.size() == M
    sampleFeature = SampleFeaturePtr(blockLen=M, shiftLen=M // 2, padZeros=1)       # the script's M/2 is Python 2's integer
    chirp = np.ones(M, np.float32)                          # what chirpFeature.next(0) hands out: a float32 vector of M samples
    # the script's fftLen = M is shorter than L + P - 1 = 2 M - 1: the reference's own check refuses it (convolution.cc:75-77)
    with pytest.raises(jdimension_error):
        OverlapAddPtr(sampleFeature, chirp, fftLen=M)
    overlapAdd = OverlapAddPtr(sampleFeature, chirp, fftLen=2 * M)
    assert overlapAdd.size() == M and overlapAdd.fftLen() == 2 * M and overlapAdd.taps() == M
    assert OverlapAddPtr(sampleFeature, chirp).fftLen() == 2 * M
