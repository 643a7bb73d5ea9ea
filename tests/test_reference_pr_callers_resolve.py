"""CPU, dev container only (skipped where the reference tree is absent): the constructor calls of the reference's
tools/filterbank/test_pr_filter_prototype.py against this repository's `btk20` names.  The script is Python 2 (print statements,
`from btk.... import *`) and does its work at import, so it is NOT executed or parsed as Python 3: its ...Ptr(...) calls are read
from the text, every name must be exported by btk20, every keyword accepted by the table generated from the reference's SWIG
interface or by the alternates, and the chain is constructed with the script's own arguments (no samples, no device)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = "/root/reference/btk20_src/tools/filterbank/test_pr_filter_prototype.py"

pytestmark = pytest.mark.skipif(not os.path.isfile(SCRIPT), reason="the reference tree is only mounted in the dev container")


def _calls():
    """[(name, [positional], {keyword: text})] of the ...Ptr( calls, innermost included."""
    text = open(SCRIPT).read()
    out = []
    for mt in re.finditer(r"(\w+Ptr)\s*\(", text):
        depth, j = 1, mt.end()
        while depth:
            depth += text[j] == "("
            depth -= text[j] == ")"
            j += 1
        args, cur, d = [], "", 0
        for ch in text[mt.end():j - 1]:
            d += ch == "("
            d -= ch == ")"
            if ch == "," and d == 0:
                args.append(cur.strip()); cur = ""
            else:
                cur += ch
        if cur.strip():
            args.append(cur.strip())
        pos = [a for a in args if not re.match(r"^\w+\s*=[^=]", a)]
        kws = dict(re.split(r"\s*=\s*", a, maxsplit=1) for a in args if re.match(r"^\w+\s*=[^=]", a))
        out.append((mt.group(1), pos, kws))
    return out


def test_names_and_keywords_resolve():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import btk20.feature, btk20.modulated, btk20.stream
    from distant_speech_recognition_amd.btk20cpp import _signatures as S, _signatures_alt as A
    calls = _calls()
    assert [c[0] for c in calls] == ["SampleFeaturePtr", "PerfectReconstructionFFTAnalysisBankPtr",
                                     "PerfectReconstructionFFTSynthesisBankPtr", "PyVectorComplexFeatureStreamPtr"]
    exported = set(btk20.feature.__all__) | set(btk20.modulated.__all__) | set(btk20.stream.__all__)
    for name, pos, kws in calls:
        assert name in exported and name in S.CTORS, name
        tables = [[p for p, _ in S.CTORS[name]]] + ([[p for p, _ in A.CTOR_KWARGS[name]]] if name in A.CTOR_KWARGS else [])
        assert any(set(kws) <= set(t) and len(pos) + len(kws) <= len(t) and not set(t[:len(pos)]) & set(kws) for t in tables), (name, pos, kws)
    by = {c[0]: c for c in calls}
    assert set(by["SampleFeaturePtr"][2]) == {"blockLen", "shiftLen", "padZeros"}
    assert by["PerfectReconstructionFFTAnalysisBankPtr"][1] == ["sampleFeature", "prototype", "M", "m", "r"]
    assert by["PerfectReconstructionFFTSynthesisBankPtr"][1] == ["PyVectorComplexFeatureStreamPtr(analysisFB)", "prototype", "M", "m", "r"]


@pytest.mark.parametrize("M", [256, 512])
@pytest.mark.parametrize("m", [2, 4])
def test_the_chain_constructs_with_the_scripts_arguments(M, m):
    from btk20.feature import SampleFeaturePtr
    from btk20.modulated import PerfectReconstructionFFTAnalysisBankPtr, PerfectReconstructionFFTSynthesisBankPtr
    from btk20.stream import PyVectorComplexFeatureStreamPtr
    r = 0
    D = M // 2 ** r
    prototype = np.ones(2 * M * m)
    sampleFeature = SampleFeaturePtr(blockLen=D, shiftLen=D, padZeros=True)
    analysisFB = PerfectReconstructionFFTAnalysisBankPtr(sampleFeature, prototype, M, m, r)
    synthesisFB = PerfectReconstructionFFTSynthesisBankPtr(PyVectorComplexFeatureStreamPtr(analysisFB), prototype, M, m, r)
    assert analysisFB.size() == 2 * M and synthesisFB.size() == D
    by_kw = PerfectReconstructionFFTSynthesisBankPtr(samp=PyVectorComplexFeatureStreamPtr(c=analysisFB), prototype=prototype, M=M, m=m, r=r)
    assert by_kw.size() == D
    assert PerfectReconstructionFFTAnalysisBankPtr(samp=sampleFeature, prototype=prototype, M=M, m=m, r=r).size() == 2 * M
