"""CPU, dev container only (skipped where the reference tree is absent): the reference's unit_test/log_power_extractor.py and
unit_test/mfcc_extractor.py against this repository's `btk20` names.  Both scripts do their work at import, so they are NOT
executed: they are parsed, only their `from btk20.... import *` lines run, and then every name they load must resolve, every
keyword of every ...Ptr(...) call must be in the table generated from the reference's SWIG interface, and every method they call
must exist.  The two chains are also constructed with the scripts' own keywords (no samples, no device)."""
import ast
import builtins
import inspect
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/btk20_src/unit_test"
SCRIPTS = ["log_power_extractor.py", "mfcc_extractor.py"]

pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is only mounted in the dev container")


def _load(script):
    tree = ast.parse(open(os.path.join(REF, script)).read())
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    ns = {}
    for node in tree.body:
        if isinstance(node, ast.ImportFrom) and node.module and node.module.startswith("btk20"):
            exec(compile(ast.Module(body=[node], type_ignores=[]), script, "exec"), ns)
    return ns, tree


@pytest.mark.parametrize("script", SCRIPTS)
def test_names_resolve(script):
    ns, tree = _load(script)
    defined = set(ns) | set(dir(builtins))
    for n in ast.walk(tree):
        if isinstance(n, ast.Name) and isinstance(n.ctx, (ast.Store, ast.Del)):
            defined.add(n.id)
        elif isinstance(n, ast.arg):
            defined.add(n.arg)
        elif isinstance(n, ast.alias):
            defined.add((n.asname or n.name).split(".")[0])
    missing = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load) and n.id not in defined}
    assert not missing, "names %s uses that btk20 lacks: %s" % (script, sorted(missing))
    for name in ("SampleFeaturePtr", "HammingFeaturePtr", "FFTFeaturePtr", "SpectralPowerFeaturePtr", "LogFeaturePtr"):
        assert name in ns, name


@pytest.mark.parametrize("script", SCRIPTS)
def test_keywords_are_in_the_generated_table(script):
    from distant_speech_recognition_amd.btk20cpp import _signatures as S
    ns, tree = _load(script)
    bad, checked = [], 0
    for n in ast.walk(tree):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id.endswith("Ptr"):
            assert n.func.id in S.CTORS, n.func.id
            accepted = {p for p, _ in S.CTORS[n.func.id]}
            checked += 1
            bad += [(n.func.id, kw.arg) for kw in n.keywords if kw.arg is not None and kw.arg not in accepted]
    assert not bad, bad
    assert checked >= (10 if script.startswith("mfcc") else 5)


@pytest.mark.parametrize("script", SCRIPTS)
def test_methods_exist(script):
    import pickle
    import numpy
    import distant_speech_recognition_amd.btk20 as b20
    ns, tree = _load(script)
    mirror = set()
    for _, cls in inspect.getmembers(b20, inspect.isclass):
        mirror |= set(dir(cls))
    other = set()
    for o in (str, numpy, numpy.ndarray, pickle, type(open(os.devnull))):
        other |= set(dir(o))
    called = {n.func.attr for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}
    missing = sorted(a for a in called if a not in mirror and a not in other)
    assert not missing, missing
    assert "read" in called and "read" in mirror


def test_the_two_chains_construct_with_the_scripts_keywords():
    from btk20.feature import (SampleFeaturePtr, StorageFeaturePtr, HammingFeaturePtr, FFTFeaturePtr, SpectralPowerFeaturePtr,
                               VTLNFeaturePtr, MelFeaturePtr, LogFeaturePtr, CepstralFeaturePtr)
    D, fft_len = 160, 256
    pow_num = fft_len // 2 + 1
    # log_power_extractor.py
    samplefe = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=False)
    hammingfe = HammingFeaturePtr(samplefe)
    fftfe = FFTFeaturePtr(hammingfe, fft_len=fft_len)
    powerfe = SpectralPowerFeaturePtr(fftfe, pow_num=pow_num)
    logfe = LogFeaturePtr(powerfe)
    assert [n.size() for n in (samplefe, fftfe, powerfe, logfe)] == [160, 256, 129, 129]
    # mfcc_extractor.py
    samplefe = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=False)
    sample_storage = StorageFeaturePtr(samplefe)
    hammingfe = HammingFeaturePtr(sample_storage)
    fftfe = FFTFeaturePtr(hammingfe, fft_len=fft_len)
    powerfe = SpectralPowerFeaturePtr(fftfe, pow_num=pow_num)
    vtlnfe = VTLNFeaturePtr(powerfe, coeff_num=pow_num, edge=0.8, version=2)
    melfe = MelFeaturePtr(vtlnfe, pow_num=pow_num, filter_num=30, rate=16000.0, low=100.0, up=6800.0, version=2)
    logfe = LogFeaturePtr(powerfe)
    cepfe = CepstralFeaturePtr(logfe, ncep=13)
    cep_storage = StorageFeaturePtr(cepfe)
    assert [n.size() for n in (samplefe, fftfe, powerfe, vtlnfe, melfe, logfe, cepfe)] == [160, 256, 129, 129, 30, 129, 13]
    assert sample_storage.size() == 160 and cep_storage.size() == 13
    assert melfe.matrix().shape == (30, 129) and vtlnfe.matrix().shape == (129, 129) and cepfe.matrix().shape == (13, 129)
    # the refusals of the reference's constructors
    from distant_speech_recognition_amd.btk20cpp import j_error
    with pytest.raises(j_error):
        SpectralPowerFeaturePtr(fftfe, pow_num=100)
    with pytest.raises(j_error):
        MelFeaturePtr(powerfe, pow_num=pow_num, low=-1.0)
    with pytest.raises(j_error):
        CepstralFeaturePtr(logfe, ncep=13, type=3)
    with pytest.raises(j_error):
        melfe.read("no_such_file")
