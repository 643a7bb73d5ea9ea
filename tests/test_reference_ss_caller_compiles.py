"""Skipped where the reference tree is absent: the reference's C++ main of the spectral subtractor, src/ss.cc,
compiles against the node layer's headers where it lies under /root/reference -- nothing of it is copied.  The rule of
tests/test_reference_cpp_callers_compile.py with a pattern of its own: the only diagnostics allowed are libsndfile's names (this
caller writes 16-bit samples with sf_writef_short) and powi()."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/btk20_src/src"
ALLOWED = re.compile(r"sndfile|SF_INFO|sfinfo|SNDFILE|waveFP|SFM_WRITE|sf_open|sf_writef_short|sf_close|powi")


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="the reference tree is absent")
def test_ss_cc_compiles_against_the_node_headers():
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-DENABLE_LEGACY_BTK_API",
           "-I" + os.path.join(ROOT, "distant_speech_recognition_amd", "host", "include"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(REF_SRC, "ss.cc")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    errors = [l for l in res.stderr.splitlines() if " error: " in l or "fatal error" in l]
    unexpected = [l for l in errors if not ALLOWED.search(l)]
    assert not unexpected, "\n".join(unexpected)
    assert errors, "expected the libsndfile diagnostics (is libsndfile installed now? then tighten this test)"
    assert not any("spectralsubtraction.h" in l for l in errors)
