"""btk20.modulated (modulated/modulated.i:46-305, :477-478): the names of that reference module, resolved to the C++ node layer
(distant_speech_recognition_amd.btk20cpp = host/libbtk20hip.so bound with pybind11).  The prototype designers of that module
(CosineModulatedPrototypeDesign, the de Haan and Nyquist(M) classes) are not part of the engine."""
from ..btk20cpp import (  # noqa: F401
    OverSampledDFTAnalysisBankPtr, OverSampledDFTSynthesisBankPtr, OverSampledDFTAnalysisBank,
    OverSampledDFTSynthesisBank,
    NormalFFTAnalysisBankPtr, NormalFFTAnalysisBank, PerfectReconstructionFFTAnalysisBankPtr, PerfectReconstructionFFTAnalysisBank,
    PerfectReconstructionFFTSynthesisBankPtr, PerfectReconstructionFFTSynthesisBank, DelayFeaturePtr, DelayFeature, get_window,
)

__all__ = ['OverSampledDFTAnalysisBankPtr', 'OverSampledDFTSynthesisBankPtr', 'OverSampledDFTAnalysisBank', 'OverSampledDFTSynthesisBank',
           'NormalFFTAnalysisBankPtr', 'NormalFFTAnalysisBank', 'PerfectReconstructionFFTAnalysisBankPtr',
           'PerfectReconstructionFFTAnalysisBank', 'PerfectReconstructionFFTSynthesisBankPtr', 'PerfectReconstructionFFTSynthesisBank',
           'DelayFeaturePtr', 'DelayFeature', 'get_window']
