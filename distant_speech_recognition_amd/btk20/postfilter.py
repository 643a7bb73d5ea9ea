"""btk20.postfilter (postfilter/postfilter.i): the names of that reference module, resolved to the C++ node layer
(distant_speech_recognition_amd.btk20cpp = host/libbtk20hip.so bound with pybind11)."""
from ..btk20cpp import (  # noqa: F401
    TYPE_ZELINSKI1_REAL, TYPE_ZELINSKI1_ABS, TYPE_APAB, TYPE_ZELINSKI2, NO_USE_POST_FILTER, ZelinskiPostFilterPtr,
    ZelinskiPostFilter, McCowanPostFilterPtr, McCowanPostFilter, LefkimmiatisPostFilterPtr, LefkimmiatisPostFilter,
    SpectralSubtractorPtr, SpectralSubtractor, WienerFilterPtr, WienerFilter, HighPassFilterPtr, HighPassFilter,
    BinaryMaskFilterPtr, BinaryMaskFilter, KimBinaryMaskFilterPtr, KimBinaryMaskFilter, KimITDThresholdEstimatorPtr,
    KimITDThresholdEstimator, IIDBinaryMaskFilterPtr, IIDBinaryMaskFilter, IIDThresholdEstimatorPtr, IIDThresholdEstimator,
    FDIIDThresholdEstimatorPtr, FDIIDThresholdEstimator,
)

__all__ = ['TYPE_ZELINSKI1_REAL', 'TYPE_ZELINSKI1_ABS', 'TYPE_APAB', 'TYPE_ZELINSKI2', 'NO_USE_POST_FILTER', 'ZelinskiPostFilterPtr', 'ZelinskiPostFilter', 'McCowanPostFilterPtr', 'McCowanPostFilter', 'LefkimmiatisPostFilterPtr', 'LefkimmiatisPostFilter',
           'SpectralSubtractorPtr', 'SpectralSubtractor', 'WienerFilterPtr', 'WienerFilter', 'HighPassFilterPtr', 'HighPassFilter',
           'BinaryMaskFilterPtr', 'BinaryMaskFilter', 'KimBinaryMaskFilterPtr', 'KimBinaryMaskFilter', 'KimITDThresholdEstimatorPtr',
           'KimITDThresholdEstimator', 'IIDBinaryMaskFilterPtr', 'IIDBinaryMaskFilter', 'IIDThresholdEstimatorPtr', 'IIDThresholdEstimator',
           'FDIIDThresholdEstimatorPtr', 'FDIIDThresholdEstimator']
