"""btk20.feature (feature/feature.i): the names of that reference module, resolved to the C++ node layer
(distant_speech_recognition_amd.btk20cpp = host/libbtk20hip.so bound with pybind11)."""
from ..btk20cpp import (  # noqa: F401
    SampleFeaturePtr, SampleFeature, HammingFeaturePtr, HammingFeature, FFTFeaturePtr, FFTFeature,
    PreemphasisFeaturePtr, PreemphasisFeature, SpectralPowerFeaturePtr, SpectralPowerFeature, SpectralPowerFloatFeaturePtr, SpectralPowerFloatFeature, VTLNFeaturePtr, VTLNFeature, MelFeaturePtr, MelFeature, LogFeaturePtr, LogFeature, CepstralFeaturePtr, CepstralFeature, StorageFeaturePtr, StorageFeature,
)

__all__ = ['SampleFeaturePtr', 'SampleFeature', 'HammingFeaturePtr', 'HammingFeature', 'FFTFeaturePtr', 'FFTFeature',
           'PreemphasisFeaturePtr', 'PreemphasisFeature', 'SpectralPowerFeaturePtr', 'SpectralPowerFeature', 'SpectralPowerFloatFeaturePtr', 'SpectralPowerFloatFeature', 'VTLNFeaturePtr', 'VTLNFeature', 'MelFeaturePtr', 'MelFeature', 'LogFeaturePtr', 'LogFeature', 'CepstralFeaturePtr', 'CepstralFeature', 'StorageFeaturePtr', 'StorageFeature']
