"""btk20.sad (sad/sad.i): the names of that reference module, resolved to the C++ node layer
(distant_speech_recognition_amd.btk20cpp = host/libbtk20hip.so bound with pybind11).  Built: the energy family -- the metrics,
SimpleEnergyVAD and the hangover features; DESIGN section 7 lists what the module has beyond them."""
from ..btk20cpp import (  # noqa: F401
    VADMetricPtr, VADMetric, EnergyVADMetricPtr, EnergyVADMetric, PowerSpectrumVADMetricPtr, PowerSpectrumVADMetric,
    NormalizedEnergyMetricPtr, NormalizedEnergyMetric, TSPSVADMetricPtr, TSPSVADMetric, VADPtr, VAD, SimpleEnergyVADPtr,
    SimpleEnergyVAD, HangoverVADFeaturePtr, HangoverVADFeature, HangoverMIVADFeaturePtr, HangoverMIVADFeature,
    HangoverMultiStageVADFeaturePtr, HangoverMultiStageVADFeature,
)

__all__ = ['VADMetricPtr', 'VADMetric', 'EnergyVADMetricPtr', 'EnergyVADMetric', 'PowerSpectrumVADMetricPtr',
           'PowerSpectrumVADMetric', 'NormalizedEnergyMetricPtr', 'NormalizedEnergyMetric', 'TSPSVADMetricPtr',
           'TSPSVADMetric', 'VADPtr', 'VAD', 'SimpleEnergyVADPtr', 'SimpleEnergyVAD', 'HangoverVADFeaturePtr',
           'HangoverVADFeature', 'HangoverMIVADFeaturePtr', 'HangoverMIVADFeature', 'HangoverMultiStageVADFeaturePtr',
           'HangoverMultiStageVADFeature']
