"""btk20.objective_measure (objective_measure/objective_measure.i): the names of that reference module, resolved to the C++
node layer (distant_speech_recognition_amd.btk20cpp = host/libbtk20hip.so bound with pybind11): the signal-to-noise ratio and
the Itakura-Saito distance over power spectra.  The reference's segmentalSNR class is empty; engine.segmental_snr is this
project's own."""
from ..btk20cpp import SNRPtr, SNR, ItakuraSaitoMeasurePSPtr, ItakuraSaitoMeasurePS  # noqa: F401

__all__ = ['SNRPtr', 'SNR', 'ItakuraSaitoMeasurePSPtr', 'ItakuraSaitoMeasurePS']
