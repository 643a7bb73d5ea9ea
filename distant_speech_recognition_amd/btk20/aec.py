"""btk20.aec (aec/aec.i): the names of that reference module, resolved to the C++ node layer
(distant_speech_recognition_amd.btk20cpp = host/libbtk20hip.so bound with pybind11).

InformationFilterEchoCancellationFeaturePtr and SquareRootInformationFilterEchoCancellationFeaturePtr are not provided: they share
one skip counter across all bins and frames, use a function-local static loading constant and invert through an eigen-solver, none
of which this engine can pin to a reference result."""
from ..btk20cpp import (  # noqa: F401
    NLMSAcousticEchoCancellationFeaturePtr, KalmanFilterEchoCancellationFeaturePtr,
    BlockKalmanFilterEchoCancellationFeaturePtr, DTDBlockKalmanFilterEchoCancellationFeaturePtr,
)

__all__ = ['NLMSAcousticEchoCancellationFeaturePtr', 'KalmanFilterEchoCancellationFeaturePtr',
           'BlockKalmanFilterEchoCancellationFeaturePtr', 'DTDBlockKalmanFilterEchoCancellationFeaturePtr']
