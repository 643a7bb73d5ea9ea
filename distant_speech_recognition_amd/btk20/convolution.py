"""btk20.convolution (convolution/convolution.i): the names of that reference module, resolved to the C++ node layer
(distant_speech_recognition_amd.btk20cpp = host/libbtk20hip.so bound with pybind11)."""
from ..btk20cpp import OverlapAddPtr, OverlapAdd, OverlapSavePtr, OverlapSave  # noqa: F401

__all__ = ['OverlapAddPtr', 'OverlapAdd', 'OverlapSavePtr', 'OverlapSave']
