"""btk20.localization (localization/localization.i:128-260): the names of that reference module, resolved to the C++ node layer
(distant_speech_recognition_amd.btk20cpp = host/libbtk20hip.so bound with pybind11): the search-grid builders and the
multichannel cross-correlation localiser and calculator over csrc/mcc_kernels.hip.  Not carried over: the GCC*
classes, SGB4CircularArray (its far-field walk does not end) and RMCCLocalizer (its next() is empty)."""
from ..btk20cpp import (SearchGridBuilderPtr, SearchGridBuilder, SGB4LinearArrayPtr, SGB4LinearArray, MCCLocalizerPtr,  # noqa: F401
                        MCCLocalizer, MCCCalculatorPtr, MCCCalculator)

__all__ = ['SearchGridBuilderPtr', 'SearchGridBuilder', 'SGB4LinearArrayPtr', 'SGB4LinearArray', 'MCCLocalizerPtr', 'MCCLocalizer',
           'MCCCalculatorPtr', 'MCCCalculator']
