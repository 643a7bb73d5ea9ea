"""btk20.beamformer (beamformer/beamformer.i): the names of that reference module, resolved to the C++ node layer
(distant_speech_recognition_amd.btk20cpp = host/libbtk20hip.so bound with pybind11)."""
from ..btk20cpp import (  # noqa: F401
    SSPEED, SnapShotArrayPtr, SpectralMatrixArrayPtr, SubbandDSPtr, SubbandGSCPtr, SubbandGSCRLSPtr, SubbandMVDRPtr,
    SubbandMVDRGSCPtr, SubbandDS, SubbandGSC, SubbandGSCRLS, SubbandMVDR, SubbandMVDRGSC, calc_all_delays,
    DOAEstimatorSRPBasePtr, DOAEstimatorSRPDSBLAPtr, DOAEstimatorSRPBase, DOAEstimatorSRPDSBLA,
)

__all__ = ['SSPEED', 'SnapShotArrayPtr', 'SpectralMatrixArrayPtr', 'SubbandDSPtr', 'SubbandGSCPtr', 'SubbandGSCRLSPtr', 'SubbandMVDRPtr', 'SubbandMVDRGSCPtr', 'SubbandDS', 'SubbandGSC', 'SubbandGSCRLS', 'SubbandMVDR', 'SubbandMVDRGSC', 'calc_all_delays',
           'DOAEstimatorSRPBasePtr', 'DOAEstimatorSRPDSBLAPtr', 'DOAEstimatorSRPBase', 'DOAEstimatorSRPDSBLA']
