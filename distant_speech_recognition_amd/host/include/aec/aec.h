// aec/aec.h -- subband acoustic echo cancellers with the reference's class names, constructors and *Ptr typedefs
// (reference aec/aec.h:34-329, aec/aec.cc), computed through btk_aec_process of libbtkhip:
//   NLMSAcousticEchoCancellationFeature, KalmanFilterEchoCancellationFeature, BlockKalmanFilterEchoCancellationFeature,
//   DTDBlockKalmanFilterEchoCancellationFeature.
// A node pulls its two sources in blocks (modulated/modulated.h, BlockSource): two analysis banks hand their sample windows over
// and the block of subband frames is computed where the canceller runs; any other pair of sources is drained through next().  The
// residual block stays on the device for a synthesis bank (device_block) and is served frame by frame from a host mirror, so
// next() keeps the reference's contract: same-frame caching, jindex_error on a non-consecutive explicit frame number,
// jiterator_error at the end of either source.  reset() follows aec.h:41,78,111-114: the one-tap filters zero their weights, the
// block filters reset their sources only -- weights, covariances, noise variances and the played history live on.
//
// Stated deviations: the NLMS filter starts at zero (the reference reads it uninitialised until the first reset()); the
// double-talk node opens no debug file and prints nothing in its destructor; state is kept for the bins 0..M/2 only.
// InformationFilterEchoCancellationFeature and SquareRootInformationFilterEchoCancellationFeature are not provided.
#pragma once
#include <vector>

#include "stream/stream.h"
#include "modulated/modulated.h"
#include "common/devmem.h"

class AcousticEchoCancellationNode_ : public VectorComplexFeatureStream, public BlockSource {
 public:
  virtual const gsl_vector_complex* next(int frame_no = -5);
  virtual void reset();
  // frames per block when the sources are drained through next() (analysis banks bring their own block_frames())
  void set_block_frames(long n) { block_frames_ = n < 0 ? 0 : n; }
  long block_frames() const { return block_frames_; }
  unsigned sample_num() const { return sampleN_; }
  // BlockSource: see modulated/modulated.h.  A consumer that takes blocks never calls next(), so the double-talk detector sees
  // the frame number a reference consumer hands over with next()'s default argument: -5 on every frame (aec.cc:902).
  virtual unsigned long block_version() { return 0; }
  virtual const std::vector<float>& block(long& T);
  virtual const void* device_block(long& T, long& T_stride);
  virtual long block_base();
  virtual bool next_block();
  virtual void advance_to(long) {}
  // Engine-specific, not in the reference's classes (which keep these members private): the adaptive state of one bin, complex128
  // [P] resp. [P][P], interleaved re / im.  A node computes a whole block ahead of next(), so these return the state AFTER THE
  // LAST FRAME OF THE CURRENT BLOCK, not after the frame last served (set_block_frames(1) makes the two coincide for sources that
  // are drained through next()); before the first block they return the constructor's values.
  std::vector<double> filter_coefficients(unsigned fbinX);
  std::vector<double> state_covariance(unsigned fbinX);
  double observation_noise_variance(unsigned fbinX);
 protected:
  AcousticEchoCancellationNode_(int kind, const VectorComplexFeatureStreamPtr& played, const VectorComplexFeatureStreamPtr& recorded,
                                unsigned sampleN, const double* params8, const String& nm);
 private:
  void alloc_state_();
  bool load_block_(long frame_arg);             // the next block of both sources through the canceller; false: a source has ended
  bool load_from_banks_(long& Tn);
  bool load_by_next_(long& Tn);
  const float* host_output_();
  void ensure_first_(long frame_arg);
  const int kind_;
  VectorComplexFeatureStreamPtr played_, recorded_;
  OverSampledDFTAnalysisBank *pbank_, *rbank_;  // both sources are analysis banks: their windows are handed over
  const unsigned fftLen_, sampleN_;
  double params_[8];
  long block_frames_;
  bool prepared_, ended_, state_ready_;
  long base_, T_, Ts_;                          // the current block: stream index of its first frame, frames, row stride
  long block_frame_arg_;                        // the frame number the block was computed for (< 0: that value on every frame)
  DeviceBuffer dV_, dA_, dE_, dPcmV_, dPcmA_;
  PinnedBuffer hV_, hA_;
  std::vector<float> Ehost_, dense_;              // host mirror of the block [K][Ts_]; its dense copy [K][T_] for block()
  bool Ehost_valid_;
  DeviceBuffer dR_, dK_, dSig_, dHist_, dDtd_;     // the recursion's state (alloc_state_)
};

class NLMSAcousticEchoCancellationFeature : public AcousticEchoCancellationNode_ {
 public:
  NLMSAcousticEchoCancellationFeature(const VectorComplexFeatureStreamPtr& original, const VectorComplexFeatureStreamPtr& distorted,
                                      double delta = 100.0, double epsilon = 1.0E-04, double threshold = 100.0, const String& nm = "AEC");
};
typedef Inherit<NLMSAcousticEchoCancellationFeature, VectorComplexFeatureStreamPtr> NLMSAcousticEchoCancellationFeaturePtr;

class KalmanFilterEchoCancellationFeature : public AcousticEchoCancellationNode_ {
 public:
  KalmanFilterEchoCancellationFeature(const VectorComplexFeatureStreamPtr& played, const VectorComplexFeatureStreamPtr& recorded,
                                      double beta = 0.95, double sigma2 = 100.0, double threshold = 100.0, const String& nm = "KFEchoCanceller");
};
typedef Inherit<KalmanFilterEchoCancellationFeature, VectorComplexFeatureStreamPtr> KalmanFilterEchoCancellationFeaturePtr;

class BlockKalmanFilterEchoCancellationFeature : public AcousticEchoCancellationNode_ {
 public:
  BlockKalmanFilterEchoCancellationFeature(const VectorComplexFeatureStreamPtr& played, const VectorComplexFeatureStreamPtr& recorded,
                                           unsigned sampleN = 1, double beta = 0.95, double sigmau2 = 10e-4, double sigmauk2 = 5.0,
                                           double threshold = 100.0, double amp4play = 1.0, const String& nm = "KFEchoCanceller");
 protected:
  BlockKalmanFilterEchoCancellationFeature(int kind, const VectorComplexFeatureStreamPtr& played, const VectorComplexFeatureStreamPtr& recorded,
                                           unsigned sampleN, const double* params8, const String& nm);
};
typedef Inherit<BlockKalmanFilterEchoCancellationFeature, VectorComplexFeatureStreamPtr> BlockKalmanFilterEchoCancellationFeaturePtr;

class DTDBlockKalmanFilterEchoCancellationFeature : public BlockKalmanFilterEchoCancellationFeature {
 public:
  DTDBlockKalmanFilterEchoCancellationFeature(const VectorComplexFeatureStreamPtr& played, const VectorComplexFeatureStreamPtr& recorded,
                                              unsigned sampleN = 1, double beta = 0.95, double sigmau2 = 10e-4, double sigmauk2 = 5.0,
                                              double snrTh = 2.0, double engTh = 100.0, double smooth = 0.9, double amp4play = 1.0,
                                              const String& nm = "DTDKFEchoCanceller");
};
typedef Inherit<DTDBlockKalmanFilterEchoCancellationFeature, BlockKalmanFilterEchoCancellationFeaturePtr> DTDBlockKalmanFilterEchoCancellationFeaturePtr;
