// postfilter/binauralprocessing.h -- BinaryMaskFilter, KimBinaryMaskFilter, KimITDThresholdEstimator, IIDBinaryMaskFilter,
// IIDThresholdEstimator, FDIIDThresholdEstimator with the reference's interface (postfilter/binauralprocessing.h:27-211) over
// btk_binaural_mask / btk_binaural_stats / btk_binaural_threshold (csrc/binaural_kernels.hip).
//
// The nodes combine two subband streams -- in the reference the outputs of two beamformers steered at the target and at the
// interferer -- into one, on the block machinery of postfilter/enhancement_node.h: both sources are gathered block by block on
// the device (analysis banks, BlockSource nodes device to device, anything else drained through next()), the result is offered
// to a synthesis bank through device_block().  set_threshold() / set_thresholds() are mode switches mid-stream: frames a
// per-frame graph would have pulled before the call keep the old threshold, later ones get the new one.
//
// An estimator's next() returns the node's own vector, which the reference never writes: zeros.  Its sums live on the device
// and grow block by block; calc_threshold() and cost_function() read them as they stand at the frame a per-frame graph would
// have reached (begin_peek_()).
//
// Kept as in the reference:
//   * reset() of the mask filters leaves prevMu_ as it is; reset() of the estimators clears the sums.
//   * IIDBinaryMaskFilter with per-bin thresholds leaves threshold() at the last bin's value once a frame has been computed;
//     KimBinaryMaskFilter ignores per-bin thresholds.
//   * Kim's default range is +-0.2 x 16000 / 340 whatever the sample rate; FD-IID's +-100000 in steps of 1000.
//   * min_fbinX_ / max_fbinX_ = (unsigned)(M x freq / (float)sampleRate), in float.
//   * BinaryMaskFilter::next() itself only counts frames.
//   * The candidates are the float32 walk `for(float t=min;t<=max;t+=width)`; the arrays have (int)((max-min)/width+1.5) slots.
// Deviations:
//   * set_thresholds() copies on its first call too (the reference only allocates there: uninitialised values).
//   * FDIIDThresholdEstimator uses beta = 3.0 (the reference never initialises its _beta).
//   * calc_threshold() is idempotent and accumulation may go on after it (the reference divides its sums in place).
//   * max_fbinX_ > M/2 + 1, a range beyond Nyquist which reads outside the vectors there, is a jdimension_error.
//   * A candidate walk longer than its arrays, with which the reference writes past them, is cut at their size.
//   * masking1() / accumStats1() on single host frames are not offered: the frames are computed in blocks on the device.
#ifndef BINAURALPROCESSING_H
#define BINAURALPROCESSING_H

#include <vector>

#include "postfilter/enhancement_node.h"

class BinaryMaskFilter : public EnhancementBlockNode_ {
 public:
  BinaryMaskFilter(unsigned chanX, VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M,
                   float threshold, float alpha, float dEta = 0.01, const String& nm = "BinaryMaskFilter");
  virtual ~BinaryMaskFilter();
  virtual const gsl_vector_complex* next(int frame_no = -5);
  void set_threshold(float threshold);
  void set_thresholds(const gsl_vector* thresholds);
  double threshold() { return threshold_; }
  gsl_vector* thresholds() { return threshold_per_freq_; }
  void setThreshold(float threshold) { set_threshold(threshold); }                               // ENABLE_LEGACY_BTK_API aliases
  void setThresholds(const gsl_vector* thresholds) { set_thresholds(thresholds); }
  double getThreshold() { return threshold(); }
  gsl_vector* getThresholds() { return thresholds(); }
  // engine-specific: prevMu_ as the stream stands, float32 [M/2 + 1] (bin 0 is never touched); empty for the estimators
  std::vector<float> prev_mu();
 protected:
  virtual size_t state_bytes_() const;
  virtual void init_state_(void* d);
  virtual void launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long frames_done);
  void zero_output_(void* dOut, long Ts, long t0, long t1);
  int mask_kind_;                       // BTK_BINAURAL_KIM / BTK_BINAURAL_IID; -1: the base class, which masks nothing
  unsigned chanX_;
  float alpha_, dEta_, threshold_;
  gsl_vector* threshold_per_freq_;
  DeviceBuffer dThresholds_;            // float32 [M/2 + 1], what the kernel reads of threshold_per_freq_
};
typedef Inherit<BinaryMaskFilter, VectorComplexFeatureStreamPtr> BinaryMaskFilterPtr;

class KimBinaryMaskFilter : public BinaryMaskFilter {
 public:
  KimBinaryMaskFilter(unsigned chanX, VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M,
                      float threshold, float alpha, float dEta = 0.01, float dPowerCoeff = 1 / 15.0,
                      const String& nm = "KimBinaryMaskFilter");
  virtual const gsl_vector_complex* next(int frame_no = -5);
 protected:
  float dpower_coeff_;
};
typedef Inherit<KimBinaryMaskFilter, BinaryMaskFilterPtr> KimBinaryMaskFilterPtr;

class IIDBinaryMaskFilter : public BinaryMaskFilter {
 public:
  IIDBinaryMaskFilter(unsigned chanX, VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M,
                      float threshold, float alpha, float dEta = 0.01, const String& nm = "IIDBinaryMaskFilter");
  virtual const gsl_vector_complex* next(int frame_no = -5);
};
typedef Inherit<IIDBinaryMaskFilter, BinaryMaskFilterPtr> IIDBinaryMaskFilterPtr;

// the sums of an estimator on the device and what reads them: shared by the Kim / IID chain and the FD-IID class
class BinauralSums_ {
 public:
  BinauralSums_() : kind(0), M(0), nCand(0), nWalk(0), uploaded_(false) {}
  void init(int kind, unsigned M, float lo, float hi, float width);
  size_t state_bytes() const;           // float64 sums | int64 frame count
  void accumulate(const void* dXL, const void* dXR, long Ts, long T, float eta, float pc, unsigned k0, unsigned k1, void* state);
  // calc_threshold on the sums at `state` (device): cost [nCand] (FD-IID [K][nCand]), per_bin [K] (FD-IID only)
  double threshold(const void* state, double beta, std::vector<double>& cost, std::vector<double>* per_bin);
  int kind;
  unsigned M, nCand, nWalk;
  std::vector<float> cands;
 private:
  DeviceBuffer dCands_, dScratch_;
  bool uploaded_;
};

class KimITDThresholdEstimator : public KimBinaryMaskFilter {
 public:
  KimITDThresholdEstimator(VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M,
                           float minThreshold = 0, float maxThreshold = 0, float width = 0.02, float minFreq = -1, float maxFreq = -1,
                           int sampleRate = -1, float dEta = 0.01, float dPowerCoeff = 1 / 15.0,
                           const String& nm = "KimITDThresholdEstimator");
  virtual ~KimITDThresholdEstimator();
  virtual const gsl_vector_complex* next(int frame_no = -5);
  virtual void reset();
  virtual double calc_threshold();
  const gsl_vector* cost_function();
  virtual double calcThreshold() { return calc_threshold(); }                                    // ENABLE_LEGACY_BTK_API aliases
  const gsl_vector* getCostFunction() { return cost_function(); }
  // engine-specific
  unsigned num_candidates() const { return sums_.nCand; }
  const std::vector<float>& candidates() const { return sums_.cands; }
  unsigned min_fbin() const { return min_fbinX_; }
  unsigned max_fbin() const { return max_fbinX_; }
  unsigned num_samples();               // nSamples_ as the stream stands
 protected:
  KimITDThresholdEstimator(int kind, VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M,
                           float minThreshold, float maxThreshold, float width, float minFreq, float maxFreq, int sampleRate,
                           float dEta, float dPowerCoeff, const String& nm);
  virtual size_t state_bytes_() const;
  virtual void init_state_(void* d);
  virtual void launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long frames_done);
  virtual double beta_() const { return 3.0; }
  float min_threshold_, max_threshold_, width_;
  unsigned min_fbinX_, max_fbinX_;
  BinauralSums_ sums_;
  gsl_vector* buffer_;
  bool cost_func_computed_;
 private:
  void setup_(int kind, unsigned M, float minThreshold, float maxThreshold, float width, float minFreq, float maxFreq, int sampleRate);
};
typedef Inherit<KimITDThresholdEstimator, KimBinaryMaskFilterPtr> KimITDThresholdEstimatorPtr;

class IIDThresholdEstimator : public KimITDThresholdEstimator {
 public:
  IIDThresholdEstimator(VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M, float minThreshold = 0,
                        float maxThreshold = 0, float width = 0.02, float minFreq = -1, float maxFreq = -1, int sampleRate = -1,
                        float dEta = 0.01, float dPowerCoeff = 0.5, const String& nm = "IIDThresholdEstimator");
};
typedef Inherit<IIDThresholdEstimator, KimITDThresholdEstimatorPtr> IIDThresholdEstimatorPtr;

class FDIIDThresholdEstimator : public BinaryMaskFilter {
 public:
  FDIIDThresholdEstimator(VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M, float minThreshold = 0,
                          float maxThreshold = 0, float width = 1000, float dEta = 0.01, float dPowerCoeff = 1 / 15.0,
                          const String& nm = "FDIIDThresholdEstimator");
  virtual ~FDIIDThresholdEstimator();
  virtual const gsl_vector_complex* next(int frame_no = -5);
  virtual void reset();
  virtual double calc_threshold();
  const gsl_vector* cost_function(unsigned freqX);
  virtual double calcThreshold() { return calc_threshold(); }                                    // ENABLE_LEGACY_BTK_API aliases
  const gsl_vector* getCostFunction(unsigned freqX) { return cost_function(freqX); }
  // engine-specific
  unsigned num_candidates() const { return sums_.nCand; }
  const std::vector<float>& candidates() const { return sums_.cands; }
 protected:
  virtual size_t state_bytes_() const;
  virtual void init_state_(void* d);
  virtual void launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long frames_done);
  float min_threshold_, max_threshold_, width_, dpower_coeff_;
  double _beta;
  BinauralSums_ sums_;
  std::vector<double> cost_;
  gsl_vector* buffer_;
  bool cost_func_computed_;
};
typedef Inherit<FDIIDThresholdEstimator, BinaryMaskFilterPtr> FDIIDThresholdEstimatorPtr;

#endif
