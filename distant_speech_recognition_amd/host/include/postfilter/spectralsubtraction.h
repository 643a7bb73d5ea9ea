// postfilter/spectralsubtraction.h -- PSDEstimator, AveragePSDEstimator, SpectralSubtractor, WienerFilter with the reference's
// constructors, defaults, snake_case methods, ENABLE_LEGACY_BTK_API aliases and *Ptr typedefs (reference
// postfilter/spectralsubtraction.h:19-156, spectralsubtraction.cc), computed through btk_ss_process / btk_wiener_process of
// libbtkhip (csrc/ss_kernels.hip).  The nodes are block nodes: postfilter/enhancement_node.h says how blocks are gathered, offered
// to a synthesis bank and how a mode switch between two next() calls keeps its per-frame meaning.
//
// Mode switches that take effect at the first frame a per-frame graph would not have pulled yet: start_training, stop_training,
// start_noise_subtraction, stop_noise_subtraction, set_noise_over_estimation_factor, clear, clear_noise_samples, read_noise_file;
// start/stop_updating_noise_PSD, set_noise_amplification_factor.
//
// Stated deviations:
//   * The noise models live on the device, inside the node (bins 0..M/2, float64); PSDEstimator / AveragePSDEstimator are host
//     classes with the reference's interface for a caller that uses them on their own; the node does not route through them.
//   * SpectralSubtractor::next has no same-frame cache in the reference (a second next(n) pulls the sources again); here it
//     follows the node layer's usual contract: next(frame_no_) returns the current vector.
//   * halfBandShift = true is stored and ignored by the subtractor, and a j_error in WienerFilter::next(), as in the reference.
//   * WienerFilter mirrors only at fbinX == fftLen2_ (spectralsubtraction.cc:352), which conjugates bin M/2 in place and leaves
//     bins M/2+1 .. M-1 zero.  The engine's hand-over is K bins with the Hermitian mirror, so the node returns the mirrored
//     vector, and H S at bin M/2.
//   * WienerFilter::reset() resets its two sources only: PSDs and frame counter live on (:364-368).  Kept.
//   * write_noise_file / read_noise_file use the reference's text format, "%lf\n" per bin, K lines; read_noise_file ends
//     training (:204-207).  average() over zero frames gives NaN (1.0/(float)0 times 0), as there.
#ifndef SPECTRALSUBTRACTION_H
#define SPECTRALSUBTRACTION_H

#include <list>
#include <vector>

#include "common/refcount.h"
#include "common/jexception.h"
#include "stream/stream.h"
#include "modulated/modulated.h"
#include "postfilter/enhancement_node.h"

class PSDEstimator : public Countable {
 public:
  PSDEstimator(unsigned fftLen2);
  virtual ~PSDEstimator();
  bool read_estimates(const String& fn);
  bool write_estimates(const String& fn);
  const gsl_vector* estimate() const { return estimates_; }
  bool readEstimates(const String& fn) { return read_estimates(fn); }                  // ENABLE_LEGACY_BTK_API aliases
  bool writeEstimates(const String& fn) { return write_estimates(fn); }
 protected:
  gsl_vector* estimates_;
};
typedef refcountable_ptr<PSDEstimator> PSDEstimatorPtr;

class AveragePSDEstimator : public PSDEstimator {
 public:
  AveragePSDEstimator(unsigned fftLen2, float alpha = -1.0);
  ~AveragePSDEstimator();
  void clear_samples();
  const gsl_vector* average();
  bool add_sample(const gsl_vector_complex* sample);
  void clear();
  void clearSamples() { clear_samples(); }
  bool addSample(const gsl_vector_complex* sample) { return add_sample(sample); }
 protected:
  float alpha_;
  bool sample_added_;
  std::list<gsl_vector*> sampleL_;
};
typedef Inherit<AveragePSDEstimator, PSDEstimatorPtr> AveragePSDEstimatorPtr;

class SpectralSubtractor : public EnhancementBlockNode_ {
 public:
  SpectralSubtractor(unsigned fftLen, bool halfBandShift = false, float ft = 1.0, float flooringV = 0.001,
                     const String& nm = "SpectralSubtractor");
  ~SpectralSubtractor();
  void clear();
  void set_noise_over_estimation_factor(float ft);
  void set_channel(VectorComplexFeatureStreamPtr& chan, double alpha = -1);
  void start_training();
  void stop_training();
  void clear_noise_samples();
  void start_noise_subtraction();
  void stop_noise_subtraction();
  bool read_noise_file(const String& fn, unsigned idx = 0);
  bool write_noise_file(const String& fn, unsigned idx = 0);
  // engine-specific: the noise PSD estimate of one channel as the stream stands (bins 0..M/2)
  std::vector<double> noise_psd(unsigned idx = 0);
  void setNoiseOverEstimationFactor(float ft) { set_noise_over_estimation_factor(ft); }   // ENABLE_LEGACY_BTK_API aliases
  void setChannel(VectorComplexFeatureStreamPtr& chan, double alpha = -1) { set_channel(chan, alpha); }
  void startTraining() { start_training(); }
  void stopTraining() { stop_training(); }
  void clearNoiseSamples() { clear_noise_samples(); }
  void startNoiseSubtraction() { start_noise_subtraction(); }
  void stopNoiseSubtraction() { stop_noise_subtraction(); }
  bool readNoiseFile(const String& fn, unsigned idx = 0) { return read_noise_file(fn, idx); }
  bool writeNoiseFile(const String& fn, unsigned idx = 0) { return write_noise_file(fn, idx); }
 protected:
  virtual size_t state_bytes_() const;
  virtual void init_state_(void* d);
  virtual void launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long frames_done);
 private:
  double* est_(void* st) const;
  double* acc_(void* st) const;
  long long* count_(void* st) const;
  unsigned char* added_(void* st) const;
  void check_idx_(unsigned idx) const;
  bool halfBandShift_;
  bool training_started_, start_noise_subtraction_;
  float ft_, flooringV_;
  std::vector<double> alphas_;
};
typedef Inherit<SpectralSubtractor, VectorComplexFeatureStreamPtr> SpectralSubtractorPtr;

class WienerFilter : public EnhancementBlockNode_ {
 public:
  WienerFilter(VectorComplexFeatureStreamPtr& targetSignal, VectorComplexFeatureStreamPtr& noiseSignal, bool halfBandShift = false,
               float alpha = 0.0, float flooringV = 0.001, double beta = 1.0, const String& nm = "WienerFilter");
  virtual const gsl_vector_complex* next(int frame_no = -5);
  void set_noise_amplification_factor(double beta);
  void start_updating_noise_PSD();
  void stop_updating_noise_PSD();
  // engine-specific: the recursively averaged PSDs as the stream stands, float64 [K] each (bin 0 is never touched)
  std::vector<double> target_psd();
  std::vector<double> noise_psd();
  void setNoiseAmplificationFactor(double beta) { set_noise_amplification_factor(beta); }     // ENABLE_LEGACY_BTK_API aliases
  void startUpdatingNoisePSD() { start_updating_noise_PSD(); }
  void stopUpdatingNoisePSD() { stop_updating_noise_PSD(); }
 protected:
  virtual size_t state_bytes_() const;
  virtual void init_state_(void* d);
  virtual void launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long frames_done);
  virtual bool keeps_frame_counter_on_reset_() const { return true; }
 private:
  std::vector<double> psd_(int which);
  bool halfBandShift_;
  float alpha_, flooringV_, beta_;
  bool update_noise_PSD_;
};
typedef Inherit<WienerFilter, VectorComplexFeatureStreamPtr> WienerFilterPtr;

#endif
