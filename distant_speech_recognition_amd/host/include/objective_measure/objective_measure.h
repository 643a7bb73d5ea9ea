// objective_measure/objective_measure.h -- SNR and ItakuraSaitoMeasurePS (reference objective_measure/objective_measure.h:41-74,
// objective_measure.cc:187-282, :333-347) over btk_obj_snr / btk_obj_is_distance of include/btkhip.h (csrc/obj_kernels.hip).
//
// SNR::getSNR opens 16-bit PCM WAV files through SampleFeature's reader and keeps the reference's rules: chX outside the
// channels of either file is a jconsistency_error (chX == 0: "Multi-channel read is not yet supported."), unequal sample rates
// and a file that cannot be opened are jio_errors, cfrom < 0 counts as 0, `to` < 0 or behind the last frame of either file
// means each file to its own end, and cfrom behind the end of a file is a jio_error.  The samples are x / 32768: the reference
// reads them with sf_readf_float, which normalises, unlike SampleFeature::read with norm == 0.
// Deviations: the sums are float64 in a fixed order; the arrays given to getSNR2 are not modified (the reference
// subtracts the means in place); option 8 with a first signal shorter than the second, where the reference reads past the first,
// and a range that leaves a signal without samples are jdimension_errors.
// ItakuraSaitoMeasurePS::getDistance serves the frames NormalFFTAnalysisBank serves over SampleFeature(D, D, false): the whole
// blocks of D samples that end before the last sample, then one zero-padded frame; samples at int16 scale.
#pragma once
#include "stream/stream.h"
#include "common/devmem.h"
#include "btkhip.h"

class SNR : public Countable {
 public:
  SNR() {}
  float getSNR(const String& fn1, const String& fn2, int normalizationOption, int chX = 1, int samplerate = 16000, int cfrom = -1,
               int to = -1);
  float getSNR2(const gsl_vector_float* original, const gsl_vector_float* enhanced, int normalizationOption);
  // mu1, mu2, a1, a2, sum, err of the call before (tests)
  const double* stats() const { return stats_; }
 private:
  float run_(const float* x1, long n1, const float* x2, long n2, int option);
  DeviceBuffer d_x_, d_ws_, d_stats_;
  double stats_[6];
};
typedef refcountable_ptr<SNR> SNRPtr;

class ItakuraSaitoMeasurePS : public Countable {
 public:
  ItakuraSaitoMeasurePS(unsigned fftLen, unsigned r = 1, unsigned windowType = 1, const String& nm = "ItakuraSaitoMeasurePS");
  ~ItakuraSaitoMeasurePS();
  float getDistance(const String& fn1, const String& fn2, int chX = 1, int samplerate = 16000, int bframe = 0, int eframe = -1);
  int frameShiftLength() const { return (int)D_; }
  long frames() const { return frames_; }            // frames in range of the call before (tests)
  double distance() const { return dist_; }          // the float64 distance of the call before
 private:
  unsigned M_, r_, window_type_, D_;
  btk_stft_t* plan_;                                 // made at the first call: construction touches no device
  DeviceBuffer d_x_, d_out_;
  long frames_;
  double dist_;
};
typedef refcountable_ptr<ItakuraSaitoMeasurePS> ItakuraSaitoMeasurePSPtr;
