// binaural_nodes.cc -- the binaural binary-mask filters and threshold estimators (postfilter/binauralprocessing.h) over
// btk_binaural_mask / btk_binaural_stats / btk_binaural_threshold (csrc/binaural_kernels.hip), on the block machinery of
// postfilter/enhancement_node.h (src/ss_nodes.cc).  Both sources are gathered channel-major: XL = rows [0, K), XR = rows [K, 2K).
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstring>

#include "postfilter/binauralprocessing.h"
#include "node_runtime.h"

namespace {

using btknode::check_abi;
using btknode::check_hip;
using btknode::nstream;
using btknode::d2h;
using btknode::h2d;
using btknode::dev_zero_async;

}  // namespace

// ================================================================================ BinaryMaskFilter
BinaryMaskFilter::BinaryMaskFilter(unsigned chanX, VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M,
                                   float threshold, float alpha, float dEta, const String& nm)
    : EnhancementBlockNode_(M, true, nm), mask_kind_(-1), chanX_(chanX), alpha_(alpha), dEta_(dEta), threshold_(threshold),
      threshold_per_freq_(NULL)
{
  if (srcL->size() != M) throw jdimension_error("Left input block length (%d) != M (%d)\n", (int)srcL->size(), (int)M);
  if (srcR->size() != M) throw jdimension_error("Right input block length (%d) != M (%d)\n", (int)srcR->size(), (int)M);
  add_source_(srcL);
  add_source_(srcR);
}

BinaryMaskFilter::~BinaryMaskFilter()
{
  if (threshold_per_freq_) gsl_vector_free(threshold_per_freq_);
}

// (:97-101) the base class pulls nothing and writes nothing
const gsl_vector_complex* BinaryMaskFilter::next(int)
{
  increment_();
  return vector_;
}

void BinaryMaskFilter::set_threshold(float threshold)
{
  begin_switch_(false);
  threshold_ = threshold;
  end_switch_();
}

// (:82-95; bins 1 .. M/2 are copied, on the first call too)
void BinaryMaskFilter::set_thresholds(const gsl_vector* thresholds)
{
  const unsigned K = fftLen_ / 2 + 1;
  if (!thresholds || thresholds->size < K)
    throw jdimension_error("%s: %d thresholds where M/2 + 1 = %d are expected\n", name().c_str(), thresholds ? (int)thresholds->size : 0, (int)K);
  begin_switch_(false);                 // frames up to the mark were computed with the old values
  if (!threshold_per_freq_) threshold_per_freq_ = gsl_vector_calloc(K);
  std::vector<float> f(K, 0.f);
  for (unsigned k = 1; k < K; k++) {
    gsl_vector_set(threshold_per_freq_, k, gsl_vector_get(thresholds, k));
    f[k] = (float)gsl_vector_get(thresholds, k);                // threshold_ = gsl_vector_get(...): a float member (:457)
  }
  h2d(dThresholds_.ensure(sizeof(float) * K), f.data(), sizeof(float) * K);
  end_switch_();
}

size_t BinaryMaskFilter::state_bytes_() const { return mask_kind_ < 0 ? 0 : sizeof(float) * (fftLen_ / 2 + 1); }    // prevMu_ [K]

void BinaryMaskFilter::init_state_(void* d)
{
  const std::vector<float> ones(fftLen_ / 2 + 1, 1.0f);         // gsl_vector_float_set_all(prevMu_, 1.0), :72
  h2d(d, ones.data(), sizeof(float) * ones.size());
}

void BinaryMaskFilter::zero_output_(void* dOut, long Ts, long t0, long t1)
{
  if (t1 > t0)
    check_hip(hipMemset2DAsync(static_cast<float*>(dOut) + 2 * t0, sizeof(float) * 2 * Ts, 0, sizeof(float) * 2 * (t1 - t0),
                               fftLen_ / 2 + 1, nstream()), "hipMemset2DAsync");
}

void BinaryMaskFilter::launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long frames_done)
{
  if (mask_kind_ < 0) { zero_output_(dOut, Ts, t0, t1); return; }
  const unsigned K = fftLen_ / 2 + 1;
  const float* xl = static_cast<const float*>(dX) + 2 * t0;
  const float* thr = (mask_kind_ == BTK_BINAURAL_IID && threshold_per_freq_) ? static_cast<const float*>(dThresholds_.get()) : NULL;
  check_abi(btk_binaural_mask(xl, xl + 2 * (size_t)K * Ts, static_cast<float*>(dOut) + 2 * t0, 1, (int)fftLen_, Ts, t1 - t0, mask_kind_,
                              (int)chanX_, threshold_, thr, alpha_, dEta_, frames_done, static_cast<float*>(state_dev_()),
                              btk_node_stream()));
}

std::vector<float> BinaryMaskFilter::prev_mu()
{
  std::vector<float> r;
  if (mask_kind_ < 0) return r;
  void* st = begin_peek_();
  r.resize(fftLen_ / 2 + 1);
  d2h(r.data(), st, sizeof(float) * r.size());
  end_peek_();
  return r;
}

// ================================================================================ KimBinaryMaskFilter, IIDBinaryMaskFilter
KimBinaryMaskFilter::KimBinaryMaskFilter(unsigned chanX, VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR,
                                         unsigned M, float threshold, float alpha, float dEta, float dPowerCoeff, const String& nm)
    : BinaryMaskFilter(chanX, srcL, srcR, M, threshold, alpha, dEta, nm), dpower_coeff_(dPowerCoeff)
{
  if (chanX > 1) throw jdimension_error("%s: channel %d where 0 (left) or 1 (right) is expected\n", nm.c_str(), (int)chanX);
  mask_kind_ = BTK_BINAURAL_KIM;
}

const gsl_vector_complex* KimBinaryMaskFilter::next(int frame_no) { return EnhancementBlockNode_::next(frame_no); }

IIDBinaryMaskFilter::IIDBinaryMaskFilter(unsigned chanX, VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR,
                                         unsigned M, float threshold, float alpha, float dEta, const String& nm)
    : BinaryMaskFilter(chanX, srcL, srcR, M, threshold, alpha, dEta, nm)
{
  if (chanX > 1) throw jdimension_error("%s: channel %d where 0 (left) or 1 (right) is expected\n", nm.c_str(), (int)chanX);
  mask_kind_ = BTK_BINAURAL_IID;
}

const gsl_vector_complex* IIDBinaryMaskFilter::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  const gsl_vector_complex* v = EnhancementBlockNode_::next(frame_no);
  // masking1 leaves threshold_ at the last bin's value (:456-457)
  if (threshold_per_freq_) threshold_ = (float)gsl_vector_get(threshold_per_freq_, fftLen_ / 2);
  return v;
}

// ================================================================================ the sums of the estimators
void BinauralSums_::init(int kind_, unsigned M_, float lo, float hi, float width)
{
  kind = kind_; M = M_;
  int nw = 0, nc = 0;
  check_abi(btk_binaural_candidates(lo, hi, width, NULL, 0, &nw, &nc));
  cands.assign((size_t)(nw > 0 ? nw : 0), 0.f);
  check_abi(btk_binaural_candidates(lo, hi, width, cands.data(), nw, &nw, &nc));
  nWalk = (unsigned)nw; nCand = (unsigned)nc;
}

size_t BinauralSums_::state_bytes() const
{
  const size_t nv = kind == BTK_BINAURAL_KIM ? 5 : (kind == BTK_BINAURAL_IID ? 6 : 3);
  const size_t rows = kind == BTK_BINAURAL_FDIID ? M / 2 + 1 : 1;
  return sizeof(double) * rows * nCand * nv + sizeof(long long);
}

void BinauralSums_::accumulate(const void* dXL, const void* dXR, long Ts, long T, float eta, float pc, unsigned k0, unsigned k1, void* state)
{
  if (T <= 0) return;
  if (!uploaded_) {
    h2d(dCands_.ensure(sizeof(float) * (nWalk ? nWalk : 1)), cands.data(), sizeof(float) * nWalk);
    uploaded_ = true;
  }
  const long need = btk_binaural_stats_scratch_bytes(kind, 1, T, (int)nCand);
  void* scratch = dScratch_.ensure(need > 0 ? (size_t)need : 8);
  double* sums = static_cast<double*>(state);
  long long* count = reinterpret_cast<long long*>(static_cast<char*>(state) + state_bytes() - sizeof(long long));
  check_abi(btk_binaural_stats(dXL, dXR, 1, (int)M, Ts, T, kind, static_cast<const float*>(dCands_.get()), (int)nWalk, (int)nCand, eta,
                               pc, (int)k0, (int)k1, sums, count, NULL, scratch, need > 0 ? need : 8, btk_node_stream()));
}

double BinauralSums_::threshold(const void* state, double beta, std::vector<double>& cost, std::vector<double>* per_bin)
{
  const size_t n = state_bytes();
  std::vector<char> h(n);
  d2h(h.data(), state, n);
  long long count;
  memcpy(&count, &h[n - sizeof(long long)], sizeof(long long));
  const unsigned K = M / 2 + 1;
  cost.assign(kind == BTK_BINAURAL_FDIID ? (size_t)K * nCand : nCand, 0.0);
  if (per_bin) per_bin->assign(K, 0.0);
  double thr = 0.0;
  const float none = 0.f;
  check_abi(btk_binaural_threshold(kind, (int)M, (int)nCand, (int)nWalk, nWalk ? cands.data() : &none,
                                   reinterpret_cast<const double*>(h.data()), count, beta, &thr, cost.data(),
                                   per_bin ? per_bin->data() : NULL));
  return thr;
}

// ================================================================================ KimITDThresholdEstimator, IIDThresholdEstimator
void KimITDThresholdEstimator::setup_(int kind, unsigned M, float minThreshold, float maxThreshold, float width, float minFreq,
                                      float maxFreq, int sampleRate)
{
  if (minThreshold == maxThreshold) {                           // (:252-255) whatever the sample rate
    min_threshold_ = -0.2 * 16000 / 340;
    max_threshold_ = 0.2 * 16000 / 340;
  } else {
    min_threshold_ = minThreshold;
    max_threshold_ = maxThreshold;
  }
  if (minFreq < 0 || maxFreq < 0 || sampleRate < 0) {
    min_fbinX_ = 1;
    max_fbinX_ = M / 2 + 1;
  } else {
    min_fbinX_ = (unsigned)(M * minFreq / (float)sampleRate);   // (:266-267) in float
    max_fbinX_ = (unsigned)(M * maxFreq / (float)sampleRate);
  }
  if (max_fbinX_ > M / 2 + 1)
    throw jdimension_error("%s: bins up to %d lie beyond M/2 + 1 = %d\n", name().c_str(), (int)max_fbinX_, (int)(M / 2 + 1));
  if (min_fbinX_ > max_fbinX_) min_fbinX_ = max_fbinX_;         // an empty loop either way
  sums_.init(kind, M, min_threshold_, max_threshold_, width);
  buffer_ = gsl_vector_calloc(sums_.nCand);
  mask_kind_ = -1;                                              // the node's state is the sums: there is no prevMu_ to read
}

KimITDThresholdEstimator::KimITDThresholdEstimator(VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M,
                                                   float minThreshold, float maxThreshold, float width, float minFreq, float maxFreq,
                                                   int sampleRate, float dEta, float dPowerCoeff, const String& nm)
    : KimBinaryMaskFilter(0, srcL, srcR, M, 0.0, 0.0 /* alpha must be zero */, dEta, dPowerCoeff, nm), width_(width), buffer_(NULL),
      cost_func_computed_(false)
{
  setup_(BTK_BINAURAL_KIM, M, minThreshold, maxThreshold, width, minFreq, maxFreq, sampleRate);
}

KimITDThresholdEstimator::KimITDThresholdEstimator(int kind, VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR,
                                                   unsigned M, float minThreshold, float maxThreshold, float width, float minFreq,
                                                   float maxFreq, int sampleRate, float dEta, float dPowerCoeff, const String& nm)
    : KimBinaryMaskFilter(0, srcL, srcR, M, 0.0, 0.0, dEta, dPowerCoeff, nm), width_(width), buffer_(NULL), cost_func_computed_(false)
{
  setup_(kind, M, minThreshold, maxThreshold, width, minFreq, maxFreq, sampleRate);
}

KimITDThresholdEstimator::~KimITDThresholdEstimator()
{
  if (buffer_) gsl_vector_free(buffer_);
}

size_t KimITDThresholdEstimator::state_bytes_() const { return sums_.state_bytes(); }
void KimITDThresholdEstimator::init_state_(void* d) { dev_zero_async(d, state_bytes_()); }

void KimITDThresholdEstimator::launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long)
{
  const unsigned K = fftLen_ / 2 + 1;
  const float* xl = static_cast<const float*>(dX) + 2 * t0;
  zero_output_(dOut, Ts, t0, t1);                               // vector_ is never written in the reference
  sums_.accumulate(xl, xl + 2 * (size_t)K * Ts, Ts, t1 - t0, dEta_, dpower_coeff_, min_fbinX_, max_fbinX_, state_dev_());
}

const gsl_vector_complex* KimITDThresholdEstimator::next(int frame_no) { return EnhancementBlockNode_::next(frame_no); }

void KimITDThresholdEstimator::reset()
{
  EnhancementBlockNode_::reset();
  void* st = begin_switch_();                                   // (:416-425) the sums and nSamples_ go
  dev_zero_async(st, state_bytes_());
  end_switch_();
  cost_func_computed_ = false;
}

double KimITDThresholdEstimator::calc_threshold()
{
  std::vector<double> cost;
  void* st = begin_peek_();
  const double thr = sums_.threshold(st, beta_(), cost, NULL);
  end_peek_();
  for (unsigned i = 0; i < sums_.nCand; i++) gsl_vector_set(buffer_, i, cost[i]);
  threshold_ = (float)thr;
  cost_func_computed_ = true;
  return thr;
}

const gsl_vector* KimITDThresholdEstimator::cost_function()
{
  if (!cost_func_computed_) fprintf(stderr, "KimITDThresholdEstimator:call calc_threshold() first\n");
  return buffer_;
}

unsigned KimITDThresholdEstimator::num_samples()
{
  const size_t n = state_bytes_();
  long long count = 0;
  void* st = begin_peek_();
  d2h(&count, static_cast<char*>(st) + n - sizeof(long long), sizeof(long long));
  end_peek_();
  return (unsigned)count;
}

IIDThresholdEstimator::IIDThresholdEstimator(VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M,
                                             float minThreshold, float maxThreshold, float width, float minFreq, float maxFreq,
                                             int sampleRate, float dEta, float dPowerCoeff, const String& nm)
    : KimITDThresholdEstimator(BTK_BINAURAL_IID, srcL, srcR, M, minThreshold, maxThreshold, width, minFreq, maxFreq, sampleRate, dEta,
                               dPowerCoeff, nm)
{
}

// ================================================================================ FDIIDThresholdEstimator
FDIIDThresholdEstimator::FDIIDThresholdEstimator(VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M,
                                                 float minThreshold, float maxThreshold, float width, float dEta, float dPowerCoeff,
                                                 const String& nm)
    : BinaryMaskFilter(0, srcL, srcR, M, 0.0, 0.0 /* alpha must be zero */, dEta, nm), width_(width), dpower_coeff_(dPowerCoeff),
      _beta(3.0), buffer_(NULL), cost_func_computed_(false)
{
  if (minThreshold == maxThreshold) {                           // (:717-720)
    min_threshold_ = -100000;
    max_threshold_ = 100000;
  } else {
    min_threshold_ = minThreshold;
    max_threshold_ = maxThreshold;
  }
  sums_.init(BTK_BINAURAL_FDIID, M, min_threshold_, max_threshold_, width);
  buffer_ = gsl_vector_calloc(sums_.nCand);
  threshold_per_freq_ = gsl_vector_calloc(M / 2 + 1);
}

FDIIDThresholdEstimator::~FDIIDThresholdEstimator()
{
  if (buffer_) gsl_vector_free(buffer_);
}

size_t FDIIDThresholdEstimator::state_bytes_() const { return sums_.state_bytes(); }
void FDIIDThresholdEstimator::init_state_(void* d) { dev_zero_async(d, state_bytes_()); }

void FDIIDThresholdEstimator::launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long)
{
  const unsigned K = fftLen_ / 2 + 1;
  const float* xl = static_cast<const float*>(dX) + 2 * t0;
  zero_output_(dOut, Ts, t0, t1);
  sums_.accumulate(xl, xl + 2 * (size_t)K * Ts, Ts, t1 - t0, dEta_, dpower_coeff_, 1, K, state_dev_());
}

const gsl_vector_complex* FDIIDThresholdEstimator::next(int frame_no) { return EnhancementBlockNode_::next(frame_no); }

void FDIIDThresholdEstimator::reset()
{
  EnhancementBlockNode_::reset();
  void* st = begin_switch_();
  dev_zero_async(st, state_bytes_());
  end_switch_();
  cost_func_computed_ = false;
}

double FDIIDThresholdEstimator::calc_threshold()
{
  std::vector<double> per_bin;
  void* st = begin_peek_();
  const double thr = sums_.threshold(st, _beta, cost_, &per_bin);
  end_peek_();
  for (unsigned k = 1; k < fftLen_ / 2 + 1; k++) gsl_vector_set(threshold_per_freq_, k, per_bin[k]);
  threshold_ = (float)thr;
  cost_func_computed_ = true;
  return threshold_;
}

const gsl_vector* FDIIDThresholdEstimator::cost_function(unsigned freqX)
{
  if (freqX > fftLen_ / 2) throw jindex_error("%s: bin %d beyond M/2 = %d\n", name().c_str(), (int)freqX, (int)(fftLen_ / 2));
  if (!cost_func_computed_) calc_threshold();
  for (unsigned i = 0; i < sums_.nCand; i++) gsl_vector_set(buffer_, i, cost_[(size_t)freqX * sums_.nCand + i]);
  return buffer_;
}
