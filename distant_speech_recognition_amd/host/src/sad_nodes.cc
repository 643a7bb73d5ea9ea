// sad_nodes.cc -- the voice activity detection nodes of sad/sad.h over the btk_vad_* calls (csrc/vad_kernels.hip): the metrics
// and the recursion evaluate blocks of frames drawn through next(), the hangover nodes run their machine over the metrics'
// value rows where the metrics left them on the device.
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "sad/sad.h"
#include "btkhip.h"
#include "node_runtime.h"

namespace {

using btknode::check_abi;
using btknode::check_hip;
using btknode::nstream;

// local: unlike btknode::d2h_async / h2d_async these issue zero-byte copies too and name the VAD in their error text
void download(void* h, const void* d, size_t bytes, hipStream_t st)
{
  check_hip(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st), "VAD download");
  btk_node_count_d2h(bytes);
}
void upload(void* d, const void* h, size_t bytes, hipStream_t st)
{
  check_hip(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st), "VAD upload");
}

}  // namespace

long btk_vad_default_block_frames() { return btknode::env_block_frames("BTK_VAD_BLOCK_FRAMES", 256); }

// ================================================================================ VADMetric: the block service
VADMetric::VADMetric()
    : cur_score_(0.0), cur_value_(0.0), cap_(0), frame_no_(-1), block_frames_(btk_vad_default_block_frames()), blk_n_(0), blk_pos_(0),
      staged_(0), launches_(0), src_end_(false)
{
}

void VADMetric::rewind_()
{
  frame_no_ = -1;
  blk_n_ = blk_pos_ = staged_ = 0;
  src_end_ = false;
}

void VADMetric::begin_block(long cap)
{
  if (blk_pos_ < blk_n_)
    throw jconsistency_error("VAD metric: %ld frames of its own block are not served yet\n", blk_n_ - blk_pos_);
  if (cap < 1) throw jdimension_error("VAD metric: a block of %ld frames\n", cap);
  cap_ = cap;
  reserve_(cap);
  d_rows_.ensure(sizeof(double) * 2 * (size_t)cap);
  h_rows_.ensure(sizeof(double) * 2 * (size_t)cap);
  staged_ = 0;
}

void VADMetric::stage_frame(int frame_no)
{
  if (staged_ >= cap_) throw jconsistency_error("VAD metric: more than %ld frames staged\n", cap_);
  pull_(frame_no, staged_);
  staged_++;
}

// the kernels over the first n staged frames; the rows are on the host when this returns
void VADMetric::run_(long n)
{
  hipStream_t st = nstream();
  double* d = static_cast<double*>(d_rows_.get());
  double* h = static_cast<double*>(h_rows_.get());
  launch_(n, d, d + cap_);
  launches_++;
  download(h, d, sizeof(double) * (size_t)n, st);
  download(h + cap_, d + cap_, sizeof(double) * (size_t)n, st);
  check_hip(hipStreamSynchronize(st), "VAD metric block");
  downloaded_(n);
}

const double* VADMetric::flush_staged(long n)
{
  if (n < 1 || n > staged_) throw jconsistency_error("VAD metric: %ld frames asked for, %ld staged\n", n, staged_);
  run_(n);
  const double* h = static_cast<const double*>(h_rows_.get());
  frame_no_ += (int)n;
  cur_value_ = h[n - 1];
  cur_score_ = h[cap_ + n - 1];
  served_(n - 1);
  blk_n_ = blk_pos_ = staged_ = 0;
  return static_cast<const double*>(d_rows_.get());
}

double VADMetric::next(int frame_no)
{
  if (frame_no == frame_no_) return cur_value_;
  if (frame_no >= 0 && frame_no - 1 != frame_no_)
    throw jindex_error("Problem in VAD metric: %d != %d\n", frame_no - 1, frame_no_);
  if (blk_pos_ >= blk_n_) {
    if (src_end_) throw jiterator_error("end of samples!");
    begin_block(block_frames_);
    long n = 0;
    try {
      for (; n < cap_; n++) pull_(frame_no_ + 1 + (int)n, n);
    } catch (jiterator_error&) {
      src_end_ = true;
      if (n == 0) throw;
    }
    staged_ = n;
    run_(n);
    staged_ = 0;
    blk_n_ = n;
    blk_pos_ = 0;
  }
  const double* h = static_cast<const double*>(h_rows_.get());
  const long pos = blk_pos_++;
  frame_no_++;
  cur_value_ = h[pos];
  cur_score_ = h[cap_ + pos];
  served_(pos);
  return cur_value_;
}

// ================================================================================ EnergyVADMetric (sad.cc:472-588)
EnergyVADMetric::EnergyVADMetric(const VectorFloatFeatureStreamPtr& source, double initialEnergy, double threshold, unsigned headN,
                                 unsigned tailN, unsigned energiesN, const String& nm)
    : source_(source), initial_energy_(initialEnergy), headN_(headN), tailN_(tailN), energiesN_(energiesN), medianX_(0), state_todo_(2)
{
  if (energiesN < 1 || btk_vad_energy_metric_state_bytes((int)energiesN) < 0)
    throw jdimension_error("%s: energiesN=%u, 1 .. 1024 are supported\n", nm.c_str(), energiesN);
  const double v = threshold * energiesN;
  if (!(v >= 0.0) || v >= (double)energiesN)      // the reference reads past its sorted array there
    throw jdimension_error("%s: threshold %g puts the median index outside 0 .. %u\n", nm.c_str(), threshold, energiesN - 1);
  medianX_ = (int)(unsigned)v;
}

void EnergyVADMetric::reset()
{
  if (state_todo_ == 0) state_todo_ = 1;
  rewind_();
}

void EnergyVADMetric::next_speaker()
{
  state_todo_ = 2;
  rewind_();
}

void EnergyVADMetric::reserve_(long cap)
{
  h_in_.ensure(sizeof(float) * (size_t)source_->size() * (size_t)cap);
  d_in_.ensure(sizeof(float) * (size_t)source_->size() * (size_t)cap);
}

void EnergyVADMetric::pull_(int frame_no, long slot)
{
  const gsl_vector_float* v = source_->next(frame_no);
  memcpy(static_cast<float*>(h_in_.get()) + (size_t)slot * source_->size(), v->data, sizeof(float) * source_->size());
}

void EnergyVADMetric::sync_state_()
{
  if (state_todo_ == 0) return;
  hipStream_t st = nstream();
  const size_t bytes = (size_t)btk_vad_energy_metric_state_bytes((int)energiesN_);
  char* d = static_cast<char*>(d_state_.get() ? d_state_.get() : d_state_.ensure(bytes));
  if (state_todo_ == 2) {
    long long* h = static_cast<long long*>(h_state_.ensure(bytes));
    h[0] = h[1] = h[2] = h[3] = 0;
    double* ring = reinterpret_cast<double*>(h + 4);
    for (unsigned i = 0; i < energiesN_; i++) ring[i] = initial_energy_;
    upload(d, h, bytes, st);
  } else {
    check_hip(hipMemsetAsync(d + 8, 0, 24, st), "VAD state");    // recognizing and the two counters; ring and position stay
  }
  state_todo_ = 0;
}

void EnergyVADMetric::launch_(long n, double* d_value, double* d_score)
{
  hipStream_t st = nstream();
  const int D = (int)source_->size();
  sync_state_();
  upload(d_in_.get(), h_in_.get(), sizeof(float) * (size_t)D * (size_t)n, st);
  check_abi(btk_vad_frame_energy(d_in_.get(), 0, 1, D, n, 0, D, 1, d_score, cap_, st));
  check_abi(btk_vad_energy_metric(d_score, cap_, 1, n, (int)energiesN_, medianX_, headN_, tailN_, d_state_.get(), d_value, cap_, st));
}

double EnergyVADMetric::energy_percentile(double percentile)
{
  if (percentile < 0.0 || percentile > 100.0) throw jdimension_error("Percentile %g is out of range [0.0, 100.0].", percentile);
  const unsigned x = (unsigned)((percentile / 100.0) * energiesN_);
  if (x >= energiesN_) throw jdimension_error("Percentile %g reads past the window of %u energies.", percentile, energiesN_);
  if (state_todo_ == 2) return initial_energy_ / energiesN_;
  hipStream_t st = nstream();
  const size_t bytes = (size_t)btk_vad_energy_metric_state_bytes((int)energiesN_);
  long long* h = static_cast<long long*>(h_state_.ensure(bytes));
  download(h, d_state_.get(), bytes, st);
  check_hip(hipStreamSynchronize(st), "VAD state download");
  const double* ring = reinterpret_cast<const double*>(h + 4);
  std::vector<double> sorted(ring, ring + energiesN_);
  std::sort(sorted.begin(), sorted.end());
  return sorted[x] / energiesN_;
}

// ================================================================================ the band-power metrics (sad.cc:593-836, :996-1063)
PowerSpectrumVADMetric::PowerSpectrumVADMetric(unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, const String& nm)
    : kind_(BTK_VAD_POWER), E0_(1.0), powN_(0), powerList_(NULL), pos_(-1)
{
  init_(fftLen, sampleRate, lowCutoff, highCutoff);
}

PowerSpectrumVADMetric::PowerSpectrumVADMetric(int kind, double E0, unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff)
    : kind_(kind), E0_(E0), powN_(0), powerList_(NULL), pos_(-1)
{
  init_(fftLen, sampleRate, lowCutoff, highCutoff);
}

void PowerSpectrumVADMetric::init_(unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff)
{
  fftLen_ = (int)fftLen;
  check_abi(btk_vad_band_limits(fftLen_, sampleRate, lowCutoff, highCutoff, &lowX_, &highX_, &binN_));
  if (fftLen_ > 2048 || lowX_ > highX_)
    throw jdimension_error("band-power metric: fftLen=%d (2 .. 2048), bins %d .. %d\n", fftLen_, lowX_, highX_);
}

PowerSpectrumVADMetric::~PowerSpectrumVADMetric()
{
  if (powerList_) gsl_vector_free(powerList_);
}

NormalizedEnergyMetric::NormalizedEnergyMetric(unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, const String& nm)
    : PowerSpectrumVADMetric(BTK_VAD_NORMALIZED, 1.0, fftLen, sampleRate, lowCutoff, highCutoff)
{
}

TSPSVADMetric::TSPSVADMetric(unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, const String& nm)
    : PowerSpectrumVADMetric(BTK_VAD_TSPS, 5000.0, fftLen, sampleRate, lowCutoff, highCutoff)
{
}

void PowerSpectrumVADMetric::set_channel(const VectorFloatFeatureStreamPtr& chan)
{
  if ((int)chan->size() <= highX_)
    throw jdimension_error("band-power metric: bin %d of spectra of %u values\n", highX_, chan->size());
  if (!channels_.empty() && chan->size() != powN_)
    throw jdimension_error("band-power metric: a channel of %u values next to channels of %u\n", chan->size(), powN_);
  if (channels_.size() >= 64) throw jdimension_error("band-power metric: at most 64 channels\n");
  powN_ = chan->size();
  channels_.push_back(chan);
}

void PowerSpectrumVADMetric::clear_channel()
{
  channels_.clear();
  if (powerList_) gsl_vector_free(powerList_);
  powerList_ = NULL;
  pos_ = -1;
}

void PowerSpectrumVADMetric::reset()
{
  for (size_t c = 0; c < channels_.size(); c++) channels_[c]->reset();
  rewind_();
  pos_ = -1;
}

void PowerSpectrumVADMetric::next_speaker() { PowerSpectrumVADMetric::reset(); }

void PowerSpectrumVADMetric::reserve_(long cap)
{
  const size_t C = channels_.size();
  if (C == 0) throw jdimension_error("band-power metric: no channel was set\n");
  h_in_.ensure(sizeof(float) * C * (size_t)cap * powN_);
  d_in_.ensure(sizeof(float) * C * (size_t)cap * powN_);
  h_P_.ensure(sizeof(double) * C * (size_t)cap);
  d_P_.ensure(sizeof(double) * C * (size_t)cap);
  pos_ = -1;
}

void PowerSpectrumVADMetric::pull_(int frame_no, long slot)
{
  float* in = static_cast<float*>(h_in_.get());
  for (size_t c = 0; c < channels_.size(); c++) {
    const gsl_vector_float* v = channels_[c]->next(frame_no);
    memcpy(in + (c * (size_t)cap_ + (size_t)slot) * powN_, v->data, sizeof(float) * powN_);
  }
}

void PowerSpectrumVADMetric::launch_(long n, double* d_value, double* d_score)
{
  hipStream_t st = nstream();
  const size_t C = channels_.size(), row = (size_t)cap_ * powN_;
  const float* hin = static_cast<const float*>(h_in_.get());
  float* din = static_cast<float*>(d_in_.get());
  for (size_t c = 0; c < C; c++) upload(din + c * row, hin + c * row, sizeof(float) * (size_t)n * powN_, st);
  double* dP = static_cast<double*>(d_P_.get());
  check_abi(btk_vad_band_power(din, kind_, 1, (int)C, fftLen_, n, 0, (long)row, (long)powN_, 1, lowX_, highX_, E0_, dP, d_score, d_value,
                               cap_, st));
  double* hP = static_cast<double*>(h_P_.get());
  for (size_t c = 0; c < C; c++) download(hP + c * (size_t)cap_, dP + c * (size_t)cap_, sizeof(double) * (size_t)n, st);
}

void PowerSpectrumVADMetric::downloaded_(long) {}

void PowerSpectrumVADMetric::served_(long pos) { pos_ = pos; }

const gsl_vector* PowerSpectrumVADMetric::get_metrics()
{
  if (pos_ < 0) return NULL;
  const size_t C = channels_.size();
  if (powerList_ && powerList_->size != C) { gsl_vector_free(powerList_); powerList_ = NULL; }
  if (!powerList_) powerList_ = gsl_vector_calloc(C);
  const double* hP = static_cast<const double*>(h_P_.get());
  for (size_t c = 0; c < C; c++) powerList_->data[c] = hP[c * (size_t)cap_ + (size_t)pos_];
  return powerList_;
}

// ================================================================================ VAD, SimpleEnergyVAD (sad.cc:126-180)
VAD::VAD(const VectorComplexFeatureStreamPtr& samp)
    : samp_(samp), frame_reset_no_(-1), fftLen_(samp->size()), is_speech_(false), frame_no_(-1),
      frame_(gsl_vector_complex_calloc(samp->size()))
{
}

VAD::~VAD() { gsl_vector_complex_free(frame_); }

SimpleEnergyVAD::SimpleEnergyVAD(const VectorComplexFeatureStreamPtr& samp, double threshold, double gamma)
    : VAD(samp), threshold_(threshold), gamma_(gamma), cur_s_(0.0), state_from_host_(true), src_end_(false),
      block_frames_(btk_vad_default_block_frames()), blk_n_(0), blk_pos_(0), launches_(0), blk_cap_(0)
{
}

// the recursion value after the frame served last goes back to the device: frames drawn ahead are evaluated again
void SimpleEnergyVAD::reset()
{
  VAD::reset();
  samp_->reset();
  blk_n_ = blk_pos_ = 0;
  src_end_ = false;
  state_from_host_ = true;
}

void SimpleEnergyVAD::next_speaker()
{
  cur_s_ = 0.0;
  reset();
}

void SimpleEnergyVAD::fill_()
{
  if (src_end_) throw jiterator_error("end of samples!");
  const size_t L = fftLen_, cap = (size_t)block_frames_;
  float* in = static_cast<float*>(h_in_.ensure(sizeof(float) * 2 * L * cap));
  long n = 0;
  try {
    for (; n < (long)cap; n++) {
      const gsl_vector_complex* X = samp_->next(frame_no_ + 1 + (int)n);
      float* f = in + 2 * L * (size_t)n;
      for (size_t i = 0; i < 2 * L; i++) f[i] = (float)X->data[i];
    }
  } catch (jiterator_error&) {
    src_end_ = true;
    if (n == 0) throw;
  }
  hipStream_t st = nstream();
  // host block: smoothed float64 [cap], the state's way up float64 [1], is_speech int32 [cap]
  double* hs = static_cast<double*>(h_out_.ensure(sizeof(double) * (cap + 1) + sizeof(int) * cap));
  int* hi = reinterpret_cast<int*>(hs + cap + 1);
  float* din = static_cast<float*>(d_in_.ensure(sizeof(float) * 2 * L * cap));
  double* de = static_cast<double*>(d_energy_.ensure(sizeof(double) * cap));
  double* ds = static_cast<double*>(d_out_.ensure(sizeof(double) * cap + sizeof(int) * cap));
  int* di = reinterpret_cast<int*>(ds + cap);
  double* dstate = static_cast<double*>(d_state_.get() ? d_state_.get() : d_state_.ensure(sizeof(double)));
  if (state_from_host_) {
    hs[cap] = cur_s_;
    upload(dstate, hs + cap, sizeof(double), st);
    state_from_host_ = false;
  }
  upload(din, in, sizeof(float) * 2 * L * (size_t)n, st);
  check_abi(btk_vad_frame_energy(din, 1, 1, (int)L, n, 0, (long)L, 1, de, (long)cap, st));
  check_abi(btk_vad_simple_energy(de, (long)cap, 1, n, gamma_, threshold_, dstate, di, ds, (long)cap, st));
  launches_++;
  download(hs, ds, sizeof(double) * (size_t)n, st);
  download(hi, di, sizeof(int) * (size_t)n, st);
  check_hip(hipStreamSynchronize(st), "SimpleEnergyVAD block");
  blk_n_ = n;
  blk_pos_ = 0;
  blk_cap_ = (long)cap;
}

bool SimpleEnergyVAD::next(int frame_no)
{
  if (frame_no == frame_no_) return is_speech_;
  if (frame_no >= 0 && frame_no - 1 != frame_no_)
    throw jindex_error("Problem speech activity detector: %d != %d\n", frame_no - 1, frame_no_);
  if (blk_pos_ >= blk_n_) fill_();
  const long pos = blk_pos_++;
  const float* f = static_cast<const float*>(h_in_.get()) + 2 * (size_t)fftLen_ * (size_t)pos;
  for (size_t i = 0; i < 2 * (size_t)fftLen_; i++) frame_->data[i] = f[i];
  const double* hs = static_cast<const double*>(h_out_.get());
  const int* hi = reinterpret_cast<const int*>(hs + blk_cap_ + 1);
  cur_s_ = hs[pos];
  is_speech_ = hi[pos] != 0;
  increment_();
  return is_speech_;
}

// ================================================================================ the hangover nodes (sad.cc:1712-1951)
HangoverVADFeature::HangoverVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& metric, double threshold,
                                       unsigned headN, unsigned tailN, const String& nm)
    : VectorFloatFeatureStream(source->size(), nm), decision_metric_(0), source_(source), headN_(headN), tailN_(tailN),
      rule_(BTK_VAD_RULE_SINGLE), block_frames_(btk_vad_default_block_frames()), launches_(0)
{
  init_(metric, threshold);
}

HangoverVADFeature::HangoverVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& metric, double threshold,
                                       unsigned headN, unsigned tailN, const String& nm, int rule)
    : VectorFloatFeatureStream(source->size(), nm), decision_metric_(0), source_(source), headN_(headN), tailN_(tailN), rule_(rule),
      block_frames_(btk_vad_default_block_frames()), launches_(0)
{
  init_(metric, threshold);
}

void HangoverVADFeature::init_(const VADMetricPtr& metric, double threshold)
{
  if (headN_ == 0) throw jdimension_error("Feature %s: headN = 0 (the reference divides by it)\n", name().c_str());
  metricList_.push_back(MetricPair_(metric, threshold));
  rewind_();
}

void HangoverVADFeature::rewind_()
{
  seen_ = 0;
  start_ = end_ = -1;
  end_code_ = 0;
  src_end_ = false;
  state_fresh_ = true;
  carry_.clear();
  queue_.clear();
  decision_metric_ = 0;
}

void HangoverVADFeature::reset()
{
  source_->reset();
  VectorFloatFeatureStream::reset();
  rewind_();
  for (size_t m = 0; m < metricList_.size(); m++) metricList_[m].first->reset();
}

void HangoverVADFeature::next_speaker()
{
  source_->reset();
  VectorFloatFeatureStream::reset();
  rewind_();
  for (size_t m = 0; m < metricList_.size(); m++) metricList_[m].first->next_speaker();
}

const gsl_vector_float* HangoverVADFeature::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  if (frame_no >= 0 && frame_no - 1 != frame_no_)
    throw jindex_error("Problem in Feature %s: %d != %d\n", name().c_str(), frame_no - 1, frame_no_);
  while (queue_.empty()) {
    if (end_ >= 0) { decision_metric_ = end_code_; is_end_ = true; throw jiterator_error("end of samples!"); }
    if (src_end_ || !fill_()) { is_end_ = true; throw jiterator_error("end of samples!"); }
  }
  memcpy(vector_->data, queue_.front().first.data(), sizeof(float) * size());
  decision_metric_ = queue_.front().second;
  queue_.pop_front();
  increment_();
  return vector_;
}

// one block: the source's frames and, frame by frame behind them, the metrics' own; the machine over the metrics' rows
bool HangoverVADFeature::fill_()
{
  const size_t D = size(), R = metricList_.size();
  const long cap = block_frames_;
  float* in = static_cast<float*>(h_in_.ensure(sizeof(float) * D * (size_t)cap));
  for (size_t m = 0; m < R; m++) metricList_[m].first->begin_block(cap);
  long n = 0;
  try {
    for (; n < cap; n++) {
      const gsl_vector_float* v = source_->next((int)(seen_ + n));
      memcpy(in + D * (size_t)n, v->data, sizeof(float) * D);
      for (size_t m = 0; m < R; m++) metricList_[m].first->stage_frame((int)(seen_ + n));
    }
  } catch (jiterator_error&) {
    src_end_ = true;
  }
  if (n == 0) return false;
  const double* rows[8];
  double thr[8];
  for (size_t m = 0; m < R; m++) {
    rows[m] = metricList_[m].first->flush_staged(n);
    thr[m] = metricList_[m].second;
  }
  hipStream_t st = nstream();
  // host block: the state int64 [8], then the decisions int32 [cap]
  long long* hstate = static_cast<long long*>(h_out_.ensure(sizeof(long long) * 8 + sizeof(int) * (size_t)cap));
  int* hdec = reinterpret_cast<int*>(hstate + 8);
  long long* dstate = static_cast<long long*>(d_state_.get() ? d_state_.get() : d_state_.ensure(sizeof(long long) * 8));
  int* ddec = static_cast<int*>(d_decision_.ensure(sizeof(int) * (size_t)cap));
  if (state_fresh_) {
    const long long init[8] = {0, 0, 0, 0, -1, -1, 0, 0};
    memcpy(hstate, init, sizeof(init));
    upload(dstate, hstate, sizeof(init), st);
    check_hip(hipStreamSynchronize(st), "hangover state");       // hstate takes the download below
    state_fresh_ = false;
  }
  check_abi(btk_vad_hangover(rows, thr, (int)R, rule_, 1, n, cap, headN_, tailN_, 0, dstate, ddec, cap, NULL, 0, NULL, st));
  launches_++;
  download(hstate, dstate, sizeof(long long) * 8, st);
  download(hdec, ddec, sizeof(int) * (size_t)n, st);
  check_hip(hipStreamSynchronize(st), "hangover block");
  const long base = seen_, lim_blk = base + n;
  seen_ = lim_blk;
  const long new_start = (long)hstate[4], new_end = (long)hstate[5];
  const long lim = new_end >= 0 ? new_end : lim_blk;
  if (start_ < 0) {
    if (new_start >= 0) {
      start_ = new_start;
      // the frames held back until the onset carry the code of the frame that made it (no metric runs while they are served)
      const long onset = start_ + (long)headN_ - 1;
      for (long f = start_; f < lim; f++) {
        const int code = hdec[std::max(f, onset) - base];
        if (f < base) queue_.push_back(std::make_pair(carry_[(size_t)(f - (base - (long)carry_.size()))], code));
        else queue_.push_back(std::make_pair(std::vector<float>(in + D * (size_t)(f - base), in + D * (size_t)(f - base + 1)), code));
      }
      carry_.clear();
    } else {
      for (long j = std::max(0l, n - ((long)headN_ - 1)); j < n; j++) carry_.push_back(std::vector<float>(in + D * (size_t)j, in + D * (size_t)(j + 1)));
      while (carry_.size() > (size_t)headN_ - 1) carry_.pop_front();
    }
  } else {
    for (long f = base; f < lim; f++)
      queue_.push_back(std::make_pair(std::vector<float>(in + D * (size_t)(f - base), in + D * (size_t)(f - base + 1)), hdec[f - base]));
  }
  if (new_end >= 0) {
    end_ = new_end;
    end_code_ = hdec[new_end - base];
  }
  return true;
}

HangoverMIVADFeature::HangoverMIVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& energyMetric,
                                           const VADMetricPtr& mutualInformationMetric, const VADMetricPtr& powerMetric,
                                           double energyThreshold, double mutualInformationThreshold, double powerThreshold,
                                           unsigned headN, unsigned tailN, const String& nm)
    : HangoverVADFeature(source, energyMetric, energyThreshold, headN, tailN, nm, BTK_VAD_RULE_MI)
{
  metricList_.push_back(MetricPair_(mutualInformationMetric, mutualInformationThreshold));
  metricList_.push_back(MetricPair_(powerMetric, powerThreshold));
}

HangoverMultiStageVADFeature::HangoverMultiStageVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& energyMetric,
                                                           double energyThreshold, unsigned headN, unsigned tailN, const String& nm)
    : HangoverVADFeature(source, energyMetric, energyThreshold, headN, tailN, nm, BTK_VAD_RULE_MULTISTAGE)
{
}

void HangoverMultiStageVADFeature::set_metric(const VADMetricPtr& metricPtr, double threshold)
{
  if (metricList_.size() >= 8) throw jdimension_error("Feature %s: at most 8 metrics\n", name().c_str());
  metricList_.push_back(MetricPair_(metricPtr, threshold));
}
