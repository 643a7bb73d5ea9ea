// ss_nodes.cc -- SpectralSubtractor, WienerFilter (postfilter/spectralsubtraction.h) and HighPassFilter (postfilter/postfilter.h)
// over btk_ss_process / btk_wiener_process / btk_spec_highpass (csrc/ss_kernels.hip), and the host classes PSDEstimator /
// AveragePSDEstimator.  The block machinery and the mode-switch protocol are described in postfilter/enhancement_node.h.
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "postfilter/spectralsubtraction.h"
#include "postfilter/postfilter.h"
#include "node_runtime.h"

namespace {

using btknode::check_abi;
using btknode::nstream;
using btknode::d2h;
using btknode::h2d;
using btknode::even_pitch;
using btknode::d2d_async;
using btknode::d2d_2d_async;
using btknode::h2d_async;
using btknode::dev_zero_async;

}  // namespace

// ================================================================================ the block machinery
EnhancementBlockNode_::EnhancementBlockNode_(unsigned fftLen, bool channel_major, const String& nm)
    : VectorComplexFeatureStream(fftLen, nm), fftLen_(fftLen), channel_major_(channel_major), block_frames_(btk_default_block_frames()),
      prepared_(false), ended_(false), state_ready_(false), dirty_(false), base_(0), T_(0), Ts_(0), seg0_(0), handed_(-1), served_(0),
      fd0_(0), version_(0), Yhost_valid_(false)
{
  if (fftLen_ < 2 || (fftLen_ & 1) || fftLen_ > 2048)
    throw jdimension_error("%s: %d subbands are outside this engine's enhancement nodes (even, at most 2048)\n", nm.c_str(), (int)fftLen_);
}

void EnhancementBlockNode_::add_source_(const VectorComplexFeatureStreamPtr& s)
{
  if (s->size() != fftLen_)
    throw jdimension_error("%s: a source of %d subbands where %d are expected\n", name().c_str(), (int)s->size(), (int)fftLen_);
  if (prepared_ || state_ready_) throw jconsistency_error("%s: set every channel before the stream runs or a noise model is read\n", name().c_str());
  if ((int)srcs_.size() >= btk_ss_max_channels())
    throw jdimension_error("%s: more than %d channels\n", name().c_str(), btk_ss_max_channels());
  srcs_.push_back(s);
  dPcm_.push_back(std::unique_ptr<DeviceBuffer>(new DeviceBuffer()));
  banks_.clear();
  for (size_t i = 0; i < srcs_.size(); i++) {
    OverSampledDFTAnalysisBank* b = dynamic_cast<OverSampledDFTAnalysisBank*>(srcs_[i].operator->());
    if (!b) { banks_.clear(); break; }
    banks_.push_back(b);
  }
  bsrcs_.clear();
  for (size_t i = 0; i < srcs_.size() && banks_.empty(); i++) {
    BlockSource* b = dynamic_cast<BlockSource*>(srcs_[i].operator->());
    if (!b || !b->has_block()) { bsrcs_.clear(); break; }
    bsrcs_.push_back(b);
  }
}

void EnhancementBlockNode_::alloc_state_()
{
  if (state_ready_) return;
  const size_t n = state_bytes_();
  if (n) {
    init_state_(dState_.ensure(n));
    d2d_async(dSnap_.ensure(n), dState_.get(), n);
  }
  state_ready_ = true;
}

// every source is an analysis bank: each hands over the window of samples its next frames need (pinned host memory) and the
// frames are computed on the device, into the rows the kernel reads
bool EnhancementBlockNode_::gather_banks_(long f0, long& Tn)
{
  const size_t C = srcs_.size();
  long f1 = -1;
  for (size_t i = 0; i < C; i++) {
    OverSampledDFTAnalysisBank* b = banks_[i];
    while (!b->at_end() && b->frames_ready() <= f0) b->pull_more();
    const long r = b->frames_ready();
    f1 = (f1 < 0 || r < f1) ? r : f1;
  }
  if (f1 <= f0) return false;                                   // unequal lengths end at the shortest source
  // blocks end on multiples of 64 of the frame counter while the stream lasts (what is left over stays in the banks' windows):
  // a scan chunk is then never cut by a block, and the results do not depend on the banks' block_frames()
  for (;;) {
    bool all_ended = true;
    for (size_t i = 0; i < C; i++) all_ended = all_ended && banks_[i]->at_end();
    if (all_ended) break;
    if ((f1 & ~63L) > f0) { f1 &= ~63L; break; }
    long r1 = -1;
    for (size_t i = 0; i < C; i++) {
      if (!banks_[i]->at_end()) banks_[i]->pull_more();
      const long r = banks_[i]->frames_ready();
      r1 = (r1 < 0 || r < r1) ? r : r1;
    }
    f1 = r1;
  }
  Tn = f1 - f0;
  const unsigned K = fftLen_ / 2 + 1;
  const long Ts = even_pitch(Tn);
  char* dx = static_cast<char*>(dX_.ensure(sizeof(float) * 2 * K * C * Ts));
  for (size_t i = 0; i < C; i++) {
    OverSampledDFTAnalysisBank* b = banks_[i];
    const long D = (long)b->shiftlen();
    const long b0 = b->first_block_of_frame(f0);
    if (b->window_first_block() > b0)
      throw jconsistency_error("%s: analysis bank %s is pulled by another node as well; this node needs its sources for itself\n",
                               name().c_str(), b->name().c_str());
    const long L = (b->blocks_pulled() - b0) * D;               // (samples past the end of an ended source read as zeros)
    float* dp = static_cast<float*>(dPcm_[i]->ensure(sizeof(float) * (L > 0 ? L : 1)));
    if (L > 0) h2d_async(dp, b->window(b0), sizeof(float) * L);
    if (C == 1) {
      check_abi(btk_fb_analysis(b->plan(), dp, L > 0 ? L : 0, L > 0 ? L : 1, 1, 1, dx, Ts, f0 - b0, Tn, nstream()));
    } else {
      void* dc = dCh_.ensure(sizeof(float) * 2 * K * Ts);
      check_abi(btk_fb_analysis(b->plan(), dp, L > 0 ? L : 0, L > 0 ? L : 1, 1, 1, dc, Ts, f0 - b0, Tn, nstream()));
      const size_t row = sizeof(float) * 2 * Ts;
      char* dst = channel_major_ ? dx + i * K * row : dx + i * row;
      d2d_2d_async(dst, channel_major_ ? row : C * row, dc, row, sizeof(float) * 2 * Tn, K);
    }
  }
  btk_node_synchronize();                                       // the windows move when the banks release what is done
  for (size_t i = 0; i < C; i++) banks_[i]->release_before(f1);
  Ts_ = Ts;
  return true;
}

// any other set of sources: frame by frame through next(), every channel in order, as the reference pulls them
bool EnhancementBlockNode_::gather_next_(long f0, long& Tn)
{
  const unsigned K = fftLen_ / 2 + 1;
  const size_t C = srcs_.size();
  std::vector<float> fr;                                        // [T][C][K]
  long T = 0;
  while (!ended_ && (block_frames_ == 0 || T < block_frames_)) {
    fr.resize((size_t)(T + 1) * C * K * 2);
    bool got = true;
    for (size_t c = 0; c < C && got; c++) {
      const gsl_vector_complex* v;
      try { v = srcs_[c]->next((int)(f0 + T)); } catch (jiterator_error&) { ended_ = true; got = false; break; }
      float* dst = &fr[2 * (((size_t)T * C + c) * K)];
      for (unsigned k = 0; k < K; k++) {
        dst[2 * k] = (float)v->data[2 * k * v->stride];
        dst[2 * k + 1] = (float)v->data[2 * k * v->stride + 1];
      }
    }
    if (!got) break;
    T++;
  }
  if (T == 0) return false;
  const long Ts = even_pitch(T);
  const size_t n = sizeof(float) * 2 * K * C * Ts;
  float* hx = static_cast<float*>(hX_.ensure(n));
  memset(hx, 0, n);
  for (long t = 0; t < T; t++)
    for (size_t c = 0; c < C; c++)
      for (unsigned k = 0; k < K; k++) {
        const size_t row = channel_major_ ? c * K + k : (size_t)k * C + c;
        hx[2 * (row * Ts + t)] = fr[2 * (((size_t)t * C + c) * K + k)];
        hx[2 * (row * Ts + t) + 1] = fr[2 * (((size_t)t * C + c) * K + k) + 1];
      }
  h2d(dX_.ensure(n), hx, n);                                    // (synchronised: the pinned rows are rewritten by the next block)
  Tn = T; Ts_ = Ts;
  return true;
}

// every source offers its block on the device: the blocks are copied into the rows the kernel reads, device to device
void EnhancementBlockNode_::copy_source_blocks_(long T)
{
  const unsigned K = fftLen_ / 2 + 1;
  const size_t C = srcs_.size();
  const size_t row = sizeof(float) * 2 * Ts_;
  char* dx = static_cast<char*>(dX_.get());
  for (size_t i = 0; i < C; i++) {
    long Ti = 0, Tsi = 0;
    const void* p = bsrcs_[i]->device_block(Ti, Tsi);
    if (!p || Ti != T)
      throw jconsistency_error("%s: source %d changed the length of its block (%ld -> %ld frames)\n", name().c_str(), (int)i, T, Ti);
    char* dst = channel_major_ ? dx + i * K * row : dx + i * row;
    d2d_2d_async(dst, channel_major_ ? row : C * row, p, sizeof(float) * 2 * Tsi, sizeof(float) * 2 * T, K);
    src_versions_[i] = bsrcs_[i]->block_version();
  }
}

bool EnhancementBlockNode_::gather_blocks_(bool advance, long f0, long& Tn)
{
  const unsigned K = fftLen_ / 2 + 1;
  const size_t C = srcs_.size();
  if (advance)
    for (size_t i = 0; i < C; i++)
      if (!bsrcs_[i]->next_block()) return false;
  long T = -1;
  for (size_t i = 0; i < C; i++) {
    long Ti = 0, Tsi = 0;
    const void* p = bsrcs_[i]->device_block(Ti, Tsi);
    if (!p || Ti <= 0) return false;
    if (bsrcs_[i]->block_base() != f0 || (T >= 0 && Ti != T))
      throw jconsistency_error("%s: the blocks of the sources do not line up (source %d: frames %ld .. %ld, expected from %ld); "
                               "give the sources one block size\n", name().c_str(), (int)i, bsrcs_[i]->block_base(),
                               bsrcs_[i]->block_base() + Ti, f0);
    T = Ti;
  }
  Ts_ = even_pitch(T);
  dX_.ensure(sizeof(float) * 2 * K * C * Ts_);
  src_versions_.assign(C, 0);
  copy_source_blocks_(T);
  Tn = T;
  return true;
}

// a source has recomputed the frames behind its mark (new weights upstream): its block is taken again, and this node's frames
// from the segment's start on are due again -- those up to the mark come out with the bits they had
void EnhancementBlockNode_::poll_sources_()
{
  if (bsrcs_.empty() || !prepared_ || T_ == 0) return;
  bool changed = false;
  for (size_t i = 0; i < bsrcs_.size(); i++) changed = changed || bsrcs_[i]->block_version() != src_versions_[i];
  if (!changed) return;
  copy_source_blocks_(T_);
  dirty_ = true;
  version_++;
}

unsigned long EnhancementBlockNode_::block_version()
{
  poll_sources_();
  return version_;
}

void EnhancementBlockNode_::advance_to(long frame_idx)
{
  if (frame_idx > handed_) handed_ = frame_idx;
  for (size_t i = 0; i < bsrcs_.size(); i++) bsrcs_[i]->advance_to(frame_idx);
}

void EnhancementBlockNode_::ensure_current_()
{
  poll_sources_();
  if (!dirty_) return;
  const size_t n = state_bytes_();
  if (n) d2d_async(dState_.get(), dSnap_.get(), n);
  if (T_ > seg0_) launch_(dX_.get(), dY_.get(), Ts_, seg0_, T_, fd0_ + base_ + seg0_);
  dirty_ = false;
  Yhost_valid_ = false;
}

bool EnhancementBlockNode_::load_block_()
{
  if (srcs_.empty()) throw jconsistency_error("%s: no channel is set\n", name().c_str());
  alloc_state_();
  ensure_current_();                                            // the state after the block that ends here
  long Tn = 0;
  const long f0 = base_ + T_;
  const bool got = !banks_.empty() ? gather_banks_(f0, Tn) : !bsrcs_.empty() ? gather_blocks_(prepared_, f0, Tn) : gather_next_(f0, Tn);
  if (!got) return false;
  const unsigned K = fftLen_ / 2 + 1;
  dY_.ensure(sizeof(float) * 2 * K * Ts_);
  const size_t n = state_bytes_();
  if (n) d2d_async(dSnap_.get(), dState_.get(), n);
  base_ = f0; T_ = Tn; seg0_ = 0;
  launch_(dX_.get(), dY_.get(), Ts_, 0, T_, fd0_ + base_);
  dirty_ = false; Yhost_valid_ = false; prepared_ = true;
  return true;
}

void* EnhancementBlockNode_::begin_switch_(bool need_state)
{
  if (!need_state && !state_ready_) return NULL;
  alloc_state_();
  const size_t n = state_bytes_();
  if (prepared_ && T_ > 0) {
    poll_sources_();
    const long n1 = std::min(std::max(handed_ + 1 - base_, seg0_), T_);
    if (n) d2d_async(dState_.get(), dSnap_.get(), n);
    if (n1 > seg0_) {
      // the frames between the segment's start and the mark once more, into a scratch block: what was handed over stays as it is
      const unsigned K = fftLen_ / 2 + 1;
      launch_(dX_.get(), dTmp_.ensure(sizeof(float) * 2 * K * Ts_), Ts_, seg0_, n1, fd0_ + base_ + seg0_);
    }
    seg0_ = n1;
    dirty_ = true;
    version_++;
  }
  return n ? dState_.get() : NULL;
}

void* EnhancementBlockNode_::begin_peek_()
{
  alloc_state_();
  const size_t n = state_bytes_();
  if (!n) return NULL;
  if (prepared_ && T_ > 0) {
    poll_sources_();
    const long n1 = std::min(std::max(handed_ + 1 - base_, seg0_), T_);
    d2d_async(dPeek_.ensure(n), dState_.get(), n);
    d2d_async(dState_.get(), dSnap_.get(), n);
    if (n1 > seg0_) {
      const unsigned K = fftLen_ / 2 + 1;
      launch_(dX_.get(), dTmp_.ensure(sizeof(float) * 2 * K * Ts_), Ts_, seg0_, n1, fd0_ + base_ + seg0_);
    }
  }
  return dState_.get();
}

void EnhancementBlockNode_::end_peek_()
{
  const size_t n = state_bytes_();
  if (n && prepared_ && T_ > 0) d2d_async(dState_.get(), dPeek_.get(), n);
}

void EnhancementBlockNode_::end_switch_()
{
  if (!state_ready_) return;
  const size_t n = state_bytes_();
  if (n) d2d_async(dSnap_.get(), dState_.get(), n);
}

const float* EnhancementBlockNode_::host_output_()
{
  ensure_current_();
  if (!Yhost_valid_) {
    Yhost_.resize((size_t)2 * (fftLen_ / 2 + 1) * Ts_);
    d2h(Yhost_.data(), dY_.get(), sizeof(float) * Yhost_.size());
    Yhost_valid_ = true;
  }
  return Yhost_.data();
}

const gsl_vector_complex* EnhancementBlockNode_::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  if (frame_no >= 0 && frame_no - 1 != frame_no_)
    throw jindex_error("Problem in Feature %s: %d != %d\n", name().c_str(), frame_no - 1, frame_no_);
  const long idx = served_;
  while (!prepared_ || idx >= base_ + T_)
    if (!load_block_()) { is_end_ = true; throw jiterator_error("end of samples!"); }
  const float* Y = host_output_();
  const unsigned M = fftLen_, K = M / 2 + 1;
  const long t = idx - base_;
  for (unsigned k = 0; k < K; k++) {
    const double re = Y[2 * ((size_t)k * Ts_ + t)], im = Y[2 * ((size_t)k * Ts_ + t) + 1];
    vector_->data[2 * k] = re; vector_->data[2 * k + 1] = im;
    if (k > 0 && k < M / 2) { vector_->data[2 * (M - k)] = re; vector_->data[2 * (M - k) + 1] = -im; }
  }
  served_++;
  advance_to(idx);
  increment_();
  return vector_;
}

// The sources restart; the recursion state lives on as a per-frame graph would have left it: at the mark (SpectralSubtractor::reset
// keeps its estimators, spectralsubtraction.cc:163-179; WienerFilter::reset its PSDs and frame counter, :364-368).
void EnhancementBlockNode_::reset()
{
  if (prepared_ && T_ > 0) {
    begin_switch_();
    end_switch_();
    fd0_ += std::max<long>(handed_ + 1, 0);
  }
  for (size_t i = 0; i < srcs_.size(); i++) srcs_[i]->reset();
  if (!keeps_frame_counter_on_reset_()) VectorComplexFeatureStream::reset();
  else is_end_ = false;
  prepared_ = false; ended_ = false; dirty_ = false; base_ = 0; T_ = 0; Ts_ = 0; seg0_ = 0; handed_ = -1; served_ = 0;
  Yhost_valid_ = false; Yhost_.clear();
  version_++;
}

void EnhancementBlockNode_::ensure_first_()
{
  if (!prepared_ && !load_block_()) { T_ = 0; prepared_ = true; }
}

const std::vector<float>& EnhancementBlockNode_::block(long& T)
{
  ensure_first_();
  T = T_;
  if (T_ == 0) { Yhost_.clear(); return Yhost_; }
  host_output_();
  if (Ts_ != T_) {                                              // the host view of a block is dense: [K][T]
    const unsigned K = fftLen_ / 2 + 1;
    dense_.resize((size_t)2 * K * T_);
    for (unsigned k = 0; k < K; k++) memcpy(&dense_[2 * (size_t)k * T_], &Yhost_[2 * (size_t)k * Ts_], sizeof(float) * 2 * T_);
    return dense_;
  }
  return Yhost_;
}

const void* EnhancementBlockNode_::device_block(long& T, long& T_stride)
{
  ensure_first_();
  ensure_current_();
  T = T_; T_stride = Ts_;
  return T_ ? dY_.get() : NULL;
}

long EnhancementBlockNode_::block_base()
{
  ensure_first_();
  return base_;
}

bool EnhancementBlockNode_::next_block()
{
  ensure_first_();
  return load_block_();
}

// ================================================================================ PSDEstimator / AveragePSDEstimator (host)
PSDEstimator::PSDEstimator(unsigned fftLen2) { estimates_ = gsl_vector_calloc(fftLen2 + 1); }
PSDEstimator::~PSDEstimator() { gsl_vector_free(estimates_); }

bool PSDEstimator::read_estimates(const String& fn)
{
  FILE* fp = fopen(fn.c_str(), "r");
  if (!fp) { fprintf(stderr, "could not read %s\n", fn.c_str()); return false; }
  for (size_t i = 0; i < estimates_->size; i++) {
    double val;
    if (fscanf(fp, "%lf\n", &val) == 1) gsl_vector_set(estimates_, i, val);
  }
  fclose(fp);
  return true;
}

bool PSDEstimator::write_estimates(const String& fn)
{
  FILE* fp = fopen(fn.c_str(), "w");
  if (!fp) { fprintf(stderr, "could not write %s\n", fn.c_str()); return false; }
  for (size_t i = 0; i < estimates_->size; i++) fprintf(fp, "%lf\n", gsl_vector_get(estimates_, i));
  fclose(fp);
  return true;
}

AveragePSDEstimator::AveragePSDEstimator(unsigned fftLen2, float alpha) : PSDEstimator(fftLen2), alpha_(alpha), sample_added_(false) {}
AveragePSDEstimator::~AveragePSDEstimator() { clear_samples(); }

void AveragePSDEstimator::clear_samples()
{
  for (std::list<gsl_vector*>::iterator it = sampleL_.begin(); it != sampleL_.end(); ++it) gsl_vector_free(*it);
  sampleL_.clear();
}

void AveragePSDEstimator::clear()
{
  sample_added_ = false;
  clear_samples();
}

const gsl_vector* AveragePSDEstimator::average()
{
  if (alpha_ < 0) {
    unsigned n = 0;
    for (size_t i = 0; i < estimates_->size; i++) gsl_vector_set(estimates_, i, 0.0);
    for (std::list<gsl_vector*>::iterator it = sampleL_.begin(); it != sampleL_.end(); ++it, n++)
      for (size_t i = 0; i < estimates_->size; i++) gsl_vector_set(estimates_, i, gsl_vector_get(estimates_, i) + gsl_vector_get(*it, i));
    const double scale = 1.0 / (float)n;
    for (size_t i = 0; i < estimates_->size; i++) gsl_vector_set(estimates_, i, gsl_vector_get(estimates_, i) * scale);
  }
  return estimates_;
}

bool AveragePSDEstimator::add_sample(const gsl_vector_complex* sample)
{
  const size_t n = estimates_->size;
  gsl_vector* tmp = gsl_vector_calloc(n);
  for (size_t i = 0; i < n; i++) {
    const double re = sample->data[2 * i * sample->stride], im = sample->data[2 * i * sample->stride + 1];
    gsl_vector_set(tmp, i, re * re + im * im);
  }
  if (alpha_ < 0) { sampleL_.push_back(tmp); return true; }
  if (!sample_added_) {
    for (size_t i = 0; i < n; i++) gsl_vector_set(estimates_, i, gsl_vector_get(tmp, i));
    sample_added_ = true;
  } else {
    for (size_t i = 0; i < n; i++)
      gsl_vector_set(estimates_, i, gsl_vector_get(estimates_, i) * alpha_ + gsl_vector_get(tmp, i) * (1.0 - alpha_));
  }
  gsl_vector_free(tmp);
  return true;
}

// ================================================================================ SpectralSubtractor
SpectralSubtractor::SpectralSubtractor(unsigned fftLen, bool halfBandShift, float ft, float flooringV, const String& nm)
    : EnhancementBlockNode_(fftLen, false, nm), halfBandShift_(halfBandShift), training_started_(true),
      start_noise_subtraction_(false), ft_(ft), flooringV_(flooringV) {}
SpectralSubtractor::~SpectralSubtractor() {}

// device state: est [C][K] | acc [C][K] float64, count [C] int64, added [C] uint8
size_t SpectralSubtractor::state_bytes_() const
{
  const size_t C = alphas_.size(), K = fftLen_ / 2 + 1;
  return sizeof(double) * 2 * C * K + sizeof(long long) * C + ((C + 15) & ~(size_t)15);
}
double* SpectralSubtractor::est_(void* st) const { return static_cast<double*>(st); }
double* SpectralSubtractor::acc_(void* st) const { return static_cast<double*>(st) + alphas_.size() * (fftLen_ / 2 + 1); }
long long* SpectralSubtractor::count_(void* st) const { return reinterpret_cast<long long*>(static_cast<double*>(st) + 2 * alphas_.size() * (fftLen_ / 2 + 1)); }
unsigned char* SpectralSubtractor::added_(void* st) const { return reinterpret_cast<unsigned char*>(count_(st) + alphas_.size()); }

void SpectralSubtractor::init_state_(void* d)
{
  dev_zero_async(d, state_bytes_());
}

void SpectralSubtractor::launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long frames_done)
{
  void* st = state_dev_();
  const int mode = (training_started_ ? BTK_SS_TRAIN : 0) | (start_noise_subtraction_ ? BTK_SS_SUBTRACT : 0);
  check_abi(btk_ss_process(static_cast<const float*>(dX) + 2 * t0, static_cast<float*>(dOut) + 2 * t0, 1, (int)fftLen_,
                           (int)alphas_.size(), Ts, t1 - t0, NULL, mode, ft_, flooringV_, alphas_.data(), frames_done, est_(st),
                           acc_(st), count_(st), added_(st), BTK_SS_FORM_AUTO, btk_node_stream()));
}

void SpectralSubtractor::set_channel(VectorComplexFeatureStreamPtr& chan, double alpha)
{
  add_source_(chan);
  alphas_.push_back((double)(float)alpha);                      // AveragePSDEstimator holds a float
}

void SpectralSubtractor::check_idx_(unsigned idx) const
{
  if (idx >= alphas_.size()) throw jindex_error("%s: channel %d of %d\n", name().c_str(), (int)idx, (int)alphas_.size());
}

void SpectralSubtractor::start_training() { begin_switch_(false); training_started_ = true; end_switch_(); }
void SpectralSubtractor::start_noise_subtraction() { begin_switch_(false); start_noise_subtraction_ = true; end_switch_(); }
void SpectralSubtractor::stop_noise_subtraction() { begin_switch_(false); start_noise_subtraction_ = false; end_switch_(); }
void SpectralSubtractor::set_noise_over_estimation_factor(float ft) { begin_switch_(false); ft_ = ft; end_switch_(); }

void SpectralSubtractor::stop_training()
{
  void* st = begin_switch_();
  training_started_ = false;
  if (!alphas_.empty())
    check_abi(btk_ss_finish_training(1, (int)fftLen_, (int)alphas_.size(), alphas_.data(), est_(st), acc_(st), count_(st), btk_node_stream()));
  end_switch_();
}

void SpectralSubtractor::clear_noise_samples()
{
  void* st = begin_switch_();
  if (!alphas_.empty()) check_abi(btk_ss_clear(1, (int)fftLen_, (int)alphas_.size(), 0, acc_(st), count_(st), added_(st), btk_node_stream()));
  end_switch_();
}

void SpectralSubtractor::clear()
{
  void* st = begin_switch_();
  if (!alphas_.empty()) check_abi(btk_ss_clear(1, (int)fftLen_, (int)alphas_.size(), 1, acc_(st), count_(st), added_(st), btk_node_stream()));
  end_switch_();
}

bool SpectralSubtractor::read_noise_file(const String& fn, unsigned idx)
{
  check_idx_(idx);
  void* st = begin_switch_();
  training_started_ = false;                                    // :204-207, whether or not the file can be read
  const unsigned K = fftLen_ / 2 + 1;
  PSDEstimator e(fftLen_ / 2);
  d2h(e.estimate()->data, est_(st) + (size_t)idx * K, sizeof(double) * K);     // bins the file does not name stay as they are
  const bool ok = e.read_estimates(fn);
  if (ok) h2d(est_(st) + (size_t)idx * K, e.estimate()->data, sizeof(double) * K);
  end_switch_();
  return ok;
}

std::vector<double> SpectralSubtractor::noise_psd(unsigned idx)
{
  check_idx_(idx);
  void* st = begin_peek_();
  const unsigned K = fftLen_ / 2 + 1;
  std::vector<double> r(K);
  d2h(r.data(), est_(st) + (size_t)idx * K, sizeof(double) * K);
  end_peek_();
  return r;
}

bool SpectralSubtractor::write_noise_file(const String& fn, unsigned idx)
{
  const std::vector<double> r = noise_psd(idx);
  PSDEstimator e(fftLen_ / 2);
  memcpy(e.estimate()->data, r.data(), sizeof(double) * r.size());
  return e.write_estimates(fn);
}

// ================================================================================ WienerFilter
WienerFilter::WienerFilter(VectorComplexFeatureStreamPtr& targetSignal, VectorComplexFeatureStreamPtr& noiseSignal, bool halfBandShift,
                           float alpha, float flooringV, double beta, const String& nm)
    : EnhancementBlockNode_(targetSignal->size(), true, nm), halfBandShift_(halfBandShift), alpha_(alpha), flooringV_(flooringV),
      beta_((float)beta), update_noise_PSD_(true)
{
  if (fftLen_ != noiseSignal->size())
    throw jdimension_error("Input block length (%d) != fftLen (%d)\n", (int)fftLen_, (int)noiseSignal->size());
  add_source_(targetSignal);
  add_source_(noiseSignal);
}

size_t WienerFilter::state_bytes_() const { return sizeof(double) * 2 * (fftLen_ / 2 + 1); }      // psd_s [K] | psd_n [K]
void WienerFilter::init_state_(void* d) { dev_zero_async(d, state_bytes_()); }

void WienerFilter::launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long frames_done)
{
  const unsigned K = fftLen_ / 2 + 1;
  double* st = static_cast<double*>(state_dev_());
  const float* sx = static_cast<const float*>(dX) + 2 * t0;
  check_abi(btk_wiener_process(sx, sx + 2 * (size_t)K * Ts, static_cast<float*>(dOut) + 2 * t0, 1, (int)fftLen_, Ts, t1 - t0, NULL,
                               update_noise_PSD_ ? BTK_WIENER_UPDATE_NOISE : 0, alpha_, flooringV_, beta_, frames_done, st, st + K,
                               btk_node_stream()));
}

const gsl_vector_complex* WienerFilter::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  if (halfBandShift_) throw j_error("WienerFilter::next() for the half band shift is not implemented\n");
  return EnhancementBlockNode_::next(frame_no);
}

void WienerFilter::set_noise_amplification_factor(double beta) { begin_switch_(false); beta_ = (float)beta; end_switch_(); }
void WienerFilter::start_updating_noise_PSD() { begin_switch_(false); update_noise_PSD_ = true; end_switch_(); }
void WienerFilter::stop_updating_noise_PSD() { begin_switch_(false); update_noise_PSD_ = false; end_switch_(); }

std::vector<double> WienerFilter::psd_(int which)
{
  const unsigned K = fftLen_ / 2 + 1;
  double* st = static_cast<double*>(begin_peek_());
  std::vector<double> r(K);
  d2h(r.data(), st + (size_t)which * K, sizeof(double) * K);
  end_peek_();
  return r;
}
std::vector<double> WienerFilter::target_psd() { return psd_(0); }
std::vector<double> WienerFilter::noise_psd() { return psd_(1); }

// ================================================================================ HighPassFilter
HighPassFilter::HighPassFilter(VectorComplexFeatureStreamPtr& output, float cutOffFreq, int sampleRate, const String& nm)
    : EnhancementBlockNode_(output->size(), false, nm)
{
  cutoff_fbinX_ = (unsigned)(fftLen_ * cutOffFreq / (float)sampleRate);
  if (cutoff_fbinX_ > fftLen_ / 2 + 1) cutoff_fbinX_ = fftLen_ / 2 + 1;      // (beyond M/2 both loops of :1221-1235 write zeros only)
  add_source_(output);
}

void HighPassFilter::launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long)
{
  check_abi(btk_spec_highpass(static_cast<const float*>(dX) + 2 * t0, static_cast<float*>(dOut) + 2 * t0, 1, (int)fftLen_,
                              (int)cutoff_fbinX_, Ts, t1 - t0, btk_node_stream()));
}
