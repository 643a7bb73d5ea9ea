// aec_nodes.cc -- the echo-canceller nodes of aec/aec.h over btk_aec_init / btk_aec_process (csrc/aec_kernels.hip).
//
// A block: up to block_frames frames of BOTH sources, cancelled in one launch, the residual left on the device for a consumer
// that takes blocks (the synthesis bank) and mirrored to the host when a frame is asked for.  All of the recursion's state --
// weights, covariances, noise variances, played history, the double-talk scalars -- stays in the device tensors btk_aec_process
// updates, so results do not depend on where the blocks are cut.
#include <algorithm>
#include <cstring>

#include "aec/aec.h"
#include "node_runtime.h"

namespace {

using btknode::check_abi;
using btknode::nstream;
using btknode::d2h;
using btknode::h2d_async;
using btknode::dev_zero_async;
using btknode::even_pitch;

}  // namespace

AcousticEchoCancellationNode_::AcousticEchoCancellationNode_(int kind, const VectorComplexFeatureStreamPtr& played,
                                                             const VectorComplexFeatureStreamPtr& recorded, unsigned sampleN,
                                                             const double* params8, const String& nm)
    : VectorComplexFeatureStream(played->size(), nm), kind_(kind), played_(played), recorded_(recorded), pbank_(NULL), rbank_(NULL),
      fftLen_(played->size()), sampleN_(sampleN), block_frames_(btk_default_block_frames()), prepared_(false), ended_(false),
      state_ready_(false), base_(0), T_(0), Ts_(0), block_frame_arg_(-5), Ehost_valid_(false)
{
  if (recorded->size() != fftLen_)
    throw jdimension_error("%s: the played and the recorded stream differ in size (%d vs. %d)\n", nm.c_str(), (int)fftLen_, (int)recorded->size());
  if (fftLen_ < 2 || (fftLen_ & 1) || fftLen_ > 2048)
    throw jdimension_error("%s: %d subbands are outside this engine's echo cancellers (even, at most 2048)\n", nm.c_str(), (int)fftLen_);
  if (sampleN_ < 1 || (int)sampleN_ > btk_aec_max_filter_length())
    throw jdimension_error("%s: sample_num = %d is outside this engine's echo cancellers (1 .. %d)\n", nm.c_str(), (int)sampleN_,
                           btk_aec_max_filter_length());
  memcpy(params_, params8, sizeof(params_));
  pbank_ = dynamic_cast<OverSampledDFTAnalysisBank*>(played_.operator->());
  rbank_ = dynamic_cast<OverSampledDFTAnalysisBank*>(recorded_.operator->());
  if (!pbank_ || !rbank_) { pbank_ = NULL; rbank_ = NULL; }
}

void AcousticEchoCancellationNode_::alloc_state_()
{
  if (state_ready_) return;
  const size_t K = fftLen_ / 2 + 1, P = sampleN_;
  dR_.ensure(sizeof(double) * 2 * K * P);
  dK_.ensure(sizeof(double) * 2 * K * P * P);
  dSig_.ensure(sizeof(double) * K);
  dHist_.ensure(sizeof(double) * 2 * K * P);
  dDtd_.ensure(sizeof(double) * 4);
  check_abi(btk_aec_init(kind_, params_, 1, (int)fftLen_, (int)sampleN_, dR_.get(), dK_.get(), static_cast<double*>(dSig_.get()),
                         dHist_.get(), static_cast<double*>(dDtd_.get()), nstream()));
  state_ready_ = true;
}

// Both sources are analysis banks: each hands over the window of samples its next frames need (pinned host memory) and the
// frames are computed into the rows the canceller reads -- they never visit the host.
bool AcousticEchoCancellationNode_::load_from_banks_(long& Tn)
{
  const long f0 = base_ + T_;
  OverSampledDFTAnalysisBank* banks[2] = {pbank_, rbank_};
  long f1 = -1;
  for (int i = 0; i < 2; i++) {
    OverSampledDFTAnalysisBank* b = banks[i];
    while (!b->at_end() && b->frames_ready() <= f0) b->pull_more();
    const long r = b->frames_ready();
    f1 = (f1 < 0 || r < f1) ? r : f1;
  }
  if (f1 <= f0) return false;                                   // unequal lengths end at the shorter source
  Tn = f1 - f0;
  const unsigned K = fftLen_ / 2 + 1;
  const long Ts = even_pitch(Tn);
  DeviceBuffer* dPcm[2] = {&dPcmV_, &dPcmA_};
  DeviceBuffer* dX[2] = {&dV_, &dA_};
  for (int i = 0; i < 2; i++) {
    OverSampledDFTAnalysisBank* b = banks[i];
    const long D = (long)b->shiftlen();
    const long b0 = b->first_block_of_frame(f0);
    if (b->window_first_block() > b0)
      throw jconsistency_error("%s: analysis bank %s is pulled by another node as well; an echo canceller needs its sources for itself\n",
                               name().c_str(), b->name().c_str());
    const long L = (b->blocks_pulled() - b0) * D;               // (samples past the end of an ended source read as zeros)
    float* dp = static_cast<float*>(dPcm[i]->ensure(sizeof(float) * (L > 0 ? L : 1)));
    void* dx = dX[i]->ensure(sizeof(float) * 2 * K * Ts);
    if (L > 0) h2d_async(dp, b->window(b0), sizeof(float) * L);
    check_abi(btk_fb_analysis(b->plan(), dp, L > 0 ? L : 0, L > 0 ? L : 1, 1, 1, dx, Ts, f0 - b0, Tn, nstream()));
  }
  btk_node_synchronize();                                       // the windows move when the banks release what is done
  for (int i = 0; i < 2; i++) banks[i]->release_before(f1);
  Ts_ = Ts;
  return true;
}

// Any other pair of sources: frame by frame through next(), as the reference pulls them (aec.cc:49-50)
bool AcousticEchoCancellationNode_::load_by_next_(long& Tn)
{
  const unsigned K = fftLen_ / 2 + 1;
  const long f0 = base_ + T_;
  std::vector<float> fv, fa;                                    // [T][K]
  long T = 0;
  while (!ended_ && (block_frames_ == 0 || T < block_frames_)) {
    const gsl_vector_complex *v, *a;
    try {
      v = played_->next((int)(f0 + T));
      a = recorded_->next((int)(f0 + T));
    } catch (jiterator_error&) { ended_ = true; break; }
    fv.resize((size_t)(T + 1) * K * 2); fa.resize((size_t)(T + 1) * K * 2);
    for (unsigned k = 0; k < K; k++) {
      fv[2 * ((size_t)T * K + k)] = (float)v->data[2 * k * v->stride]; fv[2 * ((size_t)T * K + k) + 1] = (float)v->data[2 * k * v->stride + 1];
      fa[2 * ((size_t)T * K + k)] = (float)a->data[2 * k * a->stride]; fa[2 * ((size_t)T * K + k) + 1] = (float)a->data[2 * k * a->stride + 1];
    }
    T++;
  }
  if (T == 0) return false;
  const long Ts = even_pitch(T);
  float* hv = static_cast<float*>(hV_.ensure(sizeof(float) * 2 * K * Ts));
  float* ha = static_cast<float*>(hA_.ensure(sizeof(float) * 2 * K * Ts));
  memset(hv, 0, sizeof(float) * 2 * K * Ts); memset(ha, 0, sizeof(float) * 2 * K * Ts);
  for (long t = 0; t < T; t++)
    for (unsigned k = 0; k < K; k++) {
      hv[2 * ((size_t)k * Ts + t)] = fv[2 * ((size_t)t * K + k)]; hv[2 * ((size_t)k * Ts + t) + 1] = fv[2 * ((size_t)t * K + k) + 1];
      ha[2 * ((size_t)k * Ts + t)] = fa[2 * ((size_t)t * K + k)]; ha[2 * ((size_t)k * Ts + t) + 1] = fa[2 * ((size_t)t * K + k) + 1];
    }
  void* dv = dV_.ensure(sizeof(float) * 2 * K * Ts);
  void* da = dA_.ensure(sizeof(float) * 2 * K * Ts);
  h2d_async(dv, hv, sizeof(float) * 2 * K * Ts);
  h2d_async(da, ha, sizeof(float) * 2 * K * Ts);
  btk_node_synchronize();                                       // the pinned rows are rewritten by the next block
  Tn = T; Ts_ = Ts;
  return true;
}

bool AcousticEchoCancellationNode_::load_block_(long frame_arg)
{
  alloc_state_();
  long Tn = 0;
  const long f0 = base_ + T_;
  if (!(pbank_ ? load_from_banks_(Tn) : load_by_next_(Tn))) return false;
  const unsigned K = fftLen_ / 2 + 1;
  void* de = dE_.ensure(sizeof(float) * 2 * K * Ts_);
  // explicit frame numbers count up from the block's first frame; a default-argument caller hands -5 to every frame (aec.cc:902)
  const long fn0 = frame_arg >= 0 ? f0 : frame_arg;
  check_abi(btk_aec_process(kind_, params_, dV_.get(), dA_.get(), de, NULL, 1, (int)fftLen_, (int)sampleN_, Ts_, Tn, fn0, dR_.get(),
                            dK_.get(), static_cast<double*>(dSig_.get()), dHist_.get(), static_cast<double*>(dDtd_.get()), nstream()));
  base_ = f0; T_ = Tn; block_frame_arg_ = frame_arg >= 0 ? 0 : frame_arg;
  Ehost_valid_ = false; prepared_ = true;
  return true;
}

const float* AcousticEchoCancellationNode_::host_output_()
{
  if (!Ehost_valid_) {
    Ehost_.resize((size_t)2 * (fftLen_ / 2 + 1) * Ts_);
    d2h(Ehost_.data(), dE_.get(), sizeof(float) * Ehost_.size());
    Ehost_valid_ = true;
  }
  return Ehost_.data();
}

const gsl_vector_complex* AcousticEchoCancellationNode_::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  if (frame_no >= 0 && frame_no - 1 != frame_no_)
    throw jindex_error("Problem in Feature %s: %d != %d\n", name().c_str(), frame_no - 1, frame_no_);
  const long idx = frame_no_ + 1;
  while (!prepared_ || idx >= base_ + T_)
    if (!load_block_(frame_no)) { is_end_ = true; throw jiterator_error("end of samples!"); }
  // the double-talk detector's smoothing depends on the number next() is called with (aec.cc:902): a block is computed for one
  // way of calling, and a caller who changes it inside a block would get another signal than frame-by-frame processing gives
  if (kind_ == 3 && (frame_no >= 0 ? 0 : (long)frame_no) != block_frame_arg_)
    throw jconsistency_error("%s: next() was called with explicit and with default frame numbers inside one block of %ld frames; "
                             "keep to one of them (or set_block_frames(1))\n", name().c_str(), T_);
  const float* Y = host_output_();
  const unsigned M = fftLen_, K = M / 2 + 1;
  const long t = idx - base_;
  for (unsigned k = 0; k < K; k++) {
    const double re = Y[2 * ((size_t)k * Ts_ + t)], im = Y[2 * ((size_t)k * Ts_ + t) + 1];
    vector_->data[2 * k] = re; vector_->data[2 * k + 1] = im;
    if (k > 0 && k < M / 2) { vector_->data[2 * (M - k)] = re; vector_->data[2 * (M - k) + 1] = -im; }      // aec.cc:58-59
  }
  increment_();
  return vector_;
}

void AcousticEchoCancellationNode_::reset()
{
  played_->reset(); recorded_->reset();
  VectorComplexFeatureStream::reset();
  prepared_ = false; ended_ = false; base_ = 0; T_ = 0; Ts_ = 0; Ehost_valid_ = false; Ehost_.clear();
  // aec.h:41,78: the one-tap filters zero their weights (the Kalman filter keeps sigma2_v and K); aec.h:111-114: the block
  // filters reset their sources only
  if (kind_ < 2 && state_ready_)
    dev_zero_async(dR_.get(), sizeof(double) * 2 * (fftLen_ / 2 + 1) * sampleN_);
}

void AcousticEchoCancellationNode_::ensure_first_(long frame_arg)
{
  if (!prepared_ && !load_block_(frame_arg)) { T_ = 0; prepared_ = true; }
}

const std::vector<float>& AcousticEchoCancellationNode_::block(long& T)
{
  ensure_first_(-5);
  T = T_;
  if (T_ == 0) { Ehost_.clear(); return Ehost_; }
  host_output_();
  if (Ts_ != T_) {                                              // the host view of a block is dense: [K][T]
    const unsigned K = fftLen_ / 2 + 1;
    std::vector<float> dense((size_t)2 * K * T_);
    for (unsigned k = 0; k < K; k++) memcpy(&dense[2 * (size_t)k * T_], &Ehost_[2 * (size_t)k * Ts_], sizeof(float) * 2 * T_);
    dense_.swap(dense);
    return dense_;
  }
  return Ehost_;
}

const void* AcousticEchoCancellationNode_::device_block(long& T, long& T_stride)
{
  ensure_first_(-5);
  T = T_; T_stride = Ts_;
  return T_ ? dE_.get() : NULL;
}

long AcousticEchoCancellationNode_::block_base()
{
  ensure_first_(-5);
  return base_;
}

bool AcousticEchoCancellationNode_::next_block()
{
  ensure_first_(-5);
  return load_block_(block_frame_arg_ < 0 ? block_frame_arg_ : 0);
}

std::vector<double> AcousticEchoCancellationNode_::filter_coefficients(unsigned fbinX)
{
  if (fbinX > fftLen_ / 2) throw jindex_error("%s: state is kept for the bins 0..%d (asked for %d)\n", name().c_str(), (int)(fftLen_ / 2), (int)fbinX);
  alloc_state_();
  std::vector<double> r(2 * (size_t)sampleN_);
  d2h(r.data(), static_cast<const double*>(dR_.get()) + 2 * (size_t)fbinX * sampleN_, sizeof(double) * r.size());
  return r;
}

std::vector<double> AcousticEchoCancellationNode_::state_covariance(unsigned fbinX)
{
  if (fbinX > fftLen_ / 2) throw jindex_error("%s: state is kept for the bins 0..%d (asked for %d)\n", name().c_str(), (int)(fftLen_ / 2), (int)fbinX);
  alloc_state_();
  std::vector<double> r(2 * (size_t)sampleN_ * sampleN_);
  d2h(r.data(), static_cast<const double*>(dK_.get()) + 2 * (size_t)fbinX * sampleN_ * sampleN_, sizeof(double) * r.size());
  return r;
}

double AcousticEchoCancellationNode_::observation_noise_variance(unsigned fbinX)
{
  if (fbinX > fftLen_ / 2) throw jindex_error("%s: state is kept for the bins 0..%d (asked for %d)\n", name().c_str(), (int)(fftLen_ / 2), (int)fbinX);
  alloc_state_();
  double v = 0.0;
  d2h(&v, static_cast<const double*>(dSig_.get()) + fbinX, sizeof(double));
  return v;
}

// ---- the four reference classes: constructors only (parameter slots of btk_aec_process, include/btkhip.h)
namespace {
struct P8 { double v[8]; };
P8 p8(double a, double b, double c, double d, double e, double f, double g) { P8 p = {{a, b, c, d, e, f, g, 0.0}}; return p; }
}  // namespace

NLMSAcousticEchoCancellationFeature::NLMSAcousticEchoCancellationFeature(const VectorComplexFeatureStreamPtr& original,
                                                                         const VectorComplexFeatureStreamPtr& distorted, double delta,
                                                                         double epsilon, double threshold, const String& nm)
    : AcousticEchoCancellationNode_(0, original, distorted, 1, p8(delta, epsilon, 0, threshold, 0, 0, 1).v, nm) {}

KalmanFilterEchoCancellationFeature::KalmanFilterEchoCancellationFeature(const VectorComplexFeatureStreamPtr& played,
                                                                         const VectorComplexFeatureStreamPtr& recorded, double beta,
                                                                         double sigma2, double threshold, const String& nm)
    : AcousticEchoCancellationNode_(1, played, recorded, 1, p8(beta, sigma2, 0, threshold, 0, 0, 1).v, nm) {}

BlockKalmanFilterEchoCancellationFeature::BlockKalmanFilterEchoCancellationFeature(const VectorComplexFeatureStreamPtr& played,
                                                                                   const VectorComplexFeatureStreamPtr& recorded,
                                                                                   unsigned sampleN, double beta, double sigmau2,
                                                                                   double sigmauk2, double threshold, double amp4play,
                                                                                   const String& nm)
    : AcousticEchoCancellationNode_(2, played, recorded, sampleN, p8(beta, sigmau2, sigmauk2, threshold, 0, 0, amp4play).v, nm) {}

BlockKalmanFilterEchoCancellationFeature::BlockKalmanFilterEchoCancellationFeature(int kind, const VectorComplexFeatureStreamPtr& played,
                                                                                   const VectorComplexFeatureStreamPtr& recorded,
                                                                                   unsigned sampleN, const double* params8, const String& nm)
    : AcousticEchoCancellationNode_(kind, played, recorded, sampleN, params8, nm) {}

// the base class's threshold_ is snrTh (aec.cc:805)
DTDBlockKalmanFilterEchoCancellationFeature::DTDBlockKalmanFilterEchoCancellationFeature(const VectorComplexFeatureStreamPtr& played,
                                                                                         const VectorComplexFeatureStreamPtr& recorded,
                                                                                         unsigned sampleN, double beta, double sigmau2,
                                                                                         double sigmauk2, double snrTh, double engTh,
                                                                                         double smooth, double amp4play, const String& nm)
    : BlockKalmanFilterEchoCancellationFeature(3, played, recorded, sampleN, p8(beta, sigmau2, sigmauk2, snrTh, engTh, smooth, amp4play).v, nm) {}
