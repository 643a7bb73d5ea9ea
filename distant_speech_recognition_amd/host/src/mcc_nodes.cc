// mcc_nodes.cc -- SearchGridBuilder, SGB4LinearArray, MCCLocalizer and MCCCalculator of localization/localization.h over
// btk_mcc_linear_grid / btk_mcc_cost / btk_mcc_select / btk_mcc_matrices (csrc/mcc_kernels.hip): the channels are pulled a
// block of frames ahead, the block goes to the device once and stays there until its last frame is served, every (frame, grid
// point) is scored in one launch, and the N-best list, R of the winners and R of the last grid point come back.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "localization/localization.h"
#include "node_runtime.h"

namespace {

using btknode::check_abi;
using btknode::d2h;
using btknode::env_block_frames;
using btknode::h2d;

constexpr double MCC_RESET_COST = 100000.0;            // SourceCandidate's initial cost (mcc_localizer.h:155)

}  // namespace

// ================================================================================ SearchGridBuilder
SearchGridBuilder::SearchGridBuilder(int nChan, bool isFarField, unsigned int samplingFreq)
    : is_far_field_(isFarField), sampling_freq_(samplingFreq), max_time_delay_(-1), mpos_(gsl_matrix_alloc(nChan > 0 ? nChan : 0, 3)),
      hypopos_(gsl_vector_calloc(3)), delays_(gsl_vector_calloc(nChan > 0 ? nChan : 0)), const_v_(0)
{
  if (nChan < 1) throw jdimension_error("SearchGridBuilder: %d channels", nChan);
}

SearchGridBuilder::~SearchGridBuilder()
{
  gsl_matrix_free(mpos_);
  gsl_vector_free(hypopos_);
  gsl_vector_free(delays_);
}

void SearchGridBuilder::reset()
{
  gsl_vector_set(hypopos_, 0, 0.0);
  gsl_vector_set(hypopos_, 1, 0.0);
  gsl_vector_set(hypopos_, 2, 0.0);
}

// ================================================================================ SGB4LinearArray
SGB4LinearArray::SGB4LinearArray(int nChan, bool isFarField, unsigned int samplingFreq)
    : SearchGridBuilder(nChan, isFarField, samplingFreq), at_(0)
{
}

void SGB4LinearArray::walk_(const double* positions, float distance)
{
  const int N = (int)chanN();
  int n = 0;
  check_abi(btk_mcc_linear_grid(sampling_freq_, N, positions, distance, 0, &n, &max_time_delay_, &const_v_, NULL, NULL, NULL));
  azimuths_.assign((size_t)n, 0.0);
  table_.assign((size_t)n * N, 0.0);
  check_abi(btk_mcc_linear_grid(sampling_freq_, N, positions, distance, n, &n, &max_time_delay_, &const_v_, azimuths_.data(),
                                table_.data(), NULL));
  reset();
}

void SGB4LinearArray::setDistanceBtwMicrophones(float distance)
{
  for (size_t m = 0; m < chanN(); m++) {
    gsl_matrix_set(mpos_, m, 0, 0.0);
    gsl_matrix_set(mpos_, m, 1, m * distance);
    gsl_matrix_set(mpos_, m, 2, 0.0);
  }
  walk_(NULL, distance);
}

void SGB4LinearArray::setPositionsOfMicrophones(const gsl_matrix* mpos)
{
  if (!mpos || mpos->size1 != chanN() || mpos->size2 < 3)
    throw jdimension_error("The size of the matrix for the geometry of the array should be %lu x %lu\n", (unsigned long)chanN(), 3ul);
  for (size_t m = 0; m < chanN(); m++)
    for (size_t k = 0; k < 3; k++) gsl_matrix_set(mpos_, m, k, gsl_matrix_get(mpos, m, k));
  walk_(mpos_->data, 0.f);
}

void SGB4LinearArray::reset()
{
  SearchGridBuilder::reset();
  at_ = 0;
}

const gsl_vector* SGB4LinearArray::getTimeDelays()
{
  if (azimuths_.empty()) throw j_error("SGB4LinearArray: set the geometry with setDistanceBtwMicrophones() or setPositionsOfMicrophones()\n");
  memcpy(delays_->data, &table_[at_ * chanN()], sizeof(double) * chanN());
  return delays_;
}

bool SGB4LinearArray::nextSearchGrid()
{
  if (!is_far_field_) throw j_error("SGB4LinearArray: the near-field search grid is not implemented (need to be implemented)\n");
  if (azimuths_.empty()) throw j_error("SGB4LinearArray: set the geometry with setDistanceBtwMicrophones() or setPositionsOfMicrophones()\n");
  if (at_ + 1 >= azimuths_.size()) return false;      // nextSearchGridFF returned NULL: the position stays (:140-141)
  at_++;
  gsl_vector_set(hypopos_, 1, azimuths_[at_]);
  return true;
}

// ================================================================================ MCCLocalizer
MCCLocalizer::MCCLocalizer(SearchGridBuilderPtr& sgbPtr, size_t maxSource, const String& nm)
    : VectorFeatureStream(3, nm), sgb_(sgbPtr), max_source_(maxSource), block_frames_(env_block_frames("BTK_MCC_BLOCK_FRAMES", 64)),
      launches_(0), F_(0), served_(0), sources_ended_(false), L_(0), R_(NULL), eig_(NULL), eig_fresh_(false)
{
  if (sgbPtr.is_null()) throw jparameter_error("MCCLocalizer: null SearchGridBuilder");
  if (maxSource < 1 || maxSource > 16) throw jdimension_error("MCCLocalizer: maxSource=%lu, need 1 .. 16", (unsigned long)maxSource);
  const size_t N = sgb_->chanN();
  R_ = gsl_matrix_alloc(N, N);
  eig_ = gsl_vector_calloc(N);
  cand_.resize(maxSource);
  for (Candidate& c : cand_) {
    c.cost = MCC_RESET_COST;
    c.tau.assign(N, 0);
    c.position = gsl_vector_calloc(3);
  }
  end_pos_[0] = end_pos_[1] = end_pos_[2] = 0.0;
}

MCCLocalizer::~MCCLocalizer()
{
  gsl_matrix_free(R_);
  gsl_vector_free(eig_);
  for (Candidate& c : cand_) gsl_vector_free(c.position);
}

void MCCLocalizer::setChannel(VectorFloatFeatureStreamPtr& chan)
{
  if (chan.is_null()) throw jparameter_error("MCCLocalizer::setChannel: null channel");
  channels_.push_back(chan);
}

void MCCLocalizer::check_frame_length_(size_t D) const
{
  if (L_ < 2 * D) throw j_error("Data samples are insufficient\n");      // mcc_localizer.cc:329-331
}

bool MCCLocalizer::pull_block_()
{
  const size_t N = sgb_->chanN();
  if (channels_.size() != N)
    throw jdimension_error("MCCLocalizer: %lu channels set, the search grid has %lu", (unsigned long)channels_.size(), (unsigned long)N);
  L_ = channels_[0]->size();
  for (size_t c = 1; c < N; c++)
    if (channels_[c]->size() != L_) throw jdimension_error("MCCLocalizer: channel %lu hands out %u samples, channel 0 %lu", (unsigned long)c, channels_[c]->size(), (unsigned long)L_);
  F_ = served_ = 0;
  if (sources_ended_) return false;
  const long cap = block_frames_ > 0 ? block_frames_ : LONG_MAX;
  std::vector<float> frames;                           // [F][N][L] as pulled
  long n = 0;
  try {
    for (; n < cap; n++) {
      const size_t at = frames.size();
      frames.resize(at + N * L_);
      try {
        for (size_t c = 0; c < N; c++) {
          const gsl_vector_float* v = channels_[c]->next(-5);
          for (size_t i = 0; i < L_; i++) frames[at + c * L_ + i] = gsl_vector_float_get(v, i);
        }
      } catch (...) {
        frames.resize(at);
        throw;
      }
    }
  } catch (jiterator_error&) {
    sources_ended_ = true;
  }
  if (n == 0) return false;
  x_.resize((size_t)n * N * L_);                       // [N][F L]: a channel's frames in a row, the blocks of btk_mcc_cost
  for (long f = 0; f < n; f++)
    for (size_t c = 0; c < N; c++)
      memcpy(&x_[(c * (size_t)n + (size_t)f) * L_], &frames[((size_t)f * N + c) * L_], sizeof(float) * L_);
  h2d(d_x_.ensure(sizeof(float) * x_.size()), x_.data(), sizeof(float) * x_.size());
  F_ = n;
  return true;
}

void MCCLocalizer::launch_()
{
  const size_t N = sgb_->chanN();
  const unsigned fs = sgb_->samplingFrequency();
  const long D = btk_mcc_max_sample_delay(fs, sgb_->maxTimeDelay());
  check_frame_length_((size_t)D);
  // the builder's own walk (search(), :416-446)
  tau_.clear();
  grid_pos_.clear();
  sgb_->reset();
  std::vector<int> row(N);
  for (;;) {
    const gsl_vector* pos = sgb_->getSearchPosition();
    const gsl_vector* delays = sgb_->getTimeDelays();
    if (!delays || delays->size != N) throw j_error("MCCLocalizer: the search grid hands out no time delays\n");
    std::vector<double> d(N);
    for (size_t c = 0; c < N; c++) d[c] = gsl_vector_get(delays, c);
    check_abi(btk_mcc_sample_delays(fs, (int)N, d.data(), row.data()));
    tau_.insert(tau_.end(), row.begin(), row.end());
    for (size_t k = 0; k < 3; k++) grid_pos_.push_back(gsl_vector_get(pos, k));
    if (!sgb_->nextSearchGrid()) break;
  }
  for (size_t k = 0; k < 3; k++) end_pos_[k] = gsl_vector_get(sgb_->getSearchPosition(), k);
  const int G = (int)(tau_.size() / N), nb = (int)max_source_;
  const long F = F_;
  void* st = btk_node_stream();
  double* dc = static_cast<double*>(d_cost_.ensure(sizeof(double) * (size_t)F * G));
  check_abi(btk_mcc_cost(d_x_.get(), F * (long)L_, 1, (int)N, (int)F, (int)L_, (int)D, tau_.data(), d_tau_.ensure(sizeof(int) * tau_.size()),
                         G, 1, dc, d_flag_.ensure((size_t)F * G), st));
  double* dnc = static_cast<double*>(d_nbc_.ensure(sizeof(double) * (size_t)F * nb));
  int* dni = static_cast<int*>(d_nbi_.ensure(sizeof(int) * (size_t)F * nb));
  check_abi(btk_mcc_select(dc, F, G, nb, dnc, dni, st));
  nb_cost_.resize((size_t)F * nb);
  nb_idx_.resize((size_t)F * nb);
  d2h(nb_cost_.data(), dnc, sizeof(double) * nb_cost_.size());
  d2h(nb_idx_.data(), dni, sizeof(int) * nb_idx_.size());
  // R of the winners and of the last grid point (an empty list entry asks for grid point 0 and is not read)
  std::vector<int> pairs((size_t)F * (nb + 1) * 2);
  for (long f = 0; f < F; f++)
    for (int j = 0; j <= nb; j++) {
      pairs[((size_t)f * (nb + 1) + j) * 2] = (int)f;
      pairs[((size_t)f * (nb + 1) + j) * 2 + 1] = j < nb ? std::max(nb_idx_[(size_t)f * nb + j], 0) : G - 1;
    }
  const int P = (int)(F * (nb + 1));
  Rh_.resize((size_t)P * N * N);
  double* dR = static_cast<double*>(d_R_.ensure(sizeof(double) * Rh_.size()));
  check_abi(btk_mcc_matrices(d_x_.get(), F * (long)L_, 1, (int)N, (int)F, (int)L_, (int)D, tau_.data(), d_tau_.get(), G, pairs.data(),
                             d_pairs_.ensure(sizeof(int) * pairs.size()), P, dR, st));
  d2h(Rh_.data(), dR, sizeof(double) * Rh_.size());
  launches_++;
}

void MCCLocalizer::serve_(long f)
{
  const size_t N = sgb_->chanN(), nb = max_source_;
  for (size_t j = 0; j < nb; j++) {
    const int g = nb_idx_[(size_t)f * nb + j];
    Candidate& c = cand_[j];
    c.cost = nb_cost_[(size_t)f * nb + j];               // setConstV() of every search: an empty entry is back at 100000 (:419)
    if (g < 0) continue;                                 // ... and keeps the delays and position it had
    for (size_t k = 0; k < N; k++) c.tau[k] = tau_[(size_t)g * N + k];
    for (size_t k = 0; k < 3; k++) gsl_vector_set(c.position, k, grid_pos_[(size_t)g * 3 + k]);
  }
  const double* Rf = &Rh_[(size_t)f * (nb + 1) * N * N];
  Rbest_.assign(Rf, Rf + N * N);
  eig_fresh_ = false;
  memcpy(R_->data, Rf + nb * N * N, sizeof(double) * N * N);
  for (size_t k = 0; k < 3; k++) {
    gsl_vector_set(vector_, k, gsl_vector_get(cand_[0].position, k));       // :448
    gsl_vector_set(const_cast<gsl_vector*>(sgb_->getSearchPosition()), k, end_pos_[k]);
  }
}

const gsl_vector* MCCLocalizer::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  if (served_ >= F_) {
    if (!pull_block_()) { is_end_ = true; throw jiterator_error("end of samples!"); }
    launch_();
  }
  serve_(served_++);
  increment_();
  return vector_;
}

void MCCLocalizer::reset()
{
  for (VectorFloatFeatureStreamPtr& c : channels_) c->reset();
  VectorFeatureStream::reset();
  sgb_->reset();
  F_ = served_ = 0;
  sources_ended_ = false;
}

int MCCLocalizer::getNthBestDelayedSample(int nth, int chanX)
{
  if (nth < 0 || (size_t)nth >= cand_.size() || chanX < 0 || (size_t)chanX >= sgb_->chanN())
    throw jindex_error("MCCLocalizer: candidate %d, channel %d out of range", nth, chanX);
  return cand_[nth].tau[chanX];
}

double MCCLocalizer::getNthBestMCCC(int nth)
{
  if (nth < 0 || (size_t)nth >= cand_.size()) throw jindex_error("MCCLocalizer: candidate %d out of range", nth);
  return 1 - exp(cand_[nth].cost);
}

const gsl_vector* MCCLocalizer::getNthBestPosition(int nth)
{
  if (nth < 0 || (size_t)nth >= cand_.size()) throw jindex_error("MCCLocalizer: candidate %d out of range", nth);
  return cand_[nth].position;
}

// cyclic Jacobi over the symmetric N x N matrix R, float64; the eigenvalues in ascending order
void MCCLocalizer::jacobi_(const double* R)
{
  const size_t N = sgb_->chanN();
  std::vector<double> A(R, R + N * N);
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0.0, diag = 0.0;
    for (size_t i = 0; i < N; i++) {
      diag += A[i * N + i] * A[i * N + i];
      for (size_t j = i + 1; j < N; j++) off += A[i * N + j] * A[i * N + j];
    }
    if (off <= 1e-40 * diag || off == 0.0) break;
    for (size_t p = 0; p + 1 < N; p++)
      for (size_t q = p + 1; q < N; q++) {
        const double apq = A[p * N + q];
        if (apq == 0.0) continue;
        const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (size_t k = 0; k < N; k++) {               // columns p, q
          const double akp = A[k * N + p], akq = A[k * N + q];
          A[k * N + p] = c * akp - s * akq;
          A[k * N + q] = s * akp + c * akq;
        }
        for (size_t k = 0; k < N; k++) {               // rows p, q
          const double apk = A[p * N + k], aqk = A[q * N + k];
          A[p * N + k] = c * apk - s * aqk;
          A[q * N + k] = s * apk + c * aqk;
        }
      }
  }
  std::vector<double> ev(N);
  for (size_t i = 0; i < N; i++) ev[i] = A[i * N + i];
  std::sort(ev.begin(), ev.end());
  for (size_t i = 0; i < N; i++) gsl_vector_set(eig_, i, ev[i]);
}

const gsl_vector* MCCLocalizer::getEigenValues()
{
  if (!eig_fresh_ && Rbest_.size() == sgb_->chanN() * sgb_->chanN()) {
    jacobi_(Rbest_.data());
    eig_fresh_ = true;
  }
  return eig_;
}

// ================================================================================ MCCCalculator
MCCCalculator::MCCCalculator(SearchGridBuilderPtr& sgbPtr, bool normalizeVariance, const String& nm)
    : MCCLocalizer(sgbPtr, 1, nm), have_delays_(false), normalize_(normalizeVariance), stale_(false)
{
}

void MCCCalculator::setTimeDelays(gsl_vector* delays)
{
  if (!delays) throw jparameter_error("MCCCalculator::setTimeDelays: null vector");
  delays_.resize(delays->size);
  for (size_t i = 0; i < delays->size; i++) delays_[i] = gsl_vector_get(delays, i);
  have_delays_ = true;
  stale_ = true;
}

void MCCCalculator::launch_()
{
  const size_t N = sgb_->chanN();
  const unsigned fs = sgb_->samplingFrequency();
  const long D = btk_mcc_max_sample_delay(fs, sgb_->maxTimeDelay());
  check_frame_length_((size_t)D);
  if (delays_.size() != N) throw jdimension_error("MCCCalculator: %lu time delays for %lu channels", (unsigned long)delays_.size(), (unsigned long)N);
  tau_.assign(N, 0);
  check_abi(btk_mcc_sample_delays(fs, (int)N, delays_.data(), tau_.data()));
  const long F = F_;
  void* st = btk_node_stream();
  double* dc = static_cast<double*>(d_cost_.ensure(sizeof(double) * (size_t)F));
  unsigned char* df = static_cast<unsigned char*>(d_flag_.ensure((size_t)F));
  check_abi(btk_mcc_cost(d_x_.get(), F * (long)L_, 1, (int)N, (int)F, (int)L_, (int)D, tau_.data(), d_tau_.ensure(sizeof(int) * N), 1,
                         normalize_ ? 1 : 0, dc, df, st));
  cost_h_.resize((size_t)F);
  flag_h_.resize((size_t)F);
  d2h(cost_h_.data(), dc, sizeof(double) * (size_t)F);
  d2h(flag_h_.data(), df, (size_t)F);
  std::vector<int> pairs((size_t)F * 2, 0);
  for (long f = 0; f < F; f++) pairs[(size_t)f * 2] = (int)f;
  Rh_.resize((size_t)F * N * N);
  double* dR = static_cast<double*>(d_R_.ensure(sizeof(double) * Rh_.size()));
  check_abi(btk_mcc_matrices(d_x_.get(), F * (long)L_, 1, (int)N, (int)F, (int)L_, (int)D, tau_.data(), d_tau_.get(), 1, pairs.data(),
                             d_pairs_.ensure(sizeof(int) * pairs.size()), (int)F, dR, st));
  d2h(Rh_.data(), dR, sizeof(double) * Rh_.size());
  stale_ = false;
  launches_++;
}

void MCCCalculator::serve_(long f)
{
  const size_t N = sgb_->chanN();
  gsl_vector_set(vector_, 0, cost_h_[(size_t)f]);        // elements 1 and 2 stay as they were (:550)
  Candidate& c = cand_[0];                               // setSourceInfo(_tau, vector_, costV, _eigenvalues) (:551)
  c.cost = cost_h_[(size_t)f];
  c.tau = tau_;
  for (size_t k = 0; k < 3; k++) gsl_vector_set(c.position, k, gsl_vector_get(vector_, k));
  const double* Rf = &Rh_[(size_t)f * N * N];
  Rbest_.assign(Rf, Rf + N * N);
  eig_fresh_ = false;
  memcpy(R_->data, Rf, sizeof(double) * N * N);
}

const gsl_vector* MCCCalculator::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  if (!have_delays_) throw j_error("set time delays with setTimeDelays()\n");     // :542-544
  if (served_ >= F_) {
    if (!pull_block_()) { is_end_ = true; throw jiterator_error("end of samples!"); }
    launch_();
  } else if (stale_) {
    launch_();                                           // the frames still to serve, scored again with the new delays
  }
  serve_(served_++);
  increment_();
  return vector_;
}

double MCCCalculator::getMCCC() { return 1.0 - exp(gsl_vector_get(vector_, 0)); }
