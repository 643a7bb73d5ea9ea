// fe_nodes.cc -- the recogniser's front-end nodes of feature/feature.h over btk_fe_process (csrc/fe_kernels.hip):
// PreemphasisFeature and StorageFeature on the host, SpectralPowerFeature, VTLNFeature, MelFeature, LogFeature and
// CepstralFeature as block-serving nodes (FeStageNode).
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "feature/feature.h"
#include "btkhip.h"
#include "node_runtime.h"

namespace {

using btknode::check_abi;
using btknode::check_hip;
using btknode::nstream;
using btknode::env_block_frames;

void check_frame_no(int frame_no, int current, const String& name)
{
  if (frame_no >= 0 && frame_no - 1 != current)
    throw jindex_error("Problem in Feature %s: %d != %d\n", name.c_str(), frame_no - 1, current);
}

// rows [N][3] = offset, count, start from the table entries' offset[] and count[]
void pack_rows(const std::vector<int>& off, const std::vector<int>& cnt, std::vector<int>& rows)
{
  rows.resize(3 * off.size());
  int start = 0;
  for (size_t j = 0; j < off.size(); j++) {
    rows[3 * j] = off[j]; rows[3 * j + 1] = cnt[j]; rows[3 * j + 2] = start;
    start += cnt[j];
  }
}

}  // namespace

// ================================================================================ PreemphasisFeature (feature.cc:1113-1144)
PreemphasisFeature::PreemphasisFeature(const VectorFloatFeatureStreamPtr& samp, double mu, const String& nm)
    : VectorFloatFeatureStream(samp->size(), nm), samp_(samp), prior_(0.0f), mu_(mu)
{
}

const gsl_vector_float* PreemphasisFeature::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  check_frame_no(frame_no, frame_no_, name());
  const gsl_vector_float* block = samp_->next(frame_no_ + 1);
  increment_();
  for (unsigned i = 0; i < size(); i++) {
    vector_->data[i] = (float)((double)block->data[i] - mu_ * (double)prior_);
    prior_ = block->data[i];
  }
  return vector_;
}

void PreemphasisFeature::advance_blocks(long n, const float* blocks)
{
  if (n <= 0) return;
  const unsigned D = size();
  if (n > 1) prior_ = blocks[(size_t)(n - 1) * D - 1];
  const float* block = blocks + (size_t)(n - 1) * D;
  for (unsigned i = 0; i < D; i++) {
    vector_->data[i] = (float)((double)block[i] - mu_ * (double)prior_);
    prior_ = block[i];
  }
  frame_no_ += (int)n;
}

// ================================================================================ StorageFeature (feature.cc:2905-2996)
StorageFeature::StorageFeature(const VectorFloatFeatureStreamPtr& src, const String& nm)
    : VectorFloatFeatureStream(src->size(), nm), src_(src)
{
}

StorageFeature::~StorageFeature()
{
  for (size_t i = 0; i < frames_.size(); i++) gsl_vector_float_free(frames_[i]);
}

gsl_vector_float* StorageFeature::frame_(int i)
{
  if (i >= MaxFrames) throw jdimension_error("Frame %d is greater than maximum number %d.", i, (int)MaxFrames);
  while ((int)frames_.size() <= i) frames_.push_back(gsl_vector_float_calloc(size()));
  return frames_[i];
}

const gsl_vector_float* StorageFeature::next(int frame_no)
{
  if (frame_no >= 0 && frame_no <= frame_no_) return frame_(frame_no);
  if (frame_no >= MaxFrames) throw jdimension_error("Frame %d is greater than maximum number %d.", frame_no, (int)MaxFrames);
  const gsl_vector_float* v = src_->next(frame_no_ + 1);
  gsl_vector_float* f = frame_(frame_no_ + 1);
  increment_();
  memcpy(f->data, v->data, sizeof(float) * size());
  return f;
}

void StorageFeature::store_blocks(long n, const float* blocks)
{
  for (long j = 0; j < n; j++) {
    gsl_vector_float* f = frame_(frame_no_ + 1);
    increment_();
    memcpy(f->data, blocks + (size_t)j * size(), sizeof(float) * size());
  }
}

void StorageFeature::write(const String& fileName, bool plainText) const
{
  if (frame_no_ <= 0) throw jio_error("Frame count must be > 0.\n");
  FILE* fp = fopen(fileName.c_str(), plainText ? "w" : "wb");
  if (!fp) throw jio_error("Could not open %s for writing.\n", fileName.c_str());
  const int sz = (int)size();
  if (plainText) {
    fprintf(fp, "%d %d\n", frame_no_, sz);
    for (int i = 0; i <= frame_no_; i++) {
      for (int j = 0; j < sz; j++) fprintf(fp, j < sz - 1 ? "%g " : "%g", frames_[i]->data[j]);
      fprintf(fp, "\n");
    }
  } else {
    // the count written is the last frame INDEX, as in the reference, and read() takes it as the index again
    fwrite(&frame_no_, sizeof(int), 1, fp);
    fwrite(&sz, sizeof(int), 1, fp);
    for (int i = 0; i <= frame_no_; i++) fwrite(frames_[i]->data, sizeof(float), sz, fp);
  }
  fclose(fp);
}

void StorageFeature::read(const String& fileName)
{
  FILE* fp = fopen(fileName.c_str(), "rb");
  if (!fp) throw jio_error("Could not open %s for reading.\n", fileName.c_str());
  int last = 0, sz = 0;
  if (fread(&last, sizeof(int), 1, fp) != 1 || fread(&sz, sizeof(int), 1, fp) != 1) { fclose(fp); throw jio_error("%s is too short.\n", fileName.c_str()); }
  if (sz != (int)size()) { fclose(fp); throw jdimension_error("Feature dimensions (%d vs. %d) do not match.\n", sz, (int)size()); }
  if (last < 0 || last >= MaxFrames) { fclose(fp); throw jdimension_error("Frame %d is greater than maximum number %d.", last, (int)MaxFrames); }
  for (int i = 0; i <= last; i++)
    if (fread(frame_(i)->data, sizeof(float), sz, fp) != (size_t)sz) { fclose(fp); throw jio_error("%s is too short.\n", fileName.c_str()); }
  fclose(fp);
  frame_no_ = last;
}

int StorageFeature::evaluate()
{
  reset();
  int frame_no = 0;
  try {
    while (true) next(frame_no++);
  } catch (jiterator_error&) {
  }
  return frame_no_;
}

// ================================================================================ FFTFeature: the root of a front-end chain
void FFTFeature::find_fe_chain_()
{
  fe_hamming_ = dynamic_cast<HammingFeature*>(samp_.operator->());
  fe_preemph_ = NULL; fe_storage_ = NULL; fe_sample_ = NULL;
  if (!fe_hamming_) return;
  VectorFloatFeatureStream* s = fe_hamming_->source().operator->();
  if ((fe_preemph_ = dynamic_cast<PreemphasisFeature*>(s))) s = fe_preemph_->source().operator->();
  if ((fe_storage_ = dynamic_cast<StorageFeature*>(s))) s = fe_storage_->source().operator->();
  fe_sample_ = dynamic_cast<SampleFeature*>(s);
  if (!fe_sample_) { fe_hamming_ = NULL; fe_preemph_ = NULL; fe_storage_ = NULL; }
}

long FFTFeature::pull_fe_blocks(float* dst, long nmax, int* preemph, double* mu, float* prior0)
{
  if (!fe_sample_) throw jconsistency_error("FFTFeature %s: not the root of a front-end chain\n", name().c_str());
  const long n = fe_sample_->next_blocks(dst, nmax);
  *preemph = fe_preemph_ != NULL;
  *mu = fe_preemph_ ? fe_preemph_->mu() : 0.0;
  *prior0 = fe_preemph_ ? fe_preemph_->prior() : 0.0f;
  if (n > 0) {
    if (fe_storage_) fe_storage_->store_blocks(n, dst);
    const float* last = dst + (size_t)(n - 1) * windowLen_;
    if (fe_preemph_) {
      fe_preemph_->advance_blocks(n, dst);
      last = fe_preemph_->current_vector();
    }
    fe_hamming_->advance_blocks(n, last);
  }
  blk_n_ = blk_pos_ = 0;
  if (n < nmax) is_end_ = true;
  return n;
}

void FFTFeature::fe_advance(long n, const float* last_half)
{
  if (n <= 0) return;
  frame_no_ += (int)n;
  serve_(last_half);
}

// ================================================================================ FeStageNode: the block service
FeStageNode::FeStageNode(int stage)
    : tables_dirty_(true), stage_(stage), below_(NULL), fft_(NULL), block_frames_(env_block_frames("BTK_FE_BLOCK_FRAMES", 64)), blk_n_(0), blk_pos_(0),
      launches_(0)
{
}

void FeStageNode::fe_wire_(FeStageNode* below, FFTFeature* fft)
{
  below_ = below;
  fft_ = fft;
}

void FeStageNode::set_block_frames(long n) { block_frames_ = n > 0 ? n : env_block_frames("BTK_FE_BLOCK_FRAMES", 64); }

FFTFeature* FeStageNode::root_() const
{
  const FeStageNode* p = this;
  while (p->below_) p = p->below_;
  return (p->fft_ && p->fft_->has_fe_chain()) ? p->fft_ : NULL;
}

void FeStageNode::fe_upload_(DeviceBuffer& d, const void* h, size_t bytes)
{
  void* p = d.ensure(bytes ? bytes : 16);
  if (bytes) check_hip(hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, nstream()), "front-end table upload");
  // the host arrays are pageable and may change (warp()) before the copy has run
  check_hip(hipStreamSynchronize(nstream()), "front-end table upload");
}

const float* FeStageNode::fe_next_()
{
  if (blk_pos_ >= blk_n_) {
    FFTFeature* root = root_();
    if (root) fill_chain_(root); else fill_single_();
  }
  return static_cast<const float*>(h_out_.get()) + (size_t)(blk_pos_++) * fe_dim();
}

// one launch from PCM up to this node's stage for the blocks the chain has next
void FeStageNode::fill_chain_(FFTFeature* root)
{
  const size_t D = root->windowLen(), L = root->fftLen(), K = L / 2 + 1;
  float* in = static_cast<float*>(h_in_.ensure(sizeof(float) * D * (size_t)block_frames_));
  int preemph = 0;
  double mu = 0.0;
  float prior0 = 0.0f;
  const long n = root->pull_fe_blocks(in, block_frames_, &preemph, &mu, &prior0);
  if (n <= 0) throw jiterator_error("end of samples!");
  std::vector<FeStageNode*> chain;                  // this node first, the power node last
  for (FeStageNode* p = this; p; p = p->below_) chain.push_back(p);
  btk_fe_params q;
  memset(&q, 0, sizeof(q));
  q.S = 1; q.C = 1; q.T = n; q.in_stage = BTK_FE_PCM;
  q.len = (long)(D * (size_t)n); q.pcm_stride = q.len; q.D = (int)D; q.shift = (int)D; q.L = (int)L;
  q.window = BTK_TDOA_WINDOW_HAMMING; q.preemph = preemph; q.mu = mu;
  q.log_m = 1.0; q.log_a = 1.0;
  for (size_t i = 0; i < chain.size(); i++) chain[i]->fe_params(q);
  // outputs: the spectrum (the FFTFeature's vector), then one buffer per node of the chain
  size_t total = 2 * K * (size_t)n;
  std::vector<size_t> at(chain.size());
  for (size_t i = 0; i < chain.size(); i++) { at[i] = total; total += (size_t)chain[i]->fe_dim() * (size_t)n; }
  hipStream_t st = nstream();
  float* din = static_cast<float*>(d_in_.ensure(sizeof(float) * D * (size_t)n));
  float* dout = static_cast<float*>(d_out_.ensure(sizeof(float) * total));
  check_hip(hipMemcpyAsync(din, in, sizeof(float) * D * (size_t)n, hipMemcpyHostToDevice, st), "front-end upload");
  if (preemph) {
    float* dp = static_cast<float*>(d_prior_.ensure(sizeof(float)));
    float* hp = static_cast<float*>(h_last_.ensure(sizeof(float) * (2 * K + 4)));
    hp[0] = prior0;
    check_hip(hipMemcpyAsync(dp, hp, sizeof(float), hipMemcpyHostToDevice, st), "front-end upload");
    check_hip(hipStreamSynchronize(st), "front-end upload");           // hp is reused below
    q.prior0 = dp;
  }
  q.out[BTK_FE_SPECTRUM] = dout;
  for (size_t i = 0; i < chain.size(); i++) q.out[chain[i]->stage_] = dout + at[i];
  check_abi(btk_fe_process(&q, din, st));
  launches_++;
  // this node's block, and the last frame of every node below it
  float* out = static_cast<float*>(h_out_.ensure(sizeof(float) * (size_t)fe_dim() * (size_t)n));
  check_hip(hipMemcpyAsync(out, dout + at[0], sizeof(float) * (size_t)fe_dim() * (size_t)n, hipMemcpyDeviceToHost, st), "front-end download");
  btk_node_count_d2h(sizeof(float) * (size_t)fe_dim() * (size_t)n);
  size_t lastN = 2 * K;
  for (size_t i = 1; i < chain.size(); i++) lastN += chain[i]->fe_dim();
  float* last = static_cast<float*>(h_last_.ensure(sizeof(float) * (lastN + 4)));
  check_hip(hipMemcpyAsync(last, dout + (size_t)(n - 1) * 2 * K, sizeof(float) * 2 * K, hipMemcpyDeviceToHost, st), "front-end download");
  btk_node_count_d2h(sizeof(float) * 2 * K);
  size_t o = 2 * K;
  for (size_t i = 1; i < chain.size(); i++) {
    const size_t d = chain[i]->fe_dim();
    check_hip(hipMemcpyAsync(last + o, dout + at[i] + (size_t)(n - 1) * d, sizeof(float) * d, hipMemcpyDeviceToHost, st), "front-end download");
    btk_node_count_d2h(sizeof(float) * d);
    o += d;
  }
  check_hip(hipStreamSynchronize(st), "front-end block");
  root->fe_advance(n, last);
  o = 2 * K;
  for (size_t i = 1; i < chain.size(); i++) {
    chain[i]->fe_advance(n, last + o);
    chain[i]->fe_reset_();
    o += chain[i]->fe_dim();
  }
  blk_n_ = n;
  blk_pos_ = 0;
}

// one frame of any other source, entered at this node's own stage
void FeStageNode::fill_single_()
{
  std::vector<float> in;
  int in_stage = 0, in_dim = 0, L = 0;
  fe_pull_one(in, in_stage, in_dim, L);             // throws jiterator_error at the end of the source
  btk_fe_params q;
  memset(&q, 0, sizeof(q));
  q.S = 1; q.C = 1; q.T = 1; q.in_stage = in_stage; q.in_dim = in_dim; q.L = L;
  q.log_m = 1.0; q.log_a = 1.0;
  fe_params(q);
  hipStream_t st = nstream();
  float* hin = static_cast<float*>(h_in_.ensure(sizeof(float) * in.size()));
  memcpy(hin, in.data(), sizeof(float) * in.size());
  float* din = static_cast<float*>(d_in_.ensure(sizeof(float) * in.size()));
  float* dout = static_cast<float*>(d_out_.ensure(sizeof(float) * fe_dim()));
  check_hip(hipMemcpyAsync(din, hin, sizeof(float) * in.size(), hipMemcpyHostToDevice, st), "front-end upload");
  q.out[stage_] = dout;
  check_abi(btk_fe_process(&q, din, st));
  launches_++;
  float* out = static_cast<float*>(h_out_.ensure(sizeof(float) * fe_dim()));
  check_hip(hipMemcpyAsync(out, dout, sizeof(float) * fe_dim(), hipMemcpyDeviceToHost, st), "front-end download");
  btk_node_count_d2h(sizeof(float) * fe_dim());
  check_hip(hipStreamSynchronize(st), "front-end frame");
  blk_n_ = 1;
  blk_pos_ = 0;
}

// ================================================================================ SpectralPowerFeature (feature.cc:1291-1314)
SpectralPowerFeature::SpectralPowerFeature(const VectorComplexFeatureStreamPtr& fft, unsigned powN, const String& nm)
    : VectorFeatureStream(powN == 0 ? fft->size() : powN, nm), FeStageNode(BTK_FE_POWER), fft_(fft)
{
  if (size() != fft->size() && size() != (fft->size() / 2) + 1)
    throw jconsistency_error("Number of power coefficients %d does not match FFT length %d.", size(), fft->size());
  fe_wire_(NULL, dynamic_cast<FFTFeature*>(fft_.operator->()));
}

const gsl_vector* SpectralPowerFeature::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  check_frame_no(frame_no, frame_no_, name());
  const float* p = fe_next_();
  increment_();
  for (unsigned i = 0; i < size(); i++) vector_->data[i] = p[i];
  return vector_;
}

void SpectralPowerFeature::fe_params(btk_fe_params& q) { q.powN = (int)size(); }

void SpectralPowerFeature::fe_advance(long n, const float* last)
{
  frame_no_ += (int)n;
  for (unsigned i = 0; i < size(); i++) vector_->data[i] = last[i];
}

void SpectralPowerFeature::fe_pull_one(std::vector<float>& in, int& in_stage, int& in_dim, int& L)
{
  const gsl_vector_complex* X = fft_->next(frame_no_ + 1);
  L = (int)fft_->size();
  in.resize(2 * (size_t)(L / 2 + 1));
  for (int k = 0; k <= L / 2; k++) { in[2 * k] = (float)X->data[2 * k]; in[2 * k + 1] = (float)X->data[2 * k + 1]; }
  in_stage = BTK_FE_SPECTRUM;
  in_dim = 0;
}

// ================================================================================ SpectralPowerFloatFeature (feature.cc:1263-1286)
SpectralPowerFloatFeature::SpectralPowerFloatFeature(const VectorComplexFeatureStreamPtr& fft, unsigned powN, const String& nm)
    : VectorFloatFeatureStream(powN == 0 ? fft->size() : powN, nm), fft_(fft)
{
  if (size() != fft->size() && size() != (fft->size() / 2) + 1)
    throw jconsistency_error("Number of power coefficients %d does not match FFT length %d.", size(), fft->size());
}

const gsl_vector_float* SpectralPowerFloatFeature::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  check_frame_no(frame_no, frame_no_, name());
  const gsl_vector_complex* X = fft_->next(frame_no_ + 1);
  increment_();
  for (unsigned i = 0; i < size(); i++) {
    const double re = X->data[2 * i], im = X->data[2 * i + 1];
    vector_->data[i] = (float)(re * re + im * im);
  }
  return vector_;
}

// ================================================================================ VTLNFeature (feature.cc:1662-1850)
VTLNFeature::VTLNFeature(const VectorFeatureStreamPtr& pow, unsigned coeffN, double ratio, double edge, int version, const String& nm)
    : VectorFeatureStream(coeffN == 0 ? pow->size() : coeffN, nm), FeStageNode(BTK_FE_VTLN), pow_(pow), ratio_(ratio), edge_(edge),
      version_(version)
{
  if (version != 1 && version != 2) throw jtype_error("[ERROR] VTLNFeature >> unknown version number (%d)", version);
  build_();
  fe_wire_(dynamic_cast<FeStageNode*>(pow_.operator->()), NULL);
}

void VTLNFeature::build_()
{
  const int N = (int)size(), inN = (int)pow_->size();
  std::vector<int> off(N), cnt(N);
  w_.assign((size_t)N * inN, 0.0);
  int nw = 0;
  check_abi(btk_fe_vtln_table(N, inN, ratio_, edge_, version_, off.data(), cnt.data(), w_.data(), N * inN, &nw));
  w_.resize(nw);
  pack_rows(off, cnt, rows_);
  fe_tables_changed_();
}

void VTLNFeature::warp(double w)
{
  ratio_ = w;
  build_();
}

void VTLNFeature::matrix(gsl_matrix* mat) const
{
  if (mat->size1 != size() || mat->size2 != pow_->size())
    throw jdimension_error("Matrix (%d x %d) does not match (%d x %d)", (int)mat->size1, (int)mat->size2, (int)size(), (int)pow_->size());
  for (size_t i = 0; i < mat->size1; i++)
    for (size_t j = 0; j < mat->size2; j++) gsl_matrix_set(mat, i, j, 0.0);
  for (unsigned i = 0; i < size(); i++)
    for (int j = 0; j < rows_[3 * i + 1]; j++) gsl_matrix_set(mat, i, rows_[3 * i] + j, w_[rows_[3 * i + 2] + j]);
}

const gsl_vector* VTLNFeature::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  check_frame_no(frame_no, frame_no_, name());
  const float* p = fe_next_();
  increment_();
  for (unsigned i = 0; i < size(); i++) vector_->data[i] = p[i];
  return vector_;
}

void VTLNFeature::fe_params(btk_fe_params& q)
{
  if (tables_dirty_) {
    fe_upload_(d_rows_, rows_.data(), sizeof(int) * rows_.size());
    fe_upload_(d_w_, w_.data(), sizeof(double) * w_.size());
    tables_dirty_ = false;
  }
  q.vtlnN = (int)size(); q.vtln_nw = (int)w_.size();
  q.vtln_rows = static_cast<const int*>(d_rows_.get());
  q.vtln_w = static_cast<const double*>(d_w_.get());
}

void VTLNFeature::fe_advance(long n, const float* last)
{
  frame_no_ += (int)n;
  for (unsigned i = 0; i < size(); i++) vector_->data[i] = last[i];
}

void VTLNFeature::fe_pull_one(std::vector<float>& in, int& in_stage, int& in_dim, int& L)
{
  const gsl_vector* v = pow_->next(frame_no_ + 1);
  in.resize(pow_->size());
  for (unsigned i = 0; i < pow_->size(); i++) in[i] = (float)v->data[i];
  in_stage = BTK_FE_POWER; in_dim = (int)pow_->size(); L = 0;
}

// ================================================================================ MelFeature (feature.cc:1892-2242)
MelFeature::MelFeature(const VectorFeatureStreamPtr& mag, int powN, float rate, float low, float up, unsigned filterN, unsigned version,
                       const String& nm)
    : VectorFeatureStream(filterN, nm), FeStageNode(BTK_FE_MEL), mag_(mag), powN_(powN == 0 ? mag->size() : (unsigned)powN)
{
  if (version != 1 && version != 2) throw jtype_error("[ERROR] MelFeature >> Unknown Version.\r\n");
  std::vector<int> off(filterN), cnt(filterN);
  w_.assign((size_t)filterN * powN_, 0.0f);
  int nw = 0;
  const int rc = btk_fe_mel_table((int)powN_, rate, low, up, (int)filterN, (int)version, off.data(), cnt.data(), w_.data(),
                                  (int)(filterN * powN_), &nw);
  if (rc == BTK_ERR_PARAMETER) throw j_error("mel: something wrong with\n");
  check_abi(rc);
  w_.resize(nw);
  pack_rows(off, cnt, rows_);
  fe_wire_(dynamic_cast<FeStageNode*>(mag_.operator->()), NULL);
}

void MelFeature::read(const String& fileName)
{
  throw jio_error("MelFeature %s: band matrices are not read from files (%s)\n", name().c_str(), fileName.c_str());
}

void MelFeature::matrix(gsl_matrix* mat) const
{
  if (mat->size1 != size() || mat->size2 != powN_)
    throw jdimension_error("Matrix (%d x %d) does not match (%d x %d)", (int)mat->size1, (int)mat->size2, (int)size(), (int)powN_);
  for (size_t i = 0; i < mat->size1; i++)
    for (size_t j = 0; j < mat->size2; j++) gsl_matrix_set(mat, i, j, 0.0);
  for (unsigned i = 0; i < size(); i++)
    for (int j = 0; j < rows_[3 * i + 1]; j++) gsl_matrix_set(mat, i, rows_[3 * i] + j, w_[rows_[3 * i + 2] + j]);
}

const gsl_vector* MelFeature::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  check_frame_no(frame_no, frame_no_, name());
  const float* p = fe_next_();
  increment_();
  for (unsigned i = 0; i < size(); i++) vector_->data[i] = p[i];
  return vector_;
}

void MelFeature::fe_params(btk_fe_params& q)
{
  if (tables_dirty_) {
    fe_upload_(d_rows_, rows_.data(), sizeof(int) * rows_.size());
    fe_upload_(d_w_, w_.data(), sizeof(float) * w_.size());
    tables_dirty_ = false;
  }
  q.melN = (int)size(); q.mel_nw = (int)w_.size();
  q.mel_rows = static_cast<const int*>(d_rows_.get());
  q.mel_w = static_cast<const float*>(d_w_.get());
}

void MelFeature::fe_advance(long n, const float* last)
{
  frame_no_ += (int)n;
  for (unsigned i = 0; i < size(); i++) vector_->data[i] = last[i];
}

void MelFeature::fe_pull_one(std::vector<float>& in, int& in_stage, int& in_dim, int& L)
{
  const gsl_vector* v = mag_->next(frame_no_ + 1);
  in.resize(mag_->size());
  for (unsigned i = 0; i < mag_->size(); i++) in[i] = (float)v->data[i];
  in_stage = BTK_FE_VTLN; in_dim = (int)mag_->size(); L = 0;
}

// ================================================================================ LogFeature (feature.cc:2326-2362)
LogFeature::LogFeature(const VectorFeatureStreamPtr& mel, double m, double a, bool sphinxFlooring, const String& nm)
    : VectorFloatFeatureStream(mel->size(), nm), FeStageNode(BTK_FE_LOG), mel_(mel), m_(m), a_(a), floor_(sphinxFlooring)
{
  fe_wire_(dynamic_cast<FeStageNode*>(mel_.operator->()), NULL);
}

const gsl_vector_float* LogFeature::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  check_frame_no(frame_no, frame_no_, name());
  const float* p = fe_next_();
  increment_();
  memcpy(vector_->data, p, sizeof(float) * size());
  return vector_;
}

void LogFeature::fe_params(btk_fe_params& q) { q.log_m = m_; q.log_a = a_; q.log_floor = floor_; }

void LogFeature::fe_advance(long n, const float* last)
{
  frame_no_ += (int)n;
  memcpy(vector_->data, last, sizeof(float) * size());
}

void LogFeature::fe_pull_one(std::vector<float>& in, int& in_stage, int& in_dim, int& L)
{
  const gsl_vector* v = mel_->next(frame_no_ + 1);
  in.resize(mel_->size());
  for (unsigned i = 0; i < mel_->size(); i++) in[i] = (float)v->data[i];
  in_stage = BTK_FE_MEL; in_dim = (int)mel_->size(); L = 0;
}

// ================================================================================ CepstralFeature (feature.cc:2370-2428)
CepstralFeature::CepstralFeature(const VectorFloatFeatureStreamPtr& mel, unsigned ncep, int type, const String& nm)
    : VectorFloatFeatureStream(ncep, nm), FeStageNode(BTK_FE_CEP), mel_(mel), cos_((size_t)ncep * mel->size())
{
  const int rc = btk_fe_dct_table(type, (int)ncep, (int)mel->size(), cos_.data());
  if (rc == BTK_ERR_PARAMETER) throw jindex_error("Unknown DCT type\n");
  check_abi(rc);
  fe_wire_(dynamic_cast<FeStageNode*>(mel_.operator->()), NULL);
}

gsl_matrix* CepstralFeature::matrix() const
{
  gsl_matrix* m = gsl_matrix_alloc(size(), mel_->size());
  for (size_t i = 0; i < m->size1; i++)
    for (size_t j = 0; j < m->size2; j++) gsl_matrix_set(m, i, j, cos_[i * m->size2 + j]);
  return m;
}

const gsl_vector_float* CepstralFeature::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  check_frame_no(frame_no, frame_no_, name());
  const float* p = fe_next_();
  increment_();
  memcpy(vector_->data, p, sizeof(float) * size());
  return vector_;
}

void CepstralFeature::fe_params(btk_fe_params& q)
{
  if (tables_dirty_) {
    fe_upload_(d_cos_, cos_.data(), sizeof(float) * cos_.size());
    tables_dirty_ = false;
  }
  q.cepN = (int)size();
  q.dct = static_cast<const float*>(d_cos_.get());
}

void CepstralFeature::fe_advance(long n, const float* last)
{
  frame_no_ += (int)n;
  memcpy(vector_->data, last, sizeof(float) * size());
}

void CepstralFeature::fe_pull_one(std::vector<float>& in, int& in_stage, int& in_dim, int& L)
{
  const gsl_vector_float* v = mel_->next(frame_no_ + 1);
  in.assign(v->data, v->data + mel_->size());
  in_stage = BTK_FE_LOG; in_dim = (int)mel_->size(); L = 0;
}
