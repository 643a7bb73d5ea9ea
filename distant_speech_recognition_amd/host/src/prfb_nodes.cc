// prfb_nodes.cc -- PerfectReconstructionFFTAnalysisBank, PerfectReconstructionFFTSynthesisBank, NormalFFTAnalysisBank,
// DelayFeature and get_window of modulated/modulated.h over btk_prfb_* / btk_stft_* (csrc/fb_pr_kernels.hip): block-serving
// nodes, one launch per round of frames.  A launch of the C-ABI numbers frames and blocks from the start of the samples /
// frames it is given; a round hands it a window that begins early enough for the first frame of the round to see all of its
// history, so that every frame and block has the bits of one launch over the whole stream.
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>

#include "modulated/modulated.h"
#include "feature/feature.h"
#include "btkhip.h"
#include "node_runtime.h"

namespace {

using btknode::check_abi;
using btknode::check_hip;

bool pow2(unsigned v) { return v && !(v & (v - 1)); }

// the limits of btk_prfb_create, checked where no device is touched yet
void check_pr_geometry(gsl_vector* prototype, unsigned M, unsigned m, unsigned r)
{
  if (!pow2(M) || M < 8 || M > 1024) throw jparameter_error("M=%d must be a power of two in [8, 1024]", (int)M);
  if (m < 1 || m > 64) throw jparameter_error("m=%d out of range [1, 64]", (int)m);
  if (r > 2) throw jparameter_error("r=%d out of range [0, 2]", (int)r);
  if (prototype->size != (size_t)2 * M * m)
    throw jconsistency_error("Prototype sizes do not match (%d vs. %d).", (int)prototype->size, (int)(2 * M * m));
}

std::vector<double> dense(const gsl_vector* v)
{
  std::vector<double> d(v->size);
  for (size_t i = 0; i < v->size; i++) d[i] = v->data[i * v->stride];
  return d;
}

}  // namespace

gsl_vector* get_window(unsigned winType, unsigned winLen)
{
  gsl_vector* win = gsl_vector_calloc(winLen);
  check_abi(btk_get_window((int)winType, (int)winLen, win->data));
  return win;
}

// ================================================================================ analysis nodes
BlockAnalysisBank::BlockAnalysisBank(VectorFloatFeatureStreamPtr& samp, unsigned bins, unsigned D, unsigned hist_blocks, unsigned pd,
                                     const String& nm)
    : VectorComplexFeatureStream(bins, nm), samp_(samp), sample_(dynamic_cast<SampleFeature*>(samp_.operator->())), D_(D),
      hist_blocks_(hist_blocks), pd_(pd), block_frames_(btk_default_block_frames()), launches_(0), win_b0_(0), nblk_(0), eos_(false),
      chunk_base_(0), chunk_len_(0)
{
  if (samp_->size() != D_) throw jdimension_error("Input block length (%d) != D_ (%d)\n", samp_->size(), D_);
}

void BlockAnalysisBank::reset()
{
  samp_->reset();
  VectorComplexFeatureStream::reset();
  win_.clear();
  win_b0_ = 0; nblk_ = 0; eos_ = false; chunk_base_ = 0; chunk_len_ = 0;
}

// one launch for the frames the source's next blocks complete
void BlockAnalysisBank::fill_()
{
  const long first = chunk_base_ + chunk_len_;
  if (!eos_) {
    // a short last block arrives zero-padded from a SampleFeature; any other source is pulled one block, one frame, at a time
    const long want = sample_ ? (block_frames_ > 0 ? block_frames_ : (1L << 30)) : 1;
    if (sample_) {
      const long step = std::min(want, 4096L);
      long got = 0;
      while (got < want) {
        const long ask = std::min(step, want - got);
        win_.resize((size_t)(nblk_ - win_b0_ + ask) * D_);
        const long n = sample_->next_blocks(win_.data() + (size_t)(nblk_ - win_b0_) * D_, ask);
        nblk_ += n > 0 ? n : 0;
        got += n > 0 ? n : 0;
        if (n < ask) { eos_ = true; break; }
      }
      win_.resize((size_t)(nblk_ - win_b0_) * D_);
    } else {
      try {
        const gsl_vector_float* block = samp_->next((int)nblk_);
        win_.resize((size_t)(nblk_ - win_b0_ + 1) * D_);
        float* dst = win_.data() + (size_t)(nblk_ - win_b0_) * D_;
        for (unsigned i = 0; i < D_; i++) dst[i] = block->data[i * block->stride];
        nblk_++;
      } catch (jiterator_error&) {
        eos_ = true;
      }
    }
  }
  const long end = eos_ ? nblk_ + (long)pd_ : nblk_;      // frame t reads input blocks <= t; pd_ zero blocks follow the last
  if (first >= end) { is_end_ = true; throw jiterator_error("end of samples!"); }
  const long tcount = end - first;
  const long wb0 = std::max(0L, first - (long)hist_blocks_ + 1);          // oldest block the round's first frame reads
  if (wb0 < win_b0_) throw jconsistency_error("analysis window starts at block %ld, block %ld is needed", win_b0_, wb0);
  const size_t nsamp = (size_t)(nblk_ - wb0) * D_;
  const size_t bins = size();
  hipStream_t st = static_cast<hipStream_t>(btk_node_stream());
  float* hin = static_cast<float*>(hIn_.ensure(sizeof(float) * std::max(nsamp, (size_t)1)));
  float* din = static_cast<float*>(dIn_.ensure(sizeof(float) * std::max(nsamp, (size_t)1)));
  void* dx = dX_.ensure(2 * sizeof(float) * bins * (size_t)tcount);
  void* hx = hX_.ensure(2 * sizeof(float) * bins * (size_t)tcount);
  if (nsamp) {
    memcpy(hin, win_.data() + (size_t)(wb0 - win_b0_) * D_, sizeof(float) * nsamp);
    check_hip(hipMemcpyAsync(din, hin, sizeof(float) * nsamp, hipMemcpyHostToDevice, st), "analysis window upload");
  }
  check_abi(launch_(din, (long)nsamp, dx, tcount, first - wb0, tcount, st));
  launches_++;
  check_hip(hipMemcpyAsync(hx, dx, 2 * sizeof(float) * bins * (size_t)tcount, hipMemcpyDeviceToHost, st), "analysis frames download");
  btk_node_count_d2h(2 * sizeof(float) * bins * (size_t)tcount);
  check_hip(hipStreamSynchronize(st), "analysis round");
  chunk_base_ = first;
  chunk_len_ = tcount;
  // drop the blocks only frames before `end` needed
  const long keep0 = std::max(win_b0_, std::min(nblk_, std::max(0L, end - (long)hist_blocks_ + 1)));
  if (keep0 > win_b0_) {
    win_.erase(win_.begin(), win_.begin() + (size_t)(keep0 - win_b0_) * D_);
    win_b0_ = keep0;
  }
}

const gsl_vector_complex* BlockAnalysisBank::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  if (frame_no >= 0 && frame_no - 1 != frame_no_)
    throw jindex_error("Problem in Feature %s: %d != %d\n", name().c_str(), frame_no - 1, frame_no_);
  const long idx = frame_no_ + 1;
  if (idx >= chunk_base_ + chunk_len_) fill_();
  const float* x = static_cast<const float*>(hX_.get()) + 2 * (size_t)(idx - chunk_base_);
  const size_t bins = size();
  for (size_t k = 0; k < bins; k++) {
    vector_->data[2 * k * vector_->stride] = x[2 * k * (size_t)chunk_len_];
    vector_->data[2 * k * vector_->stride + 1] = x[2 * k * (size_t)chunk_len_ + 1];
  }
  increment_();
  return vector_;
}

NormalFFTAnalysisBank::NormalFFTAnalysisBank(VectorFloatFeatureStreamPtr& samp, unsigned fftLen, unsigned r, unsigned windowType,
                                             const String& nm)
    : BlockAnalysisBank(samp, fftLen, r < 31 ? fftLen >> r : 0, 1u << (r < 31 ? r : 0), 1, nm), M_(fftLen), r_(r),
      window_type_(windowType), plan_(NULL)
{
  if (!pow2(M_) || M_ < 8 || M_ > 2048) throw jparameter_error("fftLen=%d must be a power of two in [8, 2048]", (int)M_);
  if (r_ > 11 || (M_ >> r_) < 1) throw jparameter_error("r=%d leaves no frame shift", (int)r_);
}

NormalFFTAnalysisBank::~NormalFFTAnalysisBank() { btk_stft_destroy(plan_); }

int NormalFFTAnalysisBank::launch_(const float* dpcm, long nsamples, void* dX, long T_stride, long t0, long tcount, void* stream)
{
  if (!plan_) check_abi(btk_stft_create(&plan_, (int)M_, (int)r_, (int)window_type_));
  return btk_stft_analysis(plan_, dpcm, nsamples, nsamples, 1, 1, dX, T_stride, t0, tcount, stream);
}

PerfectReconstructionFFTAnalysisBank::PerfectReconstructionFFTAnalysisBank(VectorFloatFeatureStreamPtr& samp, gsl_vector* prototype,
                                                                           unsigned M, unsigned m, unsigned r, const String& nm)
    : BlockAnalysisBank(samp, 2 * M, r < 31 ? M >> r : 0, (r + 2) * (m > 0 ? m - 1 : 0) + (2u << (r < 30 ? r : 0)), 2 * m - 1, nm),
      M_(M), m_(m), r_(r), plan_(NULL)
{
  check_pr_geometry(prototype, M, m, r);
  proto_ = dense(prototype);
}

PerfectReconstructionFFTAnalysisBank::~PerfectReconstructionFFTAnalysisBank() { btk_prfb_destroy(plan_); }

int PerfectReconstructionFFTAnalysisBank::launch_(const float* dpcm, long nsamples, void* dX, long T_stride, long t0, long tcount,
                                                  void* stream)
{
  if (!plan_) check_abi(btk_prfb_create(&plan_, (int)M_, (int)m_, (int)r_, 0, proto_.data(), (long)proto_.size()));
  return btk_prfb_analysis(plan_, dpcm, nsamples, nsamples, 1, 1, dX, T_stride, t0, tcount, stream);
}

// ================================================================================ synthesis node
PerfectReconstructionFFTSynthesisBank::PerfectReconstructionFFTSynthesisBank(VectorComplexFeatureStreamPtr& samp, gsl_vector* prototype,
                                                                             unsigned M, unsigned m, unsigned r, const String& nm)
    : VectorFloatFeatureStream(r < 31 ? M >> r : 0, nm), samp_(samp), have_source_(true), M_(M), m_(m), r_(r), D_(r < 31 ? M >> r : 0),
      plan_(NULL), block_frames_(btk_default_block_frames()), launches_(0), win_f0_(0), nframes_(0), src_ended_(false), blk_base_(0),
      nblocks_(0)
{
  init_(prototype);
  if (samp_->size() != 2 * M_) throw jdimension_error("Input frame length (%d) != 2 M (%d)\n", samp_->size(), 2 * M_);
}

PerfectReconstructionFFTSynthesisBank::PerfectReconstructionFFTSynthesisBank(gsl_vector* prototype, unsigned M, unsigned m, unsigned r,
                                                                             const String& nm)
    : VectorFloatFeatureStream(r < 31 ? M >> r : 0, nm), have_source_(false), M_(M), m_(m), r_(r), D_(r < 31 ? M >> r : 0), plan_(NULL),
      block_frames_(btk_default_block_frames()), launches_(0), win_f0_(0), nframes_(0), src_ended_(false), blk_base_(0), nblocks_(0)
{
  init_(prototype);
}

void PerfectReconstructionFFTSynthesisBank::init_(gsl_vector* prototype)
{
  check_pr_geometry(prototype, M_, m_, r_);
  proto_ = dense(prototype);
}

PerfectReconstructionFFTSynthesisBank::~PerfectReconstructionFFTSynthesisBank() { btk_prfb_destroy(plan_); }

void PerfectReconstructionFFTSynthesisBank::reset()
{
  if (have_source_) samp_->reset();
  VectorFloatFeatureStream::reset();
  frames_.clear();
  win_f0_ = 0; nframes_ = 0; src_ended_ = false; blk_base_ = 0; nblocks_ = 0;
}

// one launch for the blocks the source's next frames complete: block j reads frames j + pd - (2R-1) - q (m-1) .. j + pd
void PerfectReconstructionFFTSynthesisBank::fill_()
{
  const size_t M2 = 2 * (size_t)M_;
  const long pd = 2 * (long)m_ - 1, reach = (2L << r_) - 1 + (long)(r_ + 2) * ((long)m_ - 1);
  const long j0 = blk_base_ + nblocks_;
  if (!src_ended_) {
    // the first round primes the ring with pd frames before the frame of block 0 (modulated.cc:866-875)
    const long want = std::max(block_frames_ > 0 ? block_frames_ : (1L << 30), 1L) + (nframes_ == 0 ? pd : 0);
    for (long got = 0; got < want; got++) {
      const gsl_vector_complex* y;
      try {
        y = samp_->next((int)nframes_);
      } catch (jiterator_error&) {
        src_ended_ = true;
        break;
      }
      frames_.resize((size_t)(nframes_ - win_f0_ + 1) * 2 * M2);
      float* dst = frames_.data() + (size_t)(nframes_ - win_f0_) * 2 * M2;
      for (size_t k = 0; k < M2; k++) {
        dst[2 * k] = (float)y->data[2 * k * y->stride];
        dst[2 * k + 1] = (float)y->data[2 * k * y->stride + 1];
      }
      nframes_++;
    }
  }
  const long end = nframes_ - pd;                          // blocks 0 .. end - 1 can be computed
  if (j0 >= end) { is_end_ = true; throw jiterator_error("end of samples!"); }
  const long bcount = end - j0;
  // the launch numbers frames and blocks from the window's first frame: begun 2R - 1 + q (m-1) blocks early, no block of the
  // round is taken for one of the stream's first, whose overlap partners count as zero
  const long wf0 = std::max(0L, j0 - reach);
  if (wf0 < win_f0_) throw jconsistency_error("synthesis window starts at frame %ld, frame %ld is needed", win_f0_, wf0);
  const long T = nframes_ - wf0;
  hipStream_t st = static_cast<hipStream_t>(btk_node_stream());
  float* hy = static_cast<float*>(hY_.ensure(2 * sizeof(float) * M2 * (size_t)T));
  void* dy = dY_.ensure(2 * sizeof(float) * M2 * (size_t)T);
  float* dout = static_cast<float*>(dOut_.ensure(sizeof(float) * (size_t)bcount * D_));
  float* hout = static_cast<float*>(hOut_.ensure(sizeof(float) * (size_t)bcount * D_));
  const float* src = frames_.data() + (size_t)(wf0 - win_f0_) * 2 * M2;
  for (long t = 0; t < T; t++)                             // [frame][M2] -> [M2][T]
    for (size_t k = 0; k < M2; k++) {
      hy[2 * (k * (size_t)T + (size_t)t)] = src[2 * ((size_t)t * M2 + k)];
      hy[2 * (k * (size_t)T + (size_t)t) + 1] = src[2 * ((size_t)t * M2 + k) + 1];
    }
  check_hip(hipMemcpyAsync(dy, hy, 2 * sizeof(float) * M2 * (size_t)T, hipMemcpyHostToDevice, st), "synthesis frames upload");
  if (!plan_) check_abi(btk_prfb_create(&plan_, (int)M_, (int)m_, (int)r_, 1, proto_.data(), (long)proto_.size()));
  check_abi(btk_prfb_synthesis(plan_, dy, T, T, 1, dout, bcount * (long)D_, j0 - wf0, bcount, st));
  launches_++;
  check_hip(hipMemcpyAsync(hout, dout, sizeof(float) * (size_t)bcount * D_, hipMemcpyDeviceToHost, st), "synthesis blocks download");
  btk_node_count_d2h(sizeof(float) * (size_t)bcount * D_);
  check_hip(hipStreamSynchronize(st), "synthesis round");
  blk_base_ = j0;
  nblocks_ = bcount;
  const long keep0 = std::max(win_f0_, std::min(nframes_, std::max(0L, end - reach)));
  if (keep0 > win_f0_) {
    frames_.erase(frames_.begin(), frames_.begin() + (size_t)(keep0 - win_f0_) * 2 * M2);
    win_f0_ = keep0;
  }
}

const gsl_vector_float* PerfectReconstructionFFTSynthesisBank::next(int frame_no)
{
  if (!have_source_) throw j_error("PerfectReconstructionFFTSynthesisBank %s has no source to pull frames from", name().c_str());
  if (frame_no == frame_no_) return vector_;
  if (frame_no >= 0 && frame_no - 1 != frame_no_)
    throw jindex_error("Problem in Feature %s: %d != %d\n", name().c_str(), frame_no - 1, frame_no_);
  const long idx = frame_no_ + 1;
  if (idx >= blk_base_ + nblocks_) fill_();
  const float* b = static_cast<const float*>(hOut_.get()) + (size_t)(idx - blk_base_) * D_;
  for (unsigned i = 0; i < D_; i++) vector_->data[i * vector_->stride] = b[i];
  increment_();
  return vector_;
}

// ================================================================================ DelayFeature
DelayFeature::DelayFeature(const VectorComplexFeatureStreamPtr& samp, float time_delay, const String& nm)
    : VectorComplexFeatureStream(samp->size(), nm), samp_(samp), time_delay_(time_delay)
{
}

void DelayFeature::reset()
{
  samp_->reset();
  VectorComplexFeatureStream::reset();
}

const gsl_vector_complex* DelayFeature::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  const gsl_vector_complex* samp = samp_->next(frame_no);
  const std::complex<double> alpha = std::polar(1.0, (double)time_delay_);
  for (unsigned k = 0; k < size(); k++) {
    // gsl_blas_zscal: (ar xr - ai xi, ar xi + ai xr)
    const double xr = samp->data[2 * k * samp->stride], xi = samp->data[2 * k * samp->stride + 1];
    vector_->data[2 * k * vector_->stride] = alpha.real() * xr - alpha.imag() * xi;
    vector_->data[2 * k * vector_->stride + 1] = alpha.real() * xi + alpha.imag() * xr;
  }
  increment_();
  return vector_;
}
