// conv_nodes.cc -- OverlapAdd and OverlapSave of convolution/convolution.h over btk_conv_apply / btk_conv_blocks
// (csrc/conv_kernels.hip): block-serving nodes, one launch per block of sample blocks.
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "convolution/convolution.h"
#include "feature/feature.h"
#include "btkhip.h"
#include "node_runtime.h"

namespace {

using btknode::check_abi;
using btknode::check_hip;
using btknode::env_block_frames;

bool pow2(unsigned v) { return v && !(v & (v - 1)); }

}  // namespace

BlockConvolution::BlockConvolution(const VectorFloatFeatureStreamPtr& samp, const gsl_vector* impulseResponse, unsigned out_size,
                                   bool save, const String& nm, long block_frames)
    : VectorFloatFeatureStream(out_size, nm), N_(0), Lk_(0), Bp_(0), Q_(0), L_(samp->size()), P_((unsigned)impulseResponse->size),
      samp_(samp), sample_(dynamic_cast<SampleFeature*>(samp_.operator->())), save_(save), have_spectra_(false),
      block_frames_(block_frames > 0 ? block_frames : env_block_frames("BTK_CONV_BLOCK_FRAMES", 64)), blk_n_(0), blk_pos_(0), launches_(0)
{
  // the taps arrive as float64 and are rounded to float32 for the device
  h_.resize(P_);
  for (unsigned i = 0; i < P_; i++) h_[i] = (float)impulseResponse->data[i * impulseResponse->stride];
  if (save_) {
    N_ = (int)L_; Lk_ = (int)(L_ - P_ + 1); Bp_ = (int)P_; Q_ = 1;
  } else {
    check_abi(btk_conv_plan((int)P_, 16384, &N_, &Lk_, &Bp_, &Q_));
    // every launch covers whole blocks: a tile length that divides L puts its end on a tile boundary
    unsigned k = (L_ + (unsigned)Lk_ - 1) / (unsigned)Lk_;
    while (L_ % k) k++;
    Lk_ = (int)(L_ / k);
    N_ = 256;                                           // and the shortest transform that holds such a tile
    while (N_ < Lk_ + Bp_ - 1) N_ *= 2;
    tail_.assign(P_ - 1, 0.f);
  }
}

void BlockConvolution::set_block_frames(long n)
{
  block_frames_ = n > 0 ? n : env_block_frames("BTK_CONV_BLOCK_FRAMES", 64);
}

void BlockConvolution::reset()
{
  samp_->reset();
  VectorFloatFeatureStream::reset();
  blk_n_ = blk_pos_ = 0;
  std::fill(tail_.begin(), tail_.end(), 0.f);           // the reference zeroes its buffer (convolution.cc:133-139)
}

// one launch for the blocks the source has next
void BlockConvolution::fill_block_()
{
  const size_t L = L_, hist = save_ ? 0 : P_ - 1, out = size();
  const long want = sample_ ? block_frames_ : 1;
  float* in = static_cast<float*>(h_in_.ensure(sizeof(float) * (hist + L * (size_t)want)));
  long n = 1;
  if (sample_) {
    n = sample_->next_blocks(in + hist, want);
    if (n <= 0) { is_end_ = true; throw jiterator_error("end of samples!"); }
  } else {
    const gsl_vector_float* block;
    try {
      block = samp_->next(frame_no_ + 1);
    } catch (jiterator_error&) {
      is_end_ = true;
      throw;
    }
    memcpy(in + hist, block->data, sizeof(float) * L);
  }
  if (hist) memcpy(in, tail_.data(), sizeof(float) * hist);
  hipStream_t st = static_cast<hipStream_t>(btk_node_stream());
  const size_t nin = hist + L * (size_t)n, nout = out * (size_t)n;
  if (!have_spectra_) {
    float* dh = static_cast<float*>(d_h_.ensure(sizeof(float) * P_));
    void* dH = d_H_.ensure(2 * sizeof(float) * (size_t)Q_ * (N_ / 2 + 1));
    check_hip(hipMemcpyAsync(dh, h_.data(), sizeof(float) * P_, hipMemcpyHostToDevice, st), "convolution taps upload");
    check_hip(hipStreamSynchronize(st), "convolution taps upload");   // h_ is pageable memory
    check_abi(btk_conv_filter_spectra(dh, (long)P_, 1, (int)P_, N_, Bp_, Q_, dH, st));
    have_spectra_ = true;
  }
  float* din = static_cast<float*>(d_in_.ensure(sizeof(float) * nin));
  float* dout = static_cast<float*>(d_out_.ensure(sizeof(float) * nout));
  float* hout = static_cast<float*>(h_out_.ensure(sizeof(float) * nout));
  check_hip(hipMemcpyAsync(din, in, sizeof(float) * nin, hipMemcpyHostToDevice, st), "convolution upload");
  if (save_)
    check_abi(btk_conv_blocks(din, (long)nin, (long)nin, 1, n, (long)L, d_H_.get(), 1, 1, (int)P_, (int)L_, dout, st));
  else
    check_abi(btk_conv_apply(din + hist, (long)(L * (size_t)n), (long)hist, (long)nin, 1, d_H_.get(), 1, 1, (int)P_, N_, Lk_, Bp_,
                             Q_, dout, (long)nout, (long)nout, st));
  launches_++;
  check_hip(hipMemcpyAsync(hout, dout, sizeof(float) * nout, hipMemcpyDeviceToHost, st), "convolution download");
  btk_node_count_d2h(sizeof(float) * nout);
  check_hip(hipStreamSynchronize(st), "convolution block");
  if (hist) memcpy(tail_.data(), in + nin - hist, sizeof(float) * hist);   // nin >= hist + L: the last P - 1 samples so far
  blk_n_ = n;
  blk_pos_ = 0;
}

const gsl_vector_float* BlockConvolution::next(int frame_no)
{
  if (frame_no == frame_no_) return vector_;
  if (frame_no >= 0 && frame_no - 1 != frame_no_)
    throw jindex_error("Problem: %d != %d\n", frame_no - 1, frame_no_);
  if (blk_pos_ >= blk_n_) fill_block_();
  memcpy(vector_->data, static_cast<const float*>(h_out_.get()) + (size_t)blk_pos_ * size(), sizeof(float) * size());
  blk_pos_++;
  increment_();
  return vector_;
}

// ---- OverlapAdd
unsigned OverlapAdd::check_fftLen_(unsigned sectionLen, unsigned irLen, unsigned fftLen)
{
  if (irLen < 1) throw jdimension_error("Impulse response has no taps.");
  if (fftLen == 0) {
    fftLen = 1;
    while (fftLen < sectionLen + irLen - 1) fftLen *= 2;
    return fftLen;
  }
  if (fftLen < sectionLen + irLen - 1)
    throw jdimension_error("Section (%d) and impulse response (%d) lengths inconsistent with FFT length (%d).", sectionLen, irLen,
                           fftLen);
  if (!pow2(fftLen)) throw jdimension_error("FFT length (%d) is no power of two.", fftLen);
  return fftLen;
}

OverlapAdd::OverlapAdd(const VectorFloatFeatureStreamPtr& samp, const gsl_vector* impulseResponse, unsigned fftLen, const String& nm,
                       long block_frames)
    : BlockConvolution(samp, impulseResponse, (check_fftLen_(samp->size(), (unsigned)impulseResponse->size, fftLen), samp->size()),
                       false, nm, block_frames),
      fftLen_(check_fftLen_(samp->size(), (unsigned)impulseResponse->size, fftLen))
{
}

// ---- OverlapSave
unsigned OverlapSave::check_output_size_(const gsl_vector* impulseResponse, unsigned sampLen)
{
  const unsigned irLen = (unsigned)impulseResponse->size;
  if (irLen < 1) throw jdimension_error("Impulse response has no taps.");
  if (irLen >= sampLen) throw jdimension_error("Cannot have P = %d and L = %d", irLen, sampLen);
  if (!pow2(sampLen) || sampLen < 256 || sampLen > 16384)
    throw jdimension_error("Block length L = %d must be a power of two from 256 to 16384", sampLen);
  return sampLen - irLen;
}

OverlapSave::OverlapSave(const VectorFloatFeatureStreamPtr& samp, const gsl_vector* impulseResponse, const String& nm,
                         long block_frames)
    : BlockConvolution(samp, impulseResponse, check_output_size_(impulseResponse, samp->size()), true, nm, block_frames)
{
}
