// convolution/convolution.h -- OverlapAdd and OverlapSave (reference convolution/convolution.h:20-84, convolution/convolution.cc:24-235):
// block convolution of a float stream with an impulse response, over btk_conv_apply / btk_conv_blocks (csrc/conv_kernels.hip).
//
// OverlapAdd hands out, block after block, the linear convolution of the source's blocks LAID END TO END AS SERVED with the
// impulse response (also where the source's blocks overlap), truncated to the samples that came in: T blocks in, T blocks of
// the same size out, the last P - 1 samples of the convolution never handed out (convolution.cc:116-127).  The device computes it
// in the overlap-save arrangement; the reference's float32 running sum of float64 sections is not re-enacted.
// OverlapSave treats every block alone: an L-point circular convolution of which samples P .. L - 1 are handed out
// (convolution.cc:225-226; index P - 1, also free of wrap-around, is dropped there and here).
//
// Block service as the front-end nodes do it (feature/feature.h): over a SampleFeature (any shift) the first next() of a block
// pulls up to block_frames sample blocks with next_blocks, lays them end to end (OverlapAdd: behind the P - 1 samples kept from
// the previous launch), launches ONCE and serves the frames from a pinned host copy; over any other float source each next()
// uploads the one block the source hands out.  block_frames: constructor argument, 0 = BTK_CONV_BLOCK_FRAMES or 64.
// Construction touches no device: the taps (float64 at the interface) are rounded to float32 on the host and their spectra are
// computed on the device with the first launch.
//
// OverlapAdd's fftLen is validated as the reference validates it (convolution.cc:63-81: non-zero and < L + P - 1 is a
// jdimension_error) and, because GSL's radix-2 transform fails there, a non-zero fftLen that is no power of two is one too;
// apart from that it does not select the device's transform: btk_conv_plan does.  The node's tile length is the plan's, reduced
// to L / k for the smallest k that divides L where a block does not hold a whole number of tiles, so that every launch ends on
// a tile boundary and the frames have the same bits for every block_frames; the transform is the shortest that holds such a tile.
// OverlapSave's transform is the block length itself: L must be a power of two from 256 to 16384 (the reference leaves the
// power of two unchecked, convolution.cc:189), P >= L is the reference's jdimension_error (:180-181, :190-191).
// Not carried over: OverlapSave::update (convolution.cc:237-245 writes L entries into a vector of L/2 + 1; not in convolution.i).
#pragma once
#include <vector>
#include "stream/stream.h"
#include "common/devmem.h"

class SampleFeature;

class BlockConvolution : public VectorFloatFeatureStream {
 public:
  virtual ~BlockConvolution() {}
  virtual const gsl_vector_float* next(int frame_no = -5);
  virtual void reset();
  unsigned taps() const { return P_; }
  long block_frames() const { return block_frames_; }
  void set_block_frames(long n);
  long launches() const { return launches_; }           // launches of the tile kernel this node has made since it was built (tests)
  // the transform the device runs: N, outputs per tile, taps per partition, partitions
  void plan(int* N, int* Lk, int* Bp, int* Q) const { *N = N_; *Lk = Lk_; *Bp = Bp_; *Q = Q_; }
 protected:
  BlockConvolution(const VectorFloatFeatureStreamPtr& samp, const gsl_vector* impulseResponse, unsigned out_size, bool save,
                   const String& nm, long block_frames);
  int N_, Lk_, Bp_, Q_;
  const unsigned L_, P_;
 private:
  void fill_block_();
  VectorFloatFeatureStreamPtr samp_;
  SampleFeature* sample_;                               // samp_ when it is one
  const bool save_;
  std::vector<float> h_;                                // the taps as the device reads them
  std::vector<float> tail_;                             // OverlapAdd: the last P - 1 samples of the stream so far
  bool have_spectra_;
  long block_frames_, blk_n_, blk_pos_, launches_;
  PinnedBuffer h_in_, h_out_;
  DeviceBuffer d_in_, d_out_, d_h_, d_H_;
};

class OverlapAdd : public BlockConvolution {
 public:
  OverlapAdd(const VectorFloatFeatureStreamPtr& samp, const gsl_vector* impulseResponse, unsigned fftLen = 0,
             const String& nm = "Overlap Add", long block_frames = 0);
  unsigned fftLen() const { return fftLen_; }           // the reference's N: the argument, or the smallest power of two >= L + P - 1
 private:
  static unsigned check_fftLen_(unsigned sectionLen, unsigned irLen, unsigned fftLen);
  unsigned fftLen_;
};
typedef Inherit<OverlapAdd, VectorFloatFeatureStreamPtr> OverlapAddPtr;

class OverlapSave : public BlockConvolution {
 public:
  OverlapSave(const VectorFloatFeatureStreamPtr& samp, const gsl_vector* impulseResponse, const String& nm = "Overlap Save",
              long block_frames = 0);
 private:
  static unsigned check_output_size_(const gsl_vector* impulseResponse, unsigned sampLen);
};
typedef Inherit<OverlapSave, VectorFloatFeatureStreamPtr> OverlapSavePtr;
