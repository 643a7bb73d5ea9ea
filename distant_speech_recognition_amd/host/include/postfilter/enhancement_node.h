// postfilter/enhancement_node.h -- the block machinery shared by SpectralSubtractor, WienerFilter (postfilter/spectralsubtraction.h)
// and HighPassFilter (postfilter/postfilter.h): not part of the reference's interface.
//
// A node gathers a BLOCK of frames of its C sources on the device -- analysis banks hand their sample windows over and the frames
// are computed where the node reads them; engine nodes that offer their block on the device (BlockSource::device_block():
// beamformers, post-filters, echo cancellers, these nodes themselves) are taken block by block, device to device, with the
// consumer's advance_to() mark passed on to them and the block fetched again when their block_version() changes, so that a
// weight change upstream keeps its per-frame meaning through this node; any other source is drained through next() -- runs its
// kernel over the block, offers
// the result to a consumer that takes blocks (BlockSource, modulated/modulated.h) and serves next() from a host mirror with the
// Hermitian upper half.
//
// Mode switches mid-stream.  The reference changes a node's mode between two next() calls; a block is computed ahead of them.
// The node keeps its recursion state as it was at the start of the current SEGMENT (the block's start, or the last switch) and
// the mark a per-frame graph would have pulled to (advance_to(), or the last frame next() served).  A switch
//   1. replays the segment up to the mark from the kept state into a scratch block (frames already handed over keep their values),
//      which leaves the state exactly where a per-frame graph would have it when the switch is called,
//   2. lets the caller change state and parameters there (average(), clear(), a noise file, a new factor),
//   3. starts a new segment behind the mark, bumps block_version() and recomputes the rest of the block on demand.
// Every segment therefore has one constant mode, which is what the entry points take when no per-frame flags are given.
// Scan chunks sit on multiples of 64 of the stream's frame counter (include/btkhip.h), so blocks of 64, 128 or all frames give
// the same samples.
#pragma once
#include <memory>
#include <vector>

#include "stream/stream.h"
#include "modulated/modulated.h"
#include "common/devmem.h"

class EnhancementBlockNode_ : public VectorComplexFeatureStream, public BlockSource {
 public:
  virtual const gsl_vector_complex* next(int frame_no = -5);
  virtual void reset();
  // frames per block when the sources are drained through next() (analysis banks bring their own block_frames())
  void set_block_frames(long n) { block_frames_ = n < 0 ? 0 : n; }
  long block_frames() const { return block_frames_; }
  // BlockSource
  virtual unsigned long block_version();         // also notices a source whose block has changed
  virtual const std::vector<float>& block(long& T);
  virtual const void* device_block(long& T, long& T_stride);
  virtual long block_base();
  virtual bool next_block();
  virtual void advance_to(long frame_idx);
 protected:
  EnhancementBlockNode_(unsigned fftLen, bool channel_major, const String& nm);
  void add_source_(const VectorComplexFeatureStreamPtr& s);
  unsigned channels_() const { return (unsigned)srcs_.size(); }
  // what a subclass provides: the size of its device state, its initial value, and the kernel over frames [t0, t1) of the block.
  // dX: the sources' frames, complex64 [K][C][Ts] (or [C][K][Ts], channel_major); dOut: complex64 [K][Ts]; both point at frame 0
  virtual size_t state_bytes_() const { return 0; }
  virtual void init_state_(void*) {}
  virtual void launch_(const void* dX, void* dOut, long Ts, long t0, long t1, long frames_done) = 0;
  virtual bool keeps_frame_counter_on_reset_() const { return false; }
  // a mode switch (see above): begin_switch_() puts the state at the mark, end_switch_() keeps what the caller made of it
  // (need_state = false: a switch of parameters only; before the first block it touches no device)
  void* begin_switch_(bool need_state = true);  // returns the device state (NULL when the node has none)
  void end_switch_();
  // reading the state as a per-frame graph has it now, without a switch: the segment is replayed up to the mark, the caller
  // reads, end_peek_() puts the state back; block_version(), the segment and the computed block stay as they are
  void* begin_peek_();
  void end_peek_();
  void* state_dev_() const { return dState_.get(); }
  const unsigned fftLen_;
 private:
  bool load_block_();
  bool gather_banks_(long f0, long& Tn);
  bool gather_next_(long f0, long& Tn);
  bool gather_blocks_(bool advance, long f0, long& Tn);
  void copy_source_blocks_(long T);
  void poll_sources_();
  void ensure_first_();
  void ensure_current_();
  void alloc_state_();
  const float* host_output_();
  std::vector<VectorComplexFeatureStreamPtr> srcs_;
  std::vector<OverSampledDFTAnalysisBank*> banks_;        // all sources are analysis banks, or empty
  std::vector<BlockSource*> bsrcs_;                       // all sources offer device blocks, or empty
  std::vector<unsigned long> src_versions_;
  const bool channel_major_;
  long block_frames_;
  bool prepared_, ended_, state_ready_, dirty_;
  long base_, T_, Ts_, seg0_;                   // the current block; first frame of the current segment within it
  long handed_, served_, fd0_;                  // block protocol mark; frames next() served; frames before the last reset()
  unsigned long version_;
  DeviceBuffer dX_, dY_, dTmp_, dCh_, dState_, dSnap_, dPeek_;
  std::vector<std::unique_ptr<DeviceBuffer> > dPcm_;
  PinnedBuffer hX_;
  std::vector<float> Yhost_, dense_;
  bool Yhost_valid_;
};
