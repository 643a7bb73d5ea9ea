// feature/feature.h -- SampleFeature (reference feature/feature.h:153-206, feature/feature.cc:221-680): the utterance
// holder at the head of every beamforming graph -- 16-bit PCM WAV in (un-normalised float blocks out), the sample-level
// helpers the reference's scripts call on it, and the 16-bit WAV writer at the tail.
// Not carried over: sample-rate conversion (the reference's is behind #ifdef SRCONV, off in its build) and the non-WAV
// libsndfile containers (read()/write() raise jio_error for them).
#pragma once
#include <vector>
#include "stream/stream.h"
#include "common/devmem.h"

namespace sndfile {      // the two libsndfile constants callers of write() spell out (sndfile.h values)
enum { SF_FORMAT_WAV = 0x010000, SF_FORMAT_PCM_16 = 0x0002 };
}

class SampleFeature;
class PreemphasisFeature;
class StorageFeature;
typedef Inherit<SampleFeature, VectorFloatFeatureStreamPtr> SampleFeaturePtr;

class SampleFeature : public VectorFloatFeatureStream {
 public:
  SampleFeature(const String& fn = "", unsigned blockLen = 320, unsigned shiftLen = 160, bool padZeros = false,
                const String& nm = "Sample");
  virtual ~SampleFeature();
  // `format` is the reference's 2nd positional argument (callers pass the sample rate there)
  unsigned read(const String& fn, int format = 0, int samplerate = 16000, int chX = 1, int chN = 1,
                int cfrom = 0, int to = -1, int outsamplerate = -1, float norm = 0.0);
  // 16-bit PCM WAV, one channel; with norm == 0 at read time the samples are taken as int16-scale values, otherwise as
  // [-1, 1) values divided by that norm first (feature.cc:429-518)
  void write(const String& fn, int format = sndfile::SF_FORMAT_WAV | sndfile::SF_FORMAT_PCM_16, int sampleRate = -1);
  void cut(unsigned cfrom, unsigned cto);
  bool isEnd() { return is_end(); }                     // src/ss.cc:247 calls it (the reference's own header lost it)
  void randomize(int startX, int endX, double sigma2);
  virtual const gsl_vector_float* next(int frame_no = -5);
  virtual void reset() { cur_ = 0; VectorFloatFeatureStream::reset(); is_end_ = false; }
  void exit() { reset(); throw jiterator_error("end of samples!"); }
  const gsl_vector_float* data();
  const gsl_vector* dataDouble();
  void copySamples(SampleFeaturePtr& src, unsigned cfrom, unsigned to);
  unsigned samplesN() const { return (unsigned)samples_.size(); }
  int getSampleRate() const { return samplerate_; }
  int getChanN() const { return nChan_; }
  void zeroMean();
  void addWhiteNoise(float snr);
  void setSamples(const gsl_vector* samples, unsigned sampleRate);
  void set_samples(const float* samples, size_t n);          // in-memory source (same state as after read())
  // engine hook: up to nmax consecutive next() calls at once, the blocks stored back to back in dst (nmax * size() floats);
  // returns how many there were -- fewer than nmax: the stream has ended exactly as the throwing next() would have ended it
  long next_blocks(float* dst, long nmax);
  // engine hooks (round 6): the utterance AS 16-BIT PCM.  A WAV holds int16 samples and read() with norm == 0 hands them out as
  // un-normalised floats (feature/feature.cc:265-269), so an analysis bank on the device may take the samples as they were stored:
  // half the bytes through host memory and PCIe, and -- the widening is exact -- the same bits out of the filter bank.
  // pcm16(): the loaded samples as int16 in pinned memory, zero-padded by at least two blocks behind the last sample; NULL when a
  // sample is not an integer of the int16 range (normalised reads, randomize(), noise that overflowed) or blocks overlap
  // (shiftLen != blockLen).  Built when first asked for after the samples changed; stays where it is until they change again.
  const short* pcm16();
  // the state transitions of up to nmax next() calls WITHOUT the copies (the caller reads the blocks out of pcm16()): returns how
  // many there were and the sample index the first of them starts at; fewer than nmax: the stream has ended as next() ends it
  long advance_blocks(long nmax, size_t* first_sample);
  unsigned shiftlen() const { return shiftLen_; }
  // counts the changes of the samples (a reader that keeps the pcm16() pointer compares it before every use)
  unsigned long samples_generation() const { return samples_gen_; }
  size_t position() const { return cur_; }                   // sample index the next block starts at
 private:
  SampleFeature(const SampleFeature&);
  SampleFeature& operator=(const SampleFeature&);
  std::vector<float> samples_;
  bool have_samples_;
  float norm_;
  unsigned shiftLen_;
  size_t cur_;
  bool pad_zeros_;
  int samplerate_, nChan_, format_;
  gsl_vector_float* copy_fsamples_;
  gsl_vector* copy_dsamples_;
  PinnedBuffer pcm16_;           // int16 shadow of samples_ (pcm16())
  int pcm16_state_;              // 0: not built for the current samples, 1: valid, -1: the samples are not 16-bit PCM
  unsigned long samples_gen_;
  void samples_changed_();       // waits for uploads that still read the int16 shadow before it may be rebuilt
};

// HammingFeature (reference feature/feature.h:492-507, feature/feature.cc:1177-1200): the float64 window times the source's
// block, stored as float32 -- that rounding is part of the reference.  Host arithmetic: it is the node boundary.
class HammingFeature : public VectorFloatFeatureStream {
 public:
  HammingFeature(const VectorFloatFeatureStreamPtr& samp, const String& nm = "Hamming");
  virtual ~HammingFeature() {}
  virtual const gsl_vector_float* next(int frame_no = -5);
  virtual void reset() { samp_->reset(); VectorFloatFeatureStream::reset(); }
  // engine hooks for a consumer that takes the blocks from the source in bulk (FFTFeature): the source node, and the state
  // transitions of n next() calls whose last block was last_block (vector_ = its windowed form, as after next())
  VectorFloatFeatureStreamPtr& source() { return samp_; }
  void advance_blocks(long n, const float* last_block);
 private:
  VectorFloatFeatureStreamPtr samp_;
  std::vector<double> window_;
};
typedef Inherit<HammingFeature, VectorFloatFeatureStreamPtr> HammingFeaturePtr;

// FFTFeature (reference feature/feature.h:518-546, feature/feature.cc:1205-1258, :29-43): the source's block zero-padded to
// fftLen, forward real transform, handed out as the full spectrum -- the half spectrum plus its conjugate mirror, bins 0 and
// fftLen/2 real -- widened from the device's complex64 (btk_tdoa_spectra; fftLen a power of two from 256 to 16384, block
// length <= fftLen: the library refuses the rest at the first next()).
// Over a HammingFeature over a SampleFeature, the window and the transform of up to block_frames frames are one launch and the
// frames are served one by one from a host copy; over any other source each next() uploads one frame (no window) and launches a
// one-frame block.  block_frames: constructor argument, 0 = BTK_TDOA_BLOCK_FRAMES or 64.
class FFTFeature : public VectorComplexFeatureStream {
 public:
  FFTFeature(const VectorFloatFeatureStreamPtr& samp, unsigned fftLen = 512, const String& nm = "FFT", long block_frames = 0);
  virtual ~FFTFeature() {}
  virtual const gsl_vector_complex* next(int frame_no = -5);
  virtual void reset();
  unsigned fftLen() const { return fftLen_; }
  unsigned windowLen() const { return windowLen_; }
  unsigned nBlocks() const { return 4; }
  unsigned subsamplerate() const { return 2; }
  unsigned subSampRate() { return subsamplerate(); }
  long block_frames() const { return block_frames_; }
  void set_block_frames(long n);
  // engine hooks for a consumer that batches over channels (btk20.pytdoa): whether this node stands over a HammingFeature over
  // a SampleFeature, and then up to nmax of the SampleFeature's un-windowed blocks back to back in dst (nmax * windowLen()
  // floats) with the state transitions of as many next() calls on every node of the chain; fewer than nmax: the stream ended
  bool has_sample_chain() const { return sample_ != NULL; }
  long pull_sample_blocks(float* dst, long nmax);
  // launches this node has made since it was built (tests)
  long launches() const { return launches_; }
  // engine hooks of the front-end nodes (SpectralPowerFeature and above): whether this node stands over a HammingFeature over
  // [a PreemphasisFeature over] [a StorageFeature over] a SampleFeature (blocks may overlap), then up to nmax of the
  // SampleFeature's blocks back to back in dst with the state transitions of as many next() calls on every node BELOW this
  // one, the pre-emphasis the kernel has to apply, and this node's own transition once the block's last half spectrum is known
  bool has_fe_chain() const { return fe_sample_ != NULL; }
  long pull_fe_blocks(float* dst, long nmax, int* preemph, double* mu, float* prior0);
  void fe_advance(long n, const float* last_half);
 private:
  void find_fe_chain_();
  HammingFeature* fe_hamming_;
  PreemphasisFeature* fe_preemph_;
  StorageFeature* fe_storage_;
  SampleFeature* fe_sample_;
  void fill_block_();
  void serve_(const float* half);
  VectorFloatFeatureStreamPtr samp_;
  HammingFeature* hamming_;      // samp_ when it is one over a SampleFeature, else NULL
  SampleFeature* sample_;        // its source
  unsigned fftLen_, windowLen_;
  long block_frames_, blk_n_, blk_pos_, launches_;
  PinnedBuffer h_in_, h_out_;
  DeviceBuffer d_in_, d_out_, d_energy_;
};
typedef Inherit<FFTFeature, VectorComplexFeatureStreamPtr> FFTFeaturePtr;

// ================================================================================================ the recogniser's front end
// PreemphasisFeature, SpectralPowerFeature, VTLNFeature, MelFeature, LogFeature, CepstralFeature, StorageFeature (reference
// feature/feature.h:436-455, :548-555, :640-672, :835-905, :961-978, :986-1003, :1196-1222; feature/feature.cc:1113-1144, :1291-1314,
// :1662-1850, :1892-2242, :2326-2428, :2905-2996) over btk_fe_process (csrc/fe_kernels.hip).
//
// PreemphasisFeature and StorageFeature are host nodes (node boundaries, like HammingFeature).  The nodes from the power
// spectrum up serve BLOCKS where their sources lead, through nodes of these classes, down to an FFTFeature over a
// HammingFeature over [a PreemphasisFeature over] [a StorageFeature over] a SampleFeature: the first next() of a block pulls
// up to block_frames sample blocks, launches btk_fe_process once from PCM up to the node's own stage (the sample blocks back to
// back, shift = D at the ABI, also where the SampleFeature's blocks overlap) and serves the frames from a pinned host copy;
// every node of the chain below makes the state transitions of as many next() calls (its vector is the block's last frame).
// Over any other source a node uploads the one frame the source hands out and enters the kernel at its own stage.
// Construction touches no device: tables are built on the host and uploaded with the first launch.
class PreemphasisFeature : public VectorFloatFeatureStream {
 public:
  PreemphasisFeature(const VectorFloatFeatureStreamPtr& samp, double mu = 0.95, const String& nm = "Preemphasis");
  virtual const gsl_vector_float* next(int frame_no = -5);
  virtual void reset() { samp_->reset(); VectorFloatFeatureStream::reset(); }
  void next_speaker() { prior_ = 0.0f; }
  void nextSpeaker() { next_speaker(); }
  // engine hooks: the source, mu, the sample before the next one, and the state transitions of n next() calls over n
  // blocks stored back to back
  VectorFloatFeatureStreamPtr& source() { return samp_; }
  double mu() const { return mu_; }
  float prior() const { return prior_; }
  const float* current_vector() const { return vector_->data; }
  void advance_blocks(long n, const float* blocks);
 private:
  VectorFloatFeatureStreamPtr samp_;
  float prior_;
  double mu_;
};
typedef Inherit<PreemphasisFeature, VectorFloatFeatureStreamPtr> PreemphasisFeaturePtr;

class StorageFeature : public VectorFloatFeatureStream {
 public:
  static const int MaxFrames = 100000;
  StorageFeature(const VectorFloatFeatureStreamPtr& src, const String& nm = "Storage");
  virtual ~StorageFeature();
  // a stored frame for 0 <= frame_no <= the last one, the source's next frame otherwise (feature.cc:2920-2934)
  virtual const gsl_vector_float* next(int frame_no = -5);
  virtual void reset() { src_->reset(); VectorFloatFeatureStream::reset(); }
  void write(const String& fileName, bool plainText = false) const;
  void read(const String& fileName);
  int evaluate();
  VectorFloatFeatureStreamPtr& source() { return src_; }
  void store_blocks(long n, const float* blocks);      // engine hook: n next() calls whose source blocks lie back to back
 private:
  gsl_vector_float* frame_(int i);
  VectorFloatFeatureStreamPtr src_;
  std::vector<gsl_vector_float*> frames_;              // allocated as they are filled
};
typedef Inherit<StorageFeature, VectorFloatFeatureStreamPtr> StorageFeaturePtr;

struct btk_fe_params;

// what the nodes from POWER up share: the wiring of a chain and the block service
class FeStageNode {
 public:
  virtual ~FeStageNode() {}
  int fe_stage() const { return stage_; }
  long launches() const { return launches_; }          // launches this node has made since it was built (tests)
  long block_frames() const { return block_frames_; }
  void set_block_frames(long n);
 protected:
  FeStageNode(int stage);
  void fe_wire_(FeStageNode* below, FFTFeature* fft);  // the source, where it is a node of these classes or an FFTFeature
  const float* fe_next_();                             // this node's next frame, float32 [fe_dim()]
  void fe_reset_() { blk_n_ = blk_pos_ = 0; }
  void fe_tables_changed_() { tables_dirty_ = true; }
  virtual unsigned fe_dim() const = 0;
  virtual void fe_params(btk_fe_params& q) = 0;        // the node's own tables and constants (device copies made here)
  virtual void fe_advance(long n, const float* last) = 0;
  // one frame of a source that is no chain: its values as float32 (complex64 pairs for a spectrum), the stage they are of
  virtual void fe_pull_one(std::vector<float>& in, int& in_stage, int& in_dim, int& L) = 0;
  // a table as the kernel reads it
  void fe_upload_(DeviceBuffer& d, const void* h, size_t bytes);
  bool tables_dirty_;
 public:
  FeStageNode* fe_below() const { return below_; }
 private:
  FFTFeature* root_() const;
  void fill_chain_(FFTFeature* root);
  void fill_single_();
  int stage_;
  FeStageNode* below_;
  FFTFeature* fft_;
  long block_frames_, blk_n_, blk_pos_, launches_;
  PinnedBuffer h_in_, h_out_, h_last_;
  DeviceBuffer d_in_, d_out_, d_prior_;
};

class SpectralPowerFeature : public VectorFeatureStream, public FeStageNode {
 public:
  SpectralPowerFeature(const VectorComplexFeatureStreamPtr& fft, unsigned powN = 0, const String& nm = "Power");
  virtual const gsl_vector* next(int frame_no = -5);
  virtual void reset() { fft_->reset(); VectorFeatureStream::reset(); fe_reset_(); }
 protected:
  virtual unsigned fe_dim() const { return size(); }
  virtual void fe_params(btk_fe_params& q);
  virtual void fe_advance(long n, const float* last);
  virtual void fe_pull_one(std::vector<float>& in, int& in_stage, int& in_dim, int& L);
 private:
  VectorComplexFeatureStreamPtr fft_;
};
typedef Inherit<SpectralPowerFeature, VectorFeatureStreamPtr> SpectralPowerFeaturePtr;

// SpectralPowerFloatFeature (reference feature/feature.h:557-571, feature/feature.cc:1263-1286): |X_k|^2 as float32 -- re^2 + im^2
// summed in float64, rounded once -- for powN = fft->size() or fft->size() / 2 + 1 bins; the reference's only float stream of
// power spectra and so the source of the band-power VAD metrics (sad/sad.h).  Host arithmetic: it is a node boundary.
class SpectralPowerFloatFeature : public VectorFloatFeatureStream {
 public:
  SpectralPowerFloatFeature(const VectorComplexFeatureStreamPtr& fft, unsigned powN = 0, const String& nm = "Power");   // the name feature.i gives it
  virtual const gsl_vector_float* next(int frame_no = -5);
  virtual void reset() { fft_->reset(); VectorFloatFeatureStream::reset(); }
 private:
  VectorComplexFeatureStreamPtr fft_;
};
typedef Inherit<SpectralPowerFloatFeature, VectorFloatFeatureStreamPtr> SpectralPowerFloatFeaturePtr;

class VTLNFeature : public VectorFeatureStream, public FeStageNode {
 public:
  VTLNFeature(const VectorFeatureStreamPtr& pow, unsigned coeffN = 0, double ratio = 1.0, double edge = 1.0, int version = 1,
              const String& nm = "VTLN");
  virtual const gsl_vector* next(int frame_no = -5);
  virtual void reset() { pow_->reset(); VectorFeatureStream::reset(); fe_reset_(); }
  void warp(double w);                                 // frames served after the call use the new ratio
  void matrix(gsl_matrix* mat) const;                  // the warp as a size() x source_size() operator on the power vector
  unsigned source_size() const { return pow_->size(); }
 protected:
  virtual unsigned fe_dim() const { return size(); }
  virtual void fe_params(btk_fe_params& q);
  virtual void fe_advance(long n, const float* last);
  virtual void fe_pull_one(std::vector<float>& in, int& in_stage, int& in_dim, int& L);
 private:
  void build_();
  VectorFeatureStreamPtr pow_;
  double ratio_, edge_;
  int version_;
  std::vector<int> rows_;                              // [size()][3]: offset, count, start
  std::vector<double> w_;
  DeviceBuffer d_rows_, d_w_;
};
typedef Inherit<VTLNFeature, VectorFeatureStreamPtr> VTLNFeaturePtr;

class MelFeature : public VectorFeatureStream, public FeStageNode {
 public:
  MelFeature(const VectorFeatureStreamPtr& mag, int powN = 0, float rate = 16000.0, float low = 0.0, float up = 0.0,
             unsigned filterN = 30, unsigned version = 1, const String& nm = "MelFFT");
  virtual const gsl_vector* next(int frame_no = -5);
  virtual void reset() { mag_->reset(); VectorFeatureStream::reset(); fe_reset_(); }
  void read(const String& fileName);                   // band matrices from a file are not carried over: jio_error
  void matrix(gsl_matrix* mat) const;                  // filterN x powN
  unsigned powN() const { return powN_; }
 protected:
  virtual unsigned fe_dim() const { return size(); }
  virtual void fe_params(btk_fe_params& q);
  virtual void fe_advance(long n, const float* last);
  virtual void fe_pull_one(std::vector<float>& in, int& in_stage, int& in_dim, int& L);
 private:
  VectorFeatureStreamPtr mag_;
  unsigned powN_;
  std::vector<int> rows_;
  std::vector<float> w_;
  DeviceBuffer d_rows_, d_w_;
};
typedef Inherit<MelFeature, VectorFeatureStreamPtr> MelFeaturePtr;

class LogFeature : public VectorFloatFeatureStream, public FeStageNode {
 public:
  LogFeature(const VectorFeatureStreamPtr& mel, double m = 1.0, double a = 1.0, bool sphinxFlooring = false,
             const String& nm = "LogMel");
  virtual const gsl_vector_float* next(int frame_no = -5);
  virtual void reset() { mel_->reset(); VectorFloatFeatureStream::reset(); fe_reset_(); }
 protected:
  virtual unsigned fe_dim() const { return size(); }
  virtual void fe_params(btk_fe_params& q);
  virtual void fe_advance(long n, const float* last);
  virtual void fe_pull_one(std::vector<float>& in, int& in_stage, int& in_dim, int& L);
 private:
  VectorFeatureStreamPtr mel_;
  double m_, a_;
  bool floor_;
};
typedef Inherit<LogFeature, VectorFloatFeatureStreamPtr> LogFeaturePtr;

class CepstralFeature : public VectorFloatFeatureStream, public FeStageNode {
 public:
  CepstralFeature(const VectorFloatFeatureStreamPtr& mel, unsigned ncep = 13, int type = 1, const String& nm = "Cepstral");
  virtual const gsl_vector_float* next(int frame_no = -5);
  virtual void reset() { mel_->reset(); VectorFloatFeatureStream::reset(); fe_reset_(); }
  gsl_matrix* matrix() const;                          // a new ncep x mel->size() matrix (the caller frees it)
 protected:
  virtual unsigned fe_dim() const { return size(); }
  virtual void fe_params(btk_fe_params& q);
  virtual void fe_advance(long n, const float* last);
  virtual void fe_pull_one(std::vector<float>& in, int& in_stage, int& in_dim, int& L);
 private:
  VectorFloatFeatureStreamPtr mel_;
  std::vector<float> cos_;
  DeviceBuffer d_cos_;
};
typedef Inherit<CepstralFeature, VectorFloatFeatureStreamPtr> CepstralFeaturePtr;
