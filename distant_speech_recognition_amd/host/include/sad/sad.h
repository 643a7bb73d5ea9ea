// sad/sad.h -- the energy family of the reference's voice activity detection (reference sad/sad.h:66-112, :187-219, :225-262,
// :268-386, :540-575, :665-790; sad/sad.cc:126-180, :472-588, :593-836, :996-1063, :1712-1951) over the btk_vad_* calls of
// include/btkhip.h (csrc/vad_kernels.hip): VADMetric, EnergyVADMetric, PowerSpectrumVADMetric, NormalizedEnergyMetric,
// TSPSVADMetric, VAD, SimpleEnergyVAD, HangoverVADFeature, HangoverMIVADFeature, HangoverMultiStageVADFeature.
//
// Block service.  A metric evaluates every frame of its sources once, from frame 0, in order, so a node draws up to
// block_frames() frames from its sources through next() into pinned memory, runs the block through the kernels once and carries
// the state (window, counters, recursion value, hangover machine) on the device into the next block: a block cut anywhere gives
// the bits of one launch.  A metric on its own serves next(frame_no) from the downloaded rows of its block.  Under a hangover
// node the node leads: for every frame it draws its own source's frame, then lets every metric draw that frame from its
// sources (stage_frame; a source node that the hangover node and a metric share hands out its cached frame), and at the end of
// the block the metrics' value rows stay on the device for the hangover kernel (flush_staged).  The frames a hangover node
// serves never leave the host, so the node copies them from its own staging block; btk_vad_gather is for sources whose blocks
// lie on the device (engine.vad_gather).
// Not carried over: the log-file functions of VADMetric (_LOG_SAD_) and the classes DESIGN section 7 lists.
#pragma once
#include <deque>
#include <utility>
#include <vector>
#include "stream/stream.h"
#include "common/devmem.h"

long btk_vad_default_block_frames();       // BTK_VAD_BLOCK_FRAMES, 256 when unset

class VADMetric : public Countable {
 public:
  virtual ~VADMetric() {}
  // the value of frame frame_no (the next one for a negative number; the current one again for the current number; any other
  // number is a jindex_error); jiterator_error at the end of a source
  virtual double next(int frame_no = -5);
  virtual void reset() = 0;
  virtual void next_speaker() = 0;
  double score() const { return cur_score_; }
  void nextSpeaker() { next_speaker(); }
  int frame_no() const { return frame_no_; }
  long block_frames() const { return block_frames_; }
  void set_block_frames(long n) { block_frames_ = n > 0 ? n : btk_vad_default_block_frames(); }
  long launches() const { return launches_; }            // blocks this metric has run since it was built (tests)
  // engine hooks of the hangover nodes: begin a block of at most cap frames; draw frame frame_no of every source into the
  // staging block (jiterator_error: a source has ended, nothing was staged); run the first n staged frames and hand back the
  // value row on the device (float64 [n], written on btk_node_stream()) -- the metric then stands behind frame n - 1 of the block
  void begin_block(long cap);
  void stage_frame(int frame_no);
  const double* flush_staged(long n);
 protected:
  VADMetric();
  void rewind_();                                        // frame numbers and block back to the start (reset(), next_speaker())
  virtual void reserve_(long cap) = 0;                   // staging for cap frames
  virtual void pull_(int frame_no, long slot) = 0;       // the sources' frame frame_no into slot `slot`
  virtual void launch_(long n, double* d_value, double* d_score) = 0;   // the block's kernels on btk_node_stream()
  virtual void downloaded_(long n) {}                    // the rows are on the host (after the stream was waited for)
  virtual void served_(long pos) {}                      // frame `pos` of the block is the current one
  double cur_score_, cur_value_;
  long cap_;
 private:
  void run_(long n);
  int frame_no_;
  long block_frames_, blk_n_, blk_pos_, staged_, launches_;
  bool src_end_;                                         // a source ended inside the block served last
  PinnedBuffer h_rows_;                                  // [2][cap]: values, scores
  DeviceBuffer d_rows_;
};
typedef refcountable_ptr<VADMetric> VADMetricPtr;

// EnergyVADMetric (sad.cc:472-588): 1.0 where the frame's energy lies above the entry medianX = unsigned(threshold energiesN)
// of the sorted window of the last energiesN energies, else 0.0; score() is the energy.  threshold >= 1 (or < 0), where the
// reference reads past its array, and energiesN outside 1 .. 1024 are jdimension_errors.
class EnergyVADMetric : public VADMetric {
 public:
  EnergyVADMetric(const VectorFloatFeatureStreamPtr& source, double initialEnergy = 5.0e+07, double threshold = 0.5, unsigned headN = 4,
                  unsigned tailN = 10, unsigned energiesN = 200, const String& nm = "Energy VAD Metric");
  virtual void reset();                                  // the counters go, the window stays (:493-497)
  virtual void next_speaker();                           // the window is initialEnergy again (:499-506)
  // the division by energiesN included (:544-553); of the window as the frames EVALUATED so far left it (the block drawn last)
  double energy_percentile(double percentile = 50.0);
  double energyPercentile(double percentile = 50.0) { return energy_percentile(percentile); }
 protected:
  virtual void reserve_(long cap);
  virtual void pull_(int frame_no, long slot);
  virtual void launch_(long n, double* d_value, double* d_score);
 private:
  void sync_state_();
  VectorFloatFeatureStreamPtr source_;
  double initial_energy_;
  unsigned headN_, tailN_, energiesN_;
  int medianX_;
  int state_todo_;                                       // 0: the device state stands, 1: clear the counters, 2: write all of it
  PinnedBuffer h_in_, h_state_;
  DeviceBuffer d_in_, d_state_;
};
typedef Inherit<EnergyVADMetric, VADMetricPtr> EnergyVADMetricPtr;

// PowerSpectrumVADMetric (:667-760), NormalizedEnergyMetric (:764-836), TSPSVADMetric (:996-1063): band powers of C channels of
// power spectra (channel 0 the target's), +1.0 / -1.0.  score() is the power ratio, the normalised-energy ratio and the TSPS
// value (the reference never sets it for the first and the last).  The channels must have one size > highX.
class PowerSpectrumVADMetric : public VADMetric {
 public:
  PowerSpectrumVADMetric(unsigned fftLen, double sampleRate = 16000.0, double lowCutoff = -1.0, double highCutoff = -1.0,
                         const String& nm = "Power Spectrum VAD Metric");
  virtual ~PowerSpectrumVADMetric();
  void set_channel(const VectorFloatFeatureStreamPtr& chan);
  void setChannel(const VectorFloatFeatureStreamPtr& chan) { set_channel(chan); }
  virtual void reset();                                  // resets the channels (:741-745)
  virtual void next_speaker();                           // likewise (:747-751)
  const gsl_vector* get_metrics();                       // the current frame's band power per channel; NULL before a frame
  const gsl_vector* getMetrics() { return get_metrics(); }
  void set_E0(double E0) { E0_ = E0; }                   // holds from the next block on
  void setE0(double E0) { set_E0(E0); }
  void clear_channel();
  void clearChannel() { clear_channel(); }
  unsigned lowX() const { return (unsigned)lowX_; }
  unsigned highX() const { return (unsigned)highX_; }
  unsigned binN() const { return (unsigned)binN_; }
 protected:
  PowerSpectrumVADMetric(int kind, double E0, unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff);
  virtual void reserve_(long cap);
  virtual void pull_(int frame_no, long slot);
  virtual void launch_(long n, double* d_value, double* d_score);
  virtual void downloaded_(long n);
  virtual void served_(long pos);
 private:
  void init_(unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff);
  std::vector<VectorFloatFeatureStreamPtr> channels_;
  int kind_, fftLen_, lowX_, highX_, binN_;
  double E0_;
  unsigned powN_;
  gsl_vector* powerList_;
  long pos_;
  PinnedBuffer h_in_, h_P_;
  DeviceBuffer d_in_, d_P_;
};
typedef Inherit<PowerSpectrumVADMetric, VADMetricPtr> PowerSpectrumVADMetricPtr;

class NormalizedEnergyMetric : public PowerSpectrumVADMetric {
 public:
  NormalizedEnergyMetric(unsigned fftLen, double sampleRate = 16000.0, double lowCutoff = -1.0, double highCutoff = -1.0,
                         const String& nm = "NormalizedEnergyMetric");
};
typedef Inherit<NormalizedEnergyMetric, PowerSpectrumVADMetricPtr> NormalizedEnergyMetricPtr;

class TSPSVADMetric : public PowerSpectrumVADMetric {
 public:
  TSPSVADMetric(unsigned fftLen, double sampleRate = 16000.0, double lowCutoff = -1.0, double highCutoff = -1.0,
                const String& nm = "TSPS VAD Metric");
};
typedef Inherit<TSPSVADMetric, PowerSpectrumVADMetricPtr> TSPSVADMetricPtr;

// VAD, SimpleEnergyVAD (sad.cc:126-180): s <- gamma s + (1 - gamma) E over the energies of the complex frames, is_speech =
// E / s > threshold.  The frames are drawn in blocks (as complex64: exact for the banks' frames, which are widened complex64),
// frame() is the node's own copy of the current one.  frame_no_ starts at -1 (the reference leaves it uninitialised).
class VAD : public Countable {
 public:
  VAD(const VectorComplexFeatureStreamPtr& samp);
  virtual ~VAD();
  virtual bool next(int frame_no = -5) = 0;
  virtual void reset() { frame_no_ = frame_reset_no_; }
  const gsl_vector_complex* frame() const { return frame_; }
  virtual void next_speaker() = 0;
  void nextSpeaker() { next_speaker(); }
  int frame_no() const { return frame_no_; }
 protected:
  void increment_() { frame_no_++; }
  VectorComplexFeatureStreamPtr samp_;
  const int frame_reset_no_;
  const unsigned fftLen_;
  bool is_speech_;
  int frame_no_;
  gsl_vector_complex* frame_;
};
typedef refcountable_ptr<VAD> VADPtr;

class SimpleEnergyVAD : public VAD {
 public:
  SimpleEnergyVAD(const VectorComplexFeatureStreamPtr& samp, double threshold, double gamma = 0.995);
  virtual bool next(int frame_no = -5);
  virtual void reset();                                  // the source and the frame numbers; the recursion value stays (:177-180)
  virtual void next_speaker();                           // the recursion value is 0 again (:149-152)
  double spectral_energy() const { return cur_s_; }      // the recursion value after the current frame
  long block_frames() const { return block_frames_; }
  void set_block_frames(long n) { block_frames_ = n > 0 ? n : btk_vad_default_block_frames(); }
  long launches() const { return launches_; }
 private:
  void fill_();
  const double threshold_, gamma_;
  double cur_s_;
  bool state_from_host_, src_end_;                       // the device's recursion value is to be written from cur_s_ first
  long block_frames_, blk_n_, blk_pos_, launches_, blk_cap_;
  PinnedBuffer h_in_, h_out_;
  DeviceBuffer d_in_, d_energy_, d_out_, d_state_;
};
typedef Inherit<SimpleEnergyVAD, VADPtr> SimpleEnergyVADPtr;

// HangoverVADFeature (sad.cc:1712-1843): with q the first source frame that ends headN consecutive detections, the node hands
// out the source's frames from q - headN + 1 up to, not including, the frame on which the tailN-th consecutive miss falls (or
// up to the source's end), then raises jiterator_error.  prefixN() is the first frame handed out (0 before it is known).
// The source is read ahead to the end of the block in which the segment ends.  headN == 0 is a jdimension_error.
class HangoverVADFeature : public VectorFloatFeatureStream {
 public:
  HangoverVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& metric, double threshold = 0.5,
                     unsigned headN = 4, unsigned tailN = 10, const String& nm = "Hangover VAD Feature");
  virtual ~HangoverVADFeature() {}
  virtual const gsl_vector_float* next(int frame_no = -5);
  virtual void reset();
  virtual void next_speaker();
  void nextSpeaker() { next_speaker(); }
  int prefixN() const { return start_ >= 0 ? (int)start_ : 0; }
  long block_frames() const { return block_frames_; }
  void set_block_frames(long n) { block_frames_ = n > 0 ? n : btk_vad_default_block_frames(); }
  long launches() const { return launches_; }
 protected:
  HangoverVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& metric, double threshold, unsigned headN,
                     unsigned tailN, const String& nm, int rule);
  typedef std::pair<VADMetricPtr, double> MetricPair_;
  std::vector<MetricPair_> metricList_;
  int decision_metric_;
 private:
  void init_(const VADMetricPtr& metric, double threshold);
  void rewind_();
  bool fill_();                                          // one more block; false: nothing more will come
  VectorFloatFeatureStreamPtr source_;
  const unsigned headN_, tailN_;
  const int rule_;
  long block_frames_, launches_;
  int end_code_;                                         // decision_metric() of the frame that ended the segment
  long seen_, start_, end_;                              // source frames run through the machine; the segment as far as known
  bool src_end_, state_fresh_;
  std::deque<std::vector<float> > carry_;                // the last headN - 1 source frames before the onset is known
  std::deque<std::pair<std::vector<float>, int> > queue_;   // frames to hand out with decision_metric() after each
  PinnedBuffer h_in_, h_out_;
  DeviceBuffer d_state_, d_decision_;
};
typedef Inherit<HangoverVADFeature, VectorFloatFeatureStreamPtr> HangoverVADFeaturePtr;

// HangoverMIVADFeature (:1847-1885): three metrics, codes -1, 2, 3, -3
class HangoverMIVADFeature : public HangoverVADFeature {
 public:
  HangoverMIVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& energyMetric,
                       const VADMetricPtr& mutualInformationMetric, const VADMetricPtr& powerMetric, double energyThreshold = 0.5,
                       double mutualInformationThreshold = 0.5, double powerThreshold = 0.5, unsigned headN = 4, unsigned tailN = 10,
                       const String& nm = "Hangover MIVAD Feature");
  int decision_metric() const { return decision_metric_; }
  int decisionMetric() const { return decision_metric_; }
};
typedef Inherit<HangoverMIVADFeature, HangoverVADFeaturePtr> HangoverMIVADFeaturePtr;

// HangoverMultiStageVADFeature (:1889-1951): never a detection with fewer than three metrics; stage 0 below 0.5 vetoes the
// frame (code -1), otherwise the first stage m >= 1 above 0.5 wins (code m + 1), else the code is -(number of metrics).
// Every metric is evaluated once per frame (the reference calls later stages twice on one frame number); at most 8 metrics.
class HangoverMultiStageVADFeature : public HangoverVADFeature {
 public:
  HangoverMultiStageVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& energyMetric,
                               double energyThreshold = 0.5, unsigned headN = 4, unsigned tailN = 10,
                               const String& nm = "HangoverMultiStageVADFeature");
  int decision_metric() const { return decision_metric_; }
  int decisionMetric() const { return decision_metric_; }
  void set_metric(const VADMetricPtr& metricPtr, double threshold);
  void setMetric(const VADMetricPtr& metricPtr, double threshold) { set_metric(metricPtr, threshold); }
};
typedef Inherit<HangoverMultiStageVADFeature, HangoverVADFeaturePtr> HangoverMultiStageVADFeaturePtr;
