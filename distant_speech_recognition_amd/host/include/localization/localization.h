// localization/localization.h -- SearchGridBuilder, SGB4LinearArray, MCCLocalizer and MCCCalculator (reference
// localization/mcc_localizer.h:36-78, :153-282; mcc_localizer.cc) over btk_mcc_cost / btk_mcc_select / btk_mcc_matrices of
// include/btkhip.h (csrc/mcc_kernels.hip).
//
// The reference scores one grid point at a time on the host: per block and candidate one rank-1 update per sample and an
// eigen-decomposition.  Here a localiser pulls its channels a block of frames ahead (set_block_frames / BTK_MCC_BLOCK_FRAMES,
// default 64; 0: until the sources end), uploads the frames once, scores every (frame, grid point) in one launch, selects the
// N-best list on the device, fetches R of the winners and of the last grid point, and serves frame by frame.
//   * The reference fills its SampleHolder from the CURRENT block before it sums (mcc_localizer.cc:336), so the "previous block"
//     is the block's own tail and no state crosses a frame: frames are independent, which is what lets them be batched.
//   * The grid is the builder's own walk: reset(), then getSearchPosition() / getTimeDelays() until nextSearchGrid() is false,
//     through the virtual functions, taken again for every batch.  After next() the builder stands where that walk ends.
//   * getEigenValues(): a cyclic Jacobi on the host over the winner's downloaded R, float64, ascending (GSL's gsl_eigen_symm
//     leaves the order unspecified).  getR(): R of the last grid point (the reference's _R after search()), both triangles.
//   * A pivot or variance that is not > 0 gives cost 0.0; |tau| > D, where the reference reads outside its
//     buffers, is a jdimension_error; a frame shorter than 2 D is the reference's j_error "Data samples are insufficient".
//   * SGB4LinearArray::setPositionsOfMicrophones copies microphone 0 and measures from it (the reference's loop starts at 1 and
//     compares against an uninitialised pos0).  The near-field walk ("need to be implemented" there) is a j_error here.
// Left out: RMCCLocalizer (its next() is empty), SGB4CircularArray (its far-field walk does not end).
#pragma once
#include <vector>

#include "stream/stream.h"
#include "common/devmem.h"
#include "btkhip.h"

class SearchGridBuilder : public Countable {
 public:
  SearchGridBuilder(int nChan, bool isFarField, unsigned int samplingFreq = 16000);
  virtual ~SearchGridBuilder();
  const gsl_vector* getSearchPosition() { return hypopos_; }
  float maxTimeDelay() { return max_time_delay_; }
  size_t chanN() { return mpos_->size1; }
  unsigned int samplingFrequency() { return sampling_freq_; }
  virtual void reset();
  virtual const gsl_vector* getTimeDelays() { return NULL; }
  virtual bool nextSearchGrid() { return false; }
 protected:
  const bool is_far_field_;
  unsigned int sampling_freq_;
  float max_time_delay_;
  gsl_matrix* mpos_;
  gsl_vector* hypopos_;
  gsl_vector* delays_;
  float const_v_;
};
typedef refcountable_ptr<SearchGridBuilder> SearchGridBuilderPtr;

class SGB4LinearArray : public SearchGridBuilder {
 public:
  SGB4LinearArray(int nChan, bool isFarField, unsigned int samplingFreq = 16000);
  void setDistanceBtwMicrophones(float distance);
  void setPositionsOfMicrophones(const gsl_matrix* mpos);
  void reset() override;
  const gsl_vector* getTimeDelays() override;
  bool nextSearchGrid() override;
 private:
  void walk_(const double* positions, float distance);
  // the far-field walk of btk_mcc_linear_grid, taken when the geometry is set; nextSearchGrid() steps through it
  std::vector<double> azimuths_, table_;
  size_t at_;
};
typedef Inherit<SGB4LinearArray, SearchGridBuilderPtr> SGB4LinearArrayPtr;

class MCCLocalizer : public VectorFeatureStream {
 public:
  MCCLocalizer(SearchGridBuilderPtr& sgbPtr, size_t maxSource = 1, const String& nm = "MCCSourceLocalizer");
  ~MCCLocalizer();
  const gsl_vector* next(int frame_no = -5) override;
  void reset() override;
  void setChannel(VectorFloatFeatureStreamPtr& chan);
  int getDelayedSample(int chanX) { return getNthBestDelayedSample(0, chanX); }
  double getMaxMCCC() { return getNthBestMCCC(0); }
  const gsl_vector* getPosition() { return getNthBestPosition(0); }
  int getNthBestDelayedSample(int nth, int chanX);
  double getNthBestMCCC(int nth);
  const gsl_vector* getNthBestPosition(int nth);
  const gsl_vector* getEigenValues();
  gsl_matrix* getR() { return R_; }
  // frames pulled ahead per launch (0: until the sources end); launches so far (tests)
  void set_block_frames(long n) { block_frames_ = n < 0 ? 0 : n; }
  long block_frames() const { return block_frames_; }
  long launches() const { return launches_; }
 protected:
  struct Candidate {
    double cost;
    std::vector<int> tau;
    gsl_vector* position;
  };
  // pulls up to block_frames_ frames of every channel into x_ [N][F L] and uploads them; false at the end of the sources
  bool pull_block_();
  void check_frame_length_(size_t D) const;
  virtual void launch_();                              // scores the block on the device and downloads what serve_ reads
  virtual void serve_(long f);                         // fills vector_ and the candidates from frame f of the block
  void jacobi_(const double* R);
  std::vector<VectorFloatFeatureStreamPtr> channels_;
  SearchGridBuilderPtr sgb_;
  size_t max_source_;
  long block_frames_, launches_;
  long F_, served_;                                    // frames in the block on the device, frames of it handed out
  bool sources_ended_;
  size_t L_;
  std::vector<float> x_;
  std::vector<int> tau_;                               // [G][N] of the walk taken for the block
  std::vector<double> grid_pos_;                       // [G][3]
  double end_pos_[3];                                  // where the walk ended
  std::vector<double> nb_cost_, Rh_;                   // [F][nbest], [F][nbest + 1][N][N]
  std::vector<int> nb_idx_;
  std::vector<Candidate> cand_;
  gsl_matrix* R_;
  gsl_vector* eig_;
  bool eig_fresh_;
  std::vector<double> Rbest_;
  DeviceBuffer d_x_, d_tau_, d_cost_, d_flag_, d_nbc_, d_nbi_, d_pairs_, d_R_;
};
typedef Inherit<MCCLocalizer, VectorFeatureStreamPtr> MCCLocalizerPtr;

class MCCCalculator : public MCCLocalizer {
 public:
  MCCCalculator(SearchGridBuilderPtr& sgbPtr, bool normalizeVariance = true, const String& nm = "MCCCalculator");
  // takes effect on the very next frame: frames pulled ahead but not yet served are scored again from the block on the device
  void setTimeDelays(gsl_vector* delays);
  double getMCCC();
  double getCostV() { return gsl_vector_get(vector_, 0); }
  const gsl_vector* next(int frame_no = -5) override;
  bool normalizeVariance() const { return normalize_; }
  void setNormalizeVariance(bool v) { normalize_ = v; stale_ = true; }
 protected:
  void launch_() override;
  void serve_(long f) override;
 private:
  std::vector<double> delays_;
  bool have_delays_, normalize_, stale_;
  std::vector<double> cost_h_;
  std::vector<unsigned char> flag_h_;
};
typedef Inherit<MCCCalculator, MCCLocalizerPtr> MCCCalculatorPtr;
