// obj_nodes.cc -- SNR and ItakuraSaitoMeasurePS of objective_measure/objective_measure.h over btk_obj_snr and
// btk_obj_is_distance (csrc/obj_kernels.hip): the files are read on the host, the two signals go to the device once, the sums
// and the distance come back as a few float64 values.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "objective_measure/objective_measure.h"
#include "feature/feature.h"
#include "node_runtime.h"

namespace {

using btknode::check_abi;
using btknode::d2h;
using btknode::h2d;

// rows of a pair on the device start at multiples of four floats
long row_stride(long n) { return (std::max(n, 1L) + 3) & ~3L; }

// channel chX of a whole 16-bit PCM WAV file at int16 scale; channels and sample rate as the header states them
struct WavChannel {
  std::vector<float> x;
  int channels, rate;
};
void open_wav(const String& fn, SampleFeature& f)
{
  // channel 1 is in every file: the channel the caller asks for is checked against both files first, as the reference does
  f.read(fn, 0, 16000, 1, 1, 0, -1, -1, 0.0f);
}
void read_channel(const String& fn, int chX, WavChannel* w)
{
  SampleFeature f("", 1, 1, false);
  f.read(fn, 0, 16000, chX, 1, 0, -1, -1, 0.0f);
  const gsl_vector_float* v = f.data();
  w->x.assign(v->data, v->data + v->size);
  w->channels = f.getChanN();
  w->rate = f.getSampleRate();
}
void check_channel(int chX, int ch1, int ch2)
{
  if (chX > ch1 || chX > ch2 || chX < 1) {
    if (chX == 0) throw jconsistency_error("Multi-channel read is not yet supported.");
    throw jconsistency_error("Selected channel out of range of available channels. %d", chX);
  }
}

}  // namespace

// ================================================================================ SNR
float SNR::run_(const float* x1, long n1, const float* x2, long n2, int option)
{
  if (n1 < 1 || n2 < 1) throw jdimension_error("SNR: a signal has no samples (%ld, %ld)", n1, n2);
  const long s1 = row_stride(n1), s2 = row_stride(n2);
  float* dx = static_cast<float*>(d_x_.ensure(sizeof(float) * (size_t)(s1 + s2)));
  h2d(dx, x1, sizeof(float) * (size_t)n1);
  h2d(dx + s1, x2, sizeof(float) * (size_t)n2);
  void* ws = d_ws_.ensure((size_t)btk_obj_snr_workspace_bytes(1, std::max(n1, n2)));
  double* ds = static_cast<double*>(d_stats_.ensure(sizeof(double) * 6));
  check_abi(btk_obj_snr(dx, s1, dx + s1, s2, 1, &n1, &n2, option, ds, 0, NULL, 0, ws, btk_node_stream()));
  d2h(stats_, ds, sizeof(double) * 6);
  return btk_obj_snr_db(stats_[4], stats_[5]);
}

float SNR::getSNR(const String& fn1, const String& fn2, int normalizationOption, int chX, int samplerate, int cfrom, int to)
{
  (void)samplerate;                                                  // libsndfile takes the rate from a WAV header, as here
  {
    SampleFeature h1("", 1, 1, false), h2("", 1, 1, false);
    open_wav(fn1, h1);
    open_wav(fn2, h2);
    check_channel(chX, h1.getChanN(), h2.getChanN());
    if (h1.getSampleRate() != h2.getSampleRate())
      throw jio_error("Sampling rates must be the same but %d!=%d\n", h1.getSampleRate(), h2.getSampleRate());
  }
  WavChannel w1, w2;
  read_channel(fn1, chX, &w1);
  read_channel(fn2, chX, &w2);
  const long f1 = (long)w1.x.size(), f2 = (long)w2.x.size();
  long nsamples1, nsamples2;
  if (cfrom < 0) cfrom = 0;
  if (to < 0 || to >= f1 || to >= f2) { nsamples1 = f1 - cfrom; nsamples2 = f2 - cfrom; }      // objective_measure.cc:233-242
  else nsamples1 = nsamples2 = (long)to - cfrom + 1;
  if (cfrom > f1 || cfrom > f2) throw jio_error("Cannot load samples from %d to %d.", cfrom, to);
  if (nsamples1 < 1 || nsamples2 < 1) throw jdimension_error("Cannot load samples from %d to %d.", cfrom, to);
  // sf_readf_float: normalised samples
  for (float& v : w1.x) v *= 1.0f / 32768.0f;
  for (float& v : w2.x) v *= 1.0f / 32768.0f;
  return run_(w1.x.data() + cfrom, nsamples1, w2.x.data() + cfrom, nsamples2, normalizationOption);
}

float SNR::getSNR2(const gsl_vector_float* original, const gsl_vector_float* enhanced, int normalizationOption)
{
  if (!original || !enhanced) throw jparameter_error("SNR::getSNR2: null vector");
  if (original->stride != 1 || enhanced->stride != 1) throw jdimension_error("SNR::getSNR2: the vectors must be contiguous");
  return run_(original->data, (long)original->size, enhanced->data, (long)enhanced->size, normalizationOption);
}

// ================================================================================ ItakuraSaitoMeasurePS
ItakuraSaitoMeasurePS::ItakuraSaitoMeasurePS(unsigned fftLen, unsigned r, unsigned windowType, const String&)
    : M_(fftLen), r_(r), window_type_(windowType), D_(r < 32 ? fftLen >> r : 0), plan_(NULL), frames_(0), dist_(0.0)
{
}

ItakuraSaitoMeasurePS::~ItakuraSaitoMeasurePS()
{
  if (plan_) btk_stft_destroy(plan_);
}

float ItakuraSaitoMeasurePS::getDistance(const String& fn1, const String& fn2, int chX, int samplerate, int bframe, int eframe)
{
  (void)samplerate;
  if (!plan_) check_abi(btk_stft_create(&plan_, (int)M_, (int)r_, (int)window_type_));
  WavChannel w1, w2;
  read_channel(fn1, chX, &w1);                                       // SampleFeature::read's own errors, as in the reference
  read_channel(fn2, chX, &w2);
  if (bframe < 0) bframe = 0;                                        // frameX >= bframe holds for every frame then
  // SampleFeature(D, D, false) hands out the blocks that end before the last sample
  const long D = (long)D_;
  const long n1 = w1.x.empty() ? 0 : ((long)w1.x.size() - 1) / D * D, n2 = w2.x.empty() ? 0 : ((long)w2.x.size() - 1) / D * D;
  const long s1 = row_stride(n1), s2 = row_stride(n2);
  float* dx = static_cast<float*>(d_x_.ensure(sizeof(float) * (size_t)(s1 + s2)));
  if (n1) h2d(dx, w1.x.data(), sizeof(float) * (size_t)n1);
  if (n2) h2d(dx + s1, w2.x.data(), sizeof(float) * (size_t)n2);
  const long F = btk_stft_num_frames(plan_, std::min(n1, n2));
  // dist, count, then the rows
  double* out = static_cast<double*>(d_out_.ensure(sizeof(double) * (size_t)(2 + F)));
  check_abi(btk_obj_is_distance(plan_, dx, s1, dx + s1, s2, 1, &n1, &n2, bframe, eframe, out, reinterpret_cast<long long*>(out + 1),
                                out + 2, F, btk_node_stream()));
  double h[2];
  d2h(h, out, sizeof(h));
  dist_ = h[0];
  long long cnt;
  memcpy(&cnt, &h[1], sizeof(cnt));
  frames_ = (long)cnt;
  return (float)dist_;
}
