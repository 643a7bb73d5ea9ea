// fft_long_host.hip -- the tables behind rfft_long.h, one copy for every module that launches a long transform: the twiddle
// table of fft_long.h per device and HammingFeature's window per (device, D), built in float64 on the host, uploaded once.
#include <cmath>
#include <map>
#include <mutex>
#include <utility>
#include <vector>
#include "rfft_long.h"

namespace {

std::mutex g_mu;
std::map<int, float2*> g_tw;
std::map<std::pair<int, int>, double*> g_win;

// Windows live as long as the process: a pointer handed out may belong to a launch another host thread has not made yet, so
// nothing is ever freed.  Bounded by bytes instead (64 lengths of the largest window); a process that asks for more distinct
// lengths than fit gets BTK_ERR_ALLOCATION.  The first use of a length (and of a device) allocates and copies, so it cannot be
// part of a stream capture; every later launch with that length is capturable.
constexpr size_t WINDOW_BYTES_MAX = 64 * sizeof(double) * RFFT_MAX_L;
size_t g_win_bytes = 0;

}  // namespace

int longfft_twiddles(const float2** out)
{
  int dev = 0;
  BTK_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_tw.find(dev);
  if (it == g_tw.end()) {
    std::vector<float2> h(BTK_LONGFFT_TWN);
    for (int j = 0; j < BTK_LONGFFT_TWN; j++) {
      const double a = -2.0 * M_PI * (double)j / (double)BTK_LONGFFT_TWN;
      h[j] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    float2* d = nullptr;
    BTK_HIP_CHECK(hipMalloc(&d, sizeof(float2) * BTK_LONGFFT_TWN));
    BTK_HIP_CHECK(hipMemcpy(d, h.data(), sizeof(float2) * BTK_LONGFFT_TWN, hipMemcpyHostToDevice));
    it = g_tw.emplace(dev, d).first;
  }
  *out = it->second;
  return BTK_OK;
}

int longfft_hamming(const char* who, int D, const double** out)
{
  int dev = 0;
  BTK_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_win.find({dev, D});
  if (it == g_win.end()) {
    if (g_win_bytes + sizeof(double) * D > WINDOW_BYTES_MAX)
      return btk_set_error(BTK_ERR_ALLOCATION, "%s: more than %zu bytes of distinct window lengths in one process", who,
                           WINDOW_BYTES_MAX);
    std::vector<double> h(D);                      // HammingFeature's window, in its own order of operations (feature.cc:1181-1183)
    const double temp = 2. * M_PI / (double)(D - 1);
    for (int i = 0; i < D; i++) h[i] = 0.54 - 0.46 * std::cos(temp * i);
    double* d = nullptr;
    BTK_HIP_CHECK(hipMalloc(&d, sizeof(double) * D));
    BTK_HIP_CHECK(hipMemcpy(d, h.data(), sizeof(double) * D, hipMemcpyHostToDevice));
    g_win_bytes += sizeof(double) * D;
    it = g_win.emplace(std::make_pair(dev, D), d).first;
  }
  *out = it->second;
  return BTK_OK;
}

int longfft_log2(int L)
{
  if (L < RFFT_MIN_L || L > RFFT_MAX_L || (L & (L - 1))) return -1;
  int n = 0;
  while ((1 << n) < L) n++;
  return n;
}
