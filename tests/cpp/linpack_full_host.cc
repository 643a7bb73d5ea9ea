// linpack_full_host.cc -- TEST harness: csvdc with job = 11 (U and V) and the pseudo-inverse assembly of csrc/linpack_f32.h
// compiled by g++ with the one-thread context, for bit-for-bit comparisons with the reference's compiled csvdc without a GPU
// (tests/test_linpack_full.py).  Build: g++ -O2 -ffp-contract=off -shared -fPIC.
#include <vector>
#include <cstring>
#include "linpack_f32.h"

// a [n][p] row-major; s, e [min(n + 1, p)]; u [n * n], v [p * p] column-major (u[i + k * n]) as the reference's
extern "C" int lpk_host_csvdc_full(const float* a, int n, int p, float* s, float* e, float* u, float* v)
{
  using namespace lpk;
  std::vector<cf> x((size_t)n * p), col(n + 1), ev(p + 1), work(n + 1), sc(n + p + 2), ec(n + p + 2), t(2);
  std::memcpy(x.data(), a, sizeof(cf) * (size_t)n * p);
  int flag[2] = {0, 0};
  Work w{col.data(), ev.data(), work.data(), sc.data(), ec.data(), t.data(), flag};
  return csvdc_full(x.data(), p, n, p, w, s, e, reinterpret_cast<cf*>(u), reinterpret_cast<cf*>(v));
}

// beamformer.cc:262-280 on given s [N], u (M x M), v (N x N) column-major: inv [N][M] row-major; returns the number of s under the threshold
extern "C" int lpk_host_pinv_assemble(int M, int N, const float* s, const float* u, const float* v, float threshold, float* inv)
{
  using namespace lpk;
  std::vector<cf> sinv(N);
  const int below = pinv_sinv(N, s, threshold, sinv.data());
  SerialCtx cx;
  pinv_assemble(cx, M, N, reinterpret_cast<const cf*>(u), reinterpret_cast<const cf*>(v), sinv.data(), reinterpret_cast<cf*>(inv));
  return below;
}
