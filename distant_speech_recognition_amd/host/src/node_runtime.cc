// node_runtime.cc -- the one copy of the node layer's runtime helpers (node_runtime.h) and the bodies of common/devmem.h:
// the thread's streams, the allocation / D2H / timer counters, the copy helpers, DeviceBuffer and PinnedBuffer.
#include "node_runtime.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "common/devmem.h"
#include "common/jexception.h"

namespace btknode {

void check_abi(int rc)
{
  if (rc == BTK_OK) return;
  const char* msg = btk_last_error();
  switch (rc) {
    case BTK_ERR_DIMENSION: throw jdimension_error("%s", msg);
    case BTK_ERR_CONSISTENCY: throw jconsistency_error("%s", msg);
    case BTK_ERR_ALLOCATION: throw jallocation_error("%s", msg);
    case BTK_ERR_PARAMETER: throw jparameter_error("%s", msg);
    case BTK_ERR_NUMERIC: throw jnumeric_error("%s", msg);
    default: throw j_error("%s", msg);
  }
}

void check_hip(hipError_t e, const char* what)
{
  if (e == hipSuccess) return;
  if (e == hipErrorOutOfMemory) throw jallocation_error("%s: %s", what, hipGetErrorString(e));
  throw j_error("%s: %s", what, hipGetErrorString(e));
}

std::atomic<long> g_device_allocs(0), g_pinned_allocs(0);
std::atomic<long long> g_pull_ns(0), g_upload_ns(0), g_device_ns(0);
static std::atomic<long long> g_d2h_bytes(0);
static std::atomic<long> g_live_device_blocks(0);

hipStream_t nstream() { return static_cast<hipStream_t>(btk_node_stream()); }
static thread_local hipStream_t t_cstream = NULL;
hipStream_t cstream()
{
  if (!t_cstream) check_hip(hipStreamCreateWithFlags(&t_cstream, hipStreamNonBlocking), "hipStreamCreateWithFlags");
  return t_cstream;
}
void csync_if_open() { if (t_cstream) (void)hipStreamSynchronize(t_cstream); }
void nsync() { check_hip(hipStreamSynchronize(nstream()), "hipStreamSynchronize"); }

void h2d(void* d, const void* h, size_t n)
{
  if (!n) return;
  check_hip(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, nstream()), "hipMemcpyAsync H2D");
  nsync();
}
void d2h(void* h, const void* d, size_t n)
{
  if (!n) return;
  check_hip(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, nstream()), "hipMemcpyAsync D2H");
  btk_node_count_d2h(n);
  nsync();
}
void h2d_async(void* d, const void* h, size_t n)
{
  if (n) check_hip(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, nstream()), "hipMemcpyAsync H2D");
}
void d2h_async(void* h, const void* d, size_t n)
{
  if (!n) return;
  check_hip(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, nstream()), "hipMemcpyAsync D2H");
  btk_node_count_d2h(n);
}
void d2d_async(void* dst, const void* src, size_t n)
{
  if (n) check_hip(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, nstream()), "hipMemcpyAsync D2D");
}
// The bytes of a row behind `bytes` are zeroed.  `tab` [pinned, n entries, src filled in by the caller] and the rows (every
// channel's source owns its utterance) stay untouched until the stream has passed the call.  ONE kernel that reads the host memory
// through the table (btk_gather_rows: the link's 57 GB/s whatever the rows' length) where a copy per row reaches 27 GB/s at 0.5 MB
// per row and 49 at 4 MB (profiles/r06_ubench_host_gather.txt); rows that are not 16-byte aligned -- a shift length that is no
// multiple of 8 samples -- take the copies.  BTK_NODE_GATHER=0: always the copies.
void upload_rows(btk_row_t* tab, unsigned n, size_t bytes, char* dst, size_t pitch, hipStream_t stream)
{
  const char* env = getenv("BTK_NODE_GATHER");                      // (read per upload: a test switches it inside one process)
  const bool off = env && atoi(env) == 0;
  if (!n || !pitch) return;
  bool aligned = !off && ((reinterpret_cast<uintptr_t>(dst) | pitch) & 15) == 0;
  for (unsigned c = 0; c < n && aligned; c++) aligned = (reinterpret_cast<uintptr_t>(tab[c].src) & 15) == 0;
  if (aligned) {
    for (unsigned c = 0; c < n; c++) tab[c].bytes = (long)bytes;
    check_abi(btk_gather_rows(tab, dst, (int)n, (long)pitch, stream));
    return;
  }
  if (bytes < pitch) check_hip(hipMemset2DAsync(dst + bytes, pitch, 0, pitch - bytes, n, stream), "hipMemset2DAsync");
  if (bytes)
    for (unsigned c = 0; c < n; c++)
      check_hip(hipMemcpyAsync(dst + (size_t)c * pitch, tab[c].src, bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync H2D");
}
void d2d_2d_async(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows)
{
  if (!width || !rows) return;
  check_hip(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToDevice, nstream()), "hipMemcpy2DAsync D2D");
}
void dev_zero_async(void* d, size_t n)
{
  if (n) check_hip(hipMemsetAsync(d, 0, n, nstream()), "hipMemsetAsync");
}

long env_block_frames(const char* name, long dflt)
{
  const char* e = getenv(name);
  const long v = (e && *e) ? atol(e) : 0;
  return v > 0 ? v : dflt;
}

}  // namespace btknode

using namespace btknode;

// ================================================================================ node stream, device / pinned buffers
void* btk_node_stream()
{
  // one stream per host thread, never destroyed (a thread_local destructor would run after the HIP runtime's own teardown)
  static thread_local hipStream_t st = NULL;
  if (!st) check_hip(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreateWithFlags");
  return st;
}
void btk_node_synchronize() { nsync(); }
void btk_node_alloc_counts(long* device_allocs, long* pinned_allocs)
{
  if (device_allocs) *device_allocs = g_device_allocs.load();
  if (pinned_allocs) *pinned_allocs = g_pinned_allocs.load();
}
long btk_node_live_device_blocks() { return g_live_device_blocks.load(); }

long long btk_node_d2h_bytes() { return g_d2h_bytes.load(std::memory_order_relaxed); }
void btk_node_d2h_bytes_reset() { g_d2h_bytes.store(0, std::memory_order_relaxed); }
void btk_node_count_d2h(size_t bytes) { g_d2h_bytes.fetch_add((long long)bytes, std::memory_order_relaxed); }

void btk_node_timers(double* pull_s, double* upload_s, double* device_s)
{
  if (pull_s) *pull_s = 1e-9 * (double)g_pull_ns.load();
  if (upload_s) *upload_s = 1e-9 * (double)g_upload_ns.load();
  if (device_s) *device_s = 1e-9 * (double)g_device_ns.load();
}
void btk_node_timers_reset() { g_pull_ns = 0; g_upload_ns = 0; g_device_ns = 0; }

void* DeviceBuffer::ensure(size_t bytes)
{
  if (bytes <= cap_ && p_) return p_;
  const size_t want = std::max(bytes ? bytes : (size_t)16, cap_ + cap_ / 2);
  if (p_) { nsync(); release(); }                                         // launches that still read the old block
  check_hip(hipMalloc(&p_, want), "hipMalloc");
  g_device_allocs++; g_live_device_blocks++;
  cap_ = want;
  return p_;
}
void DeviceBuffer::release()
{
  if (p_) { (void)hipFree(p_); g_live_device_blocks--; }
  p_ = NULL; cap_ = 0;
}

void* PinnedBuffer::ensure(size_t bytes) { return ensure_keep(bytes, 0); }
void* PinnedBuffer::ensure_keep(size_t bytes, size_t keep_bytes)
{
  if (bytes <= cap_ && p_) return p_;
  const size_t want = std::max(bytes ? bytes : (size_t)16, cap_ + cap_ / 2);
  void* q = NULL;
  // (mapped: the gather kernel of upload_rows reads this memory itself; portable: whichever device of the process runs it)
  check_hip(hipHostMalloc(&q, want, hipHostMallocPortable | hipHostMallocMapped), "hipHostMalloc");
  g_pinned_allocs++;
  if (p_) {
    nsync();                                                                // copies that still read the old block
    if (keep_bytes) memcpy(q, p_, std::min(keep_bytes, cap_));
    (void)hipHostFree(p_);
  }
  p_ = q; cap_ = want;
  return p_;
}
void PinnedBuffer::release() { if (p_) (void)hipHostFree(p_); p_ = NULL; cap_ = 0; }
