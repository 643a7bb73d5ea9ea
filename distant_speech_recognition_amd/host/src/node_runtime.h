// node_runtime.h -- what every *_nodes.cc stands on (internal: not under include/, not part of the interface that mirrors the
// reference): the mapping of C-ABI and HIP errors to the j*_error classes, the calling thread's streams, the copy helpers and the
// counters behind the btk_node_* functions of common/devmem.h.  One definition each, in node_runtime.cc, hidden from the
// library's exported symbols.  A module's file starts with
//   #include "node_runtime.h"
//   namespace { using btknode::check_abi; using btknode::check_hip; using btknode::nstream; ... }
// so a new BTK_ERR_* code or a change to a copy's ordering lands in every module at once.
#pragma once
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <chrono>
#include <cstddef>

#include "btkhip.h"

#pragma GCC visibility push(hidden)
namespace btknode {

// BTK_OK returns; every other code of btkhip.h throws its j*_error with btk_last_error() as the message
void check_abi(int rc);
// hipSuccess returns; hipErrorOutOfMemory throws jallocation_error, everything else j_error ("what: hip's text")
void check_hip(hipError_t e, const char* what);

// the calling thread's node stream (btk_node_stream()) as a hipStream_t
hipStream_t nstream();
// a host thread's second stream: uploads of the block AFTER the current one (16-bit streams, SubbandBeamformer::prefetch_next_)
hipStream_t cstream();
// waits for the copies staged ahead, if this thread ever staged any (a host without a device never opens the stream)
void csync_if_open();
void nsync();

// (device and pinned memory: DeviceBuffer / PinnedBuffer of common/devmem.h, members for a node's state and locals for the
// one-off blocks of the design-time paths -- nothing else in the node layer allocates or frees)
// copies between pageable host memory and the device, complete on return, ordered on the node stream like every launch
void h2d(void* d, const void* h, size_t n);
void d2h(void* h, const void* d, size_t n);
// the asynchronous forms: `h` is pinned memory that stays untouched until the stream has passed the copy
void h2d_async(void* d, const void* h, size_t n);
void d2h_async(void* h, const void* d, size_t n);
void d2d_async(void* dst, const void* src, size_t n);
// rows x width bytes between two pitched device arrays
void d2d_2d_async(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows);
void dev_zero_async(void* d, size_t n);
// n rows of `bytes` bytes that lie in SEPARATE pinned allocations -> rows `pitch` bytes apart of one device block, on `stream`
void upload_rows(btk_row_t* tab, unsigned n, size_t bytes, char* dst, size_t pitch, hipStream_t stream);

// the value of the environment variable `name` if it is a positive number, else dflt (BTK_<X>_BLOCK_FRAMES of the modules)
long env_block_frames(const char* name, long dflt);
// Rows of a round's input window are an even number of frames apart, so that every launch of a stream can be an ALIGNED one
// (btk_fb_synthesis_aligned_form: such geometries have a second kernel form for aligned launches, <= 2 ulp from the other; a
// stream cut into rounds gives the same bits as one round only if all its launches take the same form)
inline long even_pitch(long frames) { return frames + (frames & 1); }

// the counters of btk_node_alloc_counts() and btk_node_timers()
extern std::atomic<long> g_device_allocs, g_pinned_allocs;
extern std::atomic<long long> g_pull_ns, g_upload_ns, g_device_ns;
struct ScopedNs {                                   // adds the scope's wall time to one of the counters of btk_node_timers()
  std::atomic<long long>& acc;
  std::chrono::steady_clock::time_point t0;
  explicit ScopedNs(std::atomic<long long>& a) : acc(a), t0(std::chrono::steady_clock::now()) {}
  ~ScopedNs() { acc += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
};

}  // namespace btknode
#pragma GCC visibility pop
