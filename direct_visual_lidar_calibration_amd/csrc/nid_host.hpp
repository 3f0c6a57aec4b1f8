// nid_host.hpp -- what every host translation unit of libnidreg.so needs and nothing about NID passes: the error text, the owners
// of device / host-mapped memory, device selection, the checked kernel launch, run-time value -> template argument dispatch, the
// phase clock behind the *_get_timing entry points and the one-upload staging block of the packet decoders.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/nidreg.h"

namespace nidreg {

// error text of the calling thread (nidreg_last_error); returns `code`
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t _e = (expr);                                                                             \
    if (_e != hipSuccess) return fail(NIDREG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// (internal to libnidreg.so: these helpers add nothing to its dynamic symbol table)
#define NIDREG_HIDDEN __attribute__((visibility("hidden")))

// Move-only owner of ONE device allocation (hipMalloc, or fine-grained hipExtMallocWithFlags: the shard histogram replicas and
// exchange blocks; hipFree releases both).  The destructor frees and ignores the error; reset() reports it.  Whoever destroys an
// owner makes sure first that no kernel still uses the memory (free_handle says how a handle does).
class NIDREG_HIDDEN DeviceBuf {
 public:
  DeviceBuf() = default;
  DeviceBuf(DeviceBuf&& o) noexcept : p_(o.release()) {}
  DeviceBuf& operator=(DeviceBuf&& o) noexcept {  // (frees what it held AFTER `o` was allocated: a table regrow keeps the old one on failure)
    if (this != &o) adopt(o.release());
    return *this;
  }
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  ~DeviceBuf() { (void)reset(); }
  hipError_t alloc(size_t bytes) { return (void)reset(), hipMalloc(&p_, bytes); }
  hipError_t alloc_finegrained(size_t bytes) { return (void)reset(), hipExtMallocWithFlags(&p_, bytes, hipDeviceMallocFinegrained); }
  void adopt(void* p) { (void)reset(), p_ = p; }  // a hipMalloc'ed pointer handed over as "caller owns"
  void* release() { return std::exchange(p_, nullptr); }
  hipError_t reset() { return p_ ? hipFree(release()) : hipSuccess; }
  template <typename T = void> T* as() const { return static_cast<T*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }
 private:
  void* p_ = nullptr;
};
// ... and of one host-mapped block that does not come from the per-device pool (nidreg_internal.hpp ResourcePool)
class NIDREG_HIDDEN HostBuf {
 public:
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { reset(); }
  hipError_t alloc(size_t bytes, unsigned flags) { return reset(), hipHostMalloc(&p_, bytes, flags); }
  void reset() {
    if (p_) (void)hipHostFree(std::exchange(p_, nullptr));
  }
  template <typename T = void> T* as() const { return static_cast<T*>(p_); }
 private:
  void* p_ = nullptr;
};

// entry points that take a device id: count -> range -> hipSetDevice, with the caller's name `who` in the error text
NIDREG_HIDDEN inline int count_devices(const char* who, int* ndev, const char* note = "") {
  if (hipGetDeviceCount(ndev) != hipSuccess || *ndev <= 0) return fail(NIDREG_ERR_NO_DEVICE, std::string(who) + ": no HIP device" + note);
  return NIDREG_OK;
}
NIDREG_HIDDEN inline int use_device(const char* who, int device_id, const char* note = "") {
  int ndev = 0;
  if (const int rc = count_devices(who, &ndev, note)) return rc;
  if (device_id < 0 || device_id >= ndev) return fail(NIDREG_ERR_INVALID, std::string(who) + ": device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  return NIDREG_OK;
}

// A kernel launch and its error in one expression, so that no launch goes unchecked: HIP_TRY(launch(k_x, grid, block, 0, nullptr, ...)).
// The arguments convert to the kernel's parameter types as in a direct call.
template <typename K, typename... Args>
NIDREG_HIDDEN inline hipError_t launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
  return hipGetLastError();
}
// workgroups of `threads` that cover n items
NIDREG_HIDDEN inline unsigned blocks_for(long long n, int threads) { return unsigned((n + threads - 1) / threads); }

// Host-side dispatch from a run-time value to a template argument: f(std::integral_constant<int, V>{}) for the V that equals
// `value` (false: none did, f was not called), f(std::true_type{}) / f(std::false_type{}) for a flag.  f is a generic lambda; its
// parameter converts to the template argument at compile time: k_velodyne_decode<L>, if constexpr (MULTI).  (with_model for the
// camera models: nid_device.hpp.)
template <int... V, typename F>
NIDREG_HIDDEN inline bool with_int(int value, F&& f) {
  return ((value == V ? (f(std::integral_constant<int, V>{}), true) : false) || ...);
}
template <typename F>
NIDREG_HIDDEN inline auto with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// Host wall-clock milliseconds of the N phases of an entry point's last call on this thread (one thread_local instance each):
// lap(k) stores the time since start() or the last lap into slot k.  A slot a call does not reach keeps its earlier value.
template <int N>
class NIDREG_HIDDEN PhaseClock {
 public:
  void clear() { std::memset(ms_, 0, sizeof(ms_)); }
  void start() { mark_ = std::chrono::steady_clock::now(); }
  void lap(int k) {
    const auto now = std::chrono::steady_clock::now();
    ms_[k] = std::chrono::duration<double, std::milli>(now - mark_).count();
    mark_ = now;
  }
  // the body of the getter `who`
  int read(const char* who, double* out, const char* what = "argument") const {
    if (!out) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null " + what);
    std::memcpy(out, ms_, sizeof(ms_));
    return NIDREG_OK;
  }
 private:
  double ms_[N] = {};
  std::chrono::steady_clock::time_point mark_;
};

// The packets of a message as they lie in it, `stride` bytes apart: what the packet decoders refuse about them ...
NIDREG_HIDDEN inline int check_packets(const std::string& who, int64_t num_packets, int64_t max_packets, int64_t packet_stride, int64_t packet_bytes, int64_t max_stride) {
  if (packet_stride < packet_bytes) return fail(NIDREG_ERR_INVALID, who + ": packet_stride " + std::to_string(packet_stride) + " is below the " + std::to_string(packet_bytes) + " bytes of a packet");
  if (packet_stride > max_stride) return fail(NIDREG_ERR_INVALID, who + ": packet_stride " + std::to_string(packet_stride) + " is above " + std::to_string(max_stride));
  if (num_packets < 0 || num_packets > max_packets) return fail(NIDREG_ERR_INVALID, who + ": num_packets " + std::to_string(num_packets) + " outside [0, " + std::to_string(max_packets) + "]");
  return NIDREG_OK;
}
// ... and the bytes of num_packets >= 1 of them: the last packet's tail is not the caller's to give
NIDREG_HIDDEN inline size_t packet_area_bytes(int64_t num_packets, int64_t packet_stride, int64_t packet_bytes) { return size_t(num_packets - 1) * size_t(packet_stride) + size_t(packet_bytes); }

// n zeroed bytes of host memory; none left is the refusal "`who`: no host memory for `what`" (nothing may leave an extern "C" function)
NIDREG_HIDDEN inline int host_zeros(std::vector<uint8_t>& v, size_t n, const std::string& who, const std::string& what) {
  try {
    v.assign(n, 0);
  } catch (const std::bad_alloc&) {
    return fail(NIDREG_ERR_INVALID, who + ": no host memory for " + what);
  }
  return NIDREG_OK;
}

// One host block, one copy, one device allocation for the inputs of a stateless entry point: part() lays the parts out, take()
// gets the zeroed host memory, put() fills a part, upload() allocates and copies, device<T>() is a part on the device.
class NIDREG_HIDDEN StagingBlock {
 public:
  size_t part(size_t bytes, size_t align = 8) {  // the part's offset in the block
    const size_t off = (total_ + align - 1) / align * align;
    total_ = off + bytes;
    return off;
  }
  // a packet area of `bytes` bytes: 8-byte aligned (the decoders' dword loads need 4), then padding to whole dwords and one more,
  // so that a dword load of a packet's last bytes stays inside the block
  size_t packet_part(size_t bytes) { return part((bytes + 3) / 4 * 4 + 4, 8); }
  int take(const std::string& who) { return host_zeros(host_, total_, who, "a staging block of " + std::to_string(total_) + " bytes"); }
  void put(size_t off, const void* src, size_t bytes) { std::memcpy(host_.data() + off, src, bytes); }
  hipError_t upload() {
    const hipError_t e = dev_.alloc(total_);
    return e != hipSuccess ? e : hipMemcpy(dev_.as<void>(), host_.data(), total_, hipMemcpyHostToDevice);
  }
  template <typename T> const T* device(size_t off) const { return reinterpret_cast<const T*>(dev_.as<uint8_t>() + off); }
 private:
  size_t total_ = 0;
  std::vector<uint8_t> host_;
  DeviceBuf dev_;
};

}  // namespace nidreg
