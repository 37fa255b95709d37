// device_owner.h — who frees what the host runtime takes from HIP (api_internal.h): device and pinned memory, host memory mapped
// into the device, streams and events. One move-only owner per resource; the destructor releases, so a struct of owners needs no
// free list and a failure path between an allocation and its release needs no unwinding. Host side only: no kernel includes this.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace namhip
{
// A handle H (a pointer, or hipStream_t / hipEvent_t, which are pointers too) and the call that releases it.
template <class H, class R, hipError_t (*Free)(R)>
class OwnedHandle
{
public:
  OwnedHandle() = default;
  OwnedHandle(const OwnedHandle&) = delete;
  OwnedHandle& operator=(const OwnedHandle&) = delete;
  OwnedHandle(OwnedHandle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  OwnedHandle& operator=(OwnedHandle&& o) noexcept
  {
    if (this != &o)
    {
      (void)reset();
      h_ = std::exchange(o.h_, nullptr);
    }
    return *this;
  }
  ~OwnedHandle() { (void)reset(); }

  H get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }
  // where an allocator / creator stores a fresh handle; what was held before is released first
  H* out()
  {
    (void)reset();
    return &h_;
  }
  // releases now; the runtime's answer (hipSuccess when empty: nothing is called)
  hipError_t reset()
  {
    H old = std::exchange(h_, nullptr);
    return old ? Free(old) : hipSuccess;
  }

private:
  H h_ = nullptr;
};

template <class T, hipError_t (*Free)(void*)> using Owned = OwnedHandle<T*, void*, Free>;
template <class T> using DeviceBuf = Owned<T, &hipFree>; // hipMalloc and hipExtMallocWithFlags memory alike
template <class T> using PinnedBuf = Owned<T, &hipHostFree>;
using StreamOwner = OwnedHandle<hipStream_t, hipStream_t, &hipStreamDestroy>;
using EventOwner = OwnedHandle<hipEvent_t, hipEvent_t, &hipEventDestroy>;

// `n` elements of `src` in a fresh device allocation of max(n, min_elems) elements (a blocking copy)
template <class T>
hipError_t upload(DeviceBuf<T>& dst, const T* src, size_t n, size_t min_elems = 0)
{
  hipError_t e = hipMalloc(dst.out(), (n > min_elems ? n : min_elems) * sizeof(T));
  if (e == hipSuccess && n)
    e = hipMemcpy(dst.get(), src, n * sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess)
    (void)dst.reset();
  return e;
}

// `n` elements of fine-grained device memory: local to the kernels that poll it, host-writable through the PCIe BAR
template <class T>
hipError_t alloc_fine_grained(DeviceBuf<T>& dst, size_t n)
{
  return hipExtMallocWithFlags(reinterpret_cast<void**>(dst.out()), n * sizeof(T), hipDeviceMallocFinegrained);
}

// Pinned host memory mapped into the device (coherent): one allocation, the host's address and the device's alias of it.
// Move-only through its owner.
template <class T>
class MappedBuf
{
public:
  hipError_t alloc(size_t n)
  {
    hipError_t e = hipHostMalloc(h_.out(), n * sizeof(T), hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess)
      e = hipHostGetDevicePointer(reinterpret_cast<void**>(&d_), h_.get(), 0);
    if (e != hipSuccess)
      (void)reset();
    return e;
  }
  T* host() const { return h_.get(); }
  T* dev() const { return h_ ? d_ : nullptr; } // (a moved-from buffer has given its memory away: no alias either)
  explicit operator bool() const { return (bool)h_; }
  hipError_t reset() { return h_.reset(); }

private:
  PinnedBuf<T> h_;
  T* d_ = nullptr; // (meaningful while h_ holds the memory)
};
} // namespace namhip
