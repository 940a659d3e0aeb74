// Owned device arrays and pinned, device-mapped host arrays of the agent groups (agent_group.hpp, group_core.hpp): freed with their owner.
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <memory>
#include <vector>

namespace bdr {

// a device array, and a pinned, device-mapped, zeroed host array with its device address: freed with their owner
struct HipDeviceFree { void operator()(void* p) const { (void)hipFree(p); } };
struct HipHostFree { void operator()(void* p) const { (void)hipHostFree(p); } };
template <class T> using DeviceArray = std::unique_ptr<T, HipDeviceFree>;
template <class T> struct PinnedArray { std::unique_ptr<T, HipHostFree> host; T* dev = nullptr; };

template <class T> hipError_t device_array(DeviceArray<T>& out, size_t n)
{
    T* p = nullptr;
    const hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
    if (e == hipSuccess) out.reset(p);
    return e;
}
// (`out` keeps what it held when this fails)
template <class T> hipError_t pinned_array(PinnedArray<T>& out, size_t n)
{
    PinnedArray<T> a;
    T* p = nullptr;
    hipError_t e = hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocMapped);
    if (e != hipSuccess) return e;
    a.host.reset(p);
    memset(p, 0, n * sizeof(T));
    e = hipHostGetDevicePointer((void**)&a.dev, p, 0);
    if (e == hipSuccess) out = std::move(a);
    return e;
}

// a host vector and the device array it is uploaded to (an empty one still owns one device element: its pointer is a kernel argument)
template <class T> struct StagedArray {
    std::vector<T> h; DeviceArray<T> d;
    hipError_t resize(size_t n) { h.resize(n); return device_array(d, n < 1 ? 1 : n); }
    hipError_t upload() { return h.empty() ? hipSuccess : hipMemcpy(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice); }
    T& operator[](size_t i) { return h[i]; }
};
// resize(n) / upload() of every array of a list, up to the first error
template <class... A> hipError_t staged_resize(size_t n, A&... a) { hipError_t e = hipSuccess; ((e = e == hipSuccess ? a.resize(n) : e), ...); return e; }
template <class... A> hipError_t staged_upload(A&... a) { hipError_t e = hipSuccess; ((e = e == hipSuccess ? a.upload() : e), ...); return e; }

}  // namespace bdr
