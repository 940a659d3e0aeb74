// Owned device arrays and pinned, device-mapped host arrays of the agent groups (agent_group.hpp, bc_group.hpp): freed with their owner.
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <memory>

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

}  // namespace bdr
