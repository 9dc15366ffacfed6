// A device table with one owner: allocated and filled by upload(), freed by the destructor.  Included by every part
// of p2e_hip.hip (the context's layout is the same in all of them).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace p2e {

template <class T>
class DeviceArray {
    T* p_ = nullptr;

public:
    DeviceArray() = default;
    DeviceArray(DeviceArray&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DeviceArray& operator=(DeviceArray&& o) noexcept {
        std::swap(p_, o.p_);
        return *this;
    }
    DeviceArray(const DeviceArray&) = delete;
    DeviceArray& operator=(const DeviceArray&) = delete;
    ~DeviceArray() {
        if (p_) (void)hipFree(p_);
    }
    T* get() const { return p_; }
    // Replaces the contents by a copy of src[0, count); an empty source leaves a null pointer and allocates nothing.
    // On failure the array is empty and the error is consumed (it must not resurface as a later launch error).
    hipError_t upload(const T* src, size_t count) {
        DeviceArray fresh;
        if (count) {
            hipError_t e = hipMalloc(&fresh.p_, sizeof(T) * count);
            if (e != hipSuccess)
                fresh.p_ = nullptr;
            else
                e = hipMemcpy(fresh.p_, src, sizeof(T) * count, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                *this = DeviceArray();
                return e;
            }
        }
        *this = std::move(fresh);
        return hipSuccess;
    }
    // Replaces the contents by `count` uninitialised elements (scratch); on failure the array is empty, as for upload().
    hipError_t alloc(size_t count) {
        *this = DeviceArray();
        if (!count) return hipSuccess;
        hipError_t e = hipMalloc(&p_, sizeof(T) * count);
        if (e != hipSuccess) {
            p_ = nullptr;
            (void)hipGetLastError();
        }
        return e;
    }
    hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }
};

}  // namespace p2e
