// The device allocations of one handle (a curve, a curve plan, a curve set, a batch, a batch's schedule groups) or of one
// blocking call's temporaries: the list of pointers and the first HIP error.  After an error every call does nothing and
// returns null, so a caller writes its allocations and copies in a row and tests `ok()` once.
//
// One hipMalloc per array, never a slab: the fast kernels store gamma as 16-byte pairs and in 1 KB non-temporal stores and
// rely on the alignment of each allocation; with an odd trade count sub-buffers cut from one slab would not have it.
//
// No destructor: a handle that is a view (a curve of a set) holds an empty owner and is copied freely; whoever owns memory
// calls release().
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace adr {

struct DeviceOwner {
    std::vector<void*> ptrs;
    hipError_t error = hipSuccess;
    // An empty array (0 bytes) is null.  Set: it is a real buffer of `pad` bytes - for kernels that form an address from the
    // pointer whatever the count (see the one owner that sets it).
    bool keep_empty = false;

    explicit DeviceOwner(bool keep_empty_arrays = false) : keep_empty(keep_empty_arrays) {}

    bool ok() const { return error == hipSuccess; }
    void note(hipError_t e) { if (error == hipSuccess) error = e; }

    // bytes + pad of device memory; `pad`: room behind the array for readers that fetch a neighbour of the last element.
    void* alloc(size_t bytes, size_t pad = 0) {
        if (error != hipSuccess || (bytes == 0 && !(keep_empty && pad))) return nullptr;
        void* p = nullptr;
        error = hipMalloc(&p, bytes + pad);
        if (error != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return p;
    }
    template <typename T>
    T* array(size_t count, size_t pad = 0) { return static_cast<T*>(alloc(count * sizeof(T), pad)); }

    // ... with its `bytes` (not the pad) zeroed on `stream`
    void* alloc_zeroed(size_t bytes, hipStream_t stream, size_t pad = 0) {
        void* p = alloc(bytes, pad);
        if (p && bytes) note(hipMemsetAsync(p, 0, bytes, stream));
        return p;
    }

    // ... filled from the host by an ASYNCHRONOUS copy on `stream`: `src` must outlive it - the caller synchronises the
    // stream before the memory behind `src` goes away, on its error paths too.
    void* put(const void* src, size_t bytes, hipStream_t stream, size_t pad = 0) {
        void* p = alloc(bytes, pad);
        if (p && bytes) note(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, stream));
        return p;
    }
    template <typename T>
    T* put_n(const T* src, size_t count, hipStream_t stream, size_t pad = 0) {
        return static_cast<T*>(put(src, count * sizeof(T), stream, pad));
    }
    template <typename T>
    T* put(const std::vector<T>& v, hipStream_t stream, size_t pad = 0) {
        return static_cast<T*>(put(v.data(), v.size() * sizeof(T), stream, pad));
    }

    // Frees everything and returns the error held; the owner is empty and usable again.
    hipError_t release() {
        for (void* p : ptrs) hipFree(p);
        ptrs.clear();
        const hipError_t e = error;
        error = hipSuccess;
        return e;
    }
};

}  // namespace adr
