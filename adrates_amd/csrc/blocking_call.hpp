// What the entry points that run on a ctx's stream have in common, once: the stream and device of a call, and the device
// memory of a blocking call - one allocation that every array of the call is declared into once.
#pragma once
#include <hip/hip_runtime.h>

#include <cassert>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "staging_layout.hpp"

int adr_set_error(int status, const std::string& msg);                          // capi.hip
int adr_ctx_target(const adr_ctx* ctx, int* device, hipStream_t* stream);      // capi.hip

namespace adr {
namespace call {

// The stream a call on `ctx` runs on - the caller's, or else the ctx's own - with the ctx's device made current.
inline int target_stream(const std::string& w, const adr_ctx* ctx, hipStream_t stream_or_null, hipStream_t* stream) {
    int device = 0;
    const int rc = adr_ctx_target(ctx, &device, stream);
    if (rc != ADR_OK) return rc;
    if (stream_or_null) *stream = stream_or_null;
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

// The device memory of a blocking call.  The entry declares each device array once - in(), out() or scratch(), with the
// address of the pointer to set and an element count - and the size, the cuts and both lists of copies follow from that:
//     Staging mem;
//     mem.in(&drows, rows, R);  mem.out(&dvar, var, B);  mem.scratch(&dwork, W);
//     hipError_t e = mem.begin(stream);                          // one hipMalloc, the pointers, the uploads
//     if (e == hipSuccess) e = enqueue(drows, dvar, dwork, stream);
//     return mem.finish(w, ADR_OK, e, stream);                   // the downloads, the wait, the free, the report
// A piece of count 0, or declared with on = false, gets a null pointer and no bytes.  Every other piece starts at a
// multiple of 16 bytes, and an entry may rely on no more than that.  A present in(), out() or inout() needs its host
// array (asserted): an output that is kept on the device when nobody asks for it is declared as scratch() in that case.
// The host source of in() is read when the stream gets there, not at the declaration: it must stay alive and unchanged
// until finish() returns.  Until begin() succeeds every declared pointer is null.
class Staging {
public:
    Staging() = default;
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    ~Staging() { if (base_) hipFree(base_); }

    template <class T>
    void in(T** dev, const T* src, size_t count, bool on = true) { add(dev, on ? count * sizeof(T) : 0, src, nullptr, src); }
    template <class T>
    void out(T** dev, T* dst, size_t count, bool on = true) { add(dev, on ? count * sizeof(T) : 0, nullptr, dst, dst); }
    template <class T>
    void inout(T** dev, T* both, size_t count, bool on = true) { add(dev, on ? count * sizeof(T) : 0, both, both, both); }
    template <class T>
    void scratch(T** dev, size_t count, bool on = true) { add(dev, on ? count * sizeof(T) : 0, nullptr, nullptr, dev); }
    void scratch_bytes(void** dev, size_t bytes) { add(dev, bytes, nullptr, nullptr, dev); }

    // Allocates, sets every declared pointer and enqueues the uploads in declaration order, up to the first error.
    hipError_t begin(hipStream_t stream) {
        alloc_ = hipMalloc(&base_, layout_.total);
        if (alloc_ != hipSuccess) {
            base_ = nullptr;
            return alloc_;
        }
        for (const Piece& pc : pieces_) *pc.dev = StagingLayout::at(base_, pc.at);
        return copy(true, stream);
    }

    // The end of the call: the downloads in declaration order if nothing has failed, then always the wait for the stream
    // and the free; reports the first failure, a refusal `rc` before a HIP error `e`.
    int finish(const std::string& w, int rc, hipError_t e, hipStream_t stream) {
        if (alloc_ != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": hipMalloc: " + hipGetErrorString(alloc_));
        if (rc == ADR_OK && e == hipSuccess) e = copy(false, stream);
        const hipError_t es = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = es;
        const hipError_t ef = hipFree(base_);
        base_ = nullptr;
        if (rc != ADR_OK) return rc;
        if (e == hipSuccess) e = ef;
        if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
        return ADR_OK;
    }

private:
    struct Piece {
        void** dev;
        size_t at, bytes;
        const void* src;             // an input's host source
        void* dst;                   // an output's host destination
    };

    // `needed` is the piece's host array, which a present piece must have (scratch passes a non-null placeholder).
    // begin() sets the caller's T* through a void**: every object pointer has one representation here, and clang's
    // type-based alias analysis gives all pointers one type, so the store is seen by the caller's later reads.
    template <class T>
    void add(T** dev, size_t bytes, const void* src, void* dst, const void* needed) {
        assert(needed || !bytes);
        *dev = nullptr;
        pieces_.push_back(Piece{reinterpret_cast<void**>(dev), layout_.add(bytes), bytes, src, dst});
    }

    hipError_t copy(bool up, hipStream_t stream) const {
        for (const Piece& pc : pieces_) {
            if (!pc.bytes || !(up ? pc.src : pc.dst)) continue;       // absent, or no copy in this direction
            const hipError_t e = up ? hipMemcpyAsync(*pc.dev, pc.src, pc.bytes, hipMemcpyHostToDevice, stream)
                                    : hipMemcpyAsync(pc.dst, *pc.dev, pc.bytes, hipMemcpyDeviceToHost, stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }

    StagingLayout layout_;
    std::vector<Piece> pieces_;
    void* base_ = nullptr;
    hipError_t alloc_ = hipSuccess;
};

}  // namespace call
}  // namespace adr
