// What the entry points that run on a ctx's stream have in common, once: the stream and device of a call, the copies of a
// blocking call between the host's arrays and its one device allocation, and its end.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/adrates.h"

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

// One copy of a blocking call; an empty piece is skipped.
struct Piece {
    void* dst;
    const void* src;
    size_t bytes;
};

// Enqueues the pieces in order and stops at the first error.
template <size_t N>
hipError_t copy_pieces(const Piece (&pieces)[N], hipMemcpyKind kind, hipStream_t stream) {
    for (const Piece& pc : pieces) {
        const hipError_t e = pc.bytes ? hipMemcpyAsync(pc.dst, pc.src, pc.bytes, kind, stream) : hipSuccess;
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The end of a blocking call: wait for the stream, free the call's one allocation, report the first failure.
inline int finish_blocking(const std::string& w, int rc, hipError_t e, hipStream_t stream, void* base) {
    const hipError_t es = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = es;
    const hipError_t ef = hipFree(base);
    if (rc != ADR_OK) return rc;
    if (e == hipSuccess) e = ef;
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

}  // namespace call
}  // namespace adr
