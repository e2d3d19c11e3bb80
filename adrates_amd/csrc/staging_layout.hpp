// The memory plan of a blocking call's one device allocation (blocking_call.hpp's Staging): pieces laid end to end, each
// at a multiple of 16 bytes.  No HIP here, so the arithmetic compiles and is tested with the host compiler alone
// (tools/staging_layout_check.cpp).
#pragma once
#include <cstddef>

namespace adr {
namespace call {

struct StagingLayout {
    static constexpr size_t kAlign = 16;
    static constexpr size_t kAbsent = ~size_t(0);

    size_t total = 0;                // the end of the last piece: the bytes to allocate

    // The offset of a piece of `bytes`; an empty piece takes no room and is kAbsent.
    size_t add(size_t bytes) {
        if (bytes == 0) return kAbsent;
        const size_t at = (total + kAlign - 1) / kAlign * kAlign;
        total = at + bytes;
        return at;
    }

    // The piece at `offset` of the allocation `base`; null for an absent piece.
    static void* at(void* base, size_t offset) { return offset == kAbsent ? nullptr : static_cast<char*>(base) + offset; }
};

}  // namespace call
}  // namespace adr
