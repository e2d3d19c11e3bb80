// LJ[k][p] and LC[k][p][q] of an uploaded curve, read from whichever tables it carries: the 32-wide tiles or the wide
// layout of 33-64 pillars.  Shared by the two knot-space projections (kernels_knot.hip, subbook_ladder.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace adr {
namespace {

__device__ __forceinline__ double lj_at(const CurveDev& cv, int k, int p) {
    if (cv.wide_nch > 0 && cv.lj64) return cv.lj64[static_cast<size_t>(k) * kWidePad + p];
    return cv.lj[(static_cast<size_t>(p / kPillarPad) * cv.Kc + k) * kPillarPad + p % kPillarPad];
}

// LC[k][p][q]: the wide layout's packed triangle in position space, or the 32 x 32 tiles of the general kernel
__device__ __forceinline__ double lc_at(const CurveDev& cv, const int* col_off, int k, int p, int q) {
    if (cv.wide_nch > 0 && cv.lcflat) {
        int a = cv.wide_pos[p], b = cv.wide_pos[q];
        if (a > b) { const int t = a; a = b; b = t; }
        return cv.lcflat[static_cast<size_t>(k) * (cv.wide_nch * kWideChunk) + col_off[b] + a];
    }
    int ti = p / kPillarPad, tj = q / kPillarPad;
    if (ti > tj) { int t = p; p = q; q = t; t = ti; ti = tj; tj = t; }       // (symmetric)
    const int r = p % kPillarPad, c = q % kPillarPad;
    const int lane = (r >> 2) * 8 + (c >> 2), e = (r & 3) * 4 + (c & 3);
    return cv.lc_lanes[((static_cast<size_t>(tj * (tj + 1) / 2 + ti) * cv.Kc + k) * 64 + lane) * kGammaPerLane + e];
}

// col_off[b] of the wide layout's packed triangle: column b starts there (columns padded to an even length)
__device__ __forceinline__ void fill_col_off(int* col_off) {
    col_off[0] = 0;
    for (int b = 0; b < kWidePad; ++b) col_off[b + 1] = col_off[b] + 2 * ((b + 2) / 2);
}

}  // namespace
}  // namespace adr
