// Schedule groups, the store pass: the ladders of the trades of a group from the group's two basis ladders.
//
//   out[t] = cF(t) * BF[g] + cX(t) * BX[g]          (schedule_groups.hpp)
//
// The fast kernel has priced the basis trades of every group (pseudo-trades 2g, 2g + 1 of the basis table) into the batch's
// basis buffers.  Here one wavefront takes one segment - up to R records of ONE group -, loads the group's two ladders once
// (16-byte loads, the lane owning elements 2 lane, 2 lane + 1 of every 128-element band of the flat [P][P] matrix, as in
// the fast kernel's output phase) and then, per record, forms fma(cX, BX, cF * BF) and writes the trade's matrix with
// 16-byte non-temporal stores, 1 KB contiguous per instruction, its delta row and its PV.  The record is wave-uniform
// (scalar loads), so a record costs 16 multiplies, 16 FMAs and 8 stores per lane and no LDS.  An odd pillar count leaves a
// trade's matrix 8-byte aligned only: that case owns single elements (lane + 64 band) and stores 8 bytes.
//
// Negating cF and cX negates every output exactly, doubling them doubles it exactly (one multiply and one FMA per element,
// no other rounding), and the output is as symmetric as the basis matrices are - exactly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.hpp"

namespace adr {

namespace {

typedef double nt_pair __attribute__((ext_vector_type(2)));

constexpr int kCombineThreads = 256;            // 4 wavefronts = 4 segments per block
constexpr int kAggThreads = 1024;               // group_aggregate_kernel: 64 slots x 16 slices of the groups

// PAIR: P even (16-byte path); FULL: P == 32, every band of every lane lies inside the matrix
template <bool PAIR, bool FULL>
__global__ __launch_bounds__(kCombineThreads) void combine_kernel(CombineDev cd, int P, double* __restrict__ pv,
                                                                  double* __restrict__ delta, double* __restrict__ gamma) {
    constexpr int kBands = PAIR ? 8 : 16;       // 32 * 32 / 128, 31 * 31 / 64 rounded up
    constexpr int kWidth = PAIR ? 128 : 64;     // elements of a band
    const int lane = threadIdx.x & 63;
    const int PP = P * P;
    // one segment per wave when the grid covers them all; a smaller (persistent) grid walks them with the grid's stride
    const int64_t stride = static_cast<int64_t>(gridDim.x) * (kCombineThreads / 64);
    for (int64_t s = static_cast<int64_t>(blockIdx.x) * (kCombineThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
         s < cd.n_seg; s += stride) {
        const GroupSegment sg = cd.seg[s];
        const int64_t g2 = 2 * static_cast<int64_t>(sg.group);
        const int at0 = PAIR ? 2 * lane : lane;     // this lane's first element of band 0

        // the group's two ladders, once per segment
        unsigned live = 0;                          // bit b: band b's element (pair) of this lane lies inside the matrix
#pragma unroll
        for (int b = 0; b < kBands; ++b) live |= (FULL || at0 + kWidth * b < PP) ? 1u << b : 0u;
        const double* gf = cd.b_gamma + g2 * PP + at0;
        const double* gx = gf + PP;
        double bf[PAIR ? 2 * kBands : kBands], bx[PAIR ? 2 * kBands : kBands];
#pragma unroll
        for (int b = 0; b < kBands; ++b) {
            if (PAIR) {
                nt_pair f = {0.0, 0.0}, x = {0.0, 0.0};
                if ((live >> b) & 1) {
                    f = *reinterpret_cast<const nt_pair*>(gf + kWidth * b);
                    x = *reinterpret_cast<const nt_pair*>(gx + kWidth * b);
                }
                bf[2 * b] = f.x; bf[2 * b + 1] = f.y; bx[2 * b] = x.x; bx[2 * b + 1] = x.y;
            } else {
                bf[b] = (live >> b) & 1 ? gf[kWidth * b] : 0.0;
                bx[b] = (live >> b) & 1 ? gx[kWidth * b] : 0.0;
            }
        }
        const bool has_delta = delta != nullptr && lane < P;
        const double df = has_delta ? cd.b_delta[g2 * P + lane] : 0.0, dx = has_delta ? cd.b_delta[(g2 + 1) * P + lane] : 0.0;
        const double pf = cd.b_pv[g2], px = cd.b_pv[g2 + 1];

        const GroupRecord* rec = cd.rec + sg.first;
        for (int i = 0; i < sg.count; ++i) {
            const GroupRecord r = rec[i];           // wave-uniform
            double* gm = gamma + static_cast<int64_t>(r.trade) * PP + at0;
#pragma unroll
            for (int b = 0; b < kBands; ++b) {
                if (!FULL && !((live >> b) & 1)) continue;
                if (PAIR) {
                    nt_pair v;
                    v.x = fma(r.cX, bx[2 * b], r.cF * bf[2 * b]);
                    v.y = fma(r.cX, bx[2 * b + 1], r.cF * bf[2 * b + 1]);
                    __builtin_nontemporal_store(v, reinterpret_cast<nt_pair*>(gm + kWidth * b));
                } else {
                    __builtin_nontemporal_store(fma(r.cX, bx[b], r.cF * bf[b]), gm + kWidth * b);
                }
            }
            if (has_delta) __builtin_nontemporal_store(fma(r.cX, dx, r.cF * df), delta + static_cast<int64_t>(r.trade) * P + lane);
            if (pv && lane == 0) pv[r.trade] = fma(r.cX, px, r.cF * pf);
        }
    }
}

// Block (x, y): elements 64 x .. 64 x + 63 of the padded aggregate record [pv, delta[32], gamma[32][32]], summed over the
// groups y, y + S, y + 2 S, ... (S = gridDim.y): thread (e, sl) takes every 16th of them in order, the 16 slices are added in
// order, and the block's sum goes to record `first + y` - stored, or with `add` (one record, S = 1) added to what a launch
// left there.  Records zero_from .. n_slots - 1 are zeroed.  Which group lands in which record depends on the batch and the
// launch plan alone: the same bits on every run.
__global__ __launch_bounds__(kAggThreads) void group_aggregate_kernel(CombineDev cd, int P, double* slots, int first, int add,
                                                                      int zero_from, int n_slots) {
    constexpr int kSlices = kAggThreads / 64;
    __shared__ double part[kSlices][64];
    const int e = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + e;
    const int64_t S = gridDim.y, y = blockIdx.y;
    const double* src = nullptr;                // the element in the ladder of pseudo-trade 0
    int64_t stride = 0;                         // ... and the distance to the next pseudo-trade's
    if (i == 0) {
        src = cd.b_pv; stride = 1;
    } else if (i < 1 + kPillarPad) {
        if (i - 1 < P) { src = cd.b_delta + (i - 1); stride = P; }
    } else if (i < kAggStride) {
        const int r = (i - 1 - kPillarPad) / kPillarPad, q = (i - 1 - kPillarPad) % kPillarPad;
        if (r < P && q < P) { src = cd.b_gamma + r * P + q; stride = static_cast<int64_t>(P) * P; }
    }
    double s = 0.0;
    if (src)
        for (int64_t g = y + S * sl; g < cd.n_groups; g += S * kSlices)
            s += fma(cd.sum_x[g], src[(2 * g + 1) * stride], cd.sum_f[g] * src[2 * g * stride]);
    part[sl][e] = s;
    __syncthreads();
    if (i >= kAggStride) return;
    if (sl == 0) {
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < kSlices; ++k) tot += part[k][e];
        double* dst = slots + static_cast<size_t>(first + y) * kAggStride + i;
        *dst = add ? *dst + tot : tot;
    }
    for (int64_t b = zero_from + y * kSlices + sl; b < n_slots; b += S * kSlices) slots[static_cast<size_t>(b) * kAggStride + i] = 0.0;
}

}  // namespace

hipError_t launch_combine(const CombineDev& cd, int P, double* pv, double* delta, double* gamma, hipStream_t stream) {
    if (cd.n_seg == 0) return hipSuccess;
    if (P < 1 || P > kPillarPad || !gamma) return hipErrorInvalidValue;
    int64_t blocks = (cd.n_seg + kCombineThreads / 64 - 1) / (kCombineThreads / 64);
    if (cd.max_blocks > 0 && blocks > cd.max_blocks) blocks = cd.max_blocks;
    const dim3 grid(static_cast<unsigned>(blocks));
    auto fn = P == kPillarPad ? &combine_kernel<true, true> : (P % 2 == 0 ? &combine_kernel<true, false> : &combine_kernel<false, false>);
    hipLaunchKernelGGL(fn, grid, dim3(kCombineThreads), 0, stream, cd, P, pv, delta, gamma);
    return hipGetLastError();
}

hipError_t launch_group_aggregate(const CombineDev& cd, int P, double* slots, int n_prior, int n_slots, hipStream_t stream) {
    if (P < 1 || P > kPillarPad || n_slots < 1 || n_prior < 0 || n_prior > n_slots) return hipErrorInvalidValue;
    const int free_slots = n_slots - n_prior;
    // as many group slices as there are free records (16 groups per slice and pass), one added into record 0 when none is free
    const int64_t want = (cd.n_groups + kAggThreads / 64 - 1) / (kAggThreads / 64);
    const int S = free_slots == 0 ? 1 : static_cast<int>(std::max<int64_t>(1, std::min<int64_t>({want, free_slots, 256})));
    const int first = free_slots == 0 ? 0 : n_prior;
    hipLaunchKernelGGL(group_aggregate_kernel, dim3((kAggStride + 63) / 64, S), dim3(kAggThreads), 0, stream, cd, P, slots, first,
                       free_slots == 0 ? 1 : 0, free_slots == 0 ? n_slots : first + S, n_slots);
    return hipGetLastError();
}

}  // namespace adr
