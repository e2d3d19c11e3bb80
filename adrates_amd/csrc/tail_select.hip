// VaR and ES of rows of any width (adr_scenario_tail_select*; the rule is adr_scenario_tail's, the contract:
// include/adrates.h): a radix select on the 64-bit keys finds every row's k-th smallest P&L, the values below it are
// gathered into tail[b][k], and subbook.hpp's tail_kernel sorts and adds those k - the kernel adr_scenario_tail runs on
// the whole row, so for rows it takes the bits are its bits.
//
// The keys are key_of's int64 with the sign bit flipped: their UNSIGNED order is the total order of the doubles.  A
// round fixes kDigitBits (11) more bits of the threshold key from the top, six rounds fix all 64 (the last holds nine):
//   count   grid = (segments of a row) x (rows).  A block reads its segment once, forms the keys, and histograms the
//           round's digit of those whose higher bits equal the row's prefix: 2048 bins of uint32 in LDS (8 KiB), integer
//           LDS atomics, so a count does not depend on the order of arrival.  The first round takes every key, and its
//           digit is sign and exponent - a handful of values over a whole wave -, so there a wave first adds up its
//           lanes per distinct digit (ballots, as many steps as the wave holds digits) and one lane adds the sum; it also
//           ORs the row's NaN flag.  The block writes its histogram to work.
//   scan    one block per row adds the segments' histograms in segment order, eight neighbouring bins per thread, scans
//           the 256 partial sums in LDS, and the one thread whose bins hold the k_rem-th key extends the prefix and
//           reduces k_rem.
//   gather  the count grid again: a value whose key is below the threshold key goes to tail[b][slot], slot from a per-row
//           integer counter (any order: the tail is sorted next); the block of segment 0 fills the other k - c slots
//           with the threshold value, c = k - k_rem being known from the scan.
//   tail    tail_kernel on tail[B][k] with base_col = -1, then NaN rows are patched from the flag.
// Every round re-reads the whole row (seven reads of the matrix in all): nothing is compacted, so the scratch is the
// histograms and the tail alone and a round is a pure streaming read.  The kernel boundary is the only
// synchronisation: no flags, no spin-waits, no float atomics.
//
// The ORDERED select (adr_scenario_tail_order*) keeps the scenario index: order[b][k], the first k P&L indices of a row by
// (key, index) ascending - adr_scenario_tail_alloc's order, ties to the lower index.  The six rounds are the same; then
//   gather  writes (key, index) pairs to pairs[b][k].  A pair below the threshold key takes a slot from the row's integer
//           counter (any slot: all of them are taken and the sort places them).  Of the pairs EQUAL to the threshold key
//           exactly the k_rem with the lowest indices are taken, by rank: the ties of the segments before the block's (the
//           last round's histograms hold every segment's count of them), of the 256-element chunks before this one (a
//           running count, uniform over the block) and of the lower lanes of the chunk (a ballot's popcount below the lane,
//           the four waves' counts meeting in LDS).  A tie of rank r < k_rem goes to slot below + r.  What is selected
//           depends on no atomic's return value; a block whose segment holds no tie, or whose ties all rank beyond k_rem,
//           skips the ranking and its barriers.
//   sort    one block per row: the k pairs in LDS, padded with +inf keys to a power of two, alloc_order_kernel's bitonic
//           network; it writes order, var and es (thread 0 adds the k values in order), -1 and NaN for a NaN row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "blocking_call.hpp"
#include "host_pool.hpp"
#include "subbook.hpp"
#include "tail_select.hpp"

namespace adr {
namespace tsel {

using sub::key_of;
using sub::pnl_at;
using sub::value_of;

constexpr int kDigitBits = 11;
constexpr int kBins = 1 << kDigitBits;          // 2048 uint32 = 8 KiB
constexpr int kRounds = 6;                      // 5 x 11 + 9 bits
constexpr int kThreads = 256;
constexpr int kBinsPerThread = kBins / kThreads;
constexpr int kSegMin = 8192;                   // P&L values per segment at least: its histogram is an eighth of its bytes
constexpr int kBlocksWanted = 2048;             // segments x rows aimed at, 8 blocks per CU

// The bits below round r's digit, and the digit's width.
__host__ __device__ inline int shift_of(int r) { return r < kRounds - 1 ? 64 - kDigitBits * (r + 1) : 0; }
__host__ __device__ inline int bits_of(int r) { return r < kRounds - 1 ? kDigitBits : 64 - kDigitBits * (kRounds - 1); }

__host__ __device__ inline uint64_t ukey_of(double v) { return static_cast<uint64_t>(key_of(v)) ^ (uint64_t(1) << 63); }
__host__ __device__ inline double value_of_ukey(uint64_t u) { return value_of(static_cast<int64_t>(u ^ (uint64_t(1) << 63))); }

// A row's state in work: the threshold key's bits fixed so far (right-aligned), what is left of k below them, the NaN
// flag and the gather's slot counter.
struct RowState {
    uint64_t prefix;
    int32_t k_rem, nan, count, pad;
};

// Segments per row (from S_tot, so that adr_scenario_tail_select_work needs no base_col) and a segment's length.
inline int segments(int64_t B, int S_tot) {
    const int64_t by_len = (static_cast<int64_t>(S_tot) + kSegMin - 1) / kSegMin, by_rows = (kBlocksWanted + B - 1) / B;
    return static_cast<int>(std::max<int64_t>(1, std::min(by_len, by_rows)));
}
inline int segment_len(int S_tot, int nseg) { return static_cast<int>((static_cast<int64_t>(S_tot) + nseg - 1) / nseg); }

// work: state[B] | hist[B][nseg][kBins] uint32 | tail[B][k] doubles
struct Layout {
    size_t hist, tail, bytes;
};
inline Layout layout(int64_t B, int S_tot, int k) {
    Layout l;
    l.hist = static_cast<size_t>(B) * sizeof(RowState);
    l.tail = l.hist + static_cast<size_t>(B) * segments(B, S_tot) * kBins * sizeof(uint32_t);
    l.bytes = l.tail + static_cast<size_t>(B) * k * sizeof(double);
    return l;
}

struct Args {
    const double* rows;              // [B][S_tot]
    RowState* state;                 // [B]
    uint32_t* hist;                  // [B][nseg][kBins]
    double* tail;                    // [B][k]
    int64_t S_tot;
    int base_col, m, k, nseg, seg_len;
};

// blockIdx.x = row * nseg + segment.
template <bool kFirst>
__global__ __launch_bounds__(kThreads) void select_count_kernel(Args a, int round) {
    __shared__ uint32_t h[kBins];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / a.nseg;
    const int seg = static_cast<int>(blockIdx.x - b * a.nseg);
    for (int i = tid; i < kBins; i += kThreads) h[i] = 0;
    __syncthreads();
    const double* row = a.rows + b * a.S_tot;
    const int e0 = seg * a.seg_len, e1 = a.m - e0 < a.seg_len ? a.m : e0 + a.seg_len;
    const int shift = shift_of(round);
    const uint32_t mask = (1u << bits_of(round)) - 1u;
    const uint64_t prefix = kFirst ? 0 : a.state[b].prefix;         // uniform: a scalar load
    int nan = 0;
    for (int64_t base = e0; base < e1; base += kThreads) {          // uniform bounds: whole waves stay in the loop
        const bool in = base + tid < e1;
        const double v = in ? pnl_at(row, a.base_col, static_cast<int>(base + tid)) : 0.0;
        const uint64_t u = ukey_of(v);
        const uint32_t d = static_cast<uint32_t>(u >> shift) & mask;
        if (kFirst) {
            nan |= v != v;
            uint64_t todo = __ballot(in);
            while (todo) {                                          // one step per distinct digit of the wave
                const int lead = __ffsll(static_cast<long long>(todo)) - 1;
                const uint32_t d0 = __shfl(d, lead);
                const uint64_t same = __ballot(in && d == d0) & todo;
                if ((tid & 63) == lead) atomicAdd(&h[d0], static_cast<uint32_t>(__popcll(same)));
                todo &= ~same;
            }
        } else if (in && (u >> shift >> bits_of(round)) == prefix) {
            atomicAdd(&h[d], 1u);
        }
    }
    if (kFirst && nan) atomicOr(&a.state[b].nan, 1);
    __syncthreads();
    uint32_t* out = a.hist + static_cast<size_t>(blockIdx.x) * kBins;
    for (int i = tid; i < kBins; i += kThreads) out[i] = h[i];
}

// blockIdx.x = row.  k_rem is k in the first round (the state has been zeroed).
__global__ __launch_bounds__(kThreads) void select_scan_kernel(Args a, int round) {
    __shared__ uint32_t part[kThreads];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const uint32_t* hist = a.hist + static_cast<size_t>(b) * a.nseg * kBins + tid * kBinsPerThread;
    // the state is read here, before the barriers below, and written behind them by one thread
    const uint32_t k_rem = static_cast<uint32_t>(round == 0 ? a.k : a.state[b].k_rem);
    const uint64_t prefix = round == 0 ? 0 : a.state[b].prefix;
    uint32_t c[kBinsPerThread];
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) c[i] = 0;
    for (int seg = 0; seg < a.nseg; ++seg) {
        const uint4 lo = *reinterpret_cast<const uint4*>(hist + static_cast<size_t>(seg) * kBins);
        const uint4 hi = *reinterpret_cast<const uint4*>(hist + static_cast<size_t>(seg) * kBins + 4);
        c[0] += lo.x; c[1] += lo.y; c[2] += lo.z; c[3] += lo.w;
        c[4] += hi.x; c[5] += hi.y; c[6] += hi.z; c[7] += hi.w;
    }
    uint32_t own = 0;
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) own += c[i];
    part[tid] = own;
    __syncthreads();
    for (int step = 1; step < kThreads; step <<= 1) {               // inclusive scan of the 256 partial sums
        const uint32_t add = tid >= step ? part[tid - step] : 0u;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    uint32_t below = part[tid] - own;                               // keys in the bins before this thread's
    if (below < k_rem && k_rem <= below + own) {                    // exactly one thread: the counts add up to >= k_rem
        int bin = kBinsPerThread - 1;
        bool found = false;
#pragma unroll
        for (int i = 0; i < kBinsPerThread; ++i) {                  // unrolled: c[] stays in registers
            if (!found && below + c[i] >= k_rem) {
                bin = i;
                found = true;
            }
            if (!found) below += c[i];
        }
        a.state[b].prefix = (prefix << bits_of(round)) | static_cast<uint64_t>(tid * kBinsPerThread + bin);
        a.state[b].k_rem = static_cast<int32_t>(k_rem - below);
    }
}
static_assert(kBinsPerThread == 8, "select_scan_kernel reads two uint4");

// blockIdx.x = row * nseg + segment; the prefix is the whole threshold key now.
__global__ __launch_bounds__(kThreads) void select_gather_kernel(Args a) {
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / a.nseg;
    const int seg = static_cast<int>(blockIdx.x - b * a.nseg);
    const double* row = a.rows + b * a.S_tot;
    const int e0 = seg * a.seg_len, e1 = a.m - e0 < a.seg_len ? a.m : e0 + a.seg_len;
    const uint64_t thr = a.state[b].prefix;                         // uniform: scalar loads
    const int below = a.k - a.state[b].k_rem;                       // the keys under the threshold: fewer than k
    double* tail = a.tail + b * a.k;
    for (int64_t e = static_cast<int64_t>(e0) + tid; e < e1; e += kThreads) {
        const double v = pnl_at(row, a.base_col, static_cast<int>(e));
        if (ukey_of(v) < thr) {
            const int slot = atomicAdd(&a.state[b].count, 1);
            if (slot < below) tail[slot] = v;                       // always, unless the counts were wrong: never out of bounds
        }
    }
    if (seg == 0) {
        const double t = value_of_ukey(thr);
        for (int i = below + tid; i < a.k; i += kThreads) tail[i] = t;
    }
}

__global__ __launch_bounds__(kThreads) void select_nan_kernel(const RowState* state, int64_t B, double* var, double* es) {
    const int64_t b = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (b < B && state[b].nan) {
        var[b] = NAN;
        es[b] = NAN;
    }
}

// ------------------------------------------------------------------------------------------------------ ordered select
using sub::KeyIdx;
constexpr int kWaves = kThreads / 64;

// blockIdx.x = row * nseg + segment; the prefix is the whole threshold key and hist still holds the last round's counts.
__global__ __launch_bounds__(kThreads) void order_gather_kernel(Args a, KeyIdx* pairs_all) {
    __shared__ uint32_t wave_part[kWaves];
    __shared__ uint32_t wave_ties[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x / a.nseg;
    const int seg = static_cast<int>(blockIdx.x - b * a.nseg);
    const double* row = a.rows + b * a.S_tot;
    const int e0 = seg * a.seg_len, e1 = a.m - e0 < a.seg_len ? a.m : e0 + a.seg_len;
    const uint64_t thr = a.state[b].prefix;                         // uniform: scalar loads
    const uint32_t k_rem = static_cast<uint32_t>(a.state[b].k_rem); // 1 .. the ties of the row
    const int below = a.k - static_cast<int>(k_rem);                // the keys under the threshold: fewer than k
    KeyIdx* pairs = pairs_all + b * a.k;
    // the ties of the segments before this one, and this segment's own: the last round's bin of the threshold's digit
    const uint32_t* ties_of = a.hist + static_cast<size_t>(b) * a.nseg * kBins + (static_cast<uint32_t>(thr) & ((1u << bits_of(kRounds - 1)) - 1u));
    uint32_t part = 0;
    for (int s = tid; s < seg; s += kThreads) part += ties_of[static_cast<size_t>(s) * kBins];
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
    if (lane == 0) wave_part[wave] = part;
    __syncthreads();
    uint32_t run = 0;                                               // the ties before the chunk: uniform over the block
    for (int w = 0; w < kWaves; ++w) run += wave_part[w];
    const bool rank_ties = ties_of[static_cast<size_t>(seg) * kBins] != 0 && run < k_rem;   // uniform
    for (int64_t base = e0; base < e1; base += kThreads) {          // uniform bounds: whole waves stay in the loop
        const int64_t e = base + tid;
        const bool in = e < e1;
        const double v = in ? pnl_at(row, a.base_col, static_cast<int>(e)) : 0.0;
        const uint64_t u = ukey_of(v);
        if (in && u < thr) {
            const int slot = atomicAdd(&a.state[b].count, 1);
            if (slot < below) pairs[slot] = KeyIdx{key_of(v), e};   // always, unless the counts were wrong: never out of bounds
        }
        if (rank_ties && run < k_rem) {                             // uniform: the barriers are met by every wave
            const bool tie = in && u == thr;
            const uint64_t mates = __ballot(tie);
            if (lane == 0) wave_ties[wave] = static_cast<uint32_t>(__popcll(mates));
            __syncthreads();
            uint32_t before = 0, chunk = 0;
            for (int w = 0; w < kWaves; ++w) {
                const uint32_t c = wave_ties[w];
                before += w < wave ? c : 0u;
                chunk += c;
            }
            const uint32_t r = run + before + static_cast<uint32_t>(__popcll(mates & ((uint64_t(1) << lane) - 1)));
            if (tie && r < k_rem) pairs[below + r] = KeyIdx{key_of(v), e};          // below + r < k
            run += chunk;
            __syncthreads();                                        // wave_ties is written again in the next chunk
        }
    }
}

// blockIdx.x = row.  P = the power of two >= k (the LDS holds P pairs; the padding is +inf behind every index).
__global__ __launch_bounds__(1024) void order_sort_kernel(const KeyIdx* pairs_all, const RowState* state, int k, int P, int64_t* order_all,
                                                          double* var, double* es) {
    extern __shared__ KeyIdx pairs[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t b = blockIdx.x;
    int64_t* order = order_all + b * k;
    if (state[b].nan) {                                             // uniform: a scalar load
        for (int i = tid; i < k; i += nt) order[i] = -1;
        if (tid == 0) {
            var[b] = NAN;
            es[b] = NAN;
        }
        return;
    }
    const KeyIdx* in = pairs_all + b * k;
    for (int e = tid; e < P; e += nt) pairs[e] = e < k ? in[e] : KeyIdx{key_of(INFINITY), INT64_MAX};
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += nt) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const KeyIdx x = pairs[lo], y = pairs[hi];
                if (sub::after(x, y) == ((lo & size) == 0)) {
                    pairs[lo] = y;
                    pairs[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += nt) order[i] = pairs[i].idx;
    if (tid == 0) sub::total_of_sorted(pairs, k, var + b, es + b);
}

// -------------------------------------------------------------------------------------------------------------- host
// The limit of both is on the tail: its k values, or its k (key, index) pairs, are sorted in LDS.
int check(const std::string& w, int64_t B, int S_tot, int base_col, int k) {
    return sub::check_sizes(w, B, S_tot, base_col, k,
                            sub::TailLimit{true, ADR_SCENARIO_TAIL_MAX, "a tail of ",
                                           " P&L values; a tail of at most ADR_SCENARIO_TAIL_MAX (16384) fits the LDS"});
}
int check_order(const std::string& w, int64_t B, int S_tot, int base_col, int k) {
    return sub::check_sizes(w, B, S_tot, base_col, k,
                            sub::TailLimit{true, ADR_SCENARIO_ALLOC_MAX, "a tail of ",
                                           " P&L values; a tail of at most ADR_SCENARIO_ALLOC_MAX (8192) (key, index) pairs fits the LDS"});
}

// What both selects start with: the refusal of a grid past 2^31, the kernels' arguments over `work` (the histograms at
// `hist_at`; `tail` is null for the ordered select) and the six rounds that leave every row's threshold key in its state.
int check_grid(const std::string& w, int64_t B, int S_tot) {
    if (B * segments(B, S_tot) > INT32_MAX) return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": more than 2^31 (row, segment) pairs in one launch");
    return ADR_OK;
}
inline Args args_over(const double* rows, int64_t B, int S_tot, int base_col, int k, char* work, size_t hist_at, double* tail) {
    const int nseg = segments(B, S_tot);
    return Args{rows, reinterpret_cast<RowState*>(work), reinterpret_cast<uint32_t*>(work + hist_at), tail,
                S_tot, base_col, base_col >= 0 ? S_tot - 1 : S_tot, k, nseg, segment_len(S_tot, nseg)};
}
inline dim3 pairs_grid(int64_t B, const Args& a) { return dim3(static_cast<unsigned>(B * a.nseg)); }
hipError_t enqueue_rounds(const Args& a, int64_t B, hipStream_t stream) {
    const dim3 grid = pairs_grid(B, a), rows_grid(static_cast<unsigned>(B)), block(kThreads);
    hipError_t e = hipMemsetAsync(a.state, 0, static_cast<size_t>(B) * sizeof(RowState), stream);
    for (int r = 0; r < kRounds && e == hipSuccess; ++r) {
        if (r == 0) hipLaunchKernelGGL(select_count_kernel<true>, grid, block, 0, stream, a, r);
        else hipLaunchKernelGGL(select_count_kernel<false>, grid, block, 0, stream, a, r);
        hipLaunchKernelGGL(select_scan_kernel, rows_grid, block, 0, stream, a, r);
        e = hipGetLastError();
    }
    return e;
}

// The chain on `stream`; every pointer is device memory, `work` holds layout(B, S_tot, k).bytes.
int enqueue(const std::string& w, const double* rows, int64_t B, int S_tot, int base_col, int k, double* var, double* es, void* work,
            hipStream_t stream) {
    const int rc = check_grid(w, B, S_tot);
    if (rc != ADR_OK) return rc;
    const Layout l = layout(B, S_tot, k);
    char* base = static_cast<char*>(work);
    const Args a = args_over(rows, B, S_tot, base_col, k, base, l.hist, reinterpret_cast<double*>(base + l.tail));
    const dim3 block(kThreads);
    hipError_t e = enqueue_rounds(a, B, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(select_gather_kernel, pairs_grid(B, a), block, 0, stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = sub::enqueue_tail(a.tail, B, k, -1, k, var, es, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(select_nan_kernel, dim3(static_cast<unsigned>((B + kThreads - 1) / kThreads)), block, 0, stream, a.state, B,
                           var, es);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

// work of the ordered select: state[B] | hist[B][nseg][kBins] uint32 | (to a multiple of 16) pairs[B][k].  Layout's
// `tail` is where the pairs start.
inline Layout order_layout(int64_t B, int S_tot, int k) {
    Layout l = layout(B, S_tot, 0);
    l.tail = (l.tail + 15) / 16 * 16;
    l.bytes = l.tail + static_cast<size_t>(B) * k * sizeof(KeyIdx);
    return l;
}
size_t order_work_bytes(int64_t B, int S_tot, int k) { return order_layout(B, S_tot, k).bytes; }

int enqueue_order(const std::string& w, const double* rows, int64_t B, int S_tot, int base_col, int k, int64_t* order, double* var,
                  double* es, void* work, hipStream_t stream) {
    const int rc = check_grid(w, B, S_tot);
    if (rc != ADR_OK) return rc;
    const Layout l = order_layout(B, S_tot, k);
    char* base = static_cast<char*>(work);
    const Args a = args_over(rows, B, S_tot, base_col, k, base, l.hist, nullptr);
    const dim3 rows_grid(static_cast<unsigned>(B)), block(kThreads);
    KeyIdx* pairs = reinterpret_cast<KeyIdx*>(base + l.tail);
    hipError_t e = enqueue_rounds(a, B, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(order_gather_kernel, pairs_grid(B, a), block, 0, stream, a, pairs);
        e = hipGetLastError();
    }
    const int P = sub::pow2_at_least(k);
    const size_t lds = static_cast<size_t>(P) * sizeof(KeyIdx);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&order_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(lds));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(order_sort_kernel, rows_grid, dim3(std::min(1024, std::max(64, P / 2))), lds, stream, pairs, a.state, k, P, order,
                           var, es);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

void order_host(const double* rows, int64_t B, int S_tot, int base_col, int k, int64_t* order, double* var, double* es) {
    const int m = base_col >= 0 ? S_tot - 1 : S_tot;
    const auto before = [](const KeyIdx& x, const KeyIdx& y) { return sub::after(y, x); };
    adr::parallel_ranges(B, adr::pool_threads(B, 4), [&](int, int64_t lo, int64_t hi) {
        std::vector<KeyIdx> pairs(static_cast<size_t>(m));
        for (int64_t b = lo; b < hi; ++b) {
            const double* row = rows + b * S_tot;
            bool nan = false;
            for (int e = 0; e < m; ++e) {
                const double v = pnl_at(row, base_col, e);
                nan |= v != v;
                pairs[e] = KeyIdx{key_of(v), e};
            }
            if (nan) {
                var[b] = es[b] = NAN;
                std::fill(order + b * k, order + (b + 1) * k, int64_t(-1));
                continue;
            }
            std::nth_element(pairs.begin(), pairs.begin() + (k - 1), pairs.end(), before);
            std::sort(pairs.begin(), pairs.begin() + k, before);
            for (int i = 0; i < k; ++i) order[b * k + i] = pairs[i].idx;
            sub::total_of_sorted(pairs.data(), k, var + b, es + b);
        }
    });
}

}  // namespace tsel
}  // namespace adr

namespace TS = adr::tsel;

extern "C" {

int64_t adr_scenario_tail_select_work(int64_t B, int S_tot, int k) {
    if (B < 1 || S_tot < 1 || k < 1 || k > ADR_SCENARIO_TAIL_MAX) return 0;
    return static_cast<int64_t>(TS::layout(B, S_tot, k).bytes);
}

int adr_scenario_tail_select_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, int k, double* var_dev,
                                 double* es_dev, void* work_dev, void* stream) {
    const std::string w = "adr_scenario_tail_select_dev";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = TS::check(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows_dev || !var_dev || !es_dev) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    if (!work_dev) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (adr_scenario_tail_select_work bytes are needed)");
    hipStream_t st = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &st);
    if (rc != ADR_OK) return rc;
    return TS::enqueue(w, rows_dev, B, S_tot, base_col, k, var_dev, es_dev, work_dev, st);
}

int adr_scenario_tail_select(adr_ctx* ctx, int64_t B, int S_tot, const double* rows, int base_col, int k, double* var, double* es) {
    const std::string w = "adr_scenario_tail_select";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = TS::check(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows || !var || !es) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    double *drows, *dvar, *des;
    void* dwork;
    adr::call::Staging mem;
    mem.in(&drows, rows, static_cast<size_t>(B) * S_tot);
    mem.out(&dvar, var, B);
    mem.out(&des, es, B);
    mem.scratch_bytes(&dwork, TS::layout(B, S_tot, k).bytes);
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess) rc = TS::enqueue(w, drows, B, S_tot, base_col, k, dvar, des, dwork, stream);
    return mem.finish(w, rc, e, stream);
}

int64_t adr_scenario_tail_order_work(int64_t B, int S_tot, int k) {
    if (B < 1 || S_tot < 1 || k < 1 || k > ADR_SCENARIO_ALLOC_MAX) return 0;
    return static_cast<int64_t>(TS::order_work_bytes(B, S_tot, k));
}

int adr_scenario_tail_order_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, int k, int64_t* order_dev,
                                double* var_dev, double* es_dev, void* work_dev, void* stream) {
    const std::string w = "adr_scenario_tail_order_dev";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = TS::check_order(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows_dev || !order_dev || !var_dev || !es_dev) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    if (!work_dev) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (adr_scenario_tail_order_work bytes are needed)");
    hipStream_t st = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &st);
    if (rc != ADR_OK) return rc;
    return TS::enqueue_order(w, rows_dev, B, S_tot, base_col, k, order_dev, var_dev, es_dev, work_dev, st);
}

int adr_scenario_tail_order(adr_ctx* ctx, int64_t B, int S_tot, const double* rows, int base_col, int k, int64_t* order, double* var,
                            double* es) {
    const std::string w = "adr_scenario_tail_order";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = TS::check_order(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows || !order || !var || !es) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    double *drows, *dvar, *des;
    int64_t* dorder;
    void* dwork;
    adr::call::Staging mem;
    mem.in(&drows, rows, static_cast<size_t>(B) * S_tot);
    mem.out(&dorder, order, static_cast<size_t>(B) * k);
    mem.out(&dvar, var, B);
    mem.out(&des, es, B);
    mem.scratch_bytes(&dwork, TS::order_work_bytes(B, S_tot, k));
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess) rc = TS::enqueue_order(w, drows, B, S_tot, base_col, k, dorder, dvar, des, dwork, stream);
    return mem.finish(w, rc, e, stream);
}

int adr_scenario_tail_order_host(int64_t B, int S_tot, const double* rows, int base_col, int k, int64_t* order, double* var, double* es) {
    const std::string w = "adr_scenario_tail_order_host";
    const int rc = TS::check_order(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows || !order || !var || !es) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    TS::order_host(rows, B, S_tot, base_col, k, order, var, es);
    return ADR_OK;
}

int adr_scenario_tail_select_host(int64_t B, int S_tot, const double* rows, int base_col, int k, double* var, double* es) {
    const std::string w = "adr_scenario_tail_select_host";
    const int rc = TS::check(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows || !var || !es) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    const int m = base_col >= 0 ? S_tot - 1 : S_tot;
    adr::parallel_ranges(B, adr::pool_threads(B, 4), [&](int, int64_t lo, int64_t hi) {
        std::vector<int64_t> keys(static_cast<size_t>(m));
        for (int64_t b = lo; b < hi; ++b) {
            const double* row = rows + b * S_tot;
            bool nan = false;
            for (int e = 0; e < m; ++e) {
                const double v = adr::sub::pnl_at(row, base_col, e);
                nan |= v != v;
                keys[e] = adr::sub::key_of(v);
            }
            if (nan) {
                var[b] = es[b] = NAN;
                continue;
            }
            std::nth_element(keys.begin(), keys.begin() + (k - 1), keys.end());
            std::sort(keys.begin(), keys.begin() + k);
            adr::sub::tail_of_sorted(keys.data(), k, var + b, es + b);
        }
    });
    return ADR_OK;
}

}  // extern "C"
