// Sub-books of a scenario revaluation: per-desk, per-counterparty or per-account P&L vectors from ONE launch of the
// pricing kernels (adr_scenario_subbook_pv*, adr_credit_scenario_subbook_pv*), and their tail measures
// (adr_scenario_tail*).  Declarations and semantics: include/adrates.h.
//
// The pricing kernels cut the batch into chunks at sub-book boundaries (the plan below) and write work[chunk][S] as
// they always do.  The sum kernel here then adds every sub-book's chunk rows in the parent's order - chunk j of the
// sub-book to slot j % 64 in order, then a halving tree - so that a row has the bits of the parent's book_pv on that
// sub-book alone.  One wave = one (sub-book, 64 scenarios) pair, lane = scenario: a chunk row is one coalesced 512-byte
// read, the 64 slots are registers of the lane (the inner 64 is unrolled) and the tree runs in them: no LDS, no
// barrier, no atomics.  A sub-book of more than kBigChunks chunks (a whole book as ONE sub-book has 15 625) would keep
// that one wave busy for milliseconds, so it is left to a second kernel: one block per pair, 16 waves with four slots
// each, the slots meeting in LDS for the same tree.  Both kernels are always enqueued (the host of a _dev call does not
// see the plan) and each leaves the other's pairs alone.
//
// The tail kernel: one block per row.  The P&L values go to LDS as order-preserving integer keys, padded with +inf to a
// power of two, and a bitonic network sorts them; thread 0 then adds the k smallest in ascending order.  The keys make
// the order total (-0.0 before +0.0), so the host twin's std::sort gives the same sequence.
//
// The tail allocation (adr_scenario_tail_alloc*): the firm's total per scenario, the scenarios ordered by it, and every
// row's P&L over the firm's k worst scenarios - see the section below.
#include "subbook.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/adrates.h"
#include "host_pool.hpp"
#include "scenario_common.hpp"

#pragma clang fp contract(off)

namespace adr {
namespace scen {

// The whole book's sum, the parent of the sub-book sums below: book[e] = the fixed-order sum of the chunk rows
// (scenario_common.hpp; reduce_chunks is its host form).
__global__ __launch_bounds__(kRedLanes * kRedEntries) void scenario_book_kernel(const double* work, int64_t chunks, int64_t S,
                                                                                double* book) {
    __shared__ double sh[kRedLanes][kRedEntries];
    const int ei = threadIdx.x % kRedEntries, cl = threadIdx.x / kRedEntries;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kRedEntries + ei;
    double acc = 0.0;
    if (e < S) {
#pragma unroll 8
        for (int64_t j = cl; j < chunks; j += kRedLanes) acc = acc + work[j * S + e];
    }
    sh[cl][ei] = acc;
    __syncthreads();
    for (int h = kRedLanes / 2; h >= 1; h >>= 1) {
        if (cl < h) sh[cl][ei] = sh[cl][ei] + sh[cl + h][ei];
        __syncthreads();
    }
    if (cl == 0 && e < S) book[e] = sh[0][ei];
}

hipError_t enqueue_book_sum(const double* work, int64_t chunks, int S, double* book, hipStream_t stream) {
    hipLaunchKernelGGL(scenario_book_kernel, dim3(static_cast<unsigned>((S + kRedEntries - 1) / kRedEntries)),
                       dim3(kRedLanes * kRedEntries), 0, stream, work, chunks, static_cast<int64_t>(S), book);
    return hipGetLastError();
}

void reduce_chunks(const double* work, int64_t chunks, int64_t S, double* book) {
    for (int64_t e = 0; e < S; ++e) {
        double p[kRedLanes];
        for (int cl = 0; cl < kRedLanes; ++cl) {
            p[cl] = 0.0;
            for (int64_t j = cl; j < chunks; j += kRedLanes) p[cl] = p[cl] + work[j * S + e];
        }
        for (int h = kRedLanes / 2; h >= 1; h >>= 1)
            for (int cl = 0; cl < h; ++cl) p[cl] = p[cl] + p[cl + h];
        book[e] = p[0];
    }
}

}  // namespace scen

namespace sub {

using scen::kChunk;
using scen::kWave;
constexpr int kSlots = 64;                      // the parent's reduction slots
constexpr int kSumWaves = 4;                    // (sub-book, group) pairs per block of the sum kernel
constexpr int kBigChunks = 64;                  // above (the slot index wraps): the block-per-pair kernel
constexpr int kBigWaves = 16;                   // its waves, kSlots / kBigWaves slots each

int check_offsets(const std::string& w, int64_t n, int64_t B, const int64_t* sub_off) {
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    if (!sub_off) return adr_set_error(ADR_ERR_INVALID, w + ": sub_off is NULL");
    if (sub_off[0] != 0) return adr_set_error(ADR_ERR_INVALID, w + ": sub_off must start at 0 (sub-book 0 starts at " +
                                                                std::to_string(sub_off[0]) + ")");
    for (int64_t b = 0; b < B; ++b)
        if (sub_off[b + 1] < sub_off[b])
            return adr_set_error(ADR_ERR_INVALID, w + ": sub_off decreases at sub-book " + std::to_string(b) + " (" +
                                                      std::to_string(sub_off[b]) + " .. " + std::to_string(sub_off[b + 1]) + ")");
    if (sub_off[B] != n)
        return adr_set_error(ADR_ERR_INVALID, w + ": sub_off must end at the trade count " + std::to_string(n) + " (sub-book " +
                                                  std::to_string(B - 1) + " ends at " + std::to_string(sub_off[B]) + ")");
    return ADR_OK;
}

int build_plan(const std::string& w, int64_t n, int64_t B, const int64_t* sub_off, std::vector<int64_t>& plan) {
    const int rc = check_offsets(w, n, B, sub_off);
    if (rc != ADR_OK) return rc;
    plan.resize(static_cast<size_t>(adr_scenario_subbook_plan(n, B, sub_off, nullptr)));
    adr_scenario_subbook_plan(n, B, sub_off, plan.data());
    return ADR_OK;
}

__global__ __launch_bounds__(kWave * kSumWaves) void subbook_sum_kernel(const double* work, const int64_t* chunk_off,
                                                                        int64_t chunk_cap, int64_t B, int S, int groups,
                                                                        double* sub_pv) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t pair = static_cast<int64_t>(blockIdx.x) * kSumWaves + wave;
    if (pair >= B * groups) return;
    const int64_t b = pair / groups;
    const int64_t s = (pair % groups) * kWave + lane;
    int64_t c0 = chunk_off[b], c1 = chunk_off[b + 1];      // uniform: scalar loads
    c0 = c0 < 0 ? 0 : c0;
    c1 = c1 > chunk_cap ? chunk_cap : c1;
    if (s >= S || c1 - c0 > kBigChunks) return;
    const double* col = work + s;
    double p[kSlots];
#pragma unroll
    for (int q = 0; q < kSlots; ++q) p[q] = 0.0;
    for (int64_t base = c0; base < c1; base += kSlots) {
#pragma unroll
        for (int q = 0; q < kSlots; ++q)
            if (base + q < c1) p[q] = p[q] + col[(base + q) * S];
    }
#pragma unroll
    for (int h = kSlots / 2; h >= 1; h >>= 1) {
#pragma unroll
        for (int q = 0; q < h; ++q) p[q] = p[q] + p[q + h];
    }
    sub_pv[b * S + s] = p[0];
}

// The same sum for the pairs of sub-books with more than kBigChunks chunks: wave w owns the slots 4 w .. 4 w + 3.
__global__ __launch_bounds__(kWave * kBigWaves) void subbook_sum_big_kernel(const double* work, const int64_t* chunk_off,
                                                                            int64_t chunk_cap, int S, int groups, double* sub_pv) {
    constexpr int kOwn = kSlots / kBigWaves;
    __shared__ double sh[kSlots][kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t b = blockIdx.x / groups;
    int64_t c0 = chunk_off[b], c1 = chunk_off[b + 1];      // uniform: scalar loads
    c0 = c0 < 0 ? 0 : c0;
    c1 = c1 > chunk_cap ? chunk_cap : c1;
    if (c1 - c0 <= kBigChunks) return;                      // uniform over the block
    const int64_t s = static_cast<int64_t>(blockIdx.x % groups) * kWave + lane;
    const double* col = work + (s < S ? s : S - 1);         // padding lanes add the last scenario and store nothing
    double p[kOwn];
#pragma unroll
    for (int i = 0; i < kOwn; ++i) p[i] = 0.0;
#pragma unroll 4
    for (int64_t base = c0 + wave * kOwn; base < c1; base += kSlots) {
#pragma unroll
        for (int i = 0; i < kOwn; ++i)
            if (base + i < c1) p[i] = p[i] + col[(base + i) * S];
    }
#pragma unroll
    for (int i = 0; i < kOwn; ++i) sh[wave * kOwn + i][lane] = p[i];
    __syncthreads();
    if (wave != 0) return;
    double q[kSlots];
#pragma unroll
    for (int i = 0; i < kSlots; ++i) q[i] = sh[i][lane];
#pragma unroll
    for (int h = kSlots / 2; h >= 1; h >>= 1) {
#pragma unroll
        for (int i = 0; i < h; ++i) q[i] = q[i] + q[i + h];
    }
    if (s < S) sub_pv[b * S + s] = q[0];
}

hipError_t enqueue_sum(const double* work, const int64_t* chunk_off, int64_t chunk_cap, int64_t B, int S, double* sub_pv,
                       hipStream_t stream) {
    const int groups = (S + kWave - 1) / kWave;
    const int64_t blocks = (B * groups + kSumWaves - 1) / kSumWaves;
    if (blocks > INT32_MAX) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(subbook_sum_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kWave * kSumWaves), 0, stream, work,
                       chunk_off, chunk_cap, B, S, groups, sub_pv);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (B * groups > INT32_MAX) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(subbook_sum_big_kernel, dim3(static_cast<unsigned>(B * groups)), dim3(kWave * kBigWaves), 0, stream, work,
                       chunk_off, chunk_cap, S, groups, sub_pv);
    return hipGetLastError();
}

void reduce_subbooks(const double* work, const int64_t* chunk_off, int64_t B, int64_t S, double* sub_pv) {
    for (int64_t b = 0; b < B; ++b) {
        const int64_t c0 = chunk_off[b], c1 = chunk_off[b + 1];
        for (int64_t e = 0; e < S; ++e) {
            double p[kSlots];
            for (int q = 0; q < kSlots; ++q) {
                p[q] = 0.0;
                for (int64_t j = c0 + q; j < c1; j += kSlots) p[q] = p[q] + work[j * S + e];
            }
            for (int h = kSlots / 2; h >= 1; h >>= 1)
                for (int q = 0; q < h; ++q) p[q] = p[q] + p[q + h];
            sub_pv[b * S + e] = p[0];
        }
    }
}

// ------------------------------------------------------------------------------------------------------ tail measures
// key_of, value_of, pnl_at, tail_of_sorted, tail_kernel and enqueue_tail: subbook.hpp (adr_scenario_tail_select* runs them too).
int check_sizes(const std::string& w, int64_t B, int S_tot, int base_col, int k, const TailLimit& limit) {
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one row is needed");
    if (S_tot < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one column is needed");
    if (base_col < -1 || base_col >= S_tot)
        return adr_set_error(ADR_ERR_INVALID, w + ": base_col must be -1 (the rows are P&L) or a column, 0 .. " +
                                                  std::to_string(S_tot - 1));
    const int m = base_col >= 0 ? S_tot - 1 : S_tot;
    if (m < 1) return adr_set_error(ADR_ERR_INVALID, w + ": no P&L value is left beside the base column");
    if (k < 1 || k > m)
        return adr_set_error(ADR_ERR_INVALID, w + ": k must lie in 1 .. " + std::to_string(m) + " (the P&L values per row)");
    const int limited = limit.on_tail ? k : m;
    if (limited > limit.max)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": " + limit.before + std::to_string(limited) + limit.after);
    return ADR_OK;
}
int check_tail(const std::string& w, int64_t B, int S_tot, int base_col, int k) {
    return check_sizes(w, B, S_tot, base_col, k,
                       TailLimit{false, ADR_SCENARIO_TAIL_MAX, "", " P&L values per row; a row of at most ADR_SCENARIO_TAIL_MAX (16384) fits the LDS"});
}

// ---------------------------------------------------------------------------------------------------- tail allocation
// The Euler allocation of the firm's tail to the rows (adr_scenario_tail_alloc*), three kernels in one chain:
//   1. tot[e] = the fixed-order sum over the rows of pnl[b][e]: row b to slot b % 64 in order, then the halving tree -
//      scenario_book_kernel's shape, 64 slots x 16 scenarios per block, so a slot's chain is B / 64 adds long;
//   2. one block orders the scenarios by (key(tot[e]), e) with a bitonic network over (key, index) pairs in LDS, adds
//      the firm's tail and leaves the first k indices where tot was (the scratch is S_tot doubles, k <= S_tot);
//   3. one thread per row adds the row's P&L over those k scenarios in that order.
// A NaN total is passed on as index -1 in the first slot; every output is then NaN.
// KeyIdx, after, total_of_sorted and components_of: subbook.hpp (tail_order.hip shares them).
__global__ __launch_bounds__(scen::kRedLanes * scen::kRedEntries) void alloc_total_kernel(const double* rows, int64_t B, int64_t S_tot,
                                                                                          int base_col, int m, double* tot) {
    constexpr int kLanes = scen::kRedLanes, kEntries = scen::kRedEntries;
    __shared__ double sh[kLanes][kEntries];
    const int ei = threadIdx.x % kEntries, cl = threadIdx.x / kEntries;
    const int e = blockIdx.x * kEntries + ei;
    double acc = 0.0;
    if (e < m) {
#pragma unroll 8
        for (int64_t b = cl; b < B; b += kLanes) acc = acc + pnl_at(rows + b * S_tot, base_col, e);
    }
    sh[cl][ei] = acc;
    __syncthreads();
    for (int h = kLanes / 2; h >= 1; h >>= 1) {
        if (cl < h) sh[cl][ei] = sh[cl][ei] + sh[cl + h][ei];
        __syncthreads();
    }
    if (cl == 0 && e < m) tot[e] = sh[0][ei];
}

// m totals, P = the power of two >= m (the LDS holds P pairs; the padding is +inf with indices m .. P - 1, behind
// every total).  `tot` comes in as doubles and goes out as the first k scenario indices, int64.
__global__ __launch_bounds__(1024) void alloc_order_kernel(double* tot, int m, int P, int k, double* var_tot, double* es_tot) {
    extern __shared__ KeyIdx pairs[];
    const int tid = threadIdx.x, nt = blockDim.x;
    int nan = 0;
    for (int e = tid; e < P; e += nt) {
        double v = INFINITY;
        if (e < m) {
            v = tot[e];
            nan |= v != v;
        }
        pairs[e] = KeyIdx{key_of(v), e};
    }
    int64_t* order = reinterpret_cast<int64_t*>(tot);
    if (__syncthreads_or(nan)) {                    // uniform over the block; every total has been read
        if (tid == 0) {
            order[0] = -1;
            *var_tot = NAN;
            *es_tot = NAN;
        }
        return;
    }
    for (int size = 2; size <= P; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += nt) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const KeyIdx a = pairs[lo], b = pairs[hi];
                if (after(a, b) == ((lo & size) == 0)) {
                    pairs[lo] = b;
                    pairs[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += nt) order[i] = pairs[i].idx;
    if (tid == 0) total_of_sorted(pairs, k, var_tot, es_tot);
}

__global__ __launch_bounds__(256) void alloc_rows_kernel(const double* rows, int64_t B, int64_t S_tot, int base_col, int m,
                                                         const int64_t* order, int k, double* comp_var, double* comp_es) {
    const int64_t b = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t first = order[0];                 // uniform: a scalar load
    if (first < 0 || first >= m) {                  // a NaN total
        comp_var[b] = NAN;
        comp_es[b] = NAN;
        return;
    }
    components_of(rows + b * S_tot, base_col, order, k, comp_var + b, comp_es + b);
}

int check_alloc(const std::string& w, int64_t B, int S_tot, int base_col, int k) {
    return check_sizes(w, B, S_tot, base_col, k,
                       TailLimit{false, ADR_SCENARIO_ALLOC_MAX, "", " P&L values per row; at most ADR_SCENARIO_ALLOC_MAX (8192) (key, index) pairs fit the LDS"});
}

hipError_t enqueue_alloc_total(const double* rows, int64_t B, int S_tot, int base_col, double* tot, hipStream_t stream) {
    const int m = base_col >= 0 ? S_tot - 1 : S_tot;
    hipLaunchKernelGGL(alloc_total_kernel, dim3(static_cast<unsigned>((m + scen::kRedEntries - 1) / scen::kRedEntries)),
                       dim3(scen::kRedLanes * scen::kRedEntries), 0, stream, rows, B, static_cast<int64_t>(S_tot), base_col, m, tot);
    return hipGetLastError();
}

hipError_t enqueue_alloc_rows(const double* rows, int64_t B, int S_tot, int base_col, const int64_t* order, int k, double* comp_var,
                              double* comp_es, hipStream_t stream) {
    const int64_t row_blocks = (B + 255) / 256;
    if (row_blocks > INT32_MAX) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(alloc_rows_kernel, dim3(static_cast<unsigned>(row_blocks)), dim3(256), 0, stream, rows, B,
                       static_cast<int64_t>(S_tot), base_col, base_col >= 0 ? S_tot - 1 : S_tot, order, k, comp_var, comp_es);
    return hipGetLastError();
}

void alloc_total_host(const double* rows, int64_t B, int S_tot, int base_col, double* tot) {
    const int m = base_col >= 0 ? S_tot - 1 : S_tot;
    adr::parallel_ranges(m, adr::pool_threads(m, 1024), [&](int, int64_t lo, int64_t hi) {
        for (int64_t e = lo; e < hi; ++e) {
            double p[kSlots];
            for (int q = 0; q < kSlots; ++q) {
                p[q] = 0.0;
                for (int64_t b = q; b < B; b += kSlots) p[q] = p[q] + pnl_at(rows + b * S_tot, base_col, static_cast<int>(e));
            }
            for (int h = kSlots / 2; h >= 1; h >>= 1)
                for (int q = 0; q < h; ++q) p[q] = p[q] + p[q + h];
            tot[e] = p[0];
        }
    });
}

hipError_t enqueue_alloc(const double* rows, int64_t B, int S_tot, int base_col, int k, double* var_tot, double* es_tot,
                         double* comp_var, double* comp_es, double* work, hipStream_t stream) {
    const int m = base_col >= 0 ? S_tot - 1 : S_tot, P = pow2_at_least(m);
    if ((B + 255) / 256 > INT32_MAX) return hipErrorInvalidConfiguration;
    hipError_t e = enqueue_alloc_total(rows, B, S_tot, base_col, work, stream);
    if (e != hipSuccess) return e;
    const int threads = std::min(1024, std::max(kWave, P / 2));
    const size_t lds = static_cast<size_t>(P) * sizeof(KeyIdx);
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&alloc_order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(lds));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(alloc_order_kernel, dim3(1), dim3(threads), lds, stream, work, m, P, k, var_tot, es_tot);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return enqueue_alloc_rows(rows, B, S_tot, base_col, reinterpret_cast<const int64_t*>(work), k, comp_var, comp_es, stream);
}

}  // namespace sub
}  // namespace adr

namespace SB = adr::sub;

extern "C" {

int64_t adr_scenario_subbook_work(int64_t n, int64_t B, int S) {
    if (n < 1 || B < 1 || S < 1) return 0;
    return SB::max_chunks(n, B, SB::kChunk) * S;
}

int64_t adr_scenario_subbook_plan(int64_t n, int64_t B, const int64_t* sub_off, int64_t* plan) {
    const int rc = SB::check_offsets("adr_scenario_subbook_plan", n, B, sub_off);
    if (rc != ADR_OK) return rc;
    int64_t C = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (plan) plan[b] = C;
        C += (sub_off[b + 1] - sub_off[b] + SB::kChunk - 1) / SB::kChunk;
    }
    if (plan) {
        plan[B] = C;
        int64_t* bounds = plan + B + 1;
        for (int64_t b = 0; b < B; ++b)
            for (int64_t i = sub_off[b]; i < sub_off[b + 1]; i += SB::kChunk) {
                *bounds++ = i;
                *bounds++ = std::min(i + SB::kChunk, sub_off[b + 1]);
            }
    }
    return B + 1 + 2 * C;
}

int adr_scenario_tail_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, int k, double* var_dev,
                          double* es_dev, void* stream) {
    const std::string w = "adr_scenario_tail_dev";
    int rc = SB::check_tail(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows_dev || !var_dev || !es_dev) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    hipStream_t s = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &s);
    if (rc != ADR_OK) return rc;
    const hipError_t e = SB::enqueue_tail(rows_dev, B, S_tot, base_col, k, var_dev, es_dev, s);
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

int adr_scenario_tail(adr_ctx* ctx, int64_t B, int S_tot, const double* rows, int base_col, int k, double* var, double* es) {
    const std::string w = "adr_scenario_tail";
    int rc = SB::check_tail(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows || !var || !es) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    double *drows, *dvar, *des;
    adr::call::Staging mem;
    mem.in(&drows, rows, static_cast<size_t>(B) * S_tot);
    mem.out(&dvar, var, B);
    mem.out(&des, es, B);
    hipError_t e = mem.begin(stream);
    if (e == hipSuccess) e = SB::enqueue_tail(drows, B, S_tot, base_col, k, dvar, des, stream);
    return mem.finish(w, ADR_OK, e, stream);
}

int adr_scenario_tail_host(int64_t B, int S_tot, const double* rows, int base_col, int k, double* var, double* es) {
    const std::string w = "adr_scenario_tail_host";
    const int rc = SB::check_tail(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows || !var || !es) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    const int m = base_col >= 0 ? S_tot - 1 : S_tot;
    adr::parallel_ranges(B, adr::pool_threads(B, 64), [&](int, int64_t lo, int64_t hi) {
        std::vector<int64_t> keys(static_cast<size_t>(m));
        for (int64_t b = lo; b < hi; ++b) {
            const double* row = rows + b * S_tot;
            bool nan = false;
            for (int e = 0; e < m; ++e) {
                const double v = SB::pnl_at(row, base_col, e);
                nan |= v != v;
                keys[e] = SB::key_of(v);
            }
            if (nan) {
                var[b] = es[b] = NAN;
                continue;
            }
            std::sort(keys.begin(), keys.end());
            SB::tail_of_sorted(keys.data(), k, var + b, es + b);
        }
    });
    return ADR_OK;
}

int adr_scenario_tail_alloc_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, int k,
                                double* var_tot_dev, double* es_tot_dev, double* comp_var_dev, double* comp_es_dev,
                                double* work_dev, void* stream) {
    const std::string w = "adr_scenario_tail_alloc_dev";
    int rc = SB::check_alloc(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows_dev || !var_tot_dev || !es_tot_dev || !comp_var_dev || !comp_es_dev) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    if (!work_dev) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (S_tot doubles are needed)");
    hipStream_t s = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &s);
    if (rc != ADR_OK) return rc;
    const hipError_t e = SB::enqueue_alloc(rows_dev, B, S_tot, base_col, k, var_tot_dev, es_tot_dev, comp_var_dev, comp_es_dev,
                                           work_dev, s);
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

int adr_scenario_tail_alloc(adr_ctx* ctx, int64_t B, int S_tot, const double* rows, int base_col, int k, double* var_tot,
                            double* es_tot, double* comp_var, double* comp_es) {
    const std::string w = "adr_scenario_tail_alloc";
    int rc = SB::check_alloc(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows || !var_tot || !es_tot || !comp_var || !comp_es) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    double totals[2] = {0.0, 0.0};                  // the caller's two are written only by a call that succeeds
    double *drows, *dwork, *dtot, *dcv, *dce;
    adr::call::Staging mem;
    mem.in(&drows, rows, static_cast<size_t>(B) * S_tot);
    mem.scratch(&dwork, S_tot);
    mem.out(&dtot, totals, 2);
    mem.out(&dcv, comp_var, B);
    mem.out(&dce, comp_es, B);
    hipError_t e = mem.begin(stream);
    if (e == hipSuccess) e = SB::enqueue_alloc(drows, B, S_tot, base_col, k, dtot, dtot + 1, dcv, dce, dwork, stream);
    rc = mem.finish(w, ADR_OK, e, stream);
    if (rc == ADR_OK) {
        *var_tot = totals[0];
        *es_tot = totals[1];
    }
    return rc;
}

int adr_scenario_tail_alloc_host(int64_t B, int S_tot, const double* rows, int base_col, int k, double* var_tot, double* es_tot,
                                 double* comp_var, double* comp_es) {
    const std::string w = "adr_scenario_tail_alloc_host";
    const int rc = SB::check_alloc(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows || !var_tot || !es_tot || !comp_var || !comp_es) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    const int m = base_col >= 0 ? S_tot - 1 : S_tot;
    std::vector<double> tot(static_cast<size_t>(m));
    SB::alloc_total_host(rows, B, S_tot, base_col, tot.data());
    std::vector<SB::KeyIdx> pairs(static_cast<size_t>(m));
    bool nan = false;
    for (int e = 0; e < m; ++e) {
        nan |= tot[e] != tot[e];
        pairs[e] = SB::KeyIdx{SB::key_of(tot[e]), e};
    }
    if (nan) {
        *var_tot = *es_tot = NAN;
        std::fill(comp_var, comp_var + B, NAN);
        std::fill(comp_es, comp_es + B, NAN);
        return ADR_OK;
    }
    std::sort(pairs.begin(), pairs.end(), [](const SB::KeyIdx& a, const SB::KeyIdx& b) { return SB::after(b, a); });
    SB::total_of_sorted(pairs.data(), k, var_tot, es_tot);
    std::vector<int64_t> order(static_cast<size_t>(k));
    for (int i = 0; i < k; ++i) order[i] = pairs[i].idx;
    adr::parallel_ranges(B, adr::pool_threads(B, 64), [&](int, int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) SB::components_of(rows + b * S_tot, base_col, order.data(), k, comp_var + b, comp_es + b);
    });
    return ADR_OK;
}

}  // extern "C"
