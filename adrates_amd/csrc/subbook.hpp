// Sub-books of a scenario revaluation (subbook.hip): the chunk plan, the fixed-order sum per sub-book and the tail
// measures and their allocation; shared by scenario_pv.hip, credit_scenario_pv.hip and yoy_scenario_pv.hip.  The whole book's sum, which subbook.hip holds too, is
// declared in scenario_common.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace adr {
namespace sub {

// The plan of B sub-books with C chunks in all, B + 1 + 2 C int64 (adr_scenario_subbook_plan fills it):
//   plan[0 .. B]            chunk_off: sub-book b owns the chunks chunk_off[b] .. chunk_off[b + 1] (chunk_off[B] = C)
//   plan[B + 1 + 2 c, + 1]  the first trade of chunk c and the one after its last
struct Plan {
    const int64_t* chunk_off;
    const int64_t* bounds;
};
inline Plan plan_view(const int64_t* plan, int64_t B) { return Plan{plan, plan + B + 1}; }

inline int64_t max_chunks(int64_t n, int64_t B, int chunk) { return (n + chunk - 1) / chunk + B; }

// ADR_ERR_INVALID naming the sub-book unless sub_off runs from 0 to n without decreasing.
int check_offsets(const std::string& w, int64_t n, int64_t B, const int64_t* sub_off);

// check_offsets, then `plan` resized and filled (adr_scenario_subbook_plan).
int build_plan(const std::string& w, int64_t n, int64_t B, const int64_t* sub_off, std::vector<int64_t>& plan);

// sub_pv[b][e] = the fixed-order sum of sub-book b's chunk rows: its chunk j to slot j % 64 in order, then a halving
// tree.  Chunk counts beyond chunk_cap are cut there (work holds that many rows).
hipError_t enqueue_sum(const double* work, const int64_t* chunk_off, int64_t chunk_cap, int64_t B, int S, double* sub_pv,
                       hipStream_t stream);
void reduce_subbooks(const double* work, const int64_t* chunk_off, int64_t B, int64_t S, double* sub_pv);

// ------------------------------------------------------------------------------------------------------ tail measures
// Here, not in subbook.hip, because tail_select.hip runs the same kernel on the k survivors of its select; every source
// that includes this header holds its own copy of the kernel (internal linkage).
// A double as an int64 whose signed order is the doubles' order, -0.0 before +0.0; the map is its own inverse.
__host__ __device__ inline int64_t key_of(double v) {
    int64_t b;
    memcpy(&b, &v, sizeof b);
    return b ^ ((b >> 63) & INT64_MAX);
}
__host__ __device__ inline double value_of(int64_t k) {
    const int64_t b = k ^ ((k >> 63) & INT64_MAX);
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
}

// P&L value e of a row: column e, stepping over base_col, minus the base column's value.
__host__ __device__ inline double pnl_at(const double* row, int base_col, int e) {
    if (base_col < 0) return row[e];
    return row[e >= base_col ? e + 1 : e] - row[base_col];
}

__host__ __device__ inline void tail_of_sorted(const int64_t* keys, int k, double* var, double* es) {
    double sum = 0.0;
    for (int i = 0; i < k; ++i) sum = sum + value_of(keys[i]);
    *var = -value_of(keys[k - 1]);
    *es = -sum / static_cast<double>(k);
}

// m P&L values per row, P = the power of two >= m (the LDS holds P keys).
static __global__ __launch_bounds__(1024) void tail_kernel(const double* rows, int64_t S_tot, int base_col, int m, int P, int k,
                                                           double* var, double* es) {
    extern __shared__ int64_t keys[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const double* row = rows + static_cast<int64_t>(blockIdx.x) * S_tot;
    int nan = 0;
    for (int e = tid; e < P; e += nt) {
        double v = INFINITY;
        if (e < m) {
            v = pnl_at(row, base_col, e);
            nan |= v != v;
        }
        keys[e] = key_of(v);
    }
    if (__syncthreads_or(nan)) {                    // uniform over the block
        if (tid == 0) {
            var[blockIdx.x] = NAN;
            es[blockIdx.x] = NAN;
        }
        return;
    }
    for (int size = 2; size <= P; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += nt) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const int64_t a = keys[lo], b = keys[hi];
                if ((a > b) == ((lo & size) == 0)) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) tail_of_sorted(keys, k, var + blockIdx.x, es + blockIdx.x);
}

inline int pow2_at_least(int m) {
    int p = 1;
    while (p < m) p <<= 1;
    return p;
}

// var[b], es[b] of rows[b][S_tot] (adr_scenario_tail's rule); k and the width have been checked.
inline hipError_t enqueue_tail(const double* rows, int64_t B, int S_tot, int base_col, int k, double* var, double* es, hipStream_t stream) {
    if (B > INT32_MAX) return hipErrorInvalidConfiguration;
    const int m = base_col >= 0 ? S_tot - 1 : S_tot, P = pow2_at_least(m);
    const int threads = std::min(1024, std::max(64, P / 2));
    const size_t lds = static_cast<size_t>(P) * sizeof(int64_t);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tail_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(lds));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tail_kernel, dim3(static_cast<unsigned>(B)), dim3(threads), lds, stream, rows, static_cast<int64_t>(S_tot),
                       base_col, m, P, k, var, es);
    return hipGetLastError();
}

// The size checks of every tail entry (adr_scenario_tail*, _tail_alloc*, _tail_select*, _tail_order*): the rows, the
// columns, base_col and k, then the entry's own limit - on the tail count k, or else on the row's width m - refused as
// w + ": " + before + the count + after.
struct TailLimit {
    bool on_tail;
    int max;
    const char *before, *after;
};
int check_sizes(const std::string& w, int64_t B, int S_tot, int base_col, int k, const TailLimit& limit);
int check_tail(const std::string& w, int64_t B, int S_tot, int base_col, int k);      // a row of ADR_SCENARIO_TAIL_MAX

// ---------------------------------------------------------------------------------------------------- tail allocation
// What subbook.hip's allocation and tail_order.hip's ordered select share: the (key, index) pair and its order, the
// firm's measures from the ordered pairs and a row's components over the ordered scenarios.
struct KeyIdx {
    int64_t key, idx;
};
__host__ __device__ inline bool after(const KeyIdx& a, const KeyIdx& b) { return a.key > b.key || (a.key == b.key && a.idx > b.idx); }

// The firm's measures from the ordered pairs; both sums run over the first k in order from 0.0.
__host__ __device__ inline void total_of_sorted(const KeyIdx* pairs, int k, double* var_tot, double* es_tot) {
    double sum = 0.0;
    for (int i = 0; i < k; ++i) sum = sum + value_of(pairs[i].key);
    *var_tot = -value_of(pairs[k - 1].key);
    *es_tot = -sum / static_cast<double>(k);
}

// A row's components over the k ordered scenarios.
__host__ __device__ inline void components_of(const double* row, int base_col, const int64_t* order, int k, double* comp_var,
                                              double* comp_es) {
    double sum = 0.0, last = 0.0;
    for (int i = 0; i < k; ++i) {
        last = pnl_at(row, base_col, static_cast<int>(order[i]));
        sum = sum + last;
    }
    *comp_var = -last;
    *comp_es = -sum / static_cast<double>(k);
}

// The allocation's first and last kernel on their own (tail_order.hip puts its ordered select between them):
// tot[e] = the fixed-order sum over the rows of pnl[b][e], m values; and every row's components over order[k], NaN in
// both when order[0] is no scenario.  The host forms are the same sums in the same order.
hipError_t enqueue_alloc_total(const double* rows, int64_t B, int S_tot, int base_col, double* tot, hipStream_t stream);
hipError_t enqueue_alloc_rows(const double* rows, int64_t B, int S_tot, int base_col, const int64_t* order, int k, double* comp_var,
                              double* comp_es, hipStream_t stream);
void alloc_total_host(const double* rows, int64_t B, int S_tot, int base_col, double* tot);

// The tail allocation of rows[b][S_tot] (adr_scenario_tail_alloc's rule): the firm's var and es and every row's
// components; `work` holds S_tot doubles; k and the width have been checked.  Three kernels on `stream`.
hipError_t enqueue_alloc(const double* rows, int64_t B, int S_tot, int base_col, int k, double* var_tot, double* es_tot,
                         double* comp_var, double* comp_es, double* work, hipStream_t stream);
int check_alloc(const std::string& w, int64_t B, int S_tot, int base_col, int k);     // a row of ADR_SCENARIO_ALLOC_MAX

}  // namespace sub
}  // namespace adr
