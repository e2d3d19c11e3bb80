// The firm's tail allocation beyond the row limit (the contracts: include/adrates.h), built around tail_select.hip's ordered
// select, which hands out the firm's k worst scenarios as indices in the firm's order:
//   adr_scenario_tail_alloc_select*  adr_scenario_tail_alloc for a matrix of any width: subbook.hip's alloc_total_kernel
//       (the fixed-order column sums), the ordered select on the one-row tot, subbook.hip's alloc_rows_kernel.  The limit
//       is on the tail (k pairs in LDS), not on the row.
//   adr_scenario_total*              the column sums alone - the Monte Carlo chain adds the desks' ladder rows with them.
//   adr_shock_gather*                out[i] = shocks[order[i]]: the shock rows of the firm's k worst scenarios, where
//       adr_ladder_pnl_dev prices every desk next.  One thread per output value, rows of P doubles read whole.
//   adr_tail_components*             comp_var and comp_es of a [B][k] P&L matrix already in the firm's order.  The sum of
//       a row is sequential by contract, so a row is one lane's work; a wave takes 64 rows and walks them 64 columns at a
//       time through LDS (65 doubles a row: no bank conflicts), so the reads of a row are 512 coalesced bytes, not a
//       stride of k doubles across the lanes.  One wave per block: the barriers cost nothing.
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

#pragma clang fp contract(off)

namespace adr {
namespace tord {

constexpr int kGatherThreads = 256;
constexpr int kCompRows = 64;                   // rows of a block = lanes of its one wave
constexpr int kCompCols = 64;                   // columns of a step

// out[i][p] = shocks[order[i]][p]; NaN where order[0] is negative (the firm's row held a NaN) or order[i] is no row.
__global__ __launch_bounds__(kGatherThreads) void shock_gather_kernel(const double* shocks, int S, int P, const int64_t* order, int k,
                                                                      double* out) {
    const int64_t at = static_cast<int64_t>(blockIdx.x) * kGatherThreads + threadIdx.x;
    if (at >= static_cast<int64_t>(k) * P) return;
    const int64_t i = at / P, p = at - i * P;
    const int64_t first = order[0], s = order[i];                   // first is uniform: a scalar load
    out[at] = first < 0 || s < 0 || s >= S ? NAN : shocks[s * P + p];
}

// blockIdx.x = 64 rows of pnl[B][k].
__global__ __launch_bounds__(kCompRows) void components_kernel(const double* pnl, int64_t B, int k, double* comp_var, double* comp_es) {
    __shared__ double tile[kCompRows][kCompCols + 1];
    const int lane = threadIdx.x;
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kCompRows, b = b0 + lane;
    const int rows = B - b0 < kCompRows ? static_cast<int>(B - b0) : kCompRows;
    double sum = 0.0, last = 0.0;
    for (int c0 = 0; c0 < k; c0 += kCompCols) {                     // uniform bounds
        const int cols = k - c0 < kCompCols ? k - c0 : kCompCols;
        if (lane < cols)
            for (int r = 0; r < rows; ++r) tile[r][lane] = pnl[(b0 + r) * k + c0 + lane];
        __syncthreads();
        if (lane < rows)
            for (int c = 0; c < cols; ++c) {
                last = tile[lane][c];
                sum = sum + last;
            }
        __syncthreads();
    }
    if (b < B) {
        comp_var[b] = -last;
        comp_es[b] = -sum / static_cast<double>(k);
    }
}

int check_gather(const std::string& w, int k, int P, int S) {
    if (k < 1 || S < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one index and one shock row are needed");
    if (P < 1 || P > ADR_LADDER_PNL_MAX_PILLARS)
        return adr_set_error(ADR_ERR_INVALID, w + ": P must lie in 1 .. ADR_LADDER_PNL_MAX_PILLARS (256)");
    return ADR_OK;
}

int check_components(const std::string& w, int64_t B, int k) {
    if (B < 1 || k < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one row and one column are needed");
    if ((B + kCompRows - 1) / kCompRows > INT32_MAX) return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": more than 2^37 rows in one launch");
    return ADR_OK;
}

// work of adr_scenario_tail_alloc_select_dev: tot[m] doubles (to a multiple of 16 bytes) | order[k] | the select's scratch
struct AllocLayout {
    size_t order, select, bytes;
};
inline AllocLayout alloc_layout(int S_tot, int k) {
    AllocLayout l;
    l.order = (static_cast<size_t>(S_tot) * sizeof(double) + 15) / 16 * 16;
    l.select = l.order + (static_cast<size_t>(k) * sizeof(int64_t) + 15) / 16 * 16;
    l.bytes = l.select + tsel::order_work_bytes(1, S_tot, k);
    return l;
}

int enqueue_alloc_select(const std::string& w, const double* rows, int64_t B, int S_tot, int base_col, int k, double* var_tot,
                         double* es_tot, double* comp_var, double* comp_es, void* work, hipStream_t stream) {
    const int m = base_col >= 0 ? S_tot - 1 : S_tot;
    const AllocLayout l = alloc_layout(S_tot, k);
    char* base = static_cast<char*>(work);
    double* tot = reinterpret_cast<double*>(base);
    int64_t* order = reinterpret_cast<int64_t*>(base + l.order);
    hipError_t e = sub::enqueue_alloc_total(rows, B, S_tot, base_col, tot, stream);
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    const int rc = tsel::enqueue_order(w, tot, 1, m, -1, k, order, var_tot, es_tot, base + l.select, stream);
    if (rc != ADR_OK) return rc;
    e = sub::enqueue_alloc_rows(rows, B, S_tot, base_col, order, k, comp_var, comp_es, stream);
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

}  // namespace tord
}  // namespace adr

namespace TO = adr::tord;
namespace TS = adr::tsel;

extern "C" {

int64_t adr_scenario_tail_alloc_select_work(int64_t B, int S_tot, int k) {
    if (B < 1 || S_tot < 1 || k < 1 || k > ADR_SCENARIO_ALLOC_MAX) return 0;
    return static_cast<int64_t>(TO::alloc_layout(S_tot, k).bytes);
}

int adr_scenario_tail_alloc_select_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, int k,
                                       double* var_tot_dev, double* es_tot_dev, double* comp_var_dev, double* comp_es_dev,
                                       void* work_dev, void* stream) {
    const std::string w = "adr_scenario_tail_alloc_select_dev";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = TS::check_order(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows_dev || !var_tot_dev || !es_tot_dev || !comp_var_dev || !comp_es_dev) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    if (!work_dev) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (adr_scenario_tail_alloc_select_work bytes are needed)");
    hipStream_t st = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &st);
    if (rc != ADR_OK) return rc;
    return TO::enqueue_alloc_select(w, rows_dev, B, S_tot, base_col, k, var_tot_dev, es_tot_dev, comp_var_dev, comp_es_dev, work_dev, st);
}

int adr_scenario_tail_alloc_select(adr_ctx* ctx, int64_t B, int S_tot, const double* rows, int base_col, int k, double* var_tot,
                                   double* es_tot, double* comp_var, double* comp_es) {
    const std::string w = "adr_scenario_tail_alloc_select";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = TS::check_order(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows || !var_tot || !es_tot || !comp_var || !comp_es) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    double totals[2] = {0.0, 0.0};                  // the caller's two are written only by a call that succeeds
    double *drows, *dtot, *dcv, *dce;
    void* dwork;
    adr::call::Staging mem;
    mem.in(&drows, rows, static_cast<size_t>(B) * S_tot);
    mem.out(&dtot, totals, 2);
    mem.out(&dcv, comp_var, B);
    mem.out(&dce, comp_es, B);
    mem.scratch_bytes(&dwork, TO::alloc_layout(S_tot, k).bytes);
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess) rc = TO::enqueue_alloc_select(w, drows, B, S_tot, base_col, k, dtot, dtot + 1, dcv, dce, dwork, stream);
    rc = mem.finish(w, rc, e, stream);
    if (rc == ADR_OK) {
        *var_tot = totals[0];
        *es_tot = totals[1];
    }
    return rc;
}

int adr_scenario_tail_alloc_select_host(int64_t B, int S_tot, const double* rows, int base_col, int k, double* var_tot, double* es_tot,
                                        double* comp_var, double* comp_es) {
    const std::string w = "adr_scenario_tail_alloc_select_host";
    const int rc = TS::check_order(w, B, S_tot, base_col, k);
    if (rc != ADR_OK) return rc;
    if (!rows || !var_tot || !es_tot || !comp_var || !comp_es) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    const int m = base_col >= 0 ? S_tot - 1 : S_tot;
    std::vector<double> tot(static_cast<size_t>(m));
    std::vector<int64_t> order(static_cast<size_t>(k));
    adr::sub::alloc_total_host(rows, B, S_tot, base_col, tot.data());
    TS::order_host(tot.data(), 1, m, -1, k, order.data(), var_tot, es_tot);
    if (order[0] < 0) {                                             // a NaN total
        std::fill(comp_var, comp_var + B, NAN);
        std::fill(comp_es, comp_es + B, NAN);
        return ADR_OK;
    }
    adr::parallel_ranges(B, adr::pool_threads(B, 64), [&](int, int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) adr::sub::components_of(rows + b * S_tot, base_col, order.data(), k, comp_var + b, comp_es + b);
    });
    return ADR_OK;
}

int adr_scenario_total_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, double* tot_dev, void* stream) {
    const std::string w = "adr_scenario_total_dev";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = TS::check_order(w, B, S_tot, base_col, 1);
    if (rc != ADR_OK) return rc;
    if (!rows_dev || !tot_dev) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    hipStream_t st = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &st);
    if (rc != ADR_OK) return rc;
    const hipError_t e = adr::sub::enqueue_alloc_total(rows_dev, B, S_tot, base_col, tot_dev, st);
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

int adr_scenario_total_host(int64_t B, int S_tot, const double* rows, int base_col, double* tot) {
    const std::string w = "adr_scenario_total_host";
    const int rc = TS::check_order(w, B, S_tot, base_col, 1);
    if (rc != ADR_OK) return rc;
    if (!rows || !tot) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    adr::sub::alloc_total_host(rows, B, S_tot, base_col, tot);
    return ADR_OK;
}

int adr_shock_gather_dev(adr_ctx* ctx, int k, int P, const double* shocks_dev, int S, const int64_t* order_dev, double* out_dev,
                         void* stream) {
    const std::string w = "adr_shock_gather_dev";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = TO::check_gather(w, k, P, S);
    if (rc != ADR_OK) return rc;
    if (!shocks_dev || !order_dev || !out_dev) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    hipStream_t st = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &st);
    if (rc != ADR_OK) return rc;
    const int64_t blocks = (static_cast<int64_t>(k) * P + TO::kGatherThreads - 1) / TO::kGatherThreads;      // at most 2^31: P <= 256
    hipLaunchKernelGGL(TO::shock_gather_kernel, dim3(static_cast<unsigned>(blocks)), dim3(TO::kGatherThreads), 0, st, shocks_dev, S, P,
                       order_dev, k, out_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

int adr_shock_gather_host(int k, int P, const double* shocks, int S, const int64_t* order, double* out) {
    const std::string w = "adr_shock_gather_host";
    const int rc = TO::check_gather(w, k, P, S);
    if (rc != ADR_OK) return rc;
    if (!shocks || !order || !out) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    for (int64_t i = 0; i < k; ++i) {
        const int64_t s = order[i];
        for (int p = 0; p < P; ++p) out[i * P + p] = order[0] < 0 || s < 0 || s >= S ? NAN : shocks[s * P + p];
    }
    return ADR_OK;
}

int adr_tail_components_dev(adr_ctx* ctx, int64_t B, int k, const double* pnl_dev, double* comp_var_dev, double* comp_es_dev,
                            void* stream) {
    const std::string w = "adr_tail_components_dev";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = TO::check_components(w, B, k);
    if (rc != ADR_OK) return rc;
    if (!pnl_dev || !comp_var_dev || !comp_es_dev) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    hipStream_t st = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &st);
    if (rc != ADR_OK) return rc;
    hipLaunchKernelGGL(TO::components_kernel, dim3(static_cast<unsigned>((B + TO::kCompRows - 1) / TO::kCompRows)), dim3(TO::kCompRows), 0,
                       st, pnl_dev, B, k, comp_var_dev, comp_es_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

int adr_tail_components_host(int64_t B, int k, const double* pnl, double* comp_var, double* comp_es) {
    const std::string w = "adr_tail_components_host";
    const int rc = TO::check_components(w, B, k);
    if (rc != ADR_OK) return rc;
    if (!pnl || !comp_var || !comp_es) return adr_set_error(ADR_ERR_INVALID, w + ": null array");
    adr::parallel_ranges(B, adr::pool_threads(B, 64), [&](int, int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) {
            double sum = 0.0, last = 0.0;
            for (int i = 0; i < k; ++i) {
                last = pnl[b * k + i];
                sum = sum + last;
            }
            comp_var[b] = -last;
            comp_es[b] = -sum / static_cast<double>(k);
        }
    });
    return ADR_OK;
}

}  // extern "C"
