// The two small steps between the Monte Carlo shock rows and the credit and inflation scenario kernels, and between their
// sub-book rows and one [B][S] matrix of the firm (adr_shock_columns*, adr_scenario_rows_merge*,
// adr_scenario_rows_place_dev; the contract: include/adrates.h).
//
// adr_shock_columns: adr_shock_normal_dev writes one joint row per scenario, shocks[S][ld] in basis points; the credit
// kernel reads a dense dz[S][G] in decimals, the YoY kernel a dense b[S][P_i] of breakeven rates:
//     out[s][j] = base[j] + shocks[s][col0 + j] * 1e-4          (base NULL: the product itself)
// one rounded product and one rounded sum - contraction is off - so the bits are NumPy's `b0 + x * 1e-4` and `x * 1e-4`.
// One lane per entry of out, entries in the order of memory: a wave stores 512 contiguous bytes and loads runs of n
// doubles from rows that lie 8 ld bytes apart.  bad[s] gets the constant 1 from every lane that finds a bad entry, a plain
// vector store of the same value to the same word, and is not touched otherwise.
//
// adr_scenario_rows_merge: rows[target[b]][s0 + s] = tile[b][s], or += where add[b] != 0, so the rates, credit and
// inflation launches of one tile land in the desks' rows one after another.  adr_scenario_rows_place_dev is the same
// kernel without a row map (target null: t = b) and without add.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "blocking_call.hpp"
#include "host_pool.hpp"

#pragma clang fp contract(off)      // a product and a sum, two roundings

namespace adr {
namespace scol {

constexpr int kBlock = 256;
constexpr int64_t kMaxBlocks = 1 << 20;      // beyond it a lane strides over the entries

// ------------------------------------------------------------------------------------------------------------ shared
// base: null where the entry has no base row
__host__ __device__ inline double column_value(const double* base, int j, double shock_bp) {
    const double d = shock_bp * 1e-4;
    return base ? base[j] + d : d;
}

__host__ __device__ inline bool bad_value(double v, int floor_on, double floor) {
    return !(v > -INFINITY && v < INFINITY) || (floor_on && v <= floor);
}

// ------------------------------------------------------------------------------------------------------------ device
struct Args {
    const double* shocks;            // [S][ld]
    const double* base;              // [n] or null
    double* out;                     // [S][n]
    int32_t* bad;                    // [S] or null
    double floor;
    int64_t S, ld, col0, n;
    int floor_on;
};

__global__ __launch_bounds__(kBlock) void shock_columns_kernel(Args a) {
    const int64_t total = a.S * a.n, step = static_cast<int64_t>(gridDim.x) * kBlock;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += step) {
        const int64_t s = e / a.n;
        const int j = static_cast<int>(e - s * a.n);
        const double v = column_value(a.base, j, a.shocks[s * a.ld + a.col0 + j]);
        a.out[e] = v;
        if (a.bad && bad_value(v, a.floor_on, a.floor)) a.bad[s] = 1;
    }
}

// blockIdx.y strides over the tile's rows; target null: the identity map
__global__ __launch_bounds__(kBlock) void rows_merge_kernel(int64_t B, int S_tile, const double* tile, int64_t B_tot, int64_t S_tot,
                                                            int64_t s0, double* rows, const int64_t* target, const int32_t* add) {
    const int64_t s = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (s >= S_tile) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const int64_t t = target ? target[b] : b;
        if (t < 0 || t >= B_tot) continue;
        double* at = rows + t * S_tot + s0 + s;
        const double v = tile[b * S_tile + s];
        *at = add && add[b] ? *at + v : v;
    }
}

// -------------------------------------------------------------------------------------------------------------- host
int check_columns(const std::string& w, int S, int ld, int col0, int n, const void* shocks, const void* out) {
    if (S < 1 || n < 1 || col0 < 0) return adr_set_error(ADR_ERR_INVALID, w + ": S >= 1, n >= 1 and col0 >= 0 are needed");
    if (static_cast<int64_t>(ld) < static_cast<int64_t>(col0) + n)
        return adr_set_error(ADR_ERR_INVALID, w + ": columns " + std::to_string(col0) + " .. " + std::to_string(static_cast<int64_t>(col0) + n) +
                                                  " do not fit rows of " + std::to_string(ld));
    if (!shocks || !out) return adr_set_error(ADR_ERR_INVALID, w + ": shocks_bp / out is NULL");
    return ADR_OK;
}

int enqueue_columns(const std::string& w, const Args& a, hipStream_t stream) {
    const int64_t blocks = std::min<int64_t>((a.S * a.n + kBlock - 1) / kBlock, kMaxBlocks);
    hipLaunchKernelGGL(shock_columns_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

// mapped: the entry takes B_tot and a row map; the place entry has neither (B_tot = B, target null)
int check_merge(const std::string& w, bool mapped, int64_t B, int S_tile, int64_t B_tot, int S_tot, int s0, const void* tile,
                const void* rows, const void* target) {
    if (B < 1 || S_tile < 1 || B_tot < 1 || S_tot < 1 || s0 < 0)
        return adr_set_error(ADR_ERR_INVALID, w + ": B >= 1, S_tile >= 1, " + (mapped ? "B_tot >= 1, " : "") + "S_tot >= 1 and s0 >= 0 are needed");
    if (static_cast<int64_t>(s0) + S_tile > S_tot)
        return adr_set_error(ADR_ERR_INVALID, w + ": columns " + std::to_string(s0) + " .. " + std::to_string(static_cast<int64_t>(s0) + S_tile) +
                                                  " do not fit rows of " + std::to_string(S_tot));
    if (!tile || !rows || (mapped && !target)) return adr_set_error(ADR_ERR_INVALID, w + ": tile / rows" + (mapped ? " / target" : "") + " is NULL");
    return ADR_OK;
}

// The checks and the launch of both device entries.
int enqueue_merge(const std::string& w, bool mapped, adr_ctx* ctx, int64_t B, int S_tile, const double* tile, int64_t B_tot, int S_tot,
                  int s0, double* rows, const int64_t* target, const int32_t* add, void* stream) {
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = check_merge(w, mapped, B, S_tile, B_tot, S_tot, s0, tile, rows, target);
    if (rc != ADR_OK) return rc;
    hipStream_t st = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &st);
    if (rc != ADR_OK) return rc;
    const dim3 grid(static_cast<unsigned>((S_tile + kBlock - 1) / kBlock), static_cast<unsigned>(std::min<int64_t>(B, 65535)));
    hipLaunchKernelGGL(rows_merge_kernel, grid, dim3(kBlock), 0, st, B, S_tile, tile, B_tot, static_cast<int64_t>(S_tot),
                       static_cast<int64_t>(s0), rows, target, add);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

}  // namespace scol
}  // namespace adr

namespace SQ = adr::scol;

extern "C" {

int adr_shock_columns_dev(adr_ctx* ctx, int S, int ld, const double* shocks_bp_dev, int col0, int n, const double* base_dev, int floor_on,
                          double floor, double* out_dev, int32_t* bad_dev, void* stream) {
    const std::string w = "adr_shock_columns_dev";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = SQ::check_columns(w, S, ld, col0, n, shocks_bp_dev, out_dev);
    if (rc != ADR_OK) return rc;
    hipStream_t st = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &st);
    if (rc != ADR_OK) return rc;
    return SQ::enqueue_columns(w, SQ::Args{shocks_bp_dev, base_dev, out_dev, bad_dev, floor, S, ld, col0, n, floor_on}, st);
}

int adr_shock_columns(adr_ctx* ctx, int S, int ld, const double* shocks_bp, int col0, int n, const double* base, int floor_on, double floor,
                      double* out, int32_t* bad) {
    const std::string w = "adr_shock_columns";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = SQ::check_columns(w, S, ld, col0, n, shocks_bp, out);
    if (rc != ADR_OK) return rc;
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    double *d_x, *d_base, *d_out;
    int32_t* d_bad;
    adr::call::Staging mem;
    mem.in(&d_x, shocks_bp, static_cast<size_t>(S) * ld);
    mem.in(&d_base, base, n, base != nullptr);
    mem.out(&d_out, out, static_cast<size_t>(S) * n);
    mem.inout(&d_bad, bad, S, bad != nullptr);                      // the flags are only ever raised: the caller's come in first
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess) rc = SQ::enqueue_columns(w, SQ::Args{d_x, d_base, d_out, d_bad, floor, S, ld, col0, n, floor_on}, stream);
    return mem.finish(w, rc, e, stream);
}

int adr_shock_columns_host(int S, int ld, const double* shocks_bp, int col0, int n, const double* base, int floor_on, double floor,
                           double* out, int32_t* bad) {
    const std::string w = "adr_shock_columns_host";
    const int rc = SQ::check_columns(w, S, ld, col0, n, shocks_bp, out);
    if (rc != ADR_OK) return rc;
    const int64_t grain = std::max<int64_t>(1, (int64_t(1) << 16) / n);
    adr::parallel_ranges(S, adr::pool_threads(S, grain), [&](int, int64_t lo, int64_t hi) {
        for (int64_t s = lo; s < hi; ++s)
            for (int j = 0; j < n; ++j) {
                const double v = SQ::column_value(base, j, shocks_bp[s * ld + col0 + j]);
                out[s * n + j] = v;
                if (bad && SQ::bad_value(v, floor_on, floor)) bad[s] = 1;
            }
    });
    return ADR_OK;
}

int adr_scenario_rows_merge_dev(adr_ctx* ctx, int64_t B, int S_tile, const double* tile_dev, int64_t B_tot, int S_tot, int s0,
                                double* rows_dev, const int64_t* target_dev, const int32_t* add_dev, void* stream) {
    return SQ::enqueue_merge("adr_scenario_rows_merge_dev", true, ctx, B, S_tile, tile_dev, B_tot, S_tot, s0, rows_dev, target_dev, add_dev, stream);
}

int adr_scenario_rows_place_dev(adr_ctx* ctx, int64_t B, int S_tile, const double* tile_dev, int S_tot, int s0, double* rows_dev,
                                void* stream) {
    return SQ::enqueue_merge("adr_scenario_rows_place_dev", false, ctx, B, S_tile, tile_dev, B, S_tot, s0, rows_dev, nullptr, nullptr, stream);
}

int adr_scenario_rows_merge_host(int64_t B, int S_tile, const double* tile, int64_t B_tot, int S_tot, int s0, double* rows,
                                 const int64_t* target, const int32_t* add) {
    const std::string w = "adr_scenario_rows_merge_host";
    const int rc = SQ::check_merge(w, true, B, S_tile, B_tot, S_tot, s0, tile, rows, target);
    if (rc != ADR_OK) return rc;
    std::vector<int64_t> seen;
    for (int64_t b = 0; b < B; ++b)
        if (target[b] >= 0 && target[b] < B_tot) seen.push_back(target[b]);
    std::sort(seen.begin(), seen.end());
    const auto twice = std::adjacent_find(seen.begin(), seen.end());
    if (twice != seen.end()) return adr_set_error(ADR_ERR_INVALID, w + ": row " + std::to_string(*twice) + " is the target of two rows of the tile");
    for (int64_t b = 0; b < B; ++b) {
        const int64_t t = target[b];
        if (t < 0 || t >= B_tot) continue;
        double* at = rows + t * S_tot + s0;
        const double* v = tile + b * S_tile;
        if (add && add[b])
            for (int s = 0; s < S_tile; ++s) at[s] = at[s] + v[s];
        else
            for (int s = 0; s < S_tile; ++s) at[s] = v[s];
    }
    return ADR_OK;
}

}  // extern "C"
