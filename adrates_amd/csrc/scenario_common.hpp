// What the scenario revaluation sources (scenario_pv.hip, credit_scenario_pv.hip, yoy_scenario_pv.hip, xccy_scenario_pv.hip) have in common,
// once: the launch shape, the lookup of a discount factor in weight form, the lane broadcast of a coupon description,
// the order of the book sum, and the host checks of a TradeBatch.  These are what the host twins and the device are
// held to bit for bit, so a fix to any of them is made here.  The pricing kernels, their slots and their coupon code stay
// in their sources; the slots of an ordinary TradeBatch, which scenario_pv.hip and xccy_scenario_pv.hip share, are in
// scenario_trade_slots.hpp.
//
// Layout they share: one lane = one scenario, one wave = 64 scenarios (a "group"); a block is kWaves waves of ONE
// group, which share the group's knot table in LDS as tab[k][lane].  The trades are cut into chunks of kChunk
// consecutive trades; a wave takes chunks round-robin, walks each in trade order and writes its sum to work[chunk][s].
// The book sum then adds the chunk rows in a fixed order (chunk j to slot j % 64 in order, then a halving tree; no
// atomics): scenario_book_kernel in subbook.hip, reduce_chunks its host form.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/adrates.h"
#include "blocking_call.hpp"
#include "kernels.hpp"
#include "simple_interp.hpp"

int adr_ctx_compute_units(const adr_ctx* ctx);                                  // capi.hip
const adr::TradesDev* adr_trades_device_view(const adr_trades* trades, const adr_ctx** owner);              // capi.hip
int adr_curve_set_device_view(const adr_curve_set* set, const adr_ctx** owner, int* method, int* K, int* S,
                              const double** times_dev, const double** dfs_dev);                            // capi.hip

// The host and the device evaluate the same expressions; no contraction into fma, so the two differ only by their
// exp / log implementations.  The pragma stands here at file scope, after the last include and before the first
// expression of this header: the compiler records it in every expression below where that is written, so a template
// keeps it wherever it is instantiated.  It stays in force to the end of the including source, and each source states
// it again after its includes for its own code.
#pragma clang fp contract(off)

namespace adr {
namespace scen {

constexpr int kWave = 64;
constexpr int kWaves = 16;                      // waves per block: four per SIMD, all on one scenario group
constexpr int kThreads = kWave * kWaves;
constexpr int kChunk = ADR_SCENARIO_CHUNK;      // trades per partial sum of the book
constexpr int kRedLanes = 64;                   // the book reduction's slots per scenario
constexpr int kRedEntries = 16;                 // scenarios per reduction block
constexpr size_t kLdsBudget = 160 * 1024;

// D(t) in weight form on the scenario's table T (T_k = ln d_k when kLog, else d_k):
//   kLog:  ln D = wa T_a + (b != a ? wb T_b : 0);      else:  D = T_a + (b != a ? wb (T_b - T_a) : 0).
struct DateW {
    int a, b;
    double wa, wb;
};

template <bool kLog>
__host__ __device__ inline DateW date_weights(double t, const double* x, int K, int method) {
    DateW d;
    if (kLog) {
        const si::LogWeights w = si::log_weights(t, x, K, method);
        d.a = w.a; d.b = w.b; d.wa = w.wa; d.wb = w.wb;
    } else {
        const si::Where p = si::locate(t, x, K);
        d.a = p.lo; d.b = p.hi; d.wa = 1.0; d.wb = p.w;
    }
    return d;
}

template <bool kLog, class Tab>
__host__ __device__ inline double eval_df(const DateW& d, const Tab& tab) {
    const double la = tab(d.a);
    if (kLog) {
        double s = d.wa * la;
        if (d.b != d.a) s = s + d.wb * tab(d.b);
        return exp(s);
    }
    double f = la;
    if (d.b != d.a) f = la + d.wb * (tab(d.b) - la);
    return f;
}

// The trades [i0, i1) of chunk ch.
struct ChunkRange {
    int64_t i0, i1;
};

// kSub: the chunks are those of a sub-book plan (their trade bounds come from its table, subbook.hpp) instead of
// ch * kChunk.  Either way the range is cut to the n trades.
template <bool kSub>
__device__ inline ChunkRange chunk_range(int64_t ch, const int64_t* sub_bounds, int64_t n) {
    int64_t i0 = ch * kChunk, i1 = ch * kChunk + kChunk;
    if (kSub) {
        i0 = sub_bounds[2 * ch];                        // uniform: scalar loads
        i1 = sub_bounds[2 * ch + 1];
        i0 = i0 < 0 ? 0 : i0;
    }
    i1 = i1 < n ? i1 : n;
    return ChunkRange{i0, i1};
}

// The host form; `bounds` (or null) is a plan the host has filled itself.
inline ChunkRange host_chunk_range(int64_t ch, const int64_t* bounds, int64_t n) {
    if (bounds) return ChunkRange{bounds[2 * ch], bounds[2 * ch + 1]};
    return ChunkRange{ch * kChunk, std::min(n, (ch + 1) * kChunk)};
}

// A coupon description travels from lane j to the wave's scalar registers with v_readlane: every branch on it is uniform.
__device__ inline int lane_int(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ inline double lane_dbl(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}
__device__ inline DateW lane_date(const DateW& d, int j) {
    DateW r;
    r.a = lane_int(d.a, j);
    r.b = lane_int(d.b, j);
    r.wa = lane_dbl(d.wa, j);
    r.wb = r.b != r.a ? lane_dbl(d.wb, j) : 0.0;
    return r;
}

// kLds: the group's discount table sits in LDS; otherwise (K too large) every lane reads its scenario's row of dfs.
template <bool kLog, bool kLds>
struct DevTab {
    const double* p;     // kLds: &tab[0][lane]; else &dfs[row][0]
    __device__ double operator()(int k) const {
        if (kLds) return p[k * kWave];
        return kLog ? log(p[k]) : p[k];
    }
};

struct HostTab {
    const double* p;     // the scenario's row of the converted table
    double operator()(int k) const { return p[k]; }
};

// book[s] = sum over the chunk rows of entry s: chunk j to slot j % 64 in order, then slots 0-31 += 32-63, ..., 0 += 1.
// The kernel on `stream` and its host form (subbook.hip).
hipError_t enqueue_book_sum(const double* work, int64_t chunks, int S, double* book, hipStream_t stream);
void reduce_chunks(const double* work, int64_t chunks, int64_t S, double* book);

// The pricing kernels' grid: y = the groups of 64 scenarios, x = the blocks that share a group's chunks round-robin -
// one block per compute unit when the tables fill the LDS.
inline int launch_grid(const std::string& w, const adr_ctx* ctx, int64_t chunks, int S, dim3* grid) {
    const int64_t groups = (static_cast<int64_t>(S) + kWave - 1) / kWave;
    if (groups > 65535) return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": more than 65535 * 64 scenarios in one launch");
    const int64_t per_group = std::max<int64_t>(1, (adr_ctx_compute_units(ctx) + groups - 1) / groups);
    const int64_t bx = std::min<int64_t>((chunks + kWaves - 1) / kWaves, per_group);
    *grid = dim3(static_cast<unsigned>(bx), static_cast<unsigned>(groups));
    return ADR_OK;
}

// The launch of a pricing kernel with its dynamic LDS.
template <class Kernel, class Args>
hipError_t launch_with_lds(Kernel kernel, const Args& a, size_t lds, dim3 grid, hipStream_t stream) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(lds));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), lds, stream, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------- host checks
// The first failing check decides an entry's message, so each entry calls these in its own order.
inline int check_scheme_knots(const std::string& w, int method, int K) {
    if (method != ADR_INTERP_FLAT_FWD_RATES && method != ADR_INTERP_LINEAR_FWD_RATES && method != ADR_INTERP_LINEAR_ZERO_RATES)
        return adr_set_error(ADR_ERR_INVALID, w + ": the scheme must be FLAT_FWD_RATES (1), LINEAR_FWD_RATES (2) or "
                                                  "LINEAR_ZERO_RATES (4)");
    if (K < 2 || K > ADR_SCENARIO_MAX_KNOTS)
        return adr_set_error(ADR_ERR_INVALID, w + ": the knot grid needs 2 .. ADR_SCENARIO_MAX_KNOTS (4096) knots");
    return ADR_OK;
}

// Host curves: `rows` rows of K discount factors; `row_word` is what the entry's message calls a row.
inline int check_curves(const std::string& w, int K, const double* times, int rows, const double* dfs, const char* row_word) {
    for (int k = 0; k < K; ++k)
        if (!std::isfinite(times[k]) || (k > 0 && times[k] < times[k - 1]))
            return adr_set_error(ADR_ERR_INVALID, w + ": knot times must be finite and non-decreasing");
    for (int64_t i = 0; i < static_cast<int64_t>(rows) * K; ++i)
        if (!(dfs[i] > 0.0) || !std::isfinite(dfs[i]))
            return adr_set_error(ADR_ERR_INVALID, w + ": discount factors must be positive and finite (" + row_word + " " +
                                                      std::to_string(i / K) + ", knot " + std::to_string(i % K) + ")");
    return ADR_OK;
}

struct HostBatch {       // the arrays of a TradeBatch as the _host entries take them
    int64_t n;
    const int64_t *fix_off, *flt_off;
    const double *fix_tp, *fix_pay, *flt_tp, *flt_ts, *flt_te, *flt_alpha, *flt_weight;
    const double *notional, *spread, *fix_sign, *flt_sign;
};

// The leg offsets of trades i0 .. i1 - 1; trade 0 brings the check that they start at 0.
inline int check_leg_offsets(const std::string& w, const HostBatch& t, int64_t i0, int64_t i1) {
    if (i0 == 0 && (t.fix_off[0] != 0 || t.flt_off[0] != 0)) return adr_set_error(ADR_ERR_INVALID, w + ": offsets must start at 0");
    for (int64_t i = i0; i < i1; ++i) {
        const int64_t mf = t.fix_off[i + 1] - t.fix_off[i], ml = t.flt_off[i + 1] - t.flt_off[i];
        if (mf < 0 || ml < 0 || mf > INT16_MAX || ml > INT16_MAX)
            return adr_set_error(ADR_ERR_INVALID, w + ": offsets must be non-decreasing, <= 32767 flows per leg");
    }
    return ADR_OK;
}

// The notional, spread and leg signs of trades i0 .. i1 - 1.
inline int check_trade_values(const std::string& w, const HostBatch& t, int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
        if (!std::isfinite(t.notional[i]) || !std::isfinite(t.spread[i]))
            return adr_set_error(ADR_ERR_INVALID, w + ": notionals and spreads must be finite");
        if (!(t.fix_sign[i] == 1.0 || t.fix_sign[i] == -1.0) || !(t.flt_sign[i] == 1.0 || t.flt_sign[i] == -1.0))
            return adr_set_error(ADR_ERR_INVALID, w + ": leg signs must be +1 or -1");
    }
    return ADR_OK;
}

// The cash-flow arrays: present where their leg has flows, and finite.
inline int check_flows(const std::string& w, const HostBatch& t) {
    const int64_t n_fix = t.fix_off[t.n], n_flt = t.flt_off[t.n];
    if ((n_fix > 0 && (!t.fix_tp || !t.fix_pay)) || (n_flt > 0 && (!t.flt_tp || !t.flt_ts || !t.flt_te || !t.flt_alpha)))
        return adr_set_error(ADR_ERR_INVALID, w + ": null cash-flow array");
    auto finite = [](const double* a, int64_t m) {
        bool ok = true;
        for (int64_t i = 0; i < m; ++i) ok &= std::isfinite(a[i]);
        return ok;
    };
    if (!finite(t.fix_tp, n_fix) || !finite(t.fix_pay, n_fix) || !finite(t.flt_tp, n_flt) || !finite(t.flt_ts, n_flt) ||
        !finite(t.flt_te, n_flt) || !finite(t.flt_alpha, n_flt) || (t.flt_weight && !finite(t.flt_weight, n_flt)))
        return adr_set_error(ADR_ERR_INVALID, w + ": times, amounts, accruals and weights must be finite");
    return ADR_OK;
}

// The curves of a set for a `_set` entry of `ctx`: device arrays, read where the device builder left them.
struct SetCurves {
    int method, K, S;
    const double *times, *dfs;
};

inline int curve_set_curves(const std::string& w, const adr_ctx* ctx, const adr_curve_set* set, SetCurves* c) {
    const adr_ctx* owner = nullptr;
    const int rc = adr_curve_set_device_view(set, &owner, &c->method, &c->K, &c->S, &c->times, &c->dfs);
    if (rc != ADR_OK) return rc;
    if (owner != ctx) return adr_set_error(ADR_ERR_INVALID, w + ": the curve set belongs to another ctx");
    return ADR_OK;
}

}  // namespace scen
}  // namespace adr
